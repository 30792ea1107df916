"""The Gram distance kernel on the MI355X (dlsim_gram_sqdist and its tensors
entry, model_distances(method="gram"), the Krum plugins with distance="gram")
against the longdouble oracle of tests/_krum_util.py under the contract's own
bound, 2 (P + 16) 2^-53 (S_i + S_j) (tests/_gram_util.py). Every call writes
into a guarded 0xA5-prefilled matrix; sizes come from dlsim_gramdist_geometry
(tile T, grid cap B)."""
from __future__ import annotations

import copy
import types

import numpy as np
import pytest
import torch

import _edge_util as eu
import _gram_util as gu
import _krum_util as ku
from sgd_inputs import GNLENET_SHAPES

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Bulyan, Krum, MultiKrum, model_distances  # noqa: E402

DEV = "cuda"
MULTI_TILE = {(17, "f32"), (32, "bf16"), (16, "f16")}


def _geometry(n, dtype):
    return _native.gramdist_geometry(n, eu.DTYPES[dtype], 10 ** 10)


def _gram(xs, accumulate=False, into=None):
    """One guarded call. Returns (n x n float64 host matrix, its Guarded)."""
    n = len(xs)
    h = eu.guarded(n * n * 8, "f64", DEV) if into is None else into
    _native.gram_sqdist(xs, h.view, accumulate=accumulate)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == [] and eu.unwritten(h) == 0
    return h.view.cpu().numpy().reshape(n, n).copy(), h


def _assert_matrix(got, rows, dtype, what, want=None):
    problems, worst = gu.gram_problems(got, rows, dtype, want)
    print(f"{what}: max err / bound {worst:.4f}")
    assert not problems, f"{what}: {problems}"


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _separated(n, p, dtype, seed):
    rng = np.random.default_rng(seed)
    return eu.encode(rng.standard_normal(p)[None, :] + 1e-2 * rng.standard_normal((n, p)), dtype).reshape(n, p)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", (2, 9, 16, 17, 32))
def test_flat_entry_over_sizes(n, dtype):
    T, B = _geometry(n, dtype)
    sizes = [1, 3, 5, T - 1, T, T + 1] + ([2 * B * T + T + 3] if (n, dtype) in MULTI_TILE else [])
    rows = _separated(n, sizes[-1], dtype, seed=2000 + n)
    xd = eu.place(list(rows), dtype, DEV)
    for p in sizes:
        xs = [x[:p] for x in xd]
        got, _ = _gram(xs)
        _assert_matrix(got, rows[:, :p], dtype, f"{dtype} n={n} P={p}")
        assert _same(got, _gram(xs)[0]), f"{dtype} n={n} P={p}: a second call gave other bits"
    assert eu.inputs_unchanged(xd, rows, dtype)


@pytest.mark.parametrize("tiles", (1, 16))
@pytest.mark.parametrize("n", (16, 32))
def test_cancellation(n, tiles):
    """Rows 1e3 base + 1e-3 noise: norms 10^6 x the distances. The bound is
    written in S, the distances to row 0, so a Gram matrix of uncentred rows,
    whose error scales with the norms, is not expected to meet it. At P = T + 1
    (T = 512) the uncentred bound is about 0.1 of the distances; from
    P = 16 T + 1 on it exceeds them (test_gram_cpu.py asserts both), so that
    size is run as well."""
    T, _ = _geometry(n, "f32")
    rows = gu.cancelling_rows(n, tiles * T + 1)
    got, _ = _gram(eu.place(list(rows), "f32", DEV))
    _assert_matrix(got, rows, "f32", f"cancellation n={n} P={tiles * T + 1}")


@pytest.mark.parametrize("kind", ["nan", "inf", "inf_pair"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", (17, 32))
def test_non_finite_rows_are_nan_and_the_rest_is_unaffected(n, dtype, kind):
    T, _ = _geometry(n, dtype)
    E = eu.VEC_ELEMS[dtype]
    p = 2 * T + T // 2 + E + (E - 1)
    pos = eu.edge_positions(p, T, E)
    assert len(pos) == 5
    base = eu.decode(_separated(n, p, dtype, seed=31 + n), dtype)
    flagged = (0, 5, n - 1)  # row 0 (the centre), a row of the first block, a row of the second
    for k, r in enumerate(flagged):
        for e in pos:
            x = base.copy()
            x[r, e] = np.nan if kind == "nan" else np.inf
            if kind == "inf_pair":
                x[flagged[(k + 1) % 3], e] = -np.inf
            rows = eu.encode(x, dtype).reshape(n, p)
            got, _ = _gram(eu.place(list(rows), dtype, DEV))
            _assert_matrix(got, rows, dtype, f"{dtype} n={n} {kind} in row {r} at {e}")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", (5, 17))
def test_accumulate_over_two_halves_is_exact_on_small_integers(n, dtype):
    T, _ = _geometry(n, dtype)
    p = 5 * T + 3
    rows = eu.encode(np.random.default_rng(n).integers(-8, 9, size=(n, p)).astype(np.float64), dtype).reshape(n, p)
    xd = eu.place(list(rows), dtype, DEV)
    for h in (3 * T + 2 * eu.VEC_ELEMS[dtype], 2 * T + 1):  # the second half aligned, then off alignment
        _, g = _gram([x[:h] for x in xd])
        got, _ = _gram([x[h:] for x in xd], accumulate=True, into=g)
        assert np.array_equal(got, ku.sqdist_oracle(rows, dtype).astype(np.float64))
    x = xd[0]
    for m in (1, 3):  # no element, or one input: zeros, and nothing when accumulating
        xs = [x[:0]] * m if m > 1 else [x]
        got, g = _gram(xs)
        assert not got.view(np.uint64).any()
        g.view.fill_(2.5)
        _native.gram_sqdist(xs, g.view, accumulate=True)
        torch.cuda.synchronize()
        assert bool((g.view == 2.5).all()) and eu.check_guards(g) == []


@pytest.mark.parametrize("dtype,offset", [("f32", 4), ("f32", 8), ("bf16", 2), ("bf16", 4), ("f16", 2), ("f16", 8)])
@pytest.mark.parametrize("n", (9, 17))
def test_misaligned_inputs_take_the_scalar_form(n, dtype, offset):
    rows = _separated(n, 2 * 128 + 3, dtype, seed=500 + n)
    for offs in ([offset] * n, [0] * (n - 1) + [offset]):
        xd = eu.place(list(rows), dtype, DEV, offs)
        assert any(x.data_ptr() % 16 for x in xd)
        for p in (1, 127, 129, rows.shape[1]):
            got, _ = _gram([x[:p] for x in xd])
            _assert_matrix(got, rows[:, :p], dtype, f"{dtype} n={n} P={p} offsets {offs[0]}, {offs[-1]}")
        assert _same(got, _gram(xd)[0]) and eu.inputs_unchanged(xd, rows, dtype)


@pytest.mark.parametrize("n,dtype", [(8, "f32"), (17, "bf16")])
def test_tensors_entry_equals_flat_calls_on_the_gnlenet_shapes(n, dtype):
    numels = [int(np.prod(s)) for s in GNLENET_SHAPES]
    rows = _separated(n, sum(numels), dtype, seed=11 + n)
    offs = np.concatenate([[0], np.cumsum(numels)])
    tensors = [eu.place([r[offs[k]:offs[k + 1]] for k in range(len(numels))], dtype, DEV) for r in rows]
    stream = torch.cuda.current_stream().cuda_stream
    flat, one = eu.guarded(n * n * 8, "f64", DEV), eu.guarded(n * n * 8, "f64", DEV)
    for k in range(len(numels)):
        _native.gram_sqdist([t[k] for t in tensors], flat.view, accumulate=k > 0)
    _native.gram_sqdist_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels,
                                    _native.dtype_code(eu.DTYPES[dtype]), one.view.data_ptr(), False, stream)
    torch.cuda.synchronize()
    assert eu.check_guards(one) == [] and eu.unwritten(one) == 0
    assert _same(flat.view.cpu().numpy(), one.view.cpu().numpy())


PLACES = {"host": lambda m: m, "arena": lambda m: arena.to_device_arena(m, DEV),
          "tensors": lambda m: copy.deepcopy(m).to(DEV)}


@pytest.mark.parametrize("place", sorted(PLACES))
def test_model_distances_gram_on_every_route(place):
    rows, _, want, cpu = ku.plugin_case(17, 3)
    got = model_distances([PLACES[place](m) for m in cpu], method="gram")
    assert got.shape == (17, 17) and got.dtype == torch.float64 and not got.is_cuda
    # per tensor the bound holds with that tensor's S and P: their sum is below the whole row's bound
    _assert_matrix(got.numpy(), rows, "f32", f"model_distances gram {place}", want)


def test_model_distances_gram_adds_dtype_groups():
    n = 9
    f32 = _separated(n, 33 * 7, "f32", 1)
    b16 = _separated(n, 129, "bf16", 2)

    class Mixed(torch.nn.Module):
        def __init__(self, i):
            super().__init__()
            self.a = torch.nn.Parameter(eu.to_torch(f32[i], "f32").reshape(33, 7))
            self.b = torch.nn.Parameter(eu.to_torch(b16[i], "bf16"))

    got = model_distances([Mixed(i).to(DEV) for i in range(n)], method="gram").numpy()
    _, g = _gram(eu.place(list(f32), "f32", DEV))
    manual, _ = _gram(eu.place(list(b16), "bf16", DEV), accumulate=True, into=g)
    assert _same(got, manual)
    want = ku.add_oracles([ku.sqdist_oracle(f32, "f32"), ku.sqdist_oracle(b16, "bf16")])
    lim = gu.entry_bounds(gu.centred_sums(f32, "f32")[0], 231) + gu.entry_bounds(gu.centred_sums(b16, "bf16")[0], 129)
    assert (np.abs(got.astype(np.longdouble) - want) <= lim + ku.U * want).all()


@pytest.mark.parametrize("n,f,special,byz", [(17, 3, False, None), (17, 3, True, None), (32, 8, False, None),
                                             (32, 8, True, None), (32, 7, False, None), (17, 3, True, (0, 4, 9))])
def test_plugins_with_the_gram_distance_equal_the_exact_ones(n, f, special, byz):
    """test_gram_cpu.py asserts that these inputs' score gaps exceed the Gram
    bound, so both distances select the same models and the results agree bit
    for bit. byz = (0, 4, 9) with special: model 0 is all-NaN."""
    _, _, _, cpu = ku.plugin_case(n, f, special=special, byz=byz)
    models = [arena.to_device_arena(m, DEV) for m in cpu]
    plugins = [Krum.with_params, MultiKrum.with_params, lambda f, distance: MultiKrum.with_params(f, 2, distance)]
    if n >= 4 * f + 3:
        plugins.append(Bulyan.with_params)
    for make in plugins:
        exact, gram = make(f, distance="exact").aggregate(models), make(f, distance="gram").aggregate(models)
        assert np.array_equal(ku.flat_bits(exact), ku.flat_bits(gram))
    if not special:
        s = types.SimpleNamespace(gradient_aggregation=M.MULTI_KRUM, aggregation_byzantine=f, aggregation_distance="gram")
        res = functions.aggregate(s, {"models": cpu, "round": 1, "peer": 0})
        assert np.array_equal(ku.flat_bits(res[0]), ku.flat_bits(MultiKrum.with_params(f).aggregate(cpu)))
