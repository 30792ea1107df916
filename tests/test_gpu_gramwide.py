"""The wide Gram distance kernel on the MI355X (dlsim_gram_sqdist_wide over 33
to 128 rows, method / distance "wide") against tests/_krum_util.py's longdouble
oracle under the contract's bound (tests/_gram_util.py), as tests/test_gpu_gram.py.
Sizes come from dlsim_gramwide_geometry (tile T, grid cap B)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
import _gram_util as gu
import _krum_util as ku
from test_gpu_gram import _assert_matrix, _same, _separated
from test_gramwide_cpu import WIDE_PLUGIN_CASES

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Bulyan, Krum, MultiKrum, bulyan_select, model_distances  # noqa: E402
from dasklearn_amd.gradient_aggregation.robust import MeanAroundMedian  # noqa: E402

DEV = "cuda"
DTYPES = ["f32", "bf16", "f16"]
MULTI_TILE = {"f32": 97, "bf16": 128, "f16": 33}  # the n that also runs 2 B T + T + 3 elements


def _geometry(n, dtype):
    return _native.gramwide_geometry(n, eu.DTYPES[dtype], 10 ** 10)


def _wide(xs, accumulate=False, into=None):
    """One guarded call. Returns (n x n float64 host matrix, its Guarded)."""
    n = len(xs)
    h = eu.guarded(n * n * 8, "f64", DEV) if into is None else into
    _native.gram_sqdist_wide(xs, h.view, accumulate=accumulate)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == [] and eu.unwritten(h) == 0
    return h.view.cpu().numpy().reshape(n, n).copy(), h


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (33, 48, 49, 64, 65, 96, 97, 127, 128))
def test_flat_entry_over_sizes(n, dtype):
    T, B = _geometry(n, dtype)
    sizes = [1, 3, T - 1, T, T + 1] + ([2 * B * T + T + 3] if MULTI_TILE[dtype] == n else [])
    rows = _separated(n, sizes[-1], dtype, seed=3000 + n)
    xd = eu.place(list(rows), dtype, DEV)
    for p in sizes:
        xs = [x[:p] for x in xd]
        got, _ = _wide(xs)
        _assert_matrix(got, rows[:, :p], dtype, f"{dtype} n={n} P={p}")
        assert _same(got, _wide(xs)[0]), f"{dtype} n={n} P={p}: a second call gave other bits"
    assert eu.inputs_unchanged(xd, rows, dtype)


@pytest.mark.parametrize("kind", ["nan", "inf", "inf_pair"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (49, 128))
def test_non_finite_rows_are_nan_and_the_rest_is_unaffected(n, dtype, kind):
    """Row 0 (the centre), rows of the first, second (the 16-bit deal's other parity) and last row block;
    the first element, one in each wave's K group, the tile edge, the partial tile and the tail."""
    T, _ = _geometry(n, dtype)
    E = eu.VEC_ELEMS[dtype]
    p = 2 * T + T // 2 + E + (E - 1)
    positions = (0, 17, 38, 59, 2 * T - 1, 2 * T + 5, p - 1)
    base = _separated(n, p, dtype, seed=41 + n)
    want = ku.sqdist_oracle(base, dtype)  # entries between finite rows do not move
    xd = eu.place(list(base), dtype, DEV)
    special = {v: eu.to_torch(eu.encode(np.array([v]), dtype), dtype).to(DEV) for v in (np.nan, np.inf, -np.inf)}
    flagged = (0, 5, 21, n - 1)
    for k, r in enumerate(flagged):
        r2 = flagged[(k + 1) % 4]
        for e in positions:
            rows = base.copy()
            hit = [(r, np.nan if kind == "nan" else np.inf)] + ([(r2, -np.inf)] if kind == "inf_pair" else [])
            for row, v in hit:
                rows[row, e] = eu.encode(np.array([v]), dtype)[0]
                xd[row][e:e + 1].copy_(special[v])
            got, _ = _wide(xd)
            _assert_matrix(got, rows, dtype, f"{dtype} n={n} {kind} in row {r} at {e}", want)
            for row, _ in hit:
                xd[row][e:e + 1].copy_(eu.to_torch(base[row, e:e + 1], dtype))
    assert eu.inputs_unchanged(xd, base, dtype)


@pytest.mark.parametrize("n,dtype", [(33, "f32"), (80, "bf16"), (128, "f16")])
def test_accumulate_and_the_tensors_entry_are_exact_on_small_integers(n, dtype):
    T, _ = _geometry(n, dtype)
    p = 5 * T + 3
    rows = eu.encode(np.random.default_rng(n).integers(-8, 9, size=(n, p)).astype(np.float64), dtype).reshape(n, p)
    want = ku.sqdist_oracle(rows, dtype).astype(np.float64)
    xd = eu.place(list(rows), dtype, DEV)
    for h in (3 * T + 2 * eu.VEC_ELEMS[dtype], 2 * T + 1):  # the second half aligned, then off alignment
        _, g = _wide([x[:h] for x in xd])
        got, _ = _wide([x[h:] for x in xd], accumulate=True, into=g)
        assert np.array_equal(got, want)
    # three tensors per row through the tensors entry: the bits of flat calls in order
    cuts = [0, T + 8, 3 * T + 16, p]
    flat, one = eu.guarded(n * n * 8, "f64", DEV), eu.guarded(n * n * 8, "f64", DEV)
    for k in range(3):
        _native.gram_sqdist_wide([x[cuts[k]:cuts[k + 1]] for x in xd], flat.view, accumulate=k > 0)
    _native.gram_sqdist_wide_tensors_raw([x[cuts[k]:].data_ptr() for x in xd for k in range(3)], n,
                                         [cuts[k + 1] - cuts[k] for k in range(3)], _native.dtype_code(eu.DTYPES[dtype]),
                                         one.view.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert eu.check_guards(one) == [] and eu.unwritten(one) == 0
    assert _same(flat.view.cpu().numpy(), one.view.cpu().numpy())
    assert np.array_equal(one.view.cpu().numpy().reshape(n, n), want)
    x = xd[0]
    got, g = _wide([x[:0]] * n)  # no element: zeros, and nothing when accumulating
    assert not got.view(np.uint64).any()
    g.view.fill_(2.5)
    _native.gram_sqdist_wide([x[:0]] * n, g.view, accumulate=True)
    torch.cuda.synchronize()
    assert bool((g.view == 2.5).all()) and eu.check_guards(g) == []


@pytest.mark.parametrize("dtype,offset", [("f32", 4), ("f32", 8), ("bf16", 2), ("f16", 8)])
@pytest.mark.parametrize("n", (33, 128))
def test_misaligned_inputs_take_the_scalar_form(n, dtype, offset):
    T, _ = _geometry(n, dtype)
    rows = _separated(n, 2 * T + 3, dtype, seed=600 + n)
    for offs in ([offset] * n, [0] * (n - 1) + [offset]):
        xd = eu.place(list(rows), dtype, DEV, offs)
        assert any(x.data_ptr() % 16 for x in xd)
        for p in (1, T - 1, T + 1, rows.shape[1]):
            got, _ = _wide([x[:p] for x in xd])
            _assert_matrix(got, rows[:, :p], dtype, f"{dtype} n={n} P={p} offsets {offs[0]}, {offs[-1]}")
        assert _same(got, _wide(xd)[0]) and eu.inputs_unchanged(xd, rows, dtype)


def test_cancellation():
    """Norms 10^6 x the distances: only centred operands meet a bound written in distances to row 0."""
    T, _ = _geometry(40, "f32")
    rows = gu.cancelling_rows(40, 16 * T + 1)
    got, _ = _wide(eu.place(list(rows), "f32", DEV))
    _assert_matrix(got, rows, "f32", f"cancellation n=40 P={16 * T + 1}")


@pytest.mark.parametrize("n,dtype", [(17, "f32"), (32, "bf16")])
def test_up_to_32_rows_are_forwarded_to_the_narrow_kernel(n, dtype):
    rows = _separated(n, 1500, dtype, seed=n)
    xd = eu.place(list(rows), dtype, DEV)
    h = eu.guarded(n * n * 8, "f64", DEV)
    _native.gram_sqdist(xd, h.view)
    assert _same(_wide(xd)[0], h.view.cpu().numpy().reshape(n, n))


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("n,f", WIDE_PLUGIN_CASES)
def test_plugins_with_the_wide_distance_select_what_the_oracle_selects(n, f, special):
    """test_gramwide_cpu.py: the score gaps exceed the Gram bound, so any in-bound matrix selects alike."""
    _, byz, want, cpu = ku.plugin_case(n, f, special=special)
    d2 = want.astype(np.float64)
    models = [arena.to_device_arena(m, DEV) for m in cpu]
    (best,) = ku.ref_select(d2, f, 1)
    krum = Krum.with_params(f, distance="wide").aggregate(models)
    assert np.array_equal(ku.flat_bits(krum), ku.flat_bits(cpu[best]))
    for m in (None, 2):
        chosen = ku.ref_select(d2, f, n - f if m is None else m)
        if special:
            assert byz[0] not in chosen and byz[-1] not in chosen  # the all-NaN and the all-Inf peer
        got = MultiKrum.with_params(f, m, distance="wide").aggregate(models)
        assert np.array_equal(ku.flat_bits(got), ku.flat_bits(FedAvg.aggregate([models[i] for i in chosen])))
    if n - 2 * f <= _native.MAX_ROBUST_INPUTS and n >= 4 * f + 3:
        chosen = bulyan_select(d2.tolist(), f)
        keep = len(chosen) - 2 * f
        got = Bulyan.with_params(f, distance="wide").aggregate(models)
        ref = MeanAroundMedian.aggregate([models[i] for i in chosen], keep=keep)
        assert np.array_equal(ku.flat_bits(got), ku.flat_bits(ref))
    elif n >= 4 * f + 3:
        with pytest.raises(ValueError, match="at most 32"):
            Bulyan.with_params(f, distance="wide").aggregate(models)


def test_model_distances_wide_adds_dtype_groups():
    n = 40
    f32 = _separated(n, 33 * 7, "f32", 1)
    b16 = _separated(n, 129, "bf16", 2)

    class Mixed(torch.nn.Module):
        def __init__(self, i):
            super().__init__()
            self.a = torch.nn.Parameter(eu.to_torch(f32[i], "f32").reshape(33, 7))
            self.b = torch.nn.Parameter(eu.to_torch(b16[i], "bf16"))

    got = model_distances([Mixed(i).to(DEV) for i in range(n)], method="wide").numpy()
    _, g = _wide(eu.place(list(f32), "f32", DEV))
    manual, _ = _wide(eu.place(list(b16), "bf16", DEV), accumulate=True, into=g)
    assert _same(got, manual)  # each group's call is checked against the bound above
