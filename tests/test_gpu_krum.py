"""The pairwise squared-distance kernel and the Krum plugins on the MI355X
(dlsim_pairwise_sqdist, dlsim_pairwise_sqdist_tensors, arena.model_distances,
dasklearn_amd.gradient_aggregation.krum) against the longdouble oracle and the
restated selection rule of tests/_krum_util.py.

Every call writes into a guarded 0xA5-prefilled matrix (_edge_util.guarded):
no guard byte may change and no entry may stay unwritten. Sizes come from
dlsim_pairdist_geometry: with tile T and grid cap B (B * T is at most 2 M
elements for every n and dtype, so all four dtypes run at the largest size,
2 B T + T + 3) blocks take zero, one, two and unequal numbers of tiles."""
from __future__ import annotations

import copy
import types

import numpy as np
import pytest
import torch
from torch import nn

import _edge_util as eu
import _krum_util as ku
from _sgd_util import BnNet
from sgd_inputs import GNLENET_SHAPES
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Krum, MultiKrum, krum_select, model_distances  # noqa: E402

DEV = "cuda"
HUGE = 10 ** 10
FAN_INS = (1, 2, 3, 8, 9, 16, 17, 32)


def _geometry(n, dtype):
    """(T, B): the tile and the grid cap of n inputs of dtype."""
    return _native.pairdist_geometry(n, eu.DTYPES[dtype], HUGE)


def _dist(xs, accumulate=False, into=None):
    """One guarded call. Returns (n x n float64 host matrix, its Guarded)."""
    n = len(xs)
    h = eu.guarded(n * n * 8, "f64", DEV) if into is None else into
    _native.pairwise_sqdist(xs, h.view, accumulate=accumulate)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == [], "guard bytes written"
    assert eu.unwritten(h) == 0, "entries left unwritten"
    return h.view.cpu().numpy().reshape(n, n).copy(), h


def _assert_matrix(got, want, n_elems, what):
    problems, worst = ku.matrix_problems(got, want, n_elems)
    print(f"{what}: max err / bound {worst:.4f}")
    assert not problems, f"{what}: {problems}"


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- the flat entry over shapes ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", FAN_INS)
def test_flat_entry_over_sizes(n, dtype):
    """Every size is a prefix of one set of rows; the oracle of a prefix is the
    sum of the oracles of the segments between consecutive sizes (longdouble
    additions), so one pass over the longest rows serves all sizes."""
    T, B = _geometry(n, dtype)
    assert B * T <= 4 * 1024 * 1024
    sizes = sorted({1, 3, 4, 5, T - 1, T, T + 1, B * T - 1, B * T + 1, 2 * B * T + T + 3})
    if n == 1:
        sizes = [1, 5, T + 1]
    rows = eu.random_rows(dtype, n, sizes[-1], seed=2000 + n)
    xd = eu.place(list(rows), dtype, DEV)
    acc, prev = None, 0
    for p in sizes:
        seg = ku.sqdist_oracle(rows[:, prev:p], dtype)
        acc = seg if acc is None else acc + seg
        prev = p
        xs = [x[:p] for x in xd]
        got, _ = _dist(xs)
        _assert_matrix(got, acc, p, f"{dtype} n={n} P={p}")
        again, _ = _dist(xs)
        assert _same(got, again), f"{dtype} n={n} P={p}: a second call gave other bits"
    assert eu.inputs_unchanged(xd, rows, dtype)


# ---- special values ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", (3, 8, 20))
def test_specials_at_the_edge_positions(n, dtype):
    """Specials at _edge_util.edge_positions (first and last vector of the full
    tiles, a wave's middle, the partial tile, the scalar tail), held by a row
    of the first, a middle and the last row group (n = 20: groups of 8, 8, 4)."""
    T, _ = _geometry(n, dtype)
    E = eu.VEC_ELEMS[dtype]
    p = 2 * T + T // 2 + E + (E - 1)
    pos = eu.edge_positions(p, T, E)
    assert len(pos) == 5
    base = eu.decode(eu.random_rows(dtype, n, p, seed=31 + n), dtype)
    r0, r1, r2 = 0, n // 2, n - 1

    def run(x, what, alias=None):
        rows = eu.encode(x, dtype).reshape(n, p)
        xd = eu.place(list(rows), dtype, DEV)
        if alias is not None:
            xd[alias[1]] = xd[alias[0]]
        got, _ = _dist(xd)
        _assert_matrix(got, ku.sqdist_oracle(rows, dtype), p, f"{dtype} n={n} {what}")
        assert eu.inputs_unchanged(xd, rows, dtype)
        return got

    for r in (r0, r1, r2):
        x = base.copy()
        x[r, pos] = np.nan
        got = run(x, f"NaN in row {r}")
        assert np.isnan(np.delete(got[r], r)).all() and np.isfinite(np.delete(np.delete(got, r, 0), r, 1)).all()
        x = base.copy()
        x[r, pos] = np.inf
        got = run(x, f"+Inf in row {r}")
        assert (np.delete(got[r], r) == np.inf).all()
    for a, b in ((r0, r2), (r1, r2), (r0, r1)):
        x = base.copy()
        x[a, pos] = x[b, pos] = np.inf
        got = run(x, f"+Inf in rows {a} and {b} at the same elements")
        assert np.isnan(got[a, b]) and (np.delete(got[a], [a, b]) == np.inf).all()
        x[b, pos] = -np.inf
        got = run(x, f"+Inf in row {a}, -Inf in row {b}")
        assert got[a, b] == np.inf
    # -0 against +0 is distance 0: the whole matrix is +0.0
    x = np.zeros((n, p))
    x[r1, pos] = -0.0
    x[r2] = -0.0
    got = run(x, "-0 against +0")
    assert not got.view(np.uint64).any()
    # subnormals of the dtype: exact in double for the three narrow dtypes
    # (an fp64 subnormal's square underflows; the contract keeps fp64 inputs above 1e-150)
    if dtype != "f64":
        tiny = eu._TINY[dtype]
        x = np.zeros((n, p))
        x[r1, pos] = tiny
        x[r2, pos[:2]] = -tiny
        got = run(x, "subnormals")
        assert got[r0, r1] == len(pos) * tiny * tiny and got[r0, r2] == 2 * tiny * tiny
        assert got[r1, r2] == 2 * (2 * tiny) ** 2 + (len(pos) - 2) * tiny * tiny
    # two identical rows, then one pointer passed twice: exactly +0.0, and the same matrix
    x = base.copy()
    x[r2] = x[r0]
    got = run(x, "two identical rows")
    assert got.view(np.uint64)[r0, r2] == 0
    twice = run(x, "the same pointer twice", alias=(r0, r2))
    assert _same(got, twice)


# ---- accumulate ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", (5, 17))
def test_accumulate_over_two_halves(n, dtype):
    """Two calls over [0, h) and [h, p), the second accumulating, against the
    oracles of the halves added in that order. The halves are within
    (h + 8) u and (p - h + 8) u of their exact values and the final addition
    rounds once more; all terms are non-negative, so the sum is within
    (max(h, p - h) + 9) u <= (p + 8) u of the exact whole: the bound of one
    call over p elements. Small-integer rows give exact integer distances."""
    T, _ = _geometry(n, dtype)
    E = eu.VEC_ELEMS[dtype]
    p = 5 * T + 3
    rows = eu.random_rows(dtype, n, p, seed=77 + n)
    ints = eu.encode(np.random.default_rng(n).integers(-8, 9, size=(n, p)).astype(np.float64), dtype).reshape(n, p)
    for h in (3 * T + 2 * E, 2 * T + 1):  # the second half on the vector path, then off alignment
        for what, r in (("random", rows), ("small integers", ints)):
            xd = eu.place(list(r), dtype, DEV)
            first, g = _dist([x[:h] for x in xd])
            _assert_matrix(first, ku.sqdist_oracle(r[:, :h], dtype), h, f"{dtype} n={n} first half")
            got, _ = _dist([x[h:] for x in xd], accumulate=True, into=g)
            want = ku.add_oracles([ku.sqdist_oracle(r[:, :h], dtype), ku.sqdist_oracle(r[:, h:], dtype)])
            _assert_matrix(got, want, p, f"{dtype} n={n} {what} split at {h}")
            if what == "small integers":
                assert np.array_equal(got, want.astype(np.float64)), "integer distances are exact"
            assert eu.inputs_unchanged(xd, r, dtype)


def test_zero_elements_and_one_input():
    x = torch.ones(16, device=DEV)
    for n in (1, 3):
        got, g = _dist([x[:0]] * n)  # zeros
        assert not got.view(np.uint64).any()
        g.view.fill_(2.5)
        _native.pairwise_sqdist([x[:0]] * n, g.view, accumulate=True)  # untouched
        torch.cuda.synchronize()
        assert bool((g.view == 2.5).all()) and eu.check_guards(g) == []
    got, g = _dist([x])
    assert got.view(np.uint64)[0, 0] == 0
    g.view.fill_(7.0)
    _native.pairwise_sqdist([x], g.view, accumulate=True)
    torch.cuda.synchronize()
    assert g.view.item() == 7.0


# ---- alignment -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,offset", [("f32", 4), ("bf16", 2), ("bf16", 4), ("f16", 2), ("f64", 8)])
@pytest.mark.parametrize("n", (5, 9))
def test_misaligned_inputs_take_the_scalar_path(n, dtype, offset):
    """One input off a 16-byte boundary sends the call down the scalar kernel:
    tiles of 256 elements under the same grid cap."""
    _, B = _geometry(n, dtype)
    sizes = (1, 255, 257, 2 * B * 256 + 256 + 3)
    rows = eu.random_rows(dtype, n, sizes[-1], seed=500 + n)
    for offs in ([offset] * n, [0] * (n - 1) + [offset]):
        xd = eu.place(list(rows), dtype, DEV, offs)
        assert any(x.data_ptr() % 16 for x in xd)
        for p in sizes:
            got, _ = _dist([x[:p] for x in xd])
            _assert_matrix(got, ku.sqdist_oracle(rows[:, :p], dtype), p, f"{dtype} n={n} P={p} offsets {offs[0]}, {offs[-1]}")
        again, _ = _dist(xd)
        assert _same(got, again)
        assert eu.inputs_unchanged(xd, rows, dtype)


def test_overlapping_matrix_is_refused_and_nothing_runs():
    buf = torch.ones(1000, dtype=torch.float64, device=DEV)
    xs = [buf[:400], buf[400:800]]
    torch.cuda.synchronize()
    for out in (buf[0:4], buf[398:402], buf[796:800]):
        with pytest.raises(_native.DlsimError) as e:
            _native.pairwise_sqdist(xs, out)
        assert e.value.rc == _native.DLSIM_E_ARG and "overlaps" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all())


# ---- the tensors entry -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", (8, 17))
def test_tensors_entry_equals_flat_calls_on_the_gnlenet_shapes(n, dtype):
    numels = [int(np.prod(s)) for s in GNLENET_SHAPES]
    assert len(numels) == 14 and sum(numels) == 85_354
    rows = eu.random_rows(dtype, n, sum(numels), seed=11 + n)
    offs = np.concatenate([[0], np.cumsum(numels)])
    tensors = [eu.place([r[offs[k]:offs[k + 1]] for k in range(14)], dtype, DEV) for r in rows]
    stream = torch.cuda.current_stream().cuda_stream
    code = _native.dtype_code(eu.DTYPES[dtype], single_task=True)
    for start in (False, True):  # the caller's accumulate goes to the first tensor only
        flat = eu.guarded(n * n * 8, "f64", DEV)
        one = eu.guarded(n * n * 8, "f64", DEV)
        if start:
            _dist([t[13] for t in tensors], into=flat)
            _dist([t[13] for t in tensors], into=one)
        for k in range(14):
            _native.pairwise_sqdist([t[k] for t in tensors], flat.view, accumulate=start or k > 0)
        _native.pairwise_sqdist_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels, code,
                                            one.view.data_ptr(), start, stream)
        torch.cuda.synchronize()
        assert eu.check_guards(one) == [] and eu.unwritten(one) == 0
        a, b = flat.view.cpu().numpy(), one.view.cpu().numpy()
        assert _same(a, b)
        if not start:
            _assert_matrix(b.reshape(n, n), ku.sqdist_oracle(rows, dtype), sum(numels), f"{dtype} n={n} tensors")
    # no tensor at all: zeros, or nothing when accumulating
    one.view.fill_(3.0)
    _native.pairwise_sqdist_tensors_raw([], n, [], code, one.view.data_ptr(), True, stream)
    torch.cuda.synchronize()
    assert bool((one.view == 3.0).all())
    _native.pairwise_sqdist_tensors_raw([], n, [], code, one.view.data_ptr(), False, stream)
    torch.cuda.synchronize()
    assert not one.view.cpu().numpy().view(np.uint64).any()


# ---- inputs past one launch's offsets -----------------------------------------------------------
def test_input_past_two_gib_runs_as_ranges():
    """fp32, n = 2: the first range is (2^31 - 2^20) / 4 elements, the rest
    accumulates. The rows differ by 1 at a few elements of either range, so the
    distance is their count, an exact integer."""
    first = ((1 << 31) - (1 << 20)) // 4
    p = first + 4099
    a = torch.zeros(p, device=DEV)
    b = torch.zeros(p, device=DEV)
    hot = [0, 1023, first - 1, first, first + 1, first + 4096, p - 1]
    b[hot] = 1.0
    a[5] = b[5] = float(2 ** 20)  # equal elements add nothing
    got, _ = _dist([a, b])
    assert got[0, 1] == len(hot) == got[1, 0] and got[0, 0] == 0 == got[1, 1]
    a[first + 7] = -2.0
    got, _ = _dist([a, b])
    assert got[0, 1] == len(hot) + 4


# ---- model_distances -----------------------------------------------------------------------------
class Mixed(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(33, 7))
        self.b = nn.Parameter(torch.zeros(129, dtype=torch.bfloat16))
        self.c = nn.Parameter(torch.zeros(5))
        self.d = nn.Parameter(torch.zeros(4, 9, dtype=torch.bfloat16))


PLACES = {"host": lambda m: m, "arena": lambda m: arena.to_device_arena(m, DEV),
          "tensors": lambda m: copy.deepcopy(m).to(DEV)}


@pytest.mark.parametrize("place", sorted(PLACES))
def test_model_distances_on_every_route(place):
    n = 9
    rows, _, want, cpu = ku.plugin_case(n, 2)
    got = model_distances([PLACES[place](m) for m in cpu])
    assert got.shape == (n, n) and got.dtype == torch.float64 and not got.is_cuda
    _assert_matrix(got.numpy(), want, rows.shape[1], f"model_distances {place}")
    if place != "tensors":  # one aligned row per model: the flat entry's bits
        flat, _ = _dist(eu.place(list(rows), "f32", DEV))
        assert _same(got.numpy(), flat)


@pytest.mark.parametrize("place", sorted(PLACES))
def test_model_distances_adds_dtype_groups_in_layout_order(place):
    n = 6
    rng = np.random.default_rng(9)
    f32 = eu.encode(rng.standard_normal((n, 33 * 7 + 5)), "f32")
    b16 = eu.encode(rng.standard_normal((n, 129 + 36)), "bf16").reshape(n, -1)
    cpu = []
    for i in range(n):
        m = Mixed()
        with torch.no_grad():
            m.a.copy_(eu.to_torch(f32[i, :231], "f32").reshape(33, 7))
            m.c.copy_(eu.to_torch(f32[i, 231:], "f32"))
            m.b.copy_(eu.to_torch(b16[i, :129], "bf16"))
            m.d.copy_(eu.to_torch(b16[i, 129:], "bf16").reshape(4, 9))
        cpu.append(m)
    got = model_distances([PLACES[place](m) for m in cpu]).numpy()
    want = ku.add_oracles([ku.sqdist_oracle(f32, "f32"), ku.sqdist_oracle(b16, "bf16")])
    _assert_matrix(got, want, 236 + 165, f"mixed {place}")
    if place != "tensors":  # the fp32 group first, the bf16 group accumulated onto it
        _, g = _dist(eu.place(list(f32), "f32", DEV))
        manual, _ = _dist(eu.place(list(b16), "bf16", DEV), accumulate=True, into=g)
        assert _same(got, manual)
    with pytest.raises(ValueError):
        model_distances([cpu[0], nn.Linear(3, 2), cpu[1]])


# ---- the plugins -----------------------------------------------------------------------------------
def _fedavg_oracle(rows, chosen):
    return orc.wreduce([rows[i] for i in chosen], orc.reference_weights(len(chosen), None), "f32")


def _flat(model):
    return np.concatenate([p.detach().cpu().reshape(-1).numpy() for p in model.parameters()])


@pytest.mark.parametrize("place", ["host", "arena"])
@pytest.mark.parametrize("n,f", ku.GPU_PLUGIN_CONFIGS)
def test_plugins_select_what_the_oracle_selects(n, f, place):
    rows, byz, want, cpu = ku.plugin_case(n, f)
    models = [PLACES[place](m) for m in cpu]
    before = [ku.flat_bits(m) for m in models]
    d2 = model_distances(models).tolist()
    want64 = want.astype(np.float64)
    for m in (1, 2, n - f):
        assert krum_select(d2, f, m) == ku.ref_select(d2, f, m) == ku.ref_select(want64, f, m)
    best = ku.ref_select(want64, f, 1)[0]
    out = Krum.with_params(f).aggregate(models)
    assert type(out) is type(models[0])
    for g, p0, pb in zip(out.parameters(), models[0].parameters(), models[best].parameters()):
        assert g.device == p0.device and g.shape == p0.shape and g.requires_grad == p0.requires_grad
        assert g.data_ptr() != pb.data_ptr()
    assert np.array_equal(ku.flat_bits(out), before[best]), "Krum is a bit-for-bit copy of the selected model"
    for m in (None, 1, 2):
        chosen = ku.ref_select(want64, f, n - f if m is None else m)
        out = MultiKrum.with_params(f, m).aggregate(models)
        assert orc.same_bits(_flat(out), _fedavg_oracle(rows, chosen)), f"Multi-Krum m={m}"
        ref = FedAvg.aggregate([models[i] for i in chosen])
        assert np.array_equal(ku.flat_bits(out), ku.flat_bits(ref))
        assert all(g.device == p0.device for g, p0 in zip(out.parameters(), models[0].parameters()))
    # to_host overrides where the result lives
    out = Krum.with_params(f).aggregate(models, to_host=(place != "host"))
    assert all(p.is_cuda == (place == "host") for p in out.parameters())
    assert np.array_equal(ku.flat_bits(out), before[best])
    out = MultiKrum.with_params(f, 2).aggregate(models, to_host=(place != "host"))
    assert all(p.is_cuda == (place == "host") for p in out.parameters())
    assert orc.same_bits(_flat(out), _fedavg_oracle(rows, ku.ref_select(want64, f, 2)))
    for m_, saved in zip(models, before):
        assert np.array_equal(ku.flat_bits(m_), saved), "an input model changed"


@pytest.mark.parametrize("place", ["host", "tensors"])
def test_buffers_are_those_of_model_zero_even_when_it_is_byzantine(place):
    def bn():
        m = BnNet()
        with torch.no_grad():
            m.bn.running_mean.uniform_(-1, 1)
            m.bn.num_batches_tracked.fill_(int(torch.randint(1, 99, ()).item()))
        return m
    n, f = 8, 2
    rows, byz, want, _ = ku.plugin_case(n, f, shapes=([5, 7], [5], [5], [5]), byz=(0, 5))
    torch.manual_seed(3)
    models = [PLACES[place](ku.model_of(r, None, "f32", make=bn)) for r in rows]
    want64 = want.astype(np.float64)
    for agg, m in ((Krum.with_params(f), 1), (MultiKrum.with_params(f), n - f), (MultiKrum.with_params(f, 2), 2)):
        chosen = ku.ref_select(want64, f, m)
        assert 0 not in chosen
        out = agg.aggregate(models)
        assert isinstance(out, BnNet)
        bufs, bufs0 = list(out.buffers()), list(models[0].buffers())
        assert len(bufs) == len(bufs0) == 3
        for b, b0 in zip(bufs, bufs0):
            assert b.device == b0.device and torch.equal(b, b0) and b.data_ptr() != b0.data_ptr()
        assert not torch.equal(out.bn.running_mean, models[chosen[0]].bn.running_mean)
        expect = rows[chosen[0]] if m == 1 else _fedavg_oracle(rows, chosen)
        assert orc.same_bits(_flat(out), np.asarray(expect))
        y = out.bn(out.fc(torch.ones(4, 7, device=bufs[0].device)))  # working submodules
        assert y.shape == (4, 5) and y.device == bufs[0].device


def test_a_nan_peer_and_an_inf_peer_do_not_reach_the_result():
    n, f = 8, 2
    rows, byz, want = ku.separated_models(n, f, 85_354, "f32", seed=7, nan_row=True, inf_row=True)
    cpu = [ku.model_of(r, GNLENET_SHAPES, "f32") for r in rows]
    assert np.isnan(rows[byz[0]]).all() and np.isinf(rows[byz[1]]).all()
    d2 = model_distances(cpu).numpy()
    _assert_matrix(d2, want, 85_354, "one all-NaN and one all-Inf peer")
    k = Krum.with_params(f).aggregate(cpu)
    mk = MultiKrum.with_params(f).aggregate(cpu)
    assert np.isfinite(_flat(k)).all() and np.isfinite(_flat(mk)).all()
    want64 = want.astype(np.float64)
    assert orc.same_bits(_flat(k), rows[ku.ref_select(want64, f, 1)[0]])
    assert orc.same_bits(_flat(mk), _fedavg_oracle(rows, ku.ref_select(want64, f, n - f)))
    avg = FedAvg.aggregate(cpu)
    assert not np.isfinite(_flat(avg)).any()


@pytest.mark.parametrize("method,m", [(4, None), (5, None), (5, 2)])
def test_functions_aggregate_through_model_manager(method, m):
    n, f = 8, 2
    rows, byz, want, cpu = ku.plugin_case(n, f)
    settings = types.SimpleNamespace(gradient_aggregation=method, aggregation_byzantine=f)
    if m is not None:
        settings.aggregation_multi_krum_m = m
    chosen = ku.ref_select(want.astype(np.float64), f, 1 if method == 4 else (n - f if m is None else m))
    expect = rows[chosen[0]] if method == 4 else _fedavg_oracle(rows, chosen)
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0})
    assert isinstance(res, list) and len(res) == 1
    assert not any(p.is_cuda for p in res[0].parameters())
    assert orc.same_bits(_flat(res[0]), np.asarray(expect))
    settings.aggregate_on_device = True
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": None})
    assert all(p.is_cuda for p in res[0].parameters())
    assert orc.same_bits(_flat(res[0]), np.asarray(expect))
    with pytest.raises(ValueError, match="unweighted"):
        functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0, "weights": [1 / n] * n})
