"""The fused reduce-and-measure kernel and the geometric-median and
centered-clipping plugins on the MI355X (dlsim_wreduce_dist,
dlsim_wreduce_dist_tensors, arena.reduce_with_distances,
dasklearn_amd.gradient_aggregation.geomed) against the FedAvg oracle, the
longdouble distance oracle and the restated trajectories of
tests/_geomed_util.py.

Every call writes into guarded 0xA5-prefilled `out` and `d2` buffers
(_edge_util.guarded): no guard byte may change, no d2 entry may stay unwritten
and `out` equals the oracle bit for bit. Sizes come from
dlsim_reducedist_geometry: with tile T and grid cap B blocks take zero, one,
two and unequal numbers of tiles."""
from __future__ import annotations

import copy
import types

import numpy as np
import pytest
import torch
from torch import nn

import _edge_util as eu
import _geomed_util as gu
import _krum_util as ku
from _sgd_util import BnNet
from sgd_inputs import GNLENET_SHAPES
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation import geomed  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian  # noqa: E402

DEV = "cuda"
HUGE = 10 ** 10
FAN_INS = (1, 2, 3, 8, 9, 16, 17, 32)
ALL = ["f32", "f64", "bf16", "f16"]


def _geometry(n, dtype):
    """(T, B): the tile and the grid cap of n inputs of dtype."""
    return _native.reducedist_geometry(n, eu.DTYPES[dtype], HUGE)


def _weights(n, kind, dtype):
    if kind == "dirichlet":
        return eu.special_weights(n, "dirichlet", dtype)
    return orc.reference_weights_f64(n, None) if dtype == "f64" else orc.reference_weights(n, None)


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _run(xs, w, dtype, with_out=True, accumulate=False, into=None, out_offset=0):
    """One guarded call. Returns (out storage or None, d2 host vector, d2's Guarded)."""
    n, p = len(xs), xs[0].numel()
    hd = eu.guarded(n * 8, "f64", DEV) if into is None else into
    ho = eu.guarded(p * eu.ESIZE[dtype], dtype, DEV, offset=out_offset) if with_out else None
    _native.wreduce_dist(xs, [float(v) for v in w], None if ho is None else ho.view, hd.view, accumulate=accumulate)
    torch.cuda.synchronize()
    assert eu.check_guards(hd) == [], "guard bytes around d2 written"
    assert eu.unwritten(hd) == 0, "d2 entries left unwritten"
    out = None
    if ho is not None:
        assert eu.check_guards(ho) == [], "guard bytes around out written"
        out = eu.from_torch(ho.view, dtype)
    return out, hd.view.cpu().numpy().copy(), hd


def _assert_vector(got, want, n_elems, what):
    problems, worst = gu.vector_problems(got, want, n_elems)
    print(f"{what}: max err / bound {worst:.4f}")
    assert not problems, f"{what}: {problems}"


def _wreduce(xs, w, dtype):
    ref = torch.empty_like(xs[0])
    _native.wreduce(xs, np.asarray(w, dtype=np.float64 if dtype == "f64" else np.float32), ref)
    torch.cuda.synchronize()
    return eu.from_torch(ref, dtype)


# ---- the flat entry over shapes ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("n", FAN_INS)
def test_flat_entry_over_sizes(n, dtype):
    """Every size is a prefix of one set of rows. The fold is per element, so a
    prefix's output is the prefix of the longest output; the distance oracle
    of a prefix is the sum of the oracles of the segments between consecutive
    sizes (longdouble additions)."""
    T, B = _geometry(n, dtype)
    assert B * T <= 4 * 1024 * 1024
    sizes = sorted({1, 3, 4, 5, T - 1, T, T + 1, B * T - 1, B * T + 1} | ({2 * B * T + T + 3} if n <= 9 else set()))
    rows = eu.random_rows(dtype, n, sizes[-1], seed=3000 + n)
    xd = eu.place(list(rows), dtype, DEV)
    for kind in ("dirichlet", "uniform"):
        w = _weights(n, kind, dtype)
        full = gu.fold_oracle(rows, w, dtype)
        acc, prev = None, 0
        for p in sizes:
            if kind == "uniform" and p > B * T + 1:
                continue
            seg = gu.dist_oracle(rows[:, prev:p], full[prev:p], dtype)
            acc = seg if acc is None else acc + seg
            prev = p
            xs = [x[:p] for x in xd]
            what = f"{dtype} n={n} P={p} {kind}"
            out, d2, _ = _run(xs, w, dtype)
            assert eu.same_bits(out, full[:p], dtype), f"{what}: out differs from the FedAvg oracle: " + \
                eu.diff_report(out, full[:p], dtype)
            assert np.array_equal(eu.bits_of(out, dtype), eu.bits_of(_wreduce(xs, w, dtype), dtype)), \
                f"{what}: out differs from dlsim_wreduce on the same buffers"
            _assert_vector(d2, acc, p, what)
            out2, again, _ = _run(xs, w, dtype)
            assert _same(d2, again) and np.array_equal(eu.bits_of(out, dtype), eu.bits_of(out2, dtype)), \
                f"{what}: a second call gave other bits"
    assert eu.inputs_unchanged(xd, rows, dtype)


# ---- special values ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("n", (3, 8, 20))
def test_specials_at_the_edge_positions(n, dtype):
    """Specials at _edge_util.edge_positions (first and last vector of the full
    tiles, a wave's middle, the partial tile, the scalar tail), held by the
    first, a middle and the last row."""
    T, _ = _geometry(n, dtype)
    E = T // 256
    p = 2 * T + T // 2 + E + max(E - 1, 1)
    pos = eu.edge_positions(p, T, E)
    assert len(pos) == (5 if E > 1 else 4)
    base = eu.decode(eu.random_rows(dtype, n, p, seed=131 + n), dtype)
    r0, r1, r2 = 0, n // 2, n - 1
    wd = _weights(n, "dirichlet", dtype)

    def run(x, what, w=wd, alias=None):
        rows = eu.encode(x, dtype).reshape(len(x), p)
        xd = eu.place(list(rows), dtype, DEV)
        if alias is not None:
            xd[alias[1]] = xd[alias[0]]
        out, d2, _ = _run(xd, w, dtype)
        want_out = gu.fold_oracle(rows, w, dtype)
        assert eu.same_bits(out, want_out, dtype), f"{dtype} n={n} {what}: " + eu.diff_report(out, want_out, dtype)
        _assert_vector(d2, gu.dist_oracle(rows, want_out, dtype), p, f"{dtype} n={n} {what}")
        assert eu.inputs_unchanged(xd, rows, dtype)
        return out, d2

    for r in (r0, r1, r2):
        x = base.copy()
        x[r, pos] = np.nan
        _, d2 = run(x, f"NaN in row {r}")
        assert np.isnan(d2).all()  # the output is NaN there: every term against it is
        x = base.copy()
        for v in (np.inf, -np.inf):
            x[r, pos] = v
            _, d2 = run(x, f"{v} in row {r}")
            if r == 0:  # the fold starts from x_0 * 0 = NaN
                assert np.isnan(d2).all()
            else:  # Inf - Inf in row r, finite - Inf elsewhere
                assert np.isnan(d2[r]) and (np.delete(d2, r) == np.inf).all()
    x = base.copy()
    x[r0, pos[0]], x[r2, pos[0]] = np.inf, -np.inf
    _, d2 = run(x, "+Inf against -Inf at one element")
    assert np.isnan(d2).all()
    # -0 and +0: every distance is +0.0, the output keeps the fold's zero signs
    x = np.zeros((n, p))
    x[r1, pos] = -0.0
    x[r2] = -0.0
    _, d2 = run(x, "-0 and +0")
    assert not d2.view(np.uint64).any()
    # subnormals of the dtype (an fp64 subnormal's square underflows; the contract keeps fp64 inputs above 1e-150)
    if dtype != "f64":
        tiny = eu._TINY[dtype]
        x = np.zeros((n, p))
        x[r1, pos] = tiny
        x[r2, pos[:2]] = -tiny
        run(x, "subnormals")
    # a sum that overflows to Inf from finite inputs: weight 1.0 on two rows that hold the format's large value
    big = eu._OVERFLOW[dtype][0]
    x = base.copy()
    x[r0, pos] = x[r2, pos] = big
    w1 = np.zeros(n)
    w1[r0] = w1[r2] = 1.0
    out, d2 = run(x, "overflow to Inf from finite inputs", w=w1)
    assert np.isinf(eu.decode(out, dtype)[pos]).all() and (d2 == np.inf).all()
    # two identical rows under uniform weights: the output is the row, both distances exactly +0.0;
    # then one pointer passed twice: the same bits
    ints = np.random.default_rng(n).integers(-8, 9, size=(2, p)).astype(np.float64)
    ints[1] = ints[0]
    out, d2 = run(ints, "two identical rows", w=[0.5, 0.5])
    assert not d2.view(np.uint64).any() and np.array_equal(eu.decode(out, dtype), ints[0])
    out2, twice = run(ints, "the same pointer twice", w=[0.5, 0.5], alias=(0, 1))
    assert _same(d2, twice) and np.array_equal(eu.bits_of(out, dtype), eu.bits_of(out2, dtype))


# ---- null output, accumulate, sizes 0 and n = 1 ----------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("n", (1, 5, 9, 17))
def test_null_output_gives_the_same_distances(n, dtype):
    T, _ = _geometry(n, dtype)
    p = 3 * T + T // 2 + 3
    rows = eu.random_rows(dtype, n, p, seed=900 + n)
    xd = eu.place(list(rows), dtype, DEV)
    w = _weights(n, "dirichlet", dtype)
    _, d2, _ = _run(xd, w, dtype)
    _, alone, _ = _run(xd, w, dtype, with_out=False)
    assert _same(d2, alone)
    assert eu.inputs_unchanged(xd, rows, dtype)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("n", (8, 32))
def test_accumulate_over_two_halves(n, dtype):
    """Two calls over [0, h) and [h, p), the second accumulating. Random rows:
    within the bound of one call over p elements (the halves are within their
    own bounds, the final addition rounds once more, all terms non-negative).
    Small integers under weights 1/n (n a power of two: every product, sum,
    difference and square is exact): the distances equal the oracle's exactly."""
    T, _ = _geometry(n, dtype)
    E = T // 256
    p = 5 * T + 3
    rows = eu.random_rows(dtype, n, p, seed=177 + n)
    ints = eu.encode(np.random.default_rng(n).integers(-4, 5, size=(n, p)).astype(np.float64), dtype).reshape(n, p)
    w = [1.0 / n] * n
    for h in (3 * T + 2 * E, 2 * T + 1):  # the second half on the vector path, then off alignment
        for what, r in (("random", rows), ("small integers", ints)):
            xd = eu.place(list(r), dtype, DEV)
            full = gu.fold_oracle(r, w, dtype)
            out1, first, g = _run([x[:h] for x in xd], w, dtype)
            _assert_vector(first, gu.dist_oracle(r[:, :h], full[:h], dtype), h, f"{dtype} n={n} first half")
            out2, got, _ = _run([x[h:] for x in xd], w, dtype, accumulate=True, into=g)
            assert eu.same_bits(np.concatenate([out1, out2]), full, dtype)
            want = gu.dist_oracle(r[:, :h], full[:h], dtype) + gu.dist_oracle(r[:, h:], full[h:], dtype)
            _assert_vector(got, want, p, f"{dtype} n={n} {what} split at {h}")
            if what == "small integers":
                assert np.array_equal(got, want.astype(np.float64)), "integer distances are exact"
            assert eu.inputs_unchanged(xd, r, dtype)


def test_zero_elements_and_one_input():
    x = torch.ones(16, device=DEV)
    for n in (1, 3):
        _, got, g = _run([x[:0]] * n, [0.5] * n, "f32")  # zeros
        assert not got.view(np.uint64).any()
        g.view.fill_(2.5)
        _native.wreduce_dist([x[:0]] * n, [0.5] * n, None, g.view, accumulate=True)  # untouched
        torch.cuda.synchronize()
        assert bool((g.view == 2.5).all()) and eu.check_guards(g) == []
    for dtype in ALL:
        # n = 1 with weight 1.0: the row bit for bit (zeros of both signs and subnormals too), d2 = +0.0
        T, _ = _geometry(1, dtype)
        rows = eu.random_rows(dtype, 1, T + 5, seed=5)
        v = eu.decode(rows, dtype)
        v[0, :4] = [0.0, -0.0, eu._TINY[dtype], -eu._TINY[dtype]]
        rows = eu.encode(v, dtype).reshape(1, -1)
        xd = eu.place(list(rows), dtype, DEV)
        out, d2, g = _run(xd, [1.0], dtype)
        assert np.array_equal(eu.bits_of(out, dtype), eu.bits_of(rows[0], dtype)) and d2.view(np.uint64)[0] == 0
        _, d2, _ = _run(xd, [1.0], dtype, accumulate=True, into=g)
        assert d2.view(np.uint64)[0] == 0
        for bad in (np.nan, np.inf, -np.inf):  # any other row: a non-finite d2
            v2 = v.copy()
            v2[0, T + 2] = bad
            _, d2, _ = _run(eu.place(list(eu.encode(v2, dtype).reshape(1, -1)), dtype, DEV), [1.0], dtype, with_out=False)
            assert not np.isfinite(d2[0])


# ---- alignment -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,offset", [("f32", 4), ("f32", 8), ("bf16", 2), ("bf16", 4), ("f16", 2), ("f16", 8),
                                          ("f64", 8)])
@pytest.mark.parametrize("n", (5, 9, 17))
def test_misaligned_buffers_take_the_scalar_form(n, dtype, offset):
    """One base off a 16-byte boundary (an input, or the output alone) sends
    the call to the scalar form: tiles of 256 elements under the same grid cap."""
    _, B = _geometry(n, dtype)
    sizes = (1, 255, 257, 2 * B * 256 + 256 + 3)
    rows = eu.random_rows(dtype, n, sizes[-1], seed=1500 + n)
    w = _weights(n, "dirichlet", dtype)
    full = gu.fold_oracle(rows, w, dtype)
    for offs, out_off in (([offset] * n, 0), ([0] * (n - 1) + [offset], 0), ([0] * n, offset)):
        xd = eu.place(list(rows), dtype, DEV, offs)
        assert out_off or any(x.data_ptr() % 16 for x in xd)
        for p in sizes:
            out, d2, _ = _run([x[:p] for x in xd], w, dtype, out_offset=out_off)
            assert eu.same_bits(out, full[:p], dtype)
            _assert_vector(d2, gu.dist_oracle(rows[:, :p], full[:p], dtype), p,
                           f"{dtype} n={n} P={p} offsets {offs[0]}, {offs[-1]}, out {out_off}")
        _, again, _ = _run(xd, w, dtype, out_offset=out_off)
        assert _same(d2, again)
        assert eu.inputs_unchanged(xd, rows, dtype)


def test_overlaps_are_refused_and_nothing_runs():
    buf = torch.ones(1000, dtype=torch.float64, device=DEV)
    xs = [buf[:300], buf[300:600]]
    out, d2 = buf[600:900], buf[900:902]
    torch.cuda.synchronize()
    for bad_d2 in (buf[0:2], buf[298:300], buf[598:600], buf[600:602], buf[899:901]):
        with pytest.raises(_native.DlsimError) as e:
            _native.wreduce_dist(xs, [0.5, 0.5], out, bad_d2)
        assert e.value.rc == _native.DLSIM_E_ARG and "overlaps" in str(e.value)
    for bad_out in (buf[0:300], buf[300:600], buf[1:301], buf[599:899]):
        with pytest.raises(_native.DlsimError) as e:
            _native.wreduce_dist(xs, [0.5, 0.5], bad_out, d2)
        assert e.value.rc == _native.DLSIM_E_ARG and "overlaps" in str(e.value)
    with pytest.raises(_native.DlsimError, match="not representable"):
        _native.wreduce_dist([x.float() for x in xs], [0.1, 0.5], None, d2)
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all())


# ---- the tensors entry -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", (8, 17))
def test_tensors_entry_equals_flat_calls_on_the_gnlenet_shapes(n, dtype):
    numels = [int(np.prod(s)) for s in GNLENET_SHAPES]
    assert len(numels) == 14 and sum(numels) == 85_354
    rows = eu.random_rows(dtype, n, sum(numels), seed=211 + n)
    offs = np.concatenate([[0], np.cumsum(numels)])
    tensors = [eu.place([r[offs[k]:offs[k + 1]] for k in range(14)], dtype, DEV) for r in rows]
    stream = torch.cuda.current_stream().cuda_stream
    code = _native.dtype_code(eu.DTYPES[dtype], single_task=True)
    w = [float(v) for v in _weights(n, "dirichlet", dtype)]
    for start in (False, True):  # the caller's accumulate goes to the first tensor only
        flat_d2, one_d2 = eu.guarded(n * 8, "f64", DEV), eu.guarded(n * 8, "f64", DEV)
        flat_out, one_out = eu.guarded_many(numels, dtype, DEV), eu.guarded_many(numels, dtype, DEV)
        if start:
            for g in (flat_d2, one_d2):
                _native.wreduce_dist([t[13] for t in tensors], w, None, g.view)
        for k in range(14):
            _native.wreduce_dist([t[k] for t in tensors], w, flat_out.views[k], flat_d2.view, accumulate=start or k > 0)
        base = one_out.views[0].data_ptr()
        _native.wreduce_dist_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels,
                                         [v.data_ptr() - base for v in one_out.views], w, base, code,
                                         one_d2.view.data_ptr(), start, stream)
        torch.cuda.synchronize()
        for g in (flat_d2, one_d2, flat_out, one_out):
            assert eu.check_guards(g) == []
        assert eu.unwritten(one_d2) == 0
        assert _same(flat_d2.view.cpu().numpy(), one_d2.view.cpu().numpy())
        got = np.concatenate([eu.from_torch(v, dtype) for v in one_out.views])
        assert np.array_equal(eu.bits_of(got, dtype),
                              eu.bits_of(np.concatenate([eu.from_torch(v, dtype) for v in flat_out.views]), dtype))
        if not start:
            want_out = gu.fold_oracle(rows, np.asarray(w), dtype)
            assert eu.same_bits(got, want_out, dtype)
            # 14 partial sums of non-negative terms added in order: each within (p_k + 8) u, one more
            # rounding per addition, and p - max p_k >= 13: the bound of one call over p elements holds
            plain = one_d2.view.cpu().numpy().copy()
            _assert_vector(plain, gu.dist_oracle(rows, want_out, dtype), sum(numels), f"{dtype} n={n} tensors")
    # distances only, and no tensor at all: zeros, or nothing when accumulating
    none = eu.guarded(n * 8, "f64", DEV)
    _native.wreduce_dist_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels, [0] * 14, w, None, code,
                                     none.view.data_ptr(), False, stream)
    torch.cuda.synchronize()
    assert eu.check_guards(none) == [] and _same(none.view.cpu().numpy(), plain)
    one_d2.view.fill_(3.0)
    _native.wreduce_dist_tensors_raw([], n, [], [], w, None, code, one_d2.view.data_ptr(), True, stream)
    torch.cuda.synchronize()
    assert bool((one_d2.view == 3.0).all())
    _native.wreduce_dist_tensors_raw([], n, [], [], w, None, code, one_d2.view.data_ptr(), False, stream)
    torch.cuda.synchronize()
    assert not one_d2.view.cpu().numpy().view(np.uint64).any()


# ---- buffers past one launch's offsets -----------------------------------------------------------
def test_input_past_two_gib_runs_as_pieces():
    """fp32, n = 2, weights 1/2: the first piece is (2^31 - 2^20) / 4 elements,
    the rest accumulates. The rows differ by 1 at a few elements of either
    piece: the output is 1/2 there and each distance count / 4, exactly."""
    first = ((1 << 31) - (1 << 20)) // 4
    p = first + 4099
    a = torch.zeros(p, device=DEV)
    b = torch.zeros(p, device=DEV)
    out = torch.full((p,), 7.0, device=DEV)
    hot = [0, 1023, first - 1, first, first + 1, first + 4096, p - 1]
    b[hot] = 1.0
    a[5] = b[5] = float(2 ** 20)  # equal elements add nothing
    d2 = eu.guarded(16, "f64", DEV)
    _native.wreduce_dist([a, b], [0.5, 0.5], out, d2.view)
    torch.cuda.synchronize()
    assert eu.check_guards(d2) == []
    assert d2.view.tolist() == [len(hot) / 4, len(hot) / 4]
    assert out[hot].tolist() == [0.5] * len(hot) and out[5].item() == 2 ** 20
    assert float(out.sum().item()) == 2 ** 20 + len(hot) / 2  # every other element was written, with 0


# ---- aggregate_with_distances -------------------------------------------------------------------
class Mixed(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(33, 7))
        self.b = nn.Parameter(torch.zeros(129, dtype=torch.bfloat16))
        self.c = nn.Parameter(torch.zeros(5))
        self.d = nn.Parameter(torch.zeros(4, 9, dtype=torch.bfloat16))


PLACES = {"host": lambda m: m, "arena": lambda m: arena.to_device_arena(m, DEV),
          "tensors": lambda m: copy.deepcopy(m).to(DEV)}


def _flat(model):
    return np.concatenate([p.detach().cpu().reshape(-1).numpy() for p in model.parameters()])


@pytest.mark.parametrize("place", sorted(PLACES))
def test_aggregate_with_distances_on_every_route(place):
    n = 9
    rows, _, _, cpu = ku.plugin_case(n, 2)
    alphas = gu.dirichlet(n, 3)
    w = np.asarray(alphas).astype(np.float32)
    models = [PLACES[place](m) for m in cpu]
    before = [ku.flat_bits(m) for m in models]
    out, d2 = geomed.aggregate_with_distances(models, alphas)
    assert type(out) is type(models[0]) and d2.shape == (n,) and d2.dtype == torch.float64 and not d2.is_cuda
    assert all(g.device == p0.device for g, p0 in zip(out.parameters(), models[0].parameters()))
    want_out = gu.fold_oracle(rows, w, "f32")
    assert orc.same_bits(_flat(out), want_out)
    assert np.array_equal(ku.flat_bits(out), ku.flat_bits(FedAvg.aggregate(models, alphas)))
    # (the tensors route adds four partial sums in order: still within the bound of one call, as in
    # test_tensors_entry_equals_flat_calls_on_the_gnlenet_shapes)
    _assert_vector(d2.numpy(), gu.dist_oracle(rows, want_out, "f32"), rows.shape[1], f"aggregate_with_distances {place}")
    if place != "tensors":  # one aligned row per model: the flat entry's bits
        _, flat, _ = _run(eu.place(list(rows), "f32", DEV), w, "f32")
        assert _same(d2.numpy(), flat)
    mean, d2u = geomed.consensus_distance(models)
    assert np.array_equal(ku.flat_bits(mean), ku.flat_bits(FedAvg.aggregate(models, None)))
    wu = orc.reference_weights(n, None)
    _assert_vector(d2u.numpy(), gu.dist_oracle(rows, gu.fold_oracle(rows, wu, "f32"), "f32"), rows.shape[1],
                   f"consensus_distance {place}")
    dev_out, _ = geomed.aggregate_with_distances(models, alphas, to_host=(place != "host"))
    assert all(p.is_cuda == (place == "host") for p in dev_out.parameters())
    assert orc.same_bits(_flat(dev_out), want_out)
    for m_, saved in zip(models, before):
        assert np.array_equal(ku.flat_bits(m_), saved), "an input model changed"


@pytest.mark.parametrize("place", sorted(PLACES))
def test_aggregate_with_distances_adds_dtype_groups_in_layout_order(place):
    n = 6
    rng = np.random.default_rng(19)
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
    alphas = gu.dirichlet(n, 4)
    w = np.asarray(alphas).astype(np.float32)
    out, d2 = geomed.aggregate_with_distances([PLACES[place](m) for m in cpu], alphas)
    o32, o16 = gu.fold_oracle(f32, w, "f32"), gu.fold_oracle(b16, w, "bf16")
    got32 = np.concatenate([out.a.detach().cpu().reshape(-1).numpy(), out.c.detach().cpu().numpy()])
    got16 = np.concatenate([eu.from_torch(out.b, "bf16"), eu.from_torch(out.d.reshape(-1), "bf16")])
    assert orc.same_bits(got32, o32) and eu.same_bits(got16, o16, "bf16")
    want = gu.dist_oracle(f32, o32, "f32") + gu.dist_oracle(b16, o16, "bf16")
    _assert_vector(d2.numpy(), want, 236 + 165, f"mixed {place}")
    if place != "tensors":  # the fp32 group first, the bf16 group accumulated onto it
        _, _, g = _run(eu.place(list(f32), "f32", DEV), w, "f32")
        _, manual, _ = _run(eu.place(list(b16), "bf16", DEV), w, "bf16", accumulate=True, into=g)
        assert _same(d2.numpy(), manual)
    with pytest.raises(ValueError):
        geomed.aggregate_with_distances([cpu[0], nn.Linear(3, 2), cpu[1]], [0.2, 0.3, 0.5])


# ---- the plugins -----------------------------------------------------------------------------------
def _bn():
    m = BnNet()
    with torch.no_grad():
        m.bn.running_mean.uniform_(-1, 1)
        m.bn.num_batches_tracked.fill_(int(torch.randint(1, 99, ()).item()))
    return m


def _plugin(case, iters=None):
    if case["rule"] == "gm":
        return GeometricMedian.with_params(gu.GM_ITERS if iters is None else iters, gu.GM_NU)
    return CenteredClip.with_params(case["tau"], gu.CLIP_ITERS if iters is None else iters)


def _case_models(case, rows, place):
    torch.manual_seed(3)
    if case["shapes"] is gu.BN_SHAPES:
        return [PLACES[place](ku.model_of(r, None, "f32", make=_bn)) for r in rows]
    return [PLACES[place](ku.model_of(r, case["shapes"], "f32")) for r in rows]


@pytest.mark.parametrize("place", ["host", "arena"])
@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_trajectories_equal_the_restated_ones(name, place):
    """tests/test_geomed_cpu.py asserts the separation of every case: the
    kernel's d2, within the bound of the oracle's, must then give the oracle's
    fp32 weights in every pass and its final parameters bit for bit."""
    case = gu.CASES[name]
    rows, byz, alphas, want, passes = gu.case_trajectory(case)
    numel = rows.shape[1]
    models = _case_models(case, rows, place)
    before = [ku.flat_bits(m) for m in models]
    agg = _plugin(case)
    out, trace = agg.aggregate(models, alphas, trace=True)
    assert type(out) is type(models[0]) and len(trace) == len(passes)
    for t, (got, exp) in enumerate(zip(trace, passes)):
        assert got["kept"] == exp["kept"], f"pass {t}: kept set"
        assert np.array_equal(np.asarray(got["weights"], dtype=np.float64), exp["weights"].astype(np.float64)), \
            f"pass {t}: fp32 weights differ from the oracle's"
        _assert_vector(got["d2"], exp["d2"], numel, f"{name} {place} pass {t}")
    assert orc.same_bits(_flat(out), want), f"{name}: final parameters differ from the restated trajectory"
    assert np.isfinite(_flat(out)).all()
    for g, p0 in zip(out.parameters(), models[0].parameters()):
        assert g.device == p0.device and g.shape == p0.shape and g.requires_grad == p0.requires_grad
    again = agg.aggregate(models, alphas)
    assert np.array_equal(ku.flat_bits(again), ku.flat_bits(out))
    flipped = agg.aggregate(models, alphas, to_host=(place != "host"))
    assert all(p.is_cuda == (place == "host") for p in flipped.parameters())
    assert orc.same_bits(_flat(flipped), want)
    avg = FedAvg.aggregate(models, alphas)
    zero = _plugin(case, iters=0).aggregate(models, alphas)
    if case["special"]:
        # one all-NaN and one all-Inf peer: FedAvg's result is not finite, the rule's is
        assert not np.isfinite(_flat(avg)).any()
        kept = passes[0]["kept"]
        a = [1.0 / case["n"]] * case["n"] if alphas is None else alphas
        assert np.array_equal(ku.flat_bits(zero), ku.flat_bits(
            FedAvg.aggregate([models[i] for i in kept], [a[i] / gu.seq_sum(a[j] for j in kept) for i in kept])))
    else:
        assert np.array_equal(ku.flat_bits(zero), ku.flat_bits(avg)), "zero iterations equal FedAvg bit for bit"
    if case["shapes"] is gu.BN_SHAPES:  # model 0 is excluded; its buffers are still the result's
        assert isinstance(out, BnNet) and 0 not in passes[0]["kept"]
        bufs, bufs0 = list(out.buffers()), list(models[0].buffers())
        assert len(bufs) == len(bufs0) == 3
        for b, b0 in zip(bufs, bufs0):
            assert b.device == b0.device and torch.equal(b, b0) and b.data_ptr() != b0.data_ptr()
        assert not torch.equal(out.bn.running_mean, models[passes[0]["kept"][0]].bn.running_mean)
        if place == "host":  # (to_device_arena moves parameters only: models[0]'s buffers stay on the host)
            y = out.bn(out.fc(torch.ones(4, 7)))  # working submodules
            assert y.shape == (4, 5)
    for m_, saved in zip(models, before):
        assert np.array_equal(ku.flat_bits(m_), saved), "an input model changed"


@pytest.mark.parametrize("name", ["gm-8", "gm-17", "gm-32"])
def test_the_geometric_median_is_closer_to_the_honest_mean_than_fedavg(name):
    """The oracle first (tests/test_geomed_cpu.py), then the kernel's result:
    a strict inequality on well-separated inputs, no tuned margin."""
    case = gu.CASES[name]
    rows, byz, alphas, want, passes = gu.case_trajectory(case)
    honest = np.delete(eu.decode(rows, "f32"), byz, axis=0).mean(axis=0)
    models = _case_models(case, rows, "arena")
    gm = _flat(_plugin(case).aggregate(models, alphas)).astype(np.float64)
    avg = _flat(FedAvg.aggregate(models, alphas)).astype(np.float64)
    assert np.linalg.norm(eu.decode(want, "f32") - honest) < np.linalg.norm(avg - honest)
    assert np.linalg.norm(gm - honest) < np.linalg.norm(avg - honest)


@pytest.mark.parametrize("agg", [GeometricMedian, CenteredClip])
def test_an_all_non_finite_list_returns_fedavgs_result(agg):
    rows = np.full((5, gu.NUMEL), np.nan, dtype=np.float32)
    rows[1] = np.inf
    rows[3, ::2] = -np.inf
    rows[4, 1:] = 1.0  # one NaN is enough
    cpu = [ku.model_of(r, ku.PLUGIN_SHAPES, "f32") for r in rows]
    out, trace = agg.aggregate(cpu, None, trace=True)
    assert len(trace) == 1 and trace[0]["kept"] == list(range(5))
    assert orc.same_bits(_flat(out), _flat(FedAvg.aggregate(cpu, None)))
    assert not np.isfinite(_flat(out)).any()


@pytest.mark.parametrize("method,name", [(6, "gm-8"), (7, "clip-8"), (7, "clip-8-tau")])
def test_functions_aggregate_through_model_manager(method, name):
    case = gu.CASES[name]
    rows, byz, alphas, want, passes = gu.case_trajectory(case)
    cpu = _case_models(case, rows, "host")
    settings = types.SimpleNamespace(gradient_aggregation=method)
    if case["tau"] is not None:
        settings.aggregation_clip_tau = case["tau"]
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0})
    assert isinstance(res, list) and len(res) == 1
    assert not any(p.is_cuda for p in res[0].parameters())
    assert orc.same_bits(_flat(res[0]), want)
    settings.aggregate_on_device = True
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": None})
    assert all(p.is_cuda for p in res[0].parameters())
    assert orc.same_bits(_flat(res[0]), want)
