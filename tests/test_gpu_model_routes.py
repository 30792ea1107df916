"""The layer between a list of nn.Modules and the kernels of the aggregates
over n <= 32 models (dasklearn_amd/model_inputs.py: ModelInputs, robust_modules,
model_distances, krum_modules, ReduceDistPlan) on the MI355X, on every route a
list of models can take (tests/_route_util.py), and the *_tensors entries of the
two distance families at their edges.

The references are those of the kernels' own tests: _robust_util.window_mean,
_krum_util's longdouble matrix and restated selection, _geomed_util's FedAvg
fold, distance oracle and restated trajectories. A route changes no value, so
the oracle of a case is the same on all of them.

Bounds. A distance is within (P + 8) * 2^-53 of the oracle over P elements
(_krum_util.bound). Where a route sums a model in t pieces (the tensors routes:
one launch per tensor accumulating into the result; two dtype groups: one
launch per group) every piece k is within (p_k + 8) u of its own exact value
and each of the t - 1 later additions rounds once more; all terms are
non-negative, so the total is within (max p_k + 8 + t - 1) u of the exact
whole, and with P - max p_k >= t - 1 that is at most (P + 8) u: the bound of
one call over P elements. It holds for every shape here: the smallest margin
is BnNet's (35, 5, 5, 5: P - max = 15 >= 3).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _edge_util as eu
import _geomed_util as gu
import _krum_util as ku
import _robust_util as ru
import _route_util as rt
from _sgd_util import BnNet
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402
from dasklearn_amd.gradient_aggregation import geomed  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Krum, MultiKrum, krum_select, model_distances  # noqa: E402
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian, TrimmedMean  # noqa: E402

DEV = "cuda"
ROUTES = rt.routes(DEV)
HUGE = 10 ** 10


def _same64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _everywhere(call, models, route, want, what):
    """call(to_host) under the default and both overrides: each result has
    models[0]'s form (rt.result_problems) and the expected bits. Returns the
    default's result."""
    first = None
    for to_host in (None, True, False):
        out = call(to_host)
        problems = rt.result_problems(out, models, route, to_host)
        assert not problems, f"{what} to_host={to_host}: {problems}"
        assert rt.same_params(out, want), f"{what} to_host={to_host}: the parameters differ from the oracle's"
        first = out if first is None else first
    return first


def _unchanged(models, before):
    for i, (m, saved) in enumerate(zip(models, before)):
        assert np.array_equal(ku.flat_bits(m), saved), f"input model {i} changed"


# ---- the order statistics ----------------------------------------------------------------
ROBUST_CASES = [("mixed", 5), ("mixed", 17), ("gnlenet", 5), ("gnlenet", 17), ("bn", 5)]


def _windows(n):
    aggs = {"median": CoordinateMedian, "trim1": TrimmedMean.with_trim(1), "trim0": TrimmedMean.with_trim(0)}
    return tuple((aggs[name], w) for name, w in rt.robust_windows(n))


@pytest.mark.parametrize("route", rt.NAMES)
@pytest.mark.parametrize("maker,n", ROBUST_CASES)
def test_order_statistics_on_every_route(maker, n, route):
    cpu, want = rt.robust_case(maker, n)
    models = ROUTES[route](cpu)
    before = [ku.flat_bits(m) for m in models]
    for agg, window in _windows(n):
        _everywhere(lambda to_host: agg.aggregate(models, to_host=to_host), models, route, want[window],
                    f"{agg.__name__} {maker} n={n} {route}")
    _unchanged(models, before)


# ---- the distance matrix --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat_matrix(n, f):
    """The flat entry's matrix over the case's rows, each a 128-byte aligned tensor of its own."""
    rows = ku.plugin_case(n, f)[0]
    d2 = torch.empty(n * n, dtype=torch.float64, device=DEV)
    _native.pairwise_sqdist(eu.place(list(rows), "f32", DEV), d2)
    return d2.cpu().numpy().reshape(n, n)


@pytest.mark.parametrize("route", rt.NAMES)
def test_model_distances_on_every_route(route):
    n = 9
    rows, _, want, cpu = ku.plugin_case(n, 2)
    models = ROUTES[route](cpu)
    before = [ku.flat_bits(m) for m in models]
    got = model_distances(models)
    assert got.shape == (n, n) and got.dtype == torch.float64 and not got.is_cuda
    problems, worst = ku.matrix_problems(got.numpy(), want, rows.shape[1])  # symmetry and the +0.0 diagonal too
    print(f"model_distances {route}: max err / bound {worst:.4f}")
    assert not problems, problems
    if route in rt.ONE_ROW_PER_MODEL:
        assert _same64(got.numpy(), _flat_matrix(n, 2)), "one aligned row per model: the flat entry's bits"
    _unchanged(models, before)


# ---- Krum and Multi-Krum ----------------------------------------------------------------------
@pytest.mark.parametrize("route", rt.NAMES)
@pytest.mark.parametrize("n,f,bn", [(5, 1, False), (17, 3, False), (8, 2, True)])
def test_krum_on_every_route(n, f, bn, route):
    rows, byz, want, cpu = rt.krum_case(n, f, bn)
    models = ROUTES[route](cpu)
    before = [ku.flat_bits(m) for m in models]
    want64 = want.astype(np.float64)
    d2 = model_distances(models).tolist()
    for m in (1, 2, n - f):
        assert krum_select(d2, f, m) == ku.ref_select(want64, f, m), f"selection of {m}"
    best = ku.ref_select(want64, f, 1)[0]
    if bn:
        assert best != 0  # models[0] is Byzantine: its buffers and layout are still the result's
    out = _everywhere(lambda to_host: Krum.with_params(f).aggregate(models, to_host=to_host), models, route,
                      rt.split_bits(rows[best], cpu[0]), f"Krum n={n} {route}")
    for g, pb in zip(out.parameters(), models[best].parameters()):
        assert g.data_ptr() != pb.data_ptr(), "Krum's result shares memory with the selected model"
    for m in (None, 2):
        chosen = ku.ref_select(want64, f, n - f if m is None else m)
        expect = orc.wreduce([rows[i] for i in chosen], orc.reference_weights(len(chosen), None), "f32")
        _everywhere(lambda to_host: MultiKrum.with_params(f, m).aggregate(models, to_host=to_host), models, route,
                    rt.split_bits(expect, cpu[0]), f"Multi-Krum m={m} n={n} {route}")
    _unchanged(models, before)


# ---- the geometric median and centered clipping ---------------------------------------------------
TRAJECTORY_CASES = ("gm-8-weighted", "gm-17", "gm-8-nan-inf", "clip-8-tau", "clip-17", "clip-8-nan-inf", "clip-8-bn")


def _plugin(case):
    if case["rule"] == "gm":
        return GeometricMedian.with_params(gu.GM_ITERS, gu.GM_NU)
    return CenteredClip.with_params(case["tau"], gu.CLIP_ITERS)


def _assert_trace(trace, passes, numel, what):
    """Pass by pass: the kept set, the fp32 weights handed to the kernel (the
    CPU suite asserts the separation of every case, so a d2 within the bound
    must give the oracle's weights) and d2 within the bound."""
    assert len(trace) == len(passes)
    for t, (got, exp) in enumerate(zip(trace, passes)):
        assert got["kept"] == exp["kept"], f"{what} pass {t}: kept set"
        assert np.array_equal(np.asarray(got["weights"], dtype=np.float64), exp["weights"].astype(np.float64)), \
            f"{what} pass {t}: fp32 weights differ from the oracle's"
        problems, worst = gu.vector_problems(got["d2"], exp["d2"], numel)
        print(f"{what} pass {t}: max err / bound {worst:.4f}")
        assert not problems, f"{what} pass {t}: {problems}"


@pytest.mark.parametrize("route", rt.NAMES)
@pytest.mark.parametrize("name", TRAJECTORY_CASES)
def test_trajectories_on_every_route(name, route):
    case, rows, byz, alphas, want, passes, cpu = rt.trajectory_case(name)
    pins = {}
    if name.endswith("-nan-inf") and route in rt.MIXED_PLACEMENT:
        pins = dict(host=(byz[0],), device=(byz[-1],))  # the all-NaN peer arrives on the host, the all-Inf one on the device
    models = ROUTES[route](cpu, **pins)
    if pins:
        assert not any(p.is_cuda for p in models[byz[0]].parameters()) and all(p.is_cuda for p in models[byz[-1]].parameters())
    before = [ku.flat_bits(m) for m in models]
    agg = _plugin(case)
    out, trace = agg.aggregate(models, alphas, trace=True)
    _assert_trace(trace, passes, rows.shape[1], f"{name} {route}")
    _everywhere(lambda to_host: agg.aggregate(models, alphas, to_host=to_host), models, route, rt.split_bits(want, cpu[0]),
                f"{name} {route}")
    assert rt.same_params(out, rt.split_bits(want, cpu[0]))
    if case["shapes"] is gu.BN_SHAPES:
        assert 0 not in passes[0]["kept"] and isinstance(out, BnNet)
    _unchanged(models, before)


# ---- two dtype groups through the whole iteration ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_case(name):
    case = gu.MIXED_CASES[name]
    groups, byz, outs, passes = gu.mixed_case_trajectory(case)
    return case, groups, outs, passes, rt.mixed_models(groups[0][0], groups[1][0])


@pytest.mark.parametrize("route", ["host", "arena", "tensors", "arena0_host_peers"])
@pytest.mark.parametrize("name", sorted(gu.MIXED_CASES))
def test_two_dtype_groups_through_the_whole_iteration(name, route):
    """The centre is one arena per dtype and d2 accumulates across the groups
    in layout order (fp32, then bf16) in every pass. Two partial sums (four on
    the tensors route: 231, 5, 129, 36 elements) added in order keep the bound
    of one call over all 401 elements (module docstring: 401 - 231 >= 3)."""
    case, groups, outs, passes, cpu = _mixed_case(name)
    models = ROUTES[route](cpu)
    before = [ku.flat_bits(m) for m in models]
    agg = _plugin(case)
    out, trace = agg.aggregate(models, None, trace=True)
    _assert_trace(trace, passes, gu.MIXED_NUMEL, f"{name} {route}")
    o32, o16 = eu.bits_of(outs[0], "f32"), eu.bits_of(outs[1], "bf16")
    want = [o32[:231], o16[:129], o32[231:], o16[129:]]  # parameters() order: a, b, c, d
    _everywhere(lambda to_host: agg.aggregate(models, None, to_host=to_host), models, route, want, f"{name} {route}")
    assert rt.same_params(out, want)
    _unchanged(models, before)


# ---- zero-element parameters and empty groups -----------------------------------------------------------
ZERO_N, ZERO_F, ZERO_NUMEL = 5, 1, 26


@functools.lru_cache(maxsize=None)
def _zero_case():
    rows, byz, want = ku.separated_models(ZERO_N, ZERO_F, ZERO_NUMEL, "f32", seed=9100, ms=(1,))
    return rows, want, [ku.model_of(r, None, "f32", make=rt.ZeroNet) for r in rows]


def _zero_bits(row):
    b = eu.bits_of(np.asarray(row), "f32")
    return [b[:21], b[:0], b[21:], np.zeros(0, dtype=np.uint16)]


@pytest.mark.parametrize("route", rt.BASELINE)
def test_an_empty_tensor_and_an_empty_group(route):
    rows, want, cpu = _zero_case()
    models = ROUTES[route](cpu)
    before = [ku.flat_bits(m) for m in models]
    tensors = [torch.from_numpy(np.ascontiguousarray(r)) for r in rows]
    for agg, (lo, hi) in _windows(ZERO_N):
        expect = ru.bits_of(ru.window_mean(tensors, lo, hi))
        _everywhere(lambda to_host: agg.aggregate(models, to_host=to_host), models, route, _zero_bits(expect.view(np.float32)),
                    f"{agg.__name__} {route}")
    got = model_distances(models).numpy()
    problems, _ = ku.matrix_problems(got, want, ZERO_NUMEL)
    assert not problems, problems
    best = ku.ref_select(want.astype(np.float64), ZERO_F, 1)[0]
    _everywhere(lambda to_host: Krum.with_params(ZERO_F).aggregate(models, to_host=to_host), models, route,
                _zero_bits(rows[best]), f"Krum {route}")
    alphas = gu.dirichlet(ZERO_N, 6)
    w = np.asarray(alphas).astype(np.float32)
    fold = gu.fold_oracle(rows, w, "f32")
    d2s = []
    out = _everywhere(lambda to_host: (lambda r: (d2s.append(r[1]), r[0])[1])(
        geomed.aggregate_with_distances(models, alphas, to_host=to_host)), models, route, _zero_bits(fold),
        f"aggregate_with_distances {route}")
    assert np.array_equal(ku.flat_bits(out), ku.flat_bits(FedAvg.aggregate(models, alphas))), "FedAvg's bits"
    for d2 in d2s:
        assert d2.shape == (ZERO_N,) and d2.dtype == torch.float64 and not d2.is_cuda
        problems, _ = gu.vector_problems(d2.numpy(), gu.dist_oracle(rows, fold, "f32"), ZERO_NUMEL)
        assert not problems, problems
    _unchanged(models, before)


@pytest.mark.parametrize("route", rt.BASELINE)
def test_a_model_of_one_empty_parameter(route):
    n = 5
    models = ROUTES[route]([rt.EmptyNet() for _ in range(n)])
    empty = [np.zeros(0, dtype=np.uint32)]
    for agg in (CoordinateMedian, TrimmedMean.with_trim(1), Krum.with_params(1), MultiKrum.with_params(1),
                MultiKrum.with_params(1, 2), GeometricMedian, CenteredClip):
        _everywhere(lambda to_host: agg.aggregate(models, to_host=to_host), models, route, empty, f"{agg.__name__} {route}")
    got = model_distances(models)
    assert got.shape == (n, n) and got.dtype == torch.float64 and not got.numpy().view(np.uint64).any()
    out, d2 = geomed.aggregate_with_distances(models, [1.0 / n] * n)
    assert not rt.result_problems(out, models, route) and d2.shape == (n,) and not d2.numpy().view(np.uint64).any()
    out, trace = GeometricMedian.aggregate(models, trace=True)
    assert all(not np.asarray(p["d2"]).view(np.uint64).any() for p in trace)


# ---- the *_tensors entries at their edges ------------------------------------------------------------------
def _edge_sizes(T, E):
    """Empty tensors first, in the middle and last; the vector and tile edges; a scalar tail."""
    return [0, 1, E - 1, E, E + 1, 0, T + 3, 2 * T + E + 1, 5, 0]


def _edge_tensors(rows, sizes, dtype, n, aligned):
    """tensors[i][k]: model i's tensor k on the device, one element past an
    aligned address where (i + k) % 3 == 0 (one *_tensors call then takes the
    vector form for some tensors and the scalar form for others at n = 1 and 3,
    the scalar form throughout from n = 3 on; `aligned`: every tensor aligned,
    the vector form and its tile throughout); for n = 3, model 2 is model 0."""
    esz = eu.ESIZE[dtype]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    tensors = []
    for i in range(n):
        if n == 3 and i == 2:
            tensors.append(tensors[0])
            continue
        tensors.append(eu.place([rows[i][offs[k]:offs[k + 1]] for k in range(len(sizes))], dtype, DEV,
                                offsets=[0 if aligned else esz * ((i + k) % 3 == 0) for k in range(len(sizes))]))
    return offs, tensors


def _edge_rows(dtype, n, total, seed):
    rows = eu.random_rows(dtype, n, total, seed)
    if n == 3:
        rows = rows.copy()
        rows[2] = rows[0]
    return rows


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", (1, 3, 9, 32))
def test_pairwise_tensors_entry_at_its_edges(n, dtype, aligned):
    T, _ = _native.pairdist_geometry(n, eu.DTYPES[dtype], HUGE)
    sizes = _edge_sizes(T, eu.VEC_ELEMS[dtype])
    assert sizes[0] == 0  # a memset, then accumulating launches
    total = sum(sizes)
    rows = _edge_rows(dtype, n, total, seed=5100 + n)
    offs, tensors = _edge_tensors(rows, sizes, dtype, n, aligned)
    assert {t.data_ptr() % 16 for row in tensors for t in row if t.numel()} == ({0} if aligned else {0, eu.ESIZE[dtype]})
    stream = torch.cuda.current_stream().cuda_stream
    code = _native.dtype_code(eu.DTYPES[dtype], single_task=True)
    ptrs = [t.data_ptr() for row in tensors for t in row]
    want = ku.sqdist_oracle(rows, dtype)
    prefill = ku.sqdist_oracle(rows[:, :7], dtype).astype(np.float64)  # symmetric, a +0.0 diagonal: what an earlier call leaves
    for start in (False, True):
        flat, one = eu.guarded(n * n * 8, "f64", DEV), eu.guarded(n * n * 8, "f64", DEV)
        if start:
            for g in (flat, one):
                g.view.copy_(torch.from_numpy(prefill.reshape(-1)))
        torch.cuda.synchronize()
        for k in range(len(sizes)):
            _native.pairwise_sqdist([row[k] for row in tensors], flat.view, accumulate=start or k > 0)
        _native.pairwise_sqdist_tensors_raw(ptrs, n, sizes, code, one.view.data_ptr(), start, stream)
        torch.cuda.synchronize()
        assert eu.check_guards(one) == [] and eu.check_guards(flat) == [] and eu.unwritten(one) == 0
        a, b = flat.view.cpu().numpy(), one.view.cpu().numpy()
        assert _same64(a, b), "the tensors entry differs from the chain of flat calls"
        # the prefill is within its own bound of the first 7 elements' oracle (exact value taken as given):
        # 8 non-empty pieces added onto it in order, total - max p_k >= 8
        exp = want + prefill.astype(np.longdouble) if start else want
        problems, worst = ku.matrix_problems(b.reshape(n, n), exp, total)
        print(f"{dtype} n={n} accumulate={start}: max err / bound {worst:.4f}")
        assert not problems, problems
    for row, r in zip(tensors, rows):
        assert eu.inputs_unchanged(row, [r[offs[k]:offs[k + 1]] for k in range(len(sizes))], dtype)


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("packing", ["tight", "padded"])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", (1, 3, 9, 32))
def test_reduce_and_measure_tensors_entry_at_its_edges(n, dtype, packing, aligned):
    """The outputs sit in one guarded buffer: `tight` as ParamLayout.byte_offsets
    packs them (no gap, most of them off 16-byte alignment), `padded` 16-byte
    aligned with guard bytes between neighbours."""
    esz = eu.ESIZE[dtype]
    T, _ = _native.reducedist_geometry(n, eu.DTYPES[dtype], HUGE)
    sizes = _edge_sizes(T, eu.VEC_ELEMS[dtype])
    assert sizes[0] == 0  # a memset, then accumulating launches
    total = sum(sizes)
    rows = _edge_rows(dtype, n, total, seed=5200 + n)
    offs, tensors = _edge_tensors(rows, sizes, dtype, n, aligned)
    stream = torch.cuda.current_stream().cuda_stream
    code = _native.dtype_code(eu.DTYPES[dtype], single_task=True)
    ptrs = [t.data_ptr() for row in tensors for t in row]
    w = [1.0] if n == 1 else [float(v) for v in eu.special_weights(n, "dirichlet", dtype)]
    want_out = gu.fold_oracle(rows, np.asarray(w, dtype=np.float64 if dtype == "f64" else np.float32), dtype)
    want = gu.dist_oracle(rows, want_out, dtype)
    prefill = np.abs(np.random.default_rng(n).standard_normal(n))
    kw = dict(gap=0, align=esz) if packing == "tight" else {}
    for start in (False, True):
        flat_d2, one_d2 = eu.guarded(n * 8, "f64", DEV), eu.guarded(n * 8, "f64", DEV)
        flat_out, one_out = eu.guarded_many(sizes, dtype, DEV, **kw), eu.guarded_many(sizes, dtype, DEV, **kw)
        if start:
            for g in (flat_d2, one_d2):
                g.view.copy_(torch.from_numpy(prefill))
        torch.cuda.synchronize()
        for k in range(len(sizes)):
            _native.wreduce_dist([row[k] for row in tensors], w, flat_out.views[k], flat_d2.view, accumulate=start or k > 0)
        # (offsets from the buffer's base: an empty view, as the first one here, has no address of its own)
        _native.wreduce_dist_tensors_raw(ptrs, n, sizes, [s for s, _ in one_out.regions], w, one_out.buf.data_ptr(), code,
                                         one_d2.view.data_ptr(), start, stream)
        torch.cuda.synchronize()
        for g in (flat_d2, one_d2, flat_out, one_out):
            assert eu.check_guards(g) == [], "guard bytes written"
        assert eu.unwritten(one_d2) == 0
        got = np.concatenate([eu.from_torch(v, dtype) for v in one_out.views])
        assert eu.same_bits(got, want_out, dtype), eu.diff_report(got, want_out, dtype)
        # no element left unwritten: the prefill pattern only where the oracle itself has it (a 16-bit result can)
        assert sum(eu.unwritten(one_out, k) for k in range(len(sizes))) == \
            int((eu.bits_of(want_out, dtype) == eu.fill_pattern(dtype)).sum()), "an output element left unwritten"
        assert np.array_equal(eu.bits_of(got, dtype),
                              eu.bits_of(np.concatenate([eu.from_torch(v, dtype) for v in flat_out.views]), dtype))
        a, b = flat_d2.view.cpu().numpy(), one_d2.view.cpu().numpy()
        assert _same64(a, b), "the tensors entry differs from the chain of flat calls"
        exp = want + prefill.astype(np.longdouble) if start else want
        problems, worst = gu.vector_problems(b, exp, total)  # 8 non-empty pieces in order, total - max p_k >= 8
        print(f"{dtype} n={n} {packing} accumulate={start}: max err / bound {worst:.4f}")
        assert not problems, problems
    for row, r in zip(tensors, rows):
        assert eu.inputs_unchanged(row, [r[offs[k]:offs[k + 1]] for k in range(len(sizes))], dtype)
