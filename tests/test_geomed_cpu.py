"""The geometric median, centered clipping and the fused reduce-and-measure
entry without a GPU: the longdouble distance oracle (tests/_geomed_util.py)
against float64 torch, both weight rules on hand-written vectors and against
an independent restatement, the C entries' argument errors, the geometry
diagnostic, the plugins' errors, ModelManager's selection, and the separation
of every input the GPU trajectory tests use."""
from __future__ import annotations

import ctypes
import math
import types

import numpy as np
import pytest
import torch
from torch import nn

import _edge_util as eu
import _geomed_util as gu
from dasklearn_amd import _native
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod
from dasklearn_amd.gradient_aggregation import geomed
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian, clip_weights, weiszfeld_weights
from dasklearn_amd.model_manager import ModelManager

INF, NAN = math.inf, math.nan
f32 = lambda v: float(np.float32(v))  # noqa: E731


# ---- the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", (1, 2, 3, 8, 17, 32))
def test_oracle_against_float64_torch(n, dtype):
    """Within bound(p) = (p + 8) * 2^-53 relative: ((x - out)**2).sum() in
    float64 rounds the difference (exact here), each square and each partial
    sum of p non-negative terms; the oracle's own error (p * 2^-63) is
    negligible beside it."""
    p = 1237
    rows = eu.random_rows(dtype, n, p, seed=160 + n)
    w = eu.special_weights(n, "dirichlet", dtype)
    out = gu.fold_oracle(rows, w, dtype)
    want = gu.dist_oracle(rows, out, dtype)
    assert want.dtype == np.longdouble and want.shape == (n,)
    x = torch.from_numpy(np.stack([eu.decode(r, dtype) for r in rows]))
    o = torch.from_numpy(eu.decode(out, dtype))
    ref = ((x - o) ** 2).sum(dim=1).numpy()
    w64 = want.astype(np.float64)
    assert np.all(ref[w64 == 0] == 0)  # n = 1 with weight 1.0: the row itself
    rel = np.abs(ref - w64)[w64 > 0] / w64[w64 > 0] if (w64 > 0).any() else np.zeros(1)
    print(f"n={n} {dtype}: max rel diff {rel.max():.3e}")
    assert rel.max() <= gu.bound(p)


def test_oracle_value_classes():
    rows = eu.encode(np.array([[1.0, 2.0, 3.0], [1.0, NAN, 3.0], [INF, 2.0, 3.0], [1.0, 2.0, 4.0]]), "f32")
    out = eu.encode(np.array([1.0, 2.0, 3.0]), "f32")
    assert list(gu.value_class(gu.dist_oracle(rows, out, "f32"))) == [0, 2, 1, 0]
    out = eu.encode(np.array([INF, 2.0, 3.0]), "f32")
    assert list(gu.value_class(gu.dist_oracle(rows, out, "f32"))) == [1, 2, 2, 1]  # Inf - Inf is NaN
    problems, _ = gu.vector_problems([0.0, NAN, INF, 1.0], gu.dist_oracle(rows, eu.encode([1.0, 2.0, 3.0], "f32"), "f32"), 3)
    assert problems == []
    problems, _ = gu.vector_problems([0.0, INF, INF, 1.0], gu.dist_oracle(rows, eu.encode([1.0, 2.0, 3.0], "f32"), "f32"), 3)
    assert problems and "value class" in problems[0]
    problems, _ = gu.vector_problems([0.0, NAN, INF, 1.0 + 1e-12], gu.dist_oracle(rows, eu.encode([1.0, 2.0, 3.0], "f32"), "f32"), 3)
    assert problems and "bound" in problems[0]


# ---- the weight rules on hand-written vectors -----------------------------------------
def test_weiszfeld_on_hand_written_vectors():
    # d2 = 0 and d2 below nu^2 both take nu: equal weights
    assert weiszfeld_weights([0.0, 1e-14], [0.5, 0.5], 1e-6) == [0.5, 0.5]
    # 1 / (1, 2, 4) normalised: 4/7, 2/7, 1/7
    assert weiszfeld_weights([1.0, 4.0, 16.0], [1.0, 1.0, 1.0], 1e-6) == [f32(4 / 7), f32(2 / 7), f32(1 / 7)]
    # alphas scale the betas
    assert weiszfeld_weights([1.0, 1.0], [0.25, 0.75], 1e-6) == [0.25, 0.75]
    # nu takes over exactly at sqrt(d2) = nu
    assert weiszfeld_weights([0.25, 1.0], [1.0, 1.0], 0.5) == [f32(2 / 3), f32(1 / 3)]
    assert weiszfeld_weights([0.01, 1.0], [1.0, 1.0], 0.5) == [f32(2 / 3), f32(1 / 3)]
    # a non-finite d2 is weight 0
    assert weiszfeld_weights([1.0, NAN, INF, 1.0], [0.25] * 4, 1e-6) == [0.5, 0.0, 0.0, 0.5]
    # sum beta = 0 (all non-finite, or all alphas 0) or non-finite: the iteration stops
    assert weiszfeld_weights([NAN, INF], [0.5, 0.5], 1e-6) is None
    assert weiszfeld_weights([1.0, 4.0], [0.0, 0.0], 1e-6) is None
    assert weiszfeld_weights([1.0, 4.0], [INF, 1.0], 1e-6) is None
    # every weight is an fp32 value
    w = weiszfeld_weights([3.0, 5.0, 7.0], [0.2, 0.3, 0.5], 1e-6)
    assert all(v == f32(v) for v in w)


def test_clip_on_hand_written_vectors():
    # d2 = 0 gives c = 1; distance 2 against tau 1 gives c = 1/2
    assert clip_weights([0.0, 4.0], [0.5, 0.5], 1.0) == [0.25, 0.5, 0.25]
    # everyone inside tau: the centre's weight is 0, the pass is FedAvg over the peers
    assert clip_weights([0.25, 0.81], [0.5, 0.5], 1.0) == [0.0, 0.5, 0.5]
    # a non-finite d2 is c = 0
    assert clip_weights([NAN, INF, 0.0, 0.0], [0.25] * 4, 1.0) == [0.5, 0.0, 0.0, 0.25, 0.25]
    # tau None: the lower median of the distances (1, 2, 3, 4 -> 2), ties included (2, 2, 2, 9 -> 2)
    assert clip_weights([1.0, 4.0, 9.0, 16.0], [0.25] * 4, None) == clip_weights([1.0, 4.0, 9.0, 16.0], [0.25] * 4, 2.0)
    assert clip_weights([4.0, 4.0, 4.0, 81.0], [0.25] * 4, None) == [f32(1 - 0.75 - 0.25 * 2 / 9), 0.25, 0.25, 0.25,
                                                                      f32(0.25 * 2 / 9)]
    assert clip_weights([9.0, 1.0, 4.0], [0.5, 0.25, 0.25], None)[1:] == [f32(0.5 * 2 / 3), 0.25, 0.25]
    # a non-finite distance counts as +Inf in the median: (1, inf, inf) -> inf, the finite peer unclipped
    assert clip_weights([1.0, NAN, INF], [0.5, 0.25, 0.25], None) == [0.5, 0.5, 0.0, 0.0]
    # median 0: only the peers at the centre move it
    assert clip_weights([0.0, 0.0, 4.0], [0.25, 0.25, 0.5], None) == [0.5, 0.25, 0.25, 0.0]
    w = clip_weights([3.0, 5.0, 7.0], [0.2, 0.3, 0.5], 2.0)
    assert len(w) == 4 and all(v == f32(v) for v in w)


@pytest.mark.parametrize("seed", range(8))
def test_rules_agree_with_the_restatement_on_random_vectors(seed):
    """The plugin's rules (Python floats) against the longdouble restatement:
    after the fp32 rounding they may differ only where a weight sits within a
    few double roundings of a midpoint, which these seeds do not hit."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 33))
    d2 = (rng.standard_normal(n) ** 2 * 10.0 ** rng.integers(-3, 4, n)).tolist()
    if seed % 2:
        d2[int(rng.integers(n))] = NAN if seed % 4 == 1 else INF
    alphas = gu.dirichlet(n, seed)
    nu = 1e-6 if seed < 4 else 1.0
    ref = gu.ref_weiszfeld(d2, alphas, nu)
    got = weiszfeld_weights(d2, alphas, nu)
    if ref is None:
        assert got is None
    else:
        assert gu.midpoint_margin(ref) > 1e-13
        assert np.array_equal(np.asarray(got, dtype=np.float32), gu.r32(ref)) and got == [float(v) for v in gu.r32(ref)]
    for tau in (None, 0.7):
        ref, _ = gu.ref_clip(d2, alphas, tau)
        assert gu.midpoint_margin(ref) > 1e-13
        assert clip_weights(d2, alphas, tau) == [float(v) for v in gu.r32(ref)]


# ---- the C entries --------------------------------------------------------------------
D2, OUT = 1 << 20, 1 << 21


def _flat(n=2, nelem=100, dtype=0, d2=D2, out=OUT, acc=0, ins=None, w=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (i + 1) for i in range(max(n, 1))]
    w = w if w is not None else [0.5] * max(n, 1)
    return lib.dlsim_wreduce_dist((ctypes.c_void_p * len(ins))(*ins), n, (ctypes.c_double * len(w))(*w),
                                  ctypes.c_void_p(out), nelem, dtype, ctypes.c_void_p(d2), acc, None)


def test_flat_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _flat(n=0) == -1 and b"n must be" in lib.dlsim_last_error()
    assert _flat(n=33, ins=[4096] * 33, w=[0.5] * 33) == -1 and b"<= 32" in lib.dlsim_last_error()
    assert _flat(dtype=7) == -2
    assert _flat(dtype=-1) == -2
    for acc in (2, -1):
        assert _flat(acc=acc) == -1 and b"accumulate" in lib.dlsim_last_error()
    assert _flat(d2=0) == -1 and b"null" in lib.dlsim_last_error()
    assert _flat(ins=[4096, 0]) == -1 and b"null input" in lib.dlsim_last_error()
    none_w = lib.dlsim_wreduce_dist((ctypes.c_void_p * 2)(4096, 8192), 2, None, ctypes.c_void_p(OUT), 100, 0,
                                    ctypes.c_void_p(D2), 0, None)
    assert none_w == -1 and b"null weights" in lib.dlsim_last_error()
    assert lib.dlsim_wreduce_dist(None, 2, (ctypes.c_double * 2)(0.5, 0.5), ctypes.c_void_p(OUT), 100, 0,
                                  ctypes.c_void_p(D2), 0, None) == -1
    # a weight the fp32 conversion would change: refused for the three narrow dtypes, taken for fp64
    for dtype in (0, 1, 2):
        assert _flat(dtype=dtype, w=[0.5, 0.1]) == -1 and b"weight 1" in lib.dlsim_last_error()
        assert _flat(dtype=dtype, w=[NAN, 0.5]) == -1 and b"weight 0" in lib.dlsim_last_error()
    assert _flat(dtype=3, w=[0.5, 0.1], d2=4096) == -1 and b"overlaps input 0" in lib.dlsim_last_error()  # past the weights
    # the vector (n doubles = 16 bytes) on an input (fp32: 400 bytes) or on the output
    assert _flat(d2=4096) == -1 and b"overlaps input 0" in lib.dlsim_last_error()
    assert _flat(d2=8192 + 399) == -1 and b"overlaps input 1" in lib.dlsim_last_error()
    assert _flat(d2=4096 - 15) == -1
    assert _flat(d2=OUT + 399) == -1 and b"overlaps the output" in lib.dlsim_last_error()
    assert _flat(d2=OUT - 15) == -1 and b"overlaps the output" in lib.dlsim_last_error()
    # the output on an input: exact aliasing, a shared byte at either end
    assert _flat(out=4096) == -1 and b"output overlaps input 0" in lib.dlsim_last_error()
    assert _flat(out=8192 + 399) == -1 and b"output overlaps input 1" in lib.dlsim_last_error()
    assert _flat(out=4096 - 399) == -1 and b"output overlaps input 0" in lib.dlsim_last_error()
    assert _flat(out=4096 - 799, dtype=3) == -1
    assert lib.dlsim_version() > 0  # none of them reached a HIP call: the next call still works


def _tensors(n=2, t=2, numels=(10, 20), offs=(0, 64), dtype=0, d2=D2, out=OUT, acc=0, ins=None, w=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (q + 1) for q in range(max(n * t, 1))]
    w = w if w is not None else [0.5] * max(n, 1)
    sz = ctypes.c_size_t * max(len(numels), 1)
    return lib.dlsim_wreduce_dist_tensors((ctypes.c_void_p * len(ins))(*ins), n, t, sz(*numels), sz(*offs),
                                          (ctypes.c_double * len(w))(*w), ctypes.c_void_p(out), dtype,
                                          ctypes.c_void_p(d2), acc, None)


def test_tensors_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _tensors(t=-1) == -1
    assert _tensors(n=0) == -1
    assert _tensors(n=33, w=[0.5] * 33) == -1 and b"<= 32" in lib.dlsim_last_error()
    assert _tensors(dtype=9) == -2
    assert _tensors(acc=3) == -1
    assert _tensors(d2=0) == -1
    assert _tensors(w=[0.5, 1e-50]) == -1 and b"weight 1" in lib.dlsim_last_error()
    assert _tensors(ins=[4096, 8192, 0, 16384]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_wreduce_dist_tensors(None, 2, 2, None, None, (ctypes.c_double * 2)(0.5, 0.5), ctypes.c_void_p(OUT), 0,
                                          ctypes.c_void_p(D2), 0, None) == -1
    # the vector on tensor 1 of model 1 (the fourth pointer, 80 bytes)
    assert _tensors(d2=16384 + 79) == -1 and b"tensor 1" in lib.dlsim_last_error()
    # the vector on the second output range (out + 64, 80 bytes)
    assert _tensors(d2=OUT + 64 + 72) == -1 and b"overlaps the output" in lib.dlsim_last_error()
    # output range 1 on tensor 0 of model 1 (the third pointer, 40 bytes): across tensors
    assert _tensors(out=12288 - 64 + 36) == -1 and b"output" in lib.dlsim_last_error()
    # two output ranges on each other
    assert _tensors(offs=(0, 36)) == -1 and b"outputs of tensors" in lib.dlsim_last_error()
    assert lib.dlsim_version() > 0


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_geometry_follows_the_register_plan_and_needs_no_gpu(dtype):
    dt = eu.DTYPES[dtype]
    for n in (1, 2, 4, 5, 8, 9, 16, 17, 32):
        width = max(eu.ESIZE[dtype], 16 if n <= 8 else 8 if n <= 16 else 4)  # bytes a lane takes of a row
        for numel in (0, 1, 1000, 10 ** 7, 10 ** 10):
            tile, blocks = _native.reducedist_geometry(n, dt, numel)
            assert tile == 256 * width // eu.ESIZE[dtype] and blocks >= 1
            assert blocks <= max(1, -(-numel // tile))
        cap = _native.reducedist_geometry(n, dt, 10 ** 10)[1]
        assert cap == _native.reducedist_geometry(n, dt, 10 ** 11)[1] == 1024
        assert cap * tile <= 4 * 1024 * 1024
    lib = _native.load()
    t, b = ctypes.c_size_t(0), ctypes.c_uint(0)
    assert lib.dlsim_reducedist_geometry(0, 0, 10, ctypes.byref(t), ctypes.byref(b)) == -1
    assert lib.dlsim_reducedist_geometry(33, 0, 10, ctypes.byref(t), ctypes.byref(b)) == -1
    assert lib.dlsim_reducedist_geometry(2, 5, 10, ctypes.byref(t), ctypes.byref(b)) == -2
    assert lib.dlsim_reducedist_geometry(2, 0, 10, None, ctypes.byref(b)) == -1
    assert _native.MAX_REDUCEDIST_INPUTS == 32


# ---- the plugins ------------------------------------------------------------------------
def _models(n):
    torch.manual_seed(n)
    return [nn.Linear(3, 2) for _ in range(n)]


@pytest.mark.parametrize("agg", [GeometricMedian, CenteredClip, GeometricMedian.with_params(0, 0.5),
                                 CenteredClip.with_params(2.0, 1)])
def test_plugin_errors_come_before_any_device_work(agg):
    with pytest.raises(AssertionError):
        agg.aggregate(_models(7), [0.5, 0.5])
    with pytest.raises(IndexError):
        agg.aggregate([], None)
    with pytest.raises(IndexError):
        agg.aggregate([], [])
    with pytest.raises(ValueError, match="at most 3[12]"):
        agg.aggregate(_models(33), None)
    with pytest.raises(ValueError):
        agg.aggregate([nn.Linear(3, 2), nn.Linear(4, 2), nn.Linear(3, 2)])


def test_fan_in_limits_and_with_params():
    with pytest.raises(ValueError, match="at most 31"):
        CenteredClip.aggregate(_models(32))
    for bad in (dict(iters=-1), dict(iters=1.5), dict(nu=0.0), dict(nu=-1.0), dict(nu=INF), dict(nu=NAN)):
        with pytest.raises(ValueError):
            GeometricMedian.with_params(**bad)
    for bad in (dict(iters=-1), dict(iters=0.5), dict(tau=0.0), dict(tau=-2.0), dict(tau=INF), dict(tau=NAN)):
        with pytest.raises(ValueError):
            CenteredClip.with_params(**bad)
    g = GeometricMedian.with_params(5, 1e-3)
    assert issubclass(g, GeometricMedian) and (g.iters, g.nu) == (5, 1e-3) and (GeometricMedian.iters, GeometricMedian.nu) == (3, 1e-6)
    c = CenteredClip.with_params(2.5, 0)
    assert issubclass(c, CenteredClip) and (c.tau, c.iters) == (2.5, 0) and (CenteredClip.tau, CenteredClip.iters) == (None, 3)
    assert CenteredClip.with_params().tau is None
    for fn in (geomed.aggregate_with_distances, geomed.consensus_distance):
        with pytest.raises(IndexError):
            fn([], []) if fn is geomed.aggregate_with_distances else fn([])
    with pytest.raises(ValueError, match="at most 32"):
        geomed.consensus_distance(_models(33))
    with pytest.raises(AssertionError):
        geomed.consensus_distance(_models(3), [0.5, 0.5])


def test_enum_values():
    assert [int(m) for m in GradientAggregationMethod] == [1, 2, 3, 4, 5, 6, 7]
    assert GradientAggregationMethod.GEOMETRIC_MEDIAN == 6
    assert GradientAggregationMethod.CENTERED_CLIP == 7


def test_model_manager_selects_both_rules_and_their_parameters():
    pick = lambda **kw: ModelManager(None, types.SimpleNamespace(**kw), 0).get_aggregation_method()  # noqa: E731
    g = pick(gradient_aggregation=6)
    assert issubclass(g, GeometricMedian) and (g.iters, g.nu) == (3, 1e-6)
    g = pick(gradient_aggregation=GradientAggregationMethod.GEOMETRIC_MEDIAN, aggregation_gm_iters=7, aggregation_gm_nu=0.25)
    assert issubclass(g, GeometricMedian) and (g.iters, g.nu) == (7, 0.25)
    c = pick(gradient_aggregation=7)
    assert issubclass(c, CenteredClip) and (c.tau, c.iters) == (None, 3)
    c = pick(gradient_aggregation=GradientAggregationMethod.CENTERED_CLIP, aggregation_clip_tau=1.5, aggregation_clip_iters=0)
    assert issubclass(c, CenteredClip) and (c.tau, c.iters) == (1.5, 0)
    assert pick(gradient_aggregation=1) is FedAvg and pick() is FedAvg
    assert pick(gradient_aggregation=99) is None and pick(gradient_aggregation=8) is None
    with pytest.raises(ValueError):
        pick(gradient_aggregation=6, aggregation_gm_nu=0.0)
    # the settings reach the fan-in check
    mm = ModelManager(None, types.SimpleNamespace(gradient_aggregation=7), 0)
    for i, m in enumerate(_models(32)):
        mm.process_incoming_trained_model(i, m)
    with pytest.raises(ValueError, match="at most 31"):
        mm.aggregate_trained_models(None)


# ---- the inputs of the GPU trajectory tests -----------------------------------------------
@pytest.mark.parametrize("name", sorted(gu.CASES))
def test_separation_of_every_gpu_trajectory_input(name):
    """Every oracle weight of every pass lies at least SEPARATION x
    (numel + 8) * 2^-53 relative away from an fp32 rounding midpoint, every
    sqrt(d2_i) that far from tau (from nu for the geometric median) and, under
    tau = None, from its neighbours in the median ordering; the centre weight
    of a clipping pass is at least 1e-2 (no cancellation in 1 - sum). A run
    whose d2 are within the kernel's bound of the oracle's then takes the
    oracle's fp32 weights in pass 1, so its pass-1 output and d2 are the
    oracle's (within the bound again), and so on by induction."""
    case = gu.CASES[name]
    rows, byz, alphas, out, passes = gu.case_trajectory(case)
    numel = rows.shape[1]
    assert len(passes) == 1 + (gu.GM_ITERS if case["rule"] == "gm" else gu.CLIP_ITERS)
    assert gu.separation_problems(passes, case["rule"], numel, gu.GM_NU) == []
    assert np.isfinite(eu.decode(out, "f32")).all()
    kept = passes[0]["kept"]
    if case["special"]:
        assert np.isnan(rows[byz[0]]).all() and np.isinf(rows[byz[-1]]).all()
        assert kept == [i for i in range(case["n"]) if i not in (byz[0], byz[-1])]
        if case["byz"]:
            assert 0 not in kept  # the BatchNorm case: model 0 is excluded
    else:
        assert kept == list(range(case["n"]))
    if case["rule"] == "clip" and case["tau"] is not None:
        # a fixed tau that clips some peers and not others in every pass
        for p in passes[1:]:
            w = np.asarray(p["exact"][1:], dtype=np.float64)
            a = np.asarray(alphas if alphas else [1 / case["n"]] * case["n"])[kept]
            a = a / a.sum()
            assert (w < a * (1 - 1e-9)).any() and (np.abs(w - a) < 1e-12).any()


@pytest.mark.parametrize("name", sorted(gu.MIXED_CASES))
def test_separation_of_the_two_dtype_group_inputs(name):
    """The same for the cases on the module with an fp32 and a bf16 group
    (tests/test_gpu_model_routes.py): d2 is the sum of the groups' distances
    over all 401 elements, and the separation is asked for that count."""
    case = gu.MIXED_CASES[name]
    groups, byz, outs, passes = gu.mixed_case_trajectory(case)
    assert [(dt, rows.shape) for rows, dt in groups] == [("f32", (6, 236)), ("bf16", (6, 165))]
    assert gu.MIXED_NUMEL == 401 and len(byz) == case["f"]
    assert len(passes) == 1 + (gu.GM_ITERS if case["rule"] == "gm" else gu.CLIP_ITERS)
    assert gu.separation_problems(passes, case["rule"], gu.MIXED_NUMEL, gu.GM_NU) == []
    assert passes[0]["kept"] == list(range(case["n"]))
    for (rows, dt), out in zip(groups, outs):
        assert out.shape == (rows.shape[1],) and np.isfinite(eu.decode(out, dt)).all()
    # one group alone through trajectory_groups is trajectory itself, and both groups contribute to d2
    rows, dt = groups[0]
    alone, alone_passes = gu.trajectory(list(rows), dt, None, case["rule"], 1, nu=gu.GM_NU, tau=case["tau"])
    again, again_passes = gu.trajectory_groups([(rows, dt)], None, case["rule"], 1, nu=gu.GM_NU, tau=case["tau"])
    assert np.array_equal(alone, again[0]) and np.array_equal(alone_passes[1]["d2"], again_passes[1]["d2"])
    o32, o16 = (gu.fold_oracle(r, passes[0]["weights"], d) for r, d in groups)
    want = gu.dist_oracle(groups[0][0], o32, "f32") + gu.dist_oracle(groups[1][0], o16, "bf16")
    assert np.array_equal(passes[0]["d2"], want) and (passes[0]["d2"] > alone_passes[0]["d2"]).all()


def test_the_geometric_median_of_the_oracle_is_closer_to_the_honest_mean():
    """The robustness claim the GPU test repeats on the kernel's result: with f
    far-away Byzantine rows the oracle's geometric median lies strictly closer
    to the honest mean than the oracle's FedAvg does."""
    for name in ("gm-8", "gm-17", "gm-32"):
        rows, byz, alphas, out, passes = gu.case_trajectory(gu.CASES[name])
        x = eu.decode(rows, "f32")
        honest = np.delete(x, byz, axis=0).mean(axis=0)
        avg = eu.decode(gu.fold_oracle(list(rows), passes[0]["weights"], "f32"), "f32")
        d_gm, d_avg = np.linalg.norm(eu.decode(out, "f32") - honest), np.linalg.norm(avg - honest)
        print(f"{name}: |gm - honest| {d_gm:.4f}, |fedavg - honest| {d_avg:.4f}")
        assert d_gm < d_avg
