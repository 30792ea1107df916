"""The mean around the median and Bulyan without a GPU: the CPU restatement
(tests/_nearest_util.py) against an independent brute force and against the
rank window's identities, the closed form the kernels use against the walk,
Bulyan's selection against a direct restatement, the C entries' argument
errors, ModelManager's and method_route's choices."""
from __future__ import annotations

import ctypes
import math
import types

import numpy as np
import pytest
import torch
from torch import nn

import _nearest_util as nu
import _robust_util as ru
from dasklearn_amd import _native, batch
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M
from dasklearn_amd.gradient_aggregation.krum import Bulyan, Krum, MultiKrum, bulyan_select, check_bulyan_params
from dasklearn_amd.gradient_aggregation.robust import MeanAroundMedian, TrimmedMean
from dasklearn_amd.model_manager import ModelManager

DTYPES = ["f32", "f64", "bf16", "f16"]
FAN_INS = (1, 2, 3, 4, 5, 7, 8, 11, 16, 17, 32)


def _columns(dtype, n, seed):
    """special_rows (every special in every row position) beside 300 random columns."""
    dt = ru.DTYPES[dtype]
    rows = [torch.cat([a, b]) for a, b in zip(ru.special_rows(dt, n), ru.random_rows(dt, n, 300, seed))]
    return ru.sorted_bits(rows, dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 7, 8))
def test_walk_against_the_brute_force_on_small_columns(n, dtype):
    dt = ru.DTYPES[dtype]
    sb = _columns(dtype, n, seed=100 + n)
    for keep in range(1, n + 1):
        lo = nu.nearest_lo(sb, dt, keep)
        want = np.array([nu.brute_lo(sb[:, c], dt, keep) for c in range(sb.shape[1])])
        bad = np.nonzero(lo != want)[0]
        assert bad.size == 0, f"keep {keep}: column {bad[0]}: walk {lo[bad[0]]}, brute force {want[bad[0]]}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", FAN_INS)
def test_closed_form_equals_the_walk_and_distances_never_decrease(n, dtype):
    """The kernels count l instead of walking (robust_nearest_kernels.hpp)."""
    dt = ru.DTYPES[dtype]
    sb = _columns(dtype, n, seed=200 + n)
    nan, val = nu._distances(sb, dt)
    m = (n - 1) // 2
    for a, b in [(j + 1, j) for j in range(m, n - 1)] + [(j - 1, j) for j in range(m, 0, -1)]:
        assert not nu._strictly_farther(nan[b], val[b], nan[a], val[a]).any(), f"d[{b}] > d[{a}]"
    for keep in range(1, n + 1):
        assert np.array_equal(nu.closed_form_lo(sb, dt, keep), nu.nearest_lo(sb, dt, keep)), keep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", FAN_INS)
def test_keep_one_is_the_median_and_keep_n_the_whole_window(n, dtype):
    dt = ru.DTYPES[dtype]
    sb = _columns(dtype, n, seed=300 + n)
    lo = (n - 1) // 2
    assert ru.same_bits(nu.nearest_mean_sorted(sb, dt, 1), ru.window_mean_sorted(sb, dt, lo, lo + 1))
    assert ru.same_bits(nu.nearest_mean_sorted(sb, dt, n), ru.window_mean_sorted(sb, dt, 0, n))


def test_random_rows_move_the_window_off_the_rank_window():
    """The input condition of the GPU parity tests: with n = 8 and keep = 4 the
    rank window of the same kept count starts at 2; a kernel that ran it
    could not pass on inputs where many elements start elsewhere."""
    dt = torch.float32
    sb = ru.sorted_bits(ru.random_rows(dt, 8, 20_000, seed=7, special_frac=0), dt)
    lo = nu.nearest_lo(sb, dt, 4)
    frac = float((lo != 2).mean())
    print(f"elements with lo != 2: {frac:.3f}")
    assert frac >= 0.25
    assert not ru.same_bits(nu.nearest_mean_sorted(sb, dt, 4), ru.window_mean_sorted(sb, dt, 2, 6))


def test_ties_go_left_and_a_nan_distance_is_the_farthest():
    f = lambda *v: [torch.tensor([x], dtype=torch.float32) for x in v]  # noqa: E731
    # sorted 0 1 2 3 4: m = 2; 1 and 3 tie: left first
    assert nu.nearest_mean(f(4., 0., 3., 1., 2.), 2).item() == 1.5
    assert nu.nearest_mean(f(4., 0., 3., 1., 2.), 3).item() == 2.0
    # sorted 0 1 2 2.5 inf: the window leans right, then left; never the Inf before the 0
    assert nu.nearest_mean(f(math.inf, 0., 2.5, 1., 2.), 2).item() == 2.25
    assert nu.nearest_mean(f(math.inf, 0., 2.5, 1., 2.), 4).item() == 1.375
    # sorted -inf 1 2 nan nan: -inf (distance Inf) before the NaN (distance NaN)
    assert nu.nearest_mean(f(math.nan, -math.inf, math.nan, 1., 2.), 3).item() == -math.inf
    # the median a NaN: the other NaN is at distance 0, every number at NaN
    assert math.isnan(nu.nearest_mean(f(math.nan, math.nan, math.nan, 1., 2.), 2).item())


# ---- Bulyan's selection -------------------------------------------------------------
def _select_restated(d2, f):
    n = len(d2)
    D = np.array([[v if math.isfinite(v) else math.inf for v in row] for row in d2], dtype=np.float64)
    left, out = list(range(n)), []
    for _ in range(n - 2 * f):
        r = len(left)
        k = 0 if r == 1 else min(r - 1, max(1, r - f - 2))
        scores = {}
        for i in left:
            s = 0.0
            for v in sorted(D[i, j] for j in left if j != i)[:k]:
                s = s + v
            scores[i] = s
        best = min(left, key=lambda i: (scores[i], i))
        left.remove(best)
        out.append(best)
    return sorted(out)


def _matrix(n, seed, bad=()):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 6))
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    for i in bad:
        d[i, :] = d[:, i] = math.inf
        d[i, i] = 0.0
    return d.tolist()


@pytest.mark.parametrize("n,f", [(3, 0), (5, 0), (7, 1), (8, 1), (11, 2), (15, 3), (32, 7)])
def test_bulyan_select_against_a_direct_restatement(n, f):
    for seed in range(5):
        d2 = _matrix(n, seed)
        got = bulyan_select(d2, f)
        assert got == _select_restated(d2, f)
        assert len(got) == n - 2 * f and got == sorted(set(got))
    assert bulyan_select(_matrix(n, 1), 0) == list(range(n))  # f = 0 selects everyone


def test_bulyan_select_leaves_out_an_all_inf_row_and_breaks_ties_low():
    d2 = _matrix(7, 3, bad=(0,))
    d2[4][5] = d2[5][4] = math.nan  # a non-finite entry counts as +Inf
    got = bulyan_select(d2, 1)
    assert 0 not in got and got == _select_restated(d2, 1)
    # two all-Inf rows with f = 2: never chosen while finite ones remain (7 of 11 are chosen)
    got = bulyan_select(_matrix(11, 4, bad=(2, 9)), 2)
    assert 2 not in got and 9 not in got
    # every distance equal: every score ties, the lower indices go first
    flat = [[0.0 if i == j else 1.0 for j in range(7)] for i in range(7)]
    assert bulyan_select(flat, 1) == [0, 1, 2, 3, 4]
    assert bulyan_select([[0.0 if i == j else math.inf for j in range(7)] for i in range(7)], 1) == [0, 1, 2, 3, 4]


def test_bulyan_parameters():
    for n, f in ((2, 0), (6, 1), (10, 2), (7, -1)):
        with pytest.raises(ValueError, match="4\\*f \\+ 3"):
            check_bulyan_params(n, f)
        with pytest.raises(ValueError):
            bulyan_select(_matrix(n, 0), f)
    check_bulyan_params(3, 0)
    check_bulyan_params(7, 1)
    with pytest.raises(ValueError):
        Bulyan.with_params(-1)
    assert Bulyan.f == 1 and Bulyan.with_params(2).f == 2
    assert not issubclass(Bulyan, (Krum, MultiKrum)) and not issubclass(MeanAroundMedian, TrimmedMean)


# ---- the plugins, ModelManager, the router ---------------------------------------------
def _models(n):
    torch.manual_seed(n)
    return [nn.Linear(3, 2) for _ in range(n)]


@pytest.mark.parametrize("agg", [MeanAroundMedian, MeanAroundMedian.with_trim(2), Bulyan])
def test_plugin_errors_come_before_any_device_work(agg):
    with pytest.raises(AssertionError):
        agg.aggregate(_models(3), [0.5, 0.5])
    with pytest.raises(ValueError, match="unweighted"):
        agg.aggregate(_models(3), [0.2, 0.3, 0.5])
    with pytest.raises(IndexError):
        agg.aggregate([], None)
    with pytest.raises(ValueError, match="at most 32"):
        agg.aggregate(_models(33), None)


def test_mean_around_median_parameter_errors():
    with pytest.raises(ValueError, match=r"n = 4 .*trim = 2"):
        MeanAroundMedian.with_trim(2).aggregate(_models(4))
    with pytest.raises(ValueError, match=r"n = 2 .*trim = 1"):
        MeanAroundMedian.aggregate(_models(2))
    for keep in (0, 5):
        with pytest.raises(ValueError, match=f"keep = {keep}"):
            MeanAroundMedian.aggregate(_models(4), keep=keep)
    with pytest.raises(ValueError):
        MeanAroundMedian.with_trim(-1)
    assert MeanAroundMedian.trim == 1 and MeanAroundMedian.with_trim(3).trim == 3
    with pytest.raises(ValueError, match="4\\*f \\+ 3"):
        Bulyan.aggregate(_models(6))


def _pick(**kw):
    return ModelManager(None, types.SimpleNamespace(**kw), 0).get_aggregation_method()


def test_model_manager_picks_both_variants_and_their_parameters():
    mm = _pick(gradient_aggregation=3, aggregation_trim_rule="median")
    assert issubclass(mm, MeanAroundMedian) and mm.trim == 1
    mm = _pick(gradient_aggregation=M.TRIMMED_MEAN, aggregation_trim_rule="median", aggregation_trim=3)
    assert issubclass(mm, MeanAroundMedian) and mm.trim == 3
    tm = _pick(gradient_aggregation=3, aggregation_trim_rule="rank", aggregation_trim=2)
    assert issubclass(tm, TrimmedMean) and tm.trim == 2
    assert issubclass(_pick(gradient_aggregation=3), TrimmedMean)
    b = _pick(gradient_aggregation=5, aggregation_krum_rule="bulyan")
    assert issubclass(b, Bulyan) and b.f == 1
    b = _pick(gradient_aggregation=M.MULTI_KRUM, aggregation_krum_rule="bulyan", aggregation_byzantine=2)
    assert issubclass(b, Bulyan) and b.f == 2
    mk = _pick(gradient_aggregation=5, aggregation_krum_rule="multi_krum", aggregation_multi_krum_m=3)
    assert issubclass(mk, MultiKrum) and mk.m == 3
    assert issubclass(_pick(gradient_aggregation=5), MultiKrum)
    with pytest.raises(ValueError, match="aggregation_multi_krum_m"):
        _pick(gradient_aggregation=5, aggregation_krum_rule="bulyan", aggregation_multi_krum_m=3)
    # the rules belong to their own members only; the enum is unchanged
    assert _pick(gradient_aggregation=4, aggregation_krum_rule="bulyan").__mro__[1] is Krum
    assert _pick(gradient_aggregation=8, aggregation_krum_rule="bulyan") is None
    assert [int(v) for v in M] == [1, 2, 3, 4, 5, 6, 7]


def test_unknown_rule_strings_raise():
    with pytest.raises(ValueError, match="aggregation_trim_rule"):
        _pick(gradient_aggregation=3, aggregation_trim_rule="nearest")
    with pytest.raises(ValueError, match="aggregation_krum_rule"):
        _pick(gradient_aggregation=5, aggregation_krum_rule="Bulyan")
    with pytest.raises(ValueError, match="aggregation_trim_rule"):
        batch.method_window(M.TRIMMED_MEAN, types.SimpleNamespace(aggregation_trim_rule=None))


def test_method_route_runs_both_variants_per_task():
    ns = types.SimpleNamespace
    r = batch.method_route(M.TRIMMED_MEAN, ns(aggregation_trim_rule="median", aggregation_trim=2))
    assert r.kind == batch.PLUGIN and issubclass(r.plugin, MeanAroundMedian) and r.plugin.trim == 2
    assert batch.method_window(M.TRIMMED_MEAN, ns(aggregation_trim_rule="median")) is None
    r = batch.method_route(M.MULTI_KRUM, ns(aggregation_krum_rule="bulyan", aggregation_byzantine=2))
    assert r.kind == batch.PLUGIN and issubclass(r.plugin, Bulyan) and r.plugin.f == 2
    # without the new settings: today's routes
    assert batch.method_route(M.TRIMMED_MEAN, ns()).kind == batch.WINDOW
    assert batch.method_route(M.TRIMMED_MEAN, None).kind == batch.WINDOW
    assert batch.method_route(M.TRIMMED_MEAN, ns(aggregation_trim_rule="rank")).kind == batch.WINDOW
    assert batch.method_window(M.TRIMMED_MEAN, ns(aggregation_trim=2))(8) == (2, 6)
    assert batch.method_route(M.MULTI_KRUM, ns()).kind == batch.KRUM
    assert batch.method_route(M.MULTI_KRUM, ns(aggregation_krum_rule="multi_krum")).kind == batch.KRUM
    assert batch.method_route(M.KRUM, ns(aggregation_krum_rule="bulyan")).kind == batch.KRUM


# ---- the C entries ----------------------------------------------------------------------
def _flat(n=2, keep=1, dtype=0, out=1 << 20, nelem=100, ins=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (i + 1) for i in range(max(n, 1))]
    return lib.dlsim_robust_nearest_reduce((ctypes.c_void_p * len(ins))(*ins), n, keep, ctypes.c_void_p(out), nelem,
                                           dtype, None)


def test_flat_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _flat(n=0) == -1 and b"n must be" in lib.dlsim_last_error()
    assert _flat(n=33, keep=1, ins=[4096] * 33) == -1 and b"<= 32" in lib.dlsim_last_error()
    for n, keep in ((2, 0), (2, 3), (2, -1), (32, 33)):
        assert _flat(n=n, keep=keep, ins=[4096 * (i + 1) for i in range(n)]) == -1
        assert b"keep" in lib.dlsim_last_error()
    assert _flat(dtype=7) == -2
    assert _flat(out=0) == -1
    assert _flat(ins=[4096, 0]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_robust_nearest_reduce(None, 2, 1, ctypes.c_void_p(64), 100, 0, None) == -1
    # any overlap, exact aliasing included (fp32: 400 bytes per buffer)
    assert _flat(out=4096) == -1 and b"overlap" in lib.dlsim_last_error()
    assert _flat(out=8192 + 396) == -1 and b"overlaps input 1" in lib.dlsim_last_error()
    assert _flat(out=4096 - 396) == -1
    # zero elements: a no-op, whatever the pointers; a bad keep is still refused
    assert _flat(nelem=0, out=0) == 0
    assert _flat(nelem=0, keep=3) == -1
    for dt in range(4):
        assert _flat(nelem=0, dtype=dt) == 0


def _tensors(n=2, t=2, numels=(10, 20), offs=(0, 64), keep=1, out=1 << 20, dtype=0, ins=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (q + 1) for q in range(max(n * t, 1))]
    sz = ctypes.c_size_t * max(len(numels), 1)
    return lib.dlsim_robust_nearest_reduce_tensors((ctypes.c_void_p * len(ins))(*ins), n, t, sz(*numels), sz(*offs),
                                                   keep, ctypes.c_void_p(out), dtype, None)


def test_tensors_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _tensors(t=-1) == -1
    assert _tensors(n=0) == -1
    assert _tensors(n=33, keep=2) == -1 and b"<= 32" in lib.dlsim_last_error()
    for keep in (0, 3):
        assert _tensors(keep=keep) == -1 and b"keep" in lib.dlsim_last_error()
    assert _tensors(dtype=9) == -2
    assert _tensors(out=0) == -1
    assert _tensors(ins=[4096, 8192, 0, 16384]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_robust_nearest_reduce_tensors(None, 2, 2, None, None, 1, ctypes.c_void_p(64), 0, None) == -1
    assert _tensors(out=4096 - 64) == -1 and b"overlaps" in lib.dlsim_last_error()
    assert _tensors(offs=(0, 16)) == -1 and b"outputs of tensors" in lib.dlsim_last_error()
    assert _tensors(t=0, numels=(), offs=()) == 0
    assert _tensors(numels=(0, 0), out=0) == 0
