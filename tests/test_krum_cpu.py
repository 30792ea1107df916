"""Krum, Multi-Krum and the pairwise distance without a GPU: the longdouble
oracle (tests/_krum_util.py) against torch.cdist, the scoring and ranking
rule, the C entries' argument errors, the geometry diagnostic, the plugins'
errors, ModelManager's selection, and the separation of every input the GPU
selection tests use."""
from __future__ import annotations

import ctypes
import math
import types

import numpy as np
import pytest
import torch
from torch import nn

import _edge_util as eu
import _krum_util as ku
from dasklearn_amd import _native
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg
from dasklearn_amd.gradient_aggregation.krum import (Krum, MultiKrum, check_krum_params, krum_scores, krum_select,
                                                     model_distances)
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian
from dasklearn_amd.model_manager import ModelManager

INF, NAN = math.inf, math.nan


# ---- the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", (1, 2, 3, 8, 17, 32))
def test_oracle_against_cdist_squared(n, dtype):
    """Within bound(p) = (p + 8) * 2^-53 relative. torch.cdist(x, x)**2 in
    float64 is itself a double sum of the p terms, then a square root squared
    again: three more roundings, which the 8 units of slack cover; the
    oracle's own error (p * 2^-63) is negligible beside it."""
    p = 1237
    rows = eu.random_rows(dtype, n, p, seed=60 + n)
    want = ku.sqdist_oracle(rows, dtype)
    assert want.dtype == np.longdouble and want.shape == (n, n)
    x = torch.from_numpy(np.stack([eu.decode(r, dtype) for r in rows]))
    ref = (torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") ** 2).numpy()
    off = ~np.eye(n, dtype=bool)
    assert np.all(want.diagonal() == 0)
    if n > 1:
        rel = np.abs(ref[off] - want[off].astype(np.float64)) / want[off].astype(np.float64)
        print(f"n={n} {dtype}: max rel diff {rel.max():.3e}")
        assert rel.max() <= ku.bound(p)


def test_oracle_value_classes():
    rows = np.array([[1.0, 2.0, 3.0], [1.0, INF, 3.0], [NAN, 2.0, 3.0], [1.0, INF, 0.0], [1.0, -INF, 3.0]])
    c = ku.value_class(ku.sqdist_oracle(rows, "f64"))
    assert c[0, 1] == 1 and c[0, 2] == 2 and c[1, 2] == 2
    assert c[1, 3] == 2  # Inf - Inf
    assert c[1, 4] == 1  # +Inf against -Inf
    assert c[0, 0] == 0 and c[0, 4] == 1


# ---- scores and ranking ----------------------------------------------------------------
def _sym(n, entries, fill):
    d = [[0.0 if i == j else fill for j in range(n)] for i in range(n)]
    for (i, j), v in entries.items():
        d[i][j] = d[j][i] = v
    return d


def test_scores_on_a_hand_written_matrix():
    # n = 5, f = 1: the two smallest off-diagonal entries of every row
    d = _sym(5, {(0, 1): 1.0, (0, 2): 2.0, (1, 2): 1.0, (3, 4): 1.0}, 9.0)
    assert krum_scores(d, 1) == [3.0, 2.0, 3.0, 10.0, 10.0]
    assert krum_select(d, 1, 1) == [1]
    assert krum_select(d, 1, 2) == [0, 1]  # the tie of 0 and 2 goes to 0
    assert krum_select(d, 1, 3) == [0, 1, 2]
    assert krum_select(d, 1, 4) == [0, 1, 2, 3]  # 3 and 4 tie: 3
    # f = 0 sums three entries
    assert krum_scores(d, 0) == [12.0, 11.0, 12.0, 19.0, 19.0]
    assert ku.ref_scores(d, 1) == krum_scores(d, 1) and ku.ref_select(d, 1, 2) == [0, 1]


def test_the_sum_runs_in_ascending_order():
    # 1e16 + 1 + 1 loses both ones; 1 + 1 + 1e16 keeps them
    d = _sym(5, {(0, 1): 1e16, (0, 2): 1.0, (0, 3): 1.0}, 5e16)
    assert krum_scores(d, 0)[0] == (1.0 + 1.0) + 1e16 != (1e16 + 1.0) + 1.0


def test_non_finite_entries_count_as_inf():
    d = _sym(5, {(0, 1): 1.0, (0, 2): 2.0, (1, 2): 3.0}, 4.0)
    for bad in (NAN, INF, -INF):
        e = [row[:] for row in d]
        for j in range(4):
            e[4][j] = e[j][4] = bad
        s = krum_scores(e, 1)
        assert s[4] == INF and all(math.isfinite(v) for v in s[:4]), (bad, s)
        assert s[:4] == [3.0, 4.0, 5.0, 8.0]
        assert krum_select(e, 1, 4) == [0, 1, 2, 3]
        assert ku.ref_scores(e, 1) == s


def test_all_inf_rows_rank_by_index():
    d = _sym(5, {}, INF)
    assert krum_scores(d, 1) == [INF] * 5
    assert krum_select(d, 1, 1) == [0] and krum_select(d, 1, 3) == [0, 1, 2]
    # two finite peers only: each has one finite neighbour, needs two
    d = _sym(5, {(2, 3): 1.0}, NAN)
    assert krum_scores(d, 1) == [INF] * 5 and krum_select(d, 1, 2) == [0, 1]
    # f = 0 at n = 3 sums one entry
    d = _sym(3, {(1, 2): 1.0}, INF)
    assert krum_scores(d, 0) == [INF, 1.0, 1.0] and krum_select(d, 0, 1) == [1]
    assert ku.ref_select(d, 0, 1) == [1]


def test_restatement_agrees_on_random_matrices():
    rng = np.random.default_rng(3)
    for n, f in ((3, 0), (5, 1), (8, 2), (17, 3), (32, 8), (32, 14)):
        a = rng.integers(0, 6, size=(n, n)).astype(np.float64)  # many ties
        a = a + a.T
        a[rng.random((n, n)) < 0.1] = np.nan
        a = np.where(np.isnan(a) | np.isnan(a.T), np.nan, a)
        np.fill_diagonal(a, 0.0)
        assert krum_scores(a.tolist(), f) == ku.ref_scores(a, f)
        for m in (1, 2, n - f):
            assert krum_select(a.tolist(), f, m) == ku.ref_select(a, f, m), (n, f, m)


@pytest.mark.parametrize("n,f,m", [(2, 0, 1), (4, 1, 1), (6, 2, 1), (5, -1, 1), (5, 1, 0), (5, 1, 5), (5, 1, -1),
                                   (32, 15, 1), (3, 0, 4)])
def test_every_n_f_m_error(n, f, m):
    d = _sym(n, {}, 1.0)
    with pytest.raises(ValueError):
        krum_select(d, f, m)
    with pytest.raises(ValueError):
        check_krum_params(n, f, m)
    if not (f >= 0 and n >= 2 * f + 3):
        with pytest.raises(ValueError):
            krum_scores(d, f)


def test_edges_of_the_valid_range():
    for n, f, m in ((3, 0, 1), (3, 0, 3), (5, 1, 4), (32, 14, 18), (7, 2, 5)):
        check_krum_params(n, f, m)
        assert len(krum_select(_sym(n, {}, 1.0), f, m)) == m


# ---- the C entries --------------------------------------------------------------------
D2 = 1 << 20


def _flat(n=2, nelem=100, dtype=0, d2=D2, acc=0, ins=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (i + 1) for i in range(max(n, 1))]
    return lib.dlsim_pairwise_sqdist((ctypes.c_void_p * len(ins))(*ins), n, nelem, dtype, ctypes.c_void_p(d2), acc, None)


def test_flat_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _flat(n=0) == -1 and b"n must be" in lib.dlsim_last_error()
    assert _flat(n=33, ins=[4096] * 33) == -1 and b"<= 32" in lib.dlsim_last_error()
    assert _flat(dtype=7) == -2
    assert _flat(dtype=-1) == -2
    for acc in (2, -1):
        assert _flat(acc=acc) == -1 and b"accumulate" in lib.dlsim_last_error()
    assert _flat(d2=0) == -1 and b"null" in lib.dlsim_last_error()
    assert _flat(ins=[4096, 0]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_pairwise_sqdist(None, 2, 100, 0, ctypes.c_void_p(D2), 0, None) == -1
    # the matrix (n*n doubles = 32 bytes) on an input (fp32: 400 bytes)
    assert _flat(d2=4096) == -1 and b"overlaps input 0" in lib.dlsim_last_error()
    assert _flat(d2=8192 + 399) == -1 and b"overlaps input 1" in lib.dlsim_last_error()
    assert _flat(d2=4096 - 31) == -1
    assert _flat(d2=4096 - 31, dtype=3, nelem=1) == -1
    assert lib.dlsim_version() > 0  # none of them reached a HIP call: the next call still works


def _tensors(n=2, t=2, numels=(10, 20), dtype=0, d2=D2, acc=0, ins=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (q + 1) for q in range(max(n * t, 1))]
    sz = ctypes.c_size_t * max(len(numels), 1)
    return lib.dlsim_pairwise_sqdist_tensors((ctypes.c_void_p * len(ins))(*ins), n, t, sz(*numels), dtype,
                                             ctypes.c_void_p(d2), acc, None)


def test_tensors_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _tensors(t=-1) == -1
    assert _tensors(n=0) == -1
    assert _tensors(n=33) == -1 and b"<= 32" in lib.dlsim_last_error()
    assert _tensors(dtype=9) == -2
    assert _tensors(acc=3) == -1
    assert _tensors(d2=0) == -1
    assert _tensors(ins=[4096, 8192, 0, 16384]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_pairwise_sqdist_tensors(None, 2, 2, None, 0, ctypes.c_void_p(D2), 0, None) == -1
    # the matrix on tensor 1 of model 1 (the fourth pointer, 80 bytes)
    assert _tensors(d2=16384 + 79) == -1 and b"tensor 1" in lib.dlsim_last_error()


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_geometry_is_positive_and_needs_no_gpu(dtype):
    dt = eu.DTYPES[dtype]
    for n in (1, 2, 4, 5, 8, 9, 16, 17, 32):
        for numel in (0, 1, 1000, 10 ** 7, 10 ** 10):
            tile, blocks = _native.pairdist_geometry(n, dt, numel)
            assert tile == 256 * eu.VEC_ELEMS[dtype] and blocks >= 1
            assert blocks <= max(1, -(-numel // tile))
        # the cap: a function of n alone from some size on, and within 4 M elements of a tile each
        cap = _native.pairdist_geometry(n, dt, 10 ** 10)[1]
        assert cap == _native.pairdist_geometry(n, dt, 10 ** 11)[1]
        assert cap * tile <= 4 * 1024 * 1024
    lib = _native.load()
    t, b = ctypes.c_size_t(0), ctypes.c_uint(0)
    assert lib.dlsim_pairdist_geometry(0, 0, 10, ctypes.byref(t), ctypes.byref(b)) == -1
    assert lib.dlsim_pairdist_geometry(33, 0, 10, ctypes.byref(t), ctypes.byref(b)) == -1
    assert lib.dlsim_pairdist_geometry(2, 5, 10, ctypes.byref(t), ctypes.byref(b)) == -2
    assert lib.dlsim_pairdist_geometry(2, 0, 10, None, ctypes.byref(b)) == -1
    assert _native.MAX_PAIRDIST_INPUTS == 32


# ---- the plugins ------------------------------------------------------------------------
def _models(n):
    torch.manual_seed(n)
    return [nn.Linear(3, 2) for _ in range(n)]


@pytest.mark.parametrize("agg", [Krum, MultiKrum, Krum.with_params(2), MultiKrum.with_params(1, 2)])
def test_plugin_errors_come_before_any_device_work(agg):
    with pytest.raises(AssertionError):
        agg.aggregate(_models(7), [0.5, 0.5])
    with pytest.raises(ValueError, match="unweighted"):
        agg.aggregate(_models(3), [0.2, 0.3, 0.5])
    with pytest.raises(IndexError):
        agg.aggregate([], None)
    with pytest.raises(IndexError):
        agg.aggregate([], [])
    with pytest.raises(ValueError, match="at most 32"):
        agg.aggregate(_models(33), None)
    with pytest.raises(ValueError, match=r"n = 4 .*f = "):
        agg.aggregate(_models(4))  # n >= 2f + 3 fails for f = 1 and 2


def test_m_out_of_range_and_with_params():
    with pytest.raises(ValueError, match="m = 5"):
        MultiKrum.with_params(1, 5).aggregate(_models(5))  # m <= n - f = 4
    with pytest.raises(ValueError):
        MultiKrum.with_params(1, 0)
    with pytest.raises(ValueError):
        MultiKrum.with_params(-1)
    with pytest.raises(ValueError):
        Krum.with_params(-1)
    with pytest.raises(ValueError):
        Krum.with_params(1, 2)
    k = Krum.with_params(3)
    assert issubclass(k, Krum) and k.f == 3 and Krum.f == 1
    mk = MultiKrum.with_params(2, 4)
    assert issubclass(mk, MultiKrum) and (mk.f, mk.m) == (2, 4) and MultiKrum.m is None
    with pytest.raises(IndexError):
        model_distances([])
    with pytest.raises(ValueError, match="at most 32"):
        model_distances(_models(33))


def test_enum_values():
    assert GradientAggregationMethod.FEDAVG == 1
    assert GradientAggregationMethod.MEDIAN == 2
    assert GradientAggregationMethod.TRIMMED_MEAN == 3
    assert GradientAggregationMethod.KRUM == 4
    assert GradientAggregationMethod.MULTI_KRUM == 5


def test_model_manager_selects_krum_and_multi_krum():
    pick = lambda **kw: ModelManager(None, types.SimpleNamespace(**kw), 0).get_aggregation_method()  # noqa: E731
    k = pick(gradient_aggregation=4)
    assert issubclass(k, Krum) and k.f == 1
    k = pick(gradient_aggregation=GradientAggregationMethod.KRUM, aggregation_byzantine=3)
    assert issubclass(k, Krum) and k.f == 3
    mk = pick(gradient_aggregation=5)
    assert issubclass(mk, MultiKrum) and (mk.f, mk.m) == (1, None)
    mk = pick(gradient_aggregation=GradientAggregationMethod.MULTI_KRUM, aggregation_byzantine=2,
              aggregation_multi_krum_m=3)
    assert issubclass(mk, MultiKrum) and (mk.f, mk.m) == (2, 3)
    assert pick(gradient_aggregation=1) is FedAvg and pick() is FedAvg
    assert pick(gradient_aggregation=2) is CoordinateMedian
    assert pick(gradient_aggregation=99) is None
    # the settings reach the parameter check
    mm = ModelManager(None, types.SimpleNamespace(gradient_aggregation=5, aggregation_byzantine=2), 0)
    for i, m in enumerate(_models(6)):
        mm.process_incoming_trained_model(i, m)
    with pytest.raises(ValueError, match=r"n = 6 .*f = 2"):
        mm.aggregate_trained_models(None)


# ---- the generator --------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", ku.GPU_PLUGIN_CONFIGS)
def test_separation_of_every_gpu_selection_input(n, f):
    for special in (False, True):
        if special and f < 2:
            continue
        rows, byz, want, models = ku.plugin_case(n, f, special=special)
        assert len(byz) == f and len(models) == n
        for m in (1, 2, n - f):
            chosen = ku.ref_select(want.astype(np.float64), f, m)
            assert not set(chosen) & set(byz), "a Byzantine row among the oracle's selection"
    # the BatchNorm case of the GPU tests: model 0 is Byzantine
    _, byz, want, _ = ku.plugin_case(8, 2, shapes=([5, 7], [5], [5], [5]), byz=(0, 5))
    assert byz == [0, 5] and 0 not in ku.ref_select(want.astype(np.float64), 2, 1)
    ku.separated_models(8, 2, 85_354, "f32", seed=7, nan_row=True, inf_row=True)
    ku.plugin_case(9, 2)  # test_model_distances_on_every_route
