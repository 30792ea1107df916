"""The order-statistic aggregators without a GPU: the CPU oracle
(tests/_robust_util.py) against torch, the C entries' argument errors, the
plugins' errors and ModelManager's selection."""
from __future__ import annotations

import ctypes
import types

import numpy as np
import pytest
import torch
from torch import nn

import _robust_util as ru
from dasklearn_amd import _native
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian, TrimmedMean
from dasklearn_amd.model_manager import ModelManager

FAN_INS = (1, 2, 3, 4, 5, 8, 17, 32)
P = 20_011


def _rows_without_overflow(dtype, n, p, seed):
    """random_rows, the largest finite value replaced by an ordinary one: the
    sum of finite window values then stays finite in every order."""
    rows = ru.random_rows(dtype, n, p, seed)
    sp = ru.special_bits(dtype)
    out = []
    for r in rows:
        b = ru.bits_of(r)
        b[(b == sp[10]) | (b == sp[11])] = sp[8]
        out.append(ru.from_bits(b, dtype))
    return out


def _same_value(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Both NaN, or == (so zeros of either sign are equal)."""
    return bool((((a != a) & (b != b)) | (a == b)).all())


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("n", FAN_INS)
def test_median_is_the_sorted_middle_by_value(n, dtype):
    dt = ru.DTYPES[dtype]
    xs = ru.random_rows(dt, n, P, seed=100 + n)
    got = ru.median(xs)
    want = torch.sort(torch.stack(xs).to(torch.float64), 0).values[(n - 1) // 2].to(dt)
    assert _same_value(got, want)
    # bit-identical to one of the inputs wherever the result is not NaN
    b = np.stack([ru.bits_of(x) for x in xs])
    g = ru.bits_of(got)
    ok = (b == g[None, :]).any(axis=0) | np.isnan(got.to(torch.float64).numpy())
    assert ok.all()


@pytest.mark.parametrize("n", FAN_INS)
def test_median_equals_torch_median_without_nans(n):
    xs = [torch.nan_to_num(x, nan=0.25) for x in ru.random_rows(torch.float32, n, P, seed=200 + n)]
    got = ru.median(xs)
    assert _same_value(got, torch.median(torch.stack(xs), 0).values)


def test_one_nan_of_four_is_not_selected_unlike_torch_median():
    """The documented difference: torch.median propagates any NaN."""
    xs = [torch.tensor([v], dtype=torch.float32) for v in (3.0, float("nan"), 1.0, 2.0)]
    assert torch.isnan(torch.median(torch.stack(xs), 0).values).all()
    assert ru.median(xs).item() == 2.0
    assert ru.trimmed_mean(xs, 1).item() == 2.5
    # three NaNs of four: the lower median (position 1) is a NaN, canonical
    ys = [torch.tensor([v], dtype=torch.float32) for v in (float("nan"), -float("nan"), 1.0, float("nan"))]
    assert ru.bits_of(ru.median(ys))[0] == 0x7FC00000


def test_zero_signs_are_ordered_and_a_lone_negative_zero_survives():
    xs = [torch.tensor([v], dtype=torch.float32) for v in (0.0, -0.0, 0.0)]
    s = ru.sorted_bits(xs, torch.float32)[:, 0]
    assert list(s) == [0x80000000, 0, 0]
    assert ru.bits_of(ru.window_mean(xs, 0, 1))[0] == 0x80000000  # -0.0 / 1
    assert ru.bits_of(ru.window_mean(xs, 0, 2))[0] == 0  # -0.0 + 0.0


@pytest.mark.parametrize("n,b", [(3, 1), (4, 1), (5, 0), (8, 2), (8, 3), (17, 4), (32, 7), (32, 15), (32, 0)])
def test_trimmed_mean_against_torch_sort_mean(n, b):
    """Against torch.sort(stack, 0).values[b:n-b].mean(0) in fp32.

    Non-finite results must agree exactly: a window with a NaN, or with both
    infinities, is NaN in every summation order, one with an infinity of one
    sign is that infinity (the inputs hold no finite value whose sums
    overflow). Finite results: both sides add the same m = n - 2b fp32 values,
    in two orders. The standard bound for a sum of m floats in any order is
    |err| <= (m - 1) u sum|s_j| to first order, u = 2^-24, so two orders differ
    by at most 2 (m - 1) u sum|s_j|; after the division by m that is
    2 (m - 1) 2^-24 mean|s_j|, and the two roundings of the quotients add at
    most one ulp of the result."""
    m = n - 2 * b
    xs = _rows_without_overflow(torch.float32, n, P, seed=300 + 40 * n + b)
    got = ru.trimmed_mean(xs, b)
    s = torch.sort(torch.stack(xs), 0).values[b:n - b]
    want = s.mean(0)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])
    mean_abs = s.abs().to(torch.float64).mean(0)[fin]
    ulp = torch.from_numpy(np.spacing(np.abs(want[fin].numpy()))).to(torch.float64)
    bound = 2 * (m - 1) * 2.0 ** -24 * mean_abs + ulp
    err = (got[fin].to(torch.float64) - want[fin].to(torch.float64)).abs()
    print(f"n={n} b={b}: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


def test_sixteen_bit_results_round_once():
    """bf16: 1 + 2^-8 + 2^-8 is 1 + 2^-7 in fp32 (exactly a bf16 value), but
    rounding each partial sum to bf16 would lose both small terms."""
    one, tiny = 1.0, 2.0 ** -8
    xs = [torch.tensor([v], dtype=torch.bfloat16) for v in (tiny, one * 3, tiny)]
    # sorted: tiny, tiny, 3; window [0, 3): (tiny + tiny + 3) / 3 in fp32, rounded once
    want = torch.tensor([(np.float32(tiny) + np.float32(tiny) + np.float32(3.0)) / np.float32(3.0)]).to(torch.bfloat16)
    assert ru.same_bits(ru.window_mean(xs, 0, 3), want)


# ---- the C entries ----------------------------------------------------------------
def _flat(n=2, lo=0, hi=1, dtype=0, out=1 << 20, nelem=100, ins=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (i + 1) for i in range(max(n, 1))]
    return lib.dlsim_robust_reduce((ctypes.c_void_p * len(ins))(*ins), n, lo, hi, ctypes.c_void_p(out), nelem, dtype,
                                   None)


def test_flat_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _flat(n=0) == -1 and b"n must be" in lib.dlsim_last_error()
    assert _flat(n=33, hi=33, ins=[4096] * 33) == -1 and b"<= 32" in lib.dlsim_last_error()
    for lo, hi in ((-1, 1), (1, 1), (2, 1), (0, 3)):
        assert _flat(n=2, lo=lo, hi=hi) == -1 and b"window" in lib.dlsim_last_error()
    assert _flat(dtype=7) == -2
    assert _flat(out=0) == -1
    assert _flat(ins=[4096, 0]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_robust_reduce(None, 2, 0, 1, ctypes.c_void_p(64), 100, 0, None) == -1
    # any overlap, exact aliasing included (fp32: 400 bytes per buffer)
    assert _flat(out=4096) == -1 and b"overlap" in lib.dlsim_last_error()
    assert _flat(out=8192 + 396) == -1 and b"overlaps input 1" in lib.dlsim_last_error()
    assert _flat(out=4096 - 396) == -1
    # zero elements: a no-op, whatever the pointers
    assert _flat(nelem=0, out=0) == 0
    for dt in range(4):
        assert _flat(nelem=0, dtype=dt) == 0


def _tensors(n=2, t=2, numels=(10, 20), offs=(0, 64), lo=0, hi=1, out=1 << 20, dtype=0, ins=None):
    lib = _native.load()
    ins = ins if ins is not None else [4096 * (q + 1) for q in range(max(n * t, 1))]
    sz = ctypes.c_size_t * max(len(numels), 1)
    return lib.dlsim_robust_reduce_tensors((ctypes.c_void_p * len(ins))(*ins), n, t, sz(*numels), sz(*offs), lo, hi,
                                           ctypes.c_void_p(out), dtype, None)


def test_tensors_entry_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _tensors(t=-1) == -1
    assert _tensors(n=0) == -1
    assert _tensors(n=33, hi=2) == -1 and b"<= 32" in lib.dlsim_last_error()
    assert _tensors(lo=1, hi=1) == -1
    assert _tensors(dtype=9) == -2
    assert _tensors(out=0) == -1
    assert _tensors(ins=[4096, 8192, 0, 16384]) == -1 and b"null input" in lib.dlsim_last_error()
    assert lib.dlsim_robust_reduce_tensors(None, 2, 2, None, None, 0, 1, ctypes.c_void_p(64), 0, None) == -1
    # the output of tensor 1 on an input of tensor 0; two outputs on each other
    assert _tensors(out=4096 - 64) == -1 and b"overlaps" in lib.dlsim_last_error()
    assert _tensors(offs=(0, 16)) == -1 and b"outputs of tensors" in lib.dlsim_last_error()
    # nothing to do
    assert _tensors(t=0, numels=(), offs=()) == 0
    assert _tensors(numels=(0, 0), out=0) == 0


# ---- the plugins ----------------------------------------------------------------------
def _models(n):
    torch.manual_seed(n)
    return [nn.Linear(3, 2) for _ in range(n)]


@pytest.mark.parametrize("agg", [CoordinateMedian, TrimmedMean, TrimmedMean.with_trim(2)])
def test_plugin_errors_come_before_any_device_work(agg):
    with pytest.raises(AssertionError):
        agg.aggregate(_models(3), [0.5, 0.5])
    with pytest.raises(ValueError, match="unweighted"):
        agg.aggregate(_models(3), [0.2, 0.3, 0.5])
    with pytest.raises(IndexError):
        agg.aggregate([], None)
    with pytest.raises(IndexError):
        agg.aggregate([], [])
    with pytest.raises(ValueError, match="at most 32"):
        agg.aggregate(_models(33), None)


def test_trim_too_large_names_n_and_the_trim():
    with pytest.raises(ValueError, match=r"n = 4 .*trim = 2"):
        TrimmedMean.aggregate(_models(4), None, trim=2)
    with pytest.raises(ValueError, match=r"n = 2 .*trim = 1"):
        TrimmedMean.aggregate(_models(2))  # the default trim of 1 leaves nothing of two
    with pytest.raises(ValueError, match="trim = -1"):
        TrimmedMean.aggregate(_models(4), None, trim=-1)
    with pytest.raises(ValueError):
        TrimmedMean.with_trim(-1)


def test_enum_values():
    assert GradientAggregationMethod.FEDAVG == 1
    assert GradientAggregationMethod.MEDIAN == 2
    assert GradientAggregationMethod.TRIMMED_MEAN == 3


def test_model_manager_selects_the_new_methods():
    pick = lambda **kw: ModelManager(None, types.SimpleNamespace(**kw), 0).get_aggregation_method()  # noqa: E731
    assert pick(gradient_aggregation=1) is FedAvg
    assert pick() is FedAvg
    assert pick(gradient_aggregation=2) is CoordinateMedian
    assert pick(gradient_aggregation=GradientAggregationMethod.MEDIAN) is CoordinateMedian
    tm = pick(gradient_aggregation=3)
    assert issubclass(tm, TrimmedMean) and tm.trim == 1
    tm = pick(gradient_aggregation=3, aggregation_trim=3)
    assert issubclass(tm, TrimmedMean) and tm.trim == 3
    assert pick(gradient_aggregation=99) is None
    # the trim from the settings reaches the window check
    mm = ModelManager(None, types.SimpleNamespace(gradient_aggregation=3, aggregation_trim=2), 0)
    for i, m in enumerate(_models(4)):
        mm.process_incoming_trained_model(i, m)
    with pytest.raises(ValueError, match=r"n = 4 .*trim = 2"):
        mm.aggregate_trained_models(None)
