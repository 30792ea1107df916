"""The wide order-statistic entries (dlsim_robust_reduce_wide, 33 to 128 models) without a GPU:
argument errors on made-up addresses, the geometry classes, the "wide" sort's names and the Python
errors that come before device work."""
from __future__ import annotations

import ctypes
import types

import pytest
import torch

from dasklearn_amd import _native, batch
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian, TrimmedMean
from dasklearn_amd.model_manager import ModelManager

F32 = _native.DLSIM_F32
A = 0x10000  # a made-up address; inputs of 64 fp32 elements, 0x1000 apart


def _flat(n=40, lo=3, hi=37, numel=64, dtype=F32, out=0x900000, ptrs=None):
    ptrs = _native._ptr_array([A + 0x1000 * i for i in range(n)] if ptrs is None else ptrs)
    return _native.load().dlsim_robust_reduce_wide(ptrs, n, lo, hi, out, numel, dtype, None)


def _tensors(n=40, t=2, lo=3, hi=37, numels=(64, 8), offs=(0, 256), dtype=F32, out=0x900000, ptrs=None):
    ptrs = [A + 0x1000 * i for i in range(n * max(t, 0))] if ptrs is None else ptrs
    return _native.load().dlsim_robust_reduce_wide_tensors(_native._ptr_array(ptrs), n, t, _native._size_array(numels),
                                                           _native._size_array(offs), lo, hi, out, dtype, None)


def _geom(n=40, dtype=F32, null=False):
    tile, lanes = ctypes.c_size_t(0), ctypes.c_int(0)
    return _native.load().dlsim_robust_wide_geometry(n, dtype, None if null else ctypes.byref(tile), ctypes.byref(lanes))


@pytest.mark.parametrize("call,rc", [
    (lambda: _flat(dtype=99), -2), (lambda: _flat(n=0), -1), (lambda: _flat(n=129, hi=100), -1),
    (lambda: _flat(lo=5, hi=5), -1), (lambda: _flat(hi=41), -1), (lambda: _flat(lo=-1), -1),
    (lambda: _flat(out=None), -1), (lambda: _flat(ptrs=[A] * 39 + [None]), -1), (lambda: _flat(out=A + 0x1000 + 8), -1),
    (lambda: _flat(out=A + 39 * 0x1000), -1),
    (lambda: _native.load().dlsim_robust_reduce_wide(None, 40, 3, 37, 0x900000, 64, F32, None), -1),
    (lambda: _tensors(dtype=99), -2), (lambda: _tensors(t=-1), -1), (lambda: _tensors(n=0), -1),
    (lambda: _tensors(n=129), -1), (lambda: _tensors(lo=37, hi=37), -1), (lambda: _tensors(out=None), -1),
    (lambda: _tensors(out=A + 0x5000 + 16), -1), (lambda: _tensors(offs=(0, 128)), -1),
    (lambda: _tensors(ptrs=[A] * 79 + [None]), -1),
    (lambda: _native.load().dlsim_robust_reduce_wide_tensors(None, 40, 2, None, None, 3, 37, 0x900000, F32, None), -1),
    (lambda: _geom(dtype=99), -2), (lambda: _geom(n=0), -1), (lambda: _geom(n=129), -1), (lambda: _geom(null=True), -1)])
def test_argument_errors_come_before_any_hip_call(call, rc):
    assert call() == rc
    assert _native.load().dlsim_last_error()


def test_the_limits_in_words_and_the_noops():
    assert _flat(n=129, hi=100) == _native.DLSIM_E_ARG
    assert b"n must be <= 128 (got 129)" in _native.load().dlsim_last_error()
    ptrs = _native._ptr_array([A + 0x1000 * i for i in range(33)])
    assert _native.load().dlsim_robust_reduce(ptrs, 33, 3, 30, 0x900000, 64, F32, None) == _native.DLSIM_E_ARG
    assert b"n must be <= 32 (got 33)" in _native.load().dlsim_last_error()
    assert _flat(numel=0, out=None) == 0 and _tensors(t=0, out=None) == 0 and _tensors(numels=(0, 0), out=None) == 0
    with pytest.raises(ValueError, match="at most 128 models \\(got 129\\)"):
        _native.check_robust_wide_fan_in(129)
    _native.check_robust_wide_fan_in(128)


@pytest.mark.parametrize("dt,unit", [(torch.float32, 2), (torch.float64, 1), (torch.bfloat16, 4), (torch.float16, 4)])
def test_geometry_classes(dt, unit):
    """Lanes per element 1 / 2 / 4; the tile is one 8-byte unit per group of a 256-lane block."""
    got = [_native.robust_wide_geometry(n, dt) for n in (1, 32, 33, 64, 65, 128)]
    assert [g for _, g in got] == [1, 1, 2, 2, 4, 4]
    assert [t for t, _ in got] == [8 * unit * 256, unit * 256, unit * 128, unit * 128, unit * 64, unit * 64]


def _linears(n):
    return [torch.nn.Linear(3, 2) for _ in range(n)]


def test_settings_names_and_python_errors_before_device_work():
    """Host models and no GPU: anything past these errors would fail differently."""
    def plugin(**kw):
        return ModelManager(None, types.SimpleNamespace(**kw), 0).get_aggregation_method()
    assert plugin(gradient_aggregation=M.MEDIAN) is CoordinateMedian
    assert plugin(gradient_aggregation=M.MEDIAN, aggregation_sort="wide").sort == "wide"
    tm = plugin(gradient_aggregation=M.TRIMMED_MEAN, aggregation_sort="wide", aggregation_trim=4)
    assert issubclass(tm, TrimmedMean) and (tm.sort, tm.trim) == ("wide", 4)
    assert TrimmedMean.with_trim(2).sort == "register" and TrimmedMean.with_trim(2).__name__ == "TrimmedMean2"
    for method in (M.MEDIAN, M.TRIMMED_MEAN):
        with pytest.raises(ValueError, match="aggregation_sort must be one of"):
            plugin(gradient_aggregation=method, aggregation_sort="bogus")
        wide = types.SimpleNamespace(aggregation_sort="wide")
        assert batch.method_window(method, wide) is None and batch.method_window(method, None) is not None
    with pytest.raises(ValueError, match="aggregation_sort.*aggregation_trim_rule"):
        plugin(gradient_aggregation=M.TRIMMED_MEAN, aggregation_sort="wide", aggregation_trim_rule="median")
    with pytest.raises(ValueError, match="sort must be one of"):
        CoordinateMedian.with_sort("bogus")
    for agg in (CoordinateMedian, TrimmedMean, TrimmedMean.with_trim(3)):  # the default keeps its limit
        with pytest.raises(ValueError, match="at most 32"):
            agg.aggregate(_linears(33))
    for agg in (CoordinateMedian.with_sort("wide"), TrimmedMean.with_trim(3, sort="wide")):
        with pytest.raises(ValueError, match="at most 128"):
            agg.aggregate(_linears(129))
    with pytest.raises(ValueError, match="at most 128"):
        CoordinateMedian.aggregate(_linears(129), sort="wide")
