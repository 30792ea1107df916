"""The wide Gram distance entries (dlsim_gram_sqdist_wide, 33 to 128 models) without a GPU: argument
errors on made-up addresses, the geometry, the "wide" name, the Python errors that come before device
work, and the separation of the GPU plugin tests' inputs, as tests/test_gram_cpu.py."""
from __future__ import annotations

import ctypes
import types

import numpy as np
import pytest
import torch

import _gram_util as gu
import _krum_util as ku
from dasklearn_amd import _native
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M
from dasklearn_amd.gradient_aggregation.krum import Bulyan, Krum, MultiKrum, model_distances
from dasklearn_amd.model_manager import ModelManager

F32, F64 = _native.DLSIM_F32, _native.DLSIM_F64
E_DTYPE = -2  # include/dlsim.h DLSIM_E_DTYPE
A = 0x10000  # a made-up address; inputs of 64 fp32 elements, 0x1000 apart
WIDE_PLUGIN_CASES = [(33, 7), (49, 11), (64, 15), (65, 10), (97, 20), (128, 31), (128, 10)]  # (n, f)


def _flat(n=40, numel=64, dtype=F32, out=0x900000, acc=0, ptrs=None):
    ptrs = _native._ptr_array([A + 0x1000 * i for i in range(n)] if ptrs is None else ptrs)
    return _native.load().dlsim_gram_sqdist_wide(ptrs, n, numel, dtype, out, acc, None)


def _tensors(n=40, t=2, numels=(64, 8), dtype=F32, out=0x900000, acc=0, ptrs=None):
    ptrs = [A + 0x1000 * i for i in range(n * max(t, 0))] if ptrs is None else ptrs
    return _native.load().dlsim_gram_sqdist_wide_tensors(_native._ptr_array(ptrs), n, t, _native._size_array(numels),
                                                         dtype, out, acc, None)


def _geom(n=40, dtype=F32, numel=64, null=False):
    tile, blocks = ctypes.c_size_t(0), ctypes.c_uint(0)
    return _native.load().dlsim_gramwide_geometry(n, dtype, numel, None if null else ctypes.byref(tile),
                                                  ctypes.byref(blocks))


@pytest.mark.parametrize("call,rc", [
    (lambda: _flat(dtype=F64), "dtype"), (lambda: _flat(dtype=99), "dtype"), (lambda: _flat(n=0), "arg"),
    (lambda: _flat(n=129), "arg"), (lambda: _flat(acc=2), "arg"), (lambda: _flat(out=None), "arg"),
    (lambda: _flat(ptrs=[A] * 39 + [None]), "arg"), (lambda: _flat(out=A + 0x1000 + 8), "arg"),
    (lambda: _native.load().dlsim_gram_sqdist_wide(None, 40, 64, F32, 0x900000, 0, None), "arg"),
    (lambda: _tensors(dtype=F64), "dtype"), (lambda: _tensors(t=-1), "arg"), (lambda: _tensors(n=129), "arg"),
    (lambda: _tensors(acc=-1), "arg"), (lambda: _tensors(out=None), "arg"), (lambda: _tensors(out=A + 0x5000 + 16), "arg"),
    (lambda: _tensors(ptrs=[A] * 79 + [None]), "arg"),
    (lambda: _native.load().dlsim_gram_sqdist_wide_tensors(None, 40, 2, None, F32, 0x900000, 0, None), "arg"),
    (lambda: _geom(dtype=F64), "dtype"), (lambda: _geom(n=0), "arg"), (lambda: _geom(n=129), "arg"),
    (lambda: _geom(null=True), "arg")])
def test_argument_errors_come_before_any_hip_call(call, rc):
    assert call() == {"dtype": E_DTYPE, "arg": _native.DLSIM_E_ARG}[rc]
    assert _native.load().dlsim_last_error()


def test_fp64_is_refused_before_n_is_looked_at_and_the_narrow_entry_keeps_its_limit():
    assert _flat(n=999, dtype=F64) == E_DTYPE
    assert b"fp64" in _native.load().dlsim_last_error()
    ptrs = _native._ptr_array([A + 0x1000 * i for i in range(33)])
    assert _native.load().dlsim_gram_sqdist(ptrs, 33, 64, F32, 0x900000, 0, None) == _native.DLSIM_E_ARG


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_geometry_is_monotone_and_capped(dt):
    T, cap = _native.gramwide_geometry(128, dt, 10 ** 10)
    assert T == 64 and cap == 512
    for n in (33, 64, 65, 96, 97, 128):
        prev = 0
        for p in (0, 1, T, T + 1, 7 * T, cap * T - 1, cap * T, cap * T + 1, 10 ** 9):
            t, b = _native.gramwide_geometry(n, dt, p)
            assert t == T and b == min(cap, max(1, -(-p // T))) and b >= prev
            prev = b
    for n in (1, 17, 32):  # the narrow kernel serves these
        assert _native.gramwide_geometry(n, dt, 10 ** 6) == _native.gramdist_geometry(n, dt, 10 ** 6)


@pytest.mark.parametrize("method,extra,base", [(M.KRUM, {}, Krum), (M.MULTI_KRUM, {}, MultiKrum),
                                               (M.MULTI_KRUM, {"aggregation_krum_rule": "bulyan"}, Bulyan)])
def test_the_wide_name_is_accepted(method, extra, base):
    assert base.with_params(1, distance="wide").distance == "wide"
    s = types.SimpleNamespace(gradient_aggregation=method, aggregation_distance="wide", **extra)
    cls = ModelManager(None, s, 0).get_aggregation_method()
    assert issubclass(cls, base) and cls.distance == "wide"


def _linears(n, dtype=torch.float32):
    return [torch.nn.Linear(3, 2).to(dtype) for _ in range(n)]


def test_python_errors_come_before_device_work():
    """Host models and no GPU: anything past these errors would fail differently."""
    with pytest.raises(ValueError, match="n - 2f = 44.*at most 32"):
        Bulyan.with_params(10, distance="wide").aggregate(_linears(64))
    for call in (lambda ms: model_distances(ms, method="wide"), Krum.with_params(7, distance="wide").aggregate,
                 MultiKrum.with_params(7, distance="wide").aggregate):
        with pytest.raises(ValueError, match="no fp64"):
            call(_linears(33, torch.float64))
        with pytest.raises(ValueError, match="at most 128"):
            call(_linears(129))
    for cls in (Krum, MultiKrum, Bulyan):  # the other methods keep their limit
        for name in ("exact", "gram"):
            with pytest.raises(ValueError, match="at most 32"):
                cls.with_params(1, distance=name).aggregate(_linears(33))


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("n,f", WIDE_PLUGIN_CASES)
def test_plugin_inputs_are_separated_by_more_than_the_gram_bound(n, f, special):
    """test_gram_cpu.py's assertion: the ranked scores' gaps exceed 2 n times the largest entry bound."""
    rows, _, want, _ = ku.plugin_case(n, f, special=special)
    S, bad = gu.centred_sums(rows, "f32")
    worst = 2 * n * float(gu.entry_bounds(S[~bad], rows.shape[1]).max())
    scores = np.sort(np.array(ku.ref_scores(want.astype(np.float64), f)))
    finite = scores[np.isfinite(scores)]
    for m in (1, 2, n - f, n - 2 * f):
        if m < finite.size:
            assert scores[m] - scores[m - 1] > worst
