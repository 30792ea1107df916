"""dlsim_robust_reduce_batched, dlsim_robust_reduce_tensors_batched and
dlsim_robust_batch_geometry without a GPU: every argument error is decided
before any HIP call, so it is visible here; the geometry values; and what
aggregate_batch and RoundExecutor do with a method before they reach a device."""
from __future__ import annotations

import ctypes
import types

import pytest
import torch
from torch import nn

from dasklearn_amd import _native, batch, rounds
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M

VP, SZ, INT = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
BASE = 1 << 20  # addresses are only compared, never read: no launch follows an error


def _arr(ct, vals):
    return (ct * max(len(vals), 1))(*vals)


def batched(fan, ins, lo, hi, outs, numels, dtype=_native.DLSIM_F32, b=None):
    lib = _native.load()
    rc = lib.dlsim_robust_reduce_batched(len(fan) if b is None else b, _arr(INT, fan), _arr(VP, ins), _arr(INT, lo),
                                         _arr(INT, hi), _arr(VP, outs), _arr(SZ, numels), dtype, None)
    return rc, lib.dlsim_last_error().decode()


def tensors(ins, n, numels, offs, lo, hi, out, dtype=_native.DLSIM_F32, t=None):
    lib = _native.load()
    rc = lib.dlsim_robust_reduce_tensors_batched(_arr(VP, ins), n, len(numels) if t is None else t, _arr(SZ, numels),
                                                 _arr(SZ, offs), lo, hi, out, dtype, None)
    return rc, lib.dlsim_last_error().decode()


def two_tasks(out0=BASE + 0x10000, out1=BASE + 0x20000, p=100):
    """Two well-formed tasks of fan-in 2 and 3 over p fp32 elements; inputs 4 KiB apart. Every test
    below breaks one thing in them or leaves them empty: a call that passed every check would launch."""
    ins = [BASE + 0x1000 * i for i in range(5)]
    return dict(fan=[2, 3], ins=ins, lo=[0, 1], hi=[1, 2], outs=[out0, out1], numels=[p, p])


def test_counts_and_null_arrays():
    a = two_tasks()
    rc, msg = batched(**a, b=-1)
    assert rc == _native.DLSIM_E_ARG and "b must be >= 0 (got -1)" in msg
    assert batched([], [], [], [], [], [])[0] == 0  # b == 0 is a no-op
    lib = _native.load()
    good = [_arr(INT, a["fan"]), _arr(VP, a["ins"]), _arr(INT, a["lo"]), _arr(INT, a["hi"]), _arr(VP, a["outs"]),
            _arr(SZ, a["numels"])]
    for k in range(6):
        args = list(good)
        args[k] = None
        assert lib.dlsim_robust_reduce_batched(2, *args, 0, None) == _native.DLSIM_E_ARG
        assert b"null array argument" in lib.dlsim_last_error()
    rc, msg = batched(**a, dtype=9)
    assert rc == -2 and "unsupported dtype 9" in msg


@pytest.mark.parametrize("n,text", [(0, "task 1: n must be >= 1 (got 0)"), (33, "task 1: n must be <= 32 (got 33)")])
def test_fan_in_limits(n, text):
    ins = [BASE + 0x1000 * i for i in range(2 + n)]
    rc, msg = batched([2, n], ins, [0, 0], [1, 1], [BASE + 0x100000, BASE + 0x200000], [10, 10])
    assert rc == _native.DLSIM_E_ARG and text in msg
    if n == 33:
        assert "sorting network" in msg


@pytest.mark.parametrize("lo,hi", [(-1, 1), (1, 1), (2, 1), (0, 4), (3, 4)])
def test_bad_windows(lo, hi):
    a = two_tasks()
    a["lo"][1], a["hi"][1] = lo, hi
    rc, msg = batched(**a)
    assert rc == _native.DLSIM_E_ARG
    assert f"task 1: the window must satisfy 0 <= lo < hi <= n (got lo {lo}, hi {hi}, n 3)" in msg


def test_null_pointers_and_empty_tasks():
    a = two_tasks(out1=0)
    rc, msg = batched(**a)
    assert rc == _native.DLSIM_E_ARG and "task 1: null output pointer" in msg
    a = two_tasks()
    a["ins"][3] = 0
    rc, msg = batched(**a)
    assert rc == _native.DLSIM_E_ARG and "task 1: null input pointer at index 1" in msg
    # empty tasks are never read or written: any pointer will do, and a list of them launches nothing
    a = two_tasks(out0=0, out1=0)
    a["numels"] = [0, 0]
    a["ins"] = [0] * 5
    assert batched(**a) == (0, "")


def test_output_on_own_input():
    p = 100
    for out in (BASE + 0x1000, BASE + 0x1000 + 4 * p - 1, BASE + 0x1000 - 4 * p + 1):  # exact, one byte at either end
        rc, msg = batched(**two_tasks(out0=out, p=p))
        assert rc == _native.DLSIM_E_ARG and "task 0: output overlaps input 1" in msg, (out, msg)
    # one byte further on either side task 0 passes: the verdict is then task 1's (a bad window there, so
    # that no launch follows: these addresses are not memory)
    for out in (BASE + 0x1000 + 4 * p, BASE + 0x1000 - 4 * p):
        a = two_tasks(out0=out, p=p)
        a["ins"][0] = BASE + 0x8000  # (keeps input 0 off the moved output)
        a["hi"][1] = 9
        rc, msg = batched(**a)
        assert rc == _native.DLSIM_E_ARG and msg.startswith("task 1: the window"), msg


def test_output_on_another_tasks_input_or_output():
    p = 100
    # task 0's output on task 1's input 2 (at BASE + 0x4000), one shared byte at either end
    for out in (BASE + 0x4000, BASE + 0x4000 + 4 * p - 1, BASE + 0x4000 - 4 * p + 1):
        rc, msg = batched(**two_tasks(out0=out, p=p))
        assert rc == _native.DLSIM_E_ARG and "overlaps another task's input or output" in msg, (out, msg)
    # output on output: the same range, and one shared byte
    for out1 in (BASE + 0x10000, BASE + 0x10000 + 4 * p - 1):
        rc, msg = batched(**two_tasks(out1=out1, p=p))
        assert rc == _native.DLSIM_E_ARG and "overlaps another task's input or output" in msg, (out1, msg)


def test_tensors_entry_argument_errors():
    n, numels, offs = 2, [10, 0, 6], [0, 40, 40]
    ins = [BASE + 0x1000 * i for i in range(6)]
    out = BASE + 0x100000
    assert tensors(ins, n, numels, offs, 0, 1, out, t=-1) == (_native.DLSIM_E_ARG, "t must be >= 0 (got -1)")
    assert tensors([], n, [], [], 0, 1, out)[0] == 0  # t == 0
    rc, msg = tensors(ins, 0, numels, offs, 0, 1, out)
    assert rc == _native.DLSIM_E_ARG and "n must be >= 1" in msg
    rc, msg = tensors(ins * 17, 33, numels, offs, 0, 1, out)
    assert rc == _native.DLSIM_E_ARG and "n must be <= 32 (got 33)" in msg
    rc, msg = tensors(ins, n, numels, offs, 1, 1, out)
    assert rc == _native.DLSIM_E_ARG and "the window must satisfy" in msg
    assert tensors(ins, n, numels, offs, 0, 1, out, dtype=7)[0] == -2
    lib = _native.load()
    assert lib.dlsim_robust_reduce_tensors_batched(None, n, 3, _arr(SZ, numels), _arr(SZ, offs), 0, 1, out, 0,
                                                   None) == _native.DLSIM_E_ARG
    rc, msg = tensors(ins, n, numels, offs, 0, 1, 0)
    assert rc == _native.DLSIM_E_ARG and "null output pointer" in msg
    # tensor 2's output (out + 40) on an input of tensor 0: the old entry's message
    bad = list(ins)
    bad[3] = out + 40 + 23  # model 1, tensor 0: ten elements from here; one byte shared
    rc, msg = tensors(bad, n, numels, offs, 0, 1, out)
    assert rc == _native.DLSIM_E_ARG and "output of tensor 2, inputs of tensor 0: output overlaps input 1" in msg
    rc, msg = tensors(ins, n, numels, [0, 40, 39], 0, 1, out)
    assert rc == _native.DLSIM_E_ARG and "outputs of tensors 0 and 2 overlap" in msg
    # the same lists through the existing entry: the same verdicts
    old = lib.dlsim_robust_reduce_tensors
    assert old(_arr(VP, bad), n, 3, _arr(SZ, numels), _arr(SZ, offs), 0, 1, out, 0, None) == _native.DLSIM_E_ARG
    assert tensors(ins, n, [0, 0, 0], offs, 0, 1, 0) == (0, "")


GEOMETRY = {  # elements of one full tile: kBlock * VPT vectors (VPT 4, 2, 1), kBlock 8-byte units at capacity 32
    torch.float32: {4: 4096, 8: 2048, 16: 1024, 32: 512},
    torch.float64: {4: 2048, 8: 1024, 16: 512, 32: 256},
    torch.bfloat16: {4: 8192, 8: 4096, 16: 2048, 32: 1024},
    torch.float16: {4: 8192, 8: 4096, 16: 2048, 32: 1024},
}


@pytest.mark.parametrize("dt", sorted(GEOMETRY, key=str))
def test_geometry(dt):
    for n in range(1, 33):
        cap = 4 if n <= 4 else 8 if n <= 8 else 16 if n <= 16 else 32
        assert _native.robust_batch_geometry(n, dt) == (GEOMETRY[dt][cap], 32, 192), (n, dt)
    for n in (0, 33):
        with pytest.raises(_native.DlsimError) as e:
            _native.robust_batch_geometry(n, dt)
        assert e.value.rc == _native.DLSIM_E_ARG
    lib = _native.load()
    assert lib.dlsim_robust_batch_geometry(4, 0, None, None, None) == _native.DLSIM_E_ARG
    assert lib.dlsim_robust_batch_geometry(4, 11, None, None, None) == -2


def test_python_wrapper_checks():
    x = torch.zeros(8)
    with pytest.raises(ValueError, match="device tensors"):
        _native.robust_reduce_batched([([x, x], 0, 1, torch.zeros(8))])
    with pytest.raises(IndexError):
        _native.robust_reduce_batched([([], 0, 1, x)])
    with pytest.raises(ValueError, match="at most 32"):
        _native.robust_reduce_batched([([x] * 33, 0, 1, torch.zeros(8))])
    assert _native.robust_reduce_batched([]) == []


# ---- aggregate_batch and RoundExecutor: what is decided before a device is touched ----
def _net(seed=0, width=3):
    torch.manual_seed(seed)
    return nn.Linear(width, 2)


@pytest.mark.parametrize("method", [M.MEDIAN, M.TRIMMED_MEAN])
def test_aggregate_batch_exceptions_on_host_models(method):
    ms = [_net(i) for i in range(3)]
    with pytest.raises(AssertionError):
        batch.aggregate_batch([(ms, [0.5, 0.5])], method=method)
    with pytest.raises(ValueError, match="is unweighted"):
        batch.aggregate_batch([(ms, [0.2, 0.3, 0.5])], method=method)
    with pytest.raises(IndexError):
        batch.aggregate_batch([([], None)], method=method)
    with pytest.raises(ValueError, match="at most 32 models"):
        batch.aggregate_batch([([ms[0]] * 33, None), (ms, None)], method=method)
    with pytest.raises(ValueError):  # parameter lists differ
        batch.aggregate_batch([([ms[0], _net(1, width=4)], None)], method=method)


def test_aggregate_batch_trim_comes_from_settings():
    ms = [_net(i) for i in range(4)]
    with pytest.raises(ValueError, match="trim = 2"):
        batch.aggregate_batch([(ms, None)], method=M.TRIMMED_MEAN, settings=types.SimpleNamespace(aggregation_trim=2))
    with pytest.raises(ValueError, match="trim = 1"):  # the default, as ModelManager's
        batch.aggregate_batch([(ms[:2], None)], method=M.TRIMMED_MEAN)
    with pytest.raises(ValueError, match="trim must be >= 0"):
        batch.aggregate_batch([(ms, None)], method=M.TRIMMED_MEAN, settings=types.SimpleNamespace(aggregation_trim=-1))
    assert batch.method_window(M.TRIMMED_MEAN, types.SimpleNamespace(aggregation_trim=3))(9) == (3, 6)
    assert batch.method_window(M.MEDIAN, None)(8) == (3, 4)
    assert all(batch.method_window(m, None) is None for m in (M.FEDAVG, M.KRUM, M.MULTI_KRUM, M.GEOMETRIC_MEDIAN,
                                                              M.CENTERED_CLIP, 99))


def test_method_plugin_follows_model_manager():
    s = types.SimpleNamespace(aggregation_trim=2, aggregation_byzantine=2, gradient_aggregation=M.FEDAVG)
    assert batch.method_plugin(M.TRIMMED_MEAN, s).trim == 2
    assert batch.method_plugin(M.MEDIAN, None).__name__ == "CoordinateMedian"
    assert batch.method_plugin(M.KRUM, s).__mro__[1].__name__ == "Krum"
    assert batch.method_plugin(99, s) is None
    with pytest.raises(AttributeError):  # an unknown method fails as functions.aggregate fails
        batch.aggregate_batch([([_net()], None)], method=99)
    assert batch.aggregate_batch([], method=M.MEDIAN) == []


def _executor(method, monkeypatch, **settings):
    """A RoundExecutor whose three ways out of _aggregate_wave are recorded
    instead of run: (the FedAvg launches, the batched order statistics, a plugin)."""
    seen = []
    ex = rounds.RoundExecutor({}, types.SimpleNamespace(gradient_aggregation=method, **settings))
    monkeypatch.setattr(rounds, "aggregate_arena_tasks", lambda prepared, mode, cb=None: seen.append("fedavg") or [])
    monkeypatch.setattr(rounds, "robust_arena_tasks",
                        lambda prepared, window, cb=None: seen.append(("window", window(9))) or [])
    monkeypatch.setattr(ex, "_upload_host_models", lambda *a: None)
    monkeypatch.setattr(ex, "_arena_of", lambda *a: pytest.fail("no model is resolved in this test"))
    return ex, seen


@pytest.mark.parametrize("method,expect", [(M.FEDAVG, "fedavg"), (M.MEDIAN, ("window", (4, 5))),
                                           (M.TRIMMED_MEAN, ("window", (2, 7)))])
def test_round_executor_picks_the_batched_path(method, expect, monkeypatch):
    ex, seen = _executor(method, monkeypatch, aggregation_trim=2)
    assert ex._aggregate_wave([]) == []
    assert seen == [expect]


def test_round_executor_without_the_setting_is_fedavg(monkeypatch):
    ex, seen = _executor(M.FEDAVG, monkeypatch)
    del ex.settings.gradient_aggregation
    ex._aggregate_wave([])
    assert seen == ["fedavg"]


@pytest.mark.parametrize("method", [M.KRUM, M.MULTI_KRUM, M.GEOMETRIC_MEDIAN, M.CENTERED_CLIP])
def test_round_executor_runs_the_plugin_per_task(method, monkeypatch):
    ex, seen = _executor(method, monkeypatch)
    calls = []

    class Plugin:
        @staticmethod
        def aggregate(models, weights=None, to_host=None):
            calls.append((models, weights, to_host))
            return "out"
    monkeypatch.setattr(rounds.ModelManager, "get_aggregation_method", lambda self: Plugin)
    a, b = _net(0), _net(1)
    outs = ex._aggregate_wave([("t0", "aggregate", {"models": [a, b]}),
                               ("t1", "aggregate", {"models": [b], "weights": [1.0]})])
    assert outs == ["out", "out"] and seen == []
    assert calls == [([a, b], None, False), ([b], [1.0], False)]


def test_round_executor_unknown_method_and_weights_fail_as_the_plugins(monkeypatch):
    ex, _ = _executor(99, monkeypatch)
    with pytest.raises(AttributeError):
        ex._aggregate_wave([("t0", "aggregate", {"models": [_net()]})])
    ex, seen = _executor(M.MEDIAN, monkeypatch)
    ms = [_net(i) for i in range(3)]
    with pytest.raises(ValueError, match="CoordinateMedian is unweighted"):
        ex._aggregate_wave([("t0", "aggregate", {"models": ms, "weights": [0.2, 0.3, 0.5]})])
    with pytest.raises(AssertionError):
        ex._aggregate_wave([("t0", "aggregate", {"models": ms, "weights": [1.0]})])
    ex, seen = _executor(M.TRIMMED_MEAN, monkeypatch)
    with pytest.raises(ValueError, match="TrimmedMean is unweighted"):
        ex._aggregate_wave([("t0", "aggregate", {"models": ms, "weights": [0.2, 0.3, 0.5]})])
    with pytest.raises(ValueError, match="n = 2 models with trim = 1"):
        ex._aggregate_wave([("t0", "aggregate", {"models": ms[:2]})])
    assert seen == []
