"""The batched pairwise-distance entry and the batched Krum / Multi-Krum route
without a GPU: every argument error of dlsim_pairwise_sqdist_batched with its
code and before any HIP call, the launch-limit diagnostic, the Python
wrapper's checks, the exceptions of aggregate_batch(method=KRUM / MULTI_KRUM)
on host models, and RoundExecutor's choice of the batched route."""
from __future__ import annotations

import ctypes
import types

import pytest
import torch
from torch import nn

import _edge_util as eu
from dasklearn_amd import _native, batch, model_inputs, rounds
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M
from dasklearn_amd.gradient_aggregation.krum import Krum, MultiKrum, model_distances_batch
from dasklearn_amd.wave_tasks import ArenaTask

D2 = 1 << 20  # far from every input below


def _batched(fan=(2,), nts=(1,), ins=None, numels=None, dtype=0, d2s=None, acc=0, b=None):
    """dlsim_pairwise_sqdist_batched on made-up addresses: inputs 4096 apart
    from 4096 on, 100 elements each, matrices 4096 apart from D2 on."""
    lib = _native.load()
    count = sum(n * t for n, t in zip(fan, nts))
    ins = ins if ins is not None else [4096 * (q + 1) for q in range(count)]
    numels = numels if numels is not None else [100] * sum(nts)
    d2s = d2s if d2s is not None else [D2 + 4096 * k for k in range(len(fan))]
    return lib.dlsim_pairwise_sqdist_batched(
        len(fan) if b is None else b, (ctypes.c_int * max(len(fan), 1))(*fan), (ctypes.c_int * max(len(nts), 1))(*nts),
        (ctypes.c_void_p * max(len(ins), 1))(*ins), (ctypes.c_size_t * max(len(numels), 1))(*numels), dtype,
        (ctypes.c_void_p * max(len(d2s), 1))(*d2s), acc, None)


def test_batched_entry_counts_and_null_arrays():
    lib = _native.load()
    assert _batched(b=-1) == -1 and b"b must be" in lib.dlsim_last_error()
    assert _batched(fan=(), nts=(), b=0) == 0  # a no-op
    assert lib.dlsim_pairwise_sqdist_batched(0, None, None, None, None, 0, None, 0, None) == 0
    one, vp, sz = (ctypes.c_int * 1)(2), (ctypes.c_void_p * 2)(4096, 8192), (ctypes.c_size_t * 1)(100)
    d2 = (ctypes.c_void_p * 1)(D2)
    for args in ((None, one, vp, sz, 0, d2), (one, None, vp, sz, 0, d2), (one, one, None, sz, 0, d2),
                 (one, one, vp, None, 0, d2), (one, one, vp, sz, 0, None)):
        assert lib.dlsim_pairwise_sqdist_batched(1, *args, 0, None) == -1
        assert b"null array" in lib.dlsim_last_error()
    assert lib.dlsim_version() > 0  # none of them reached a HIP call: the next call still works


def test_batched_entry_task_errors():
    lib = _native.load()
    assert _batched(fan=(2, 0), nts=(1, 1), ins=[4096, 8192]) == -1 and b"task 1: n must be >= 1" in lib.dlsim_last_error()
    assert _batched(fan=(33,), ins=[4096] * 33) == -1 and b"<= 32" in lib.dlsim_last_error()
    assert _batched(fan=(2, 2), nts=(1, -1), ins=[4096, 8192], numels=[100]) == -1
    assert b"task 1: n_tensors" in lib.dlsim_last_error()
    assert _batched(ins=[4096, 0]) == -1 and b"null input pointer at index 1" in lib.dlsim_last_error()
    assert _batched(fan=(2, 2), nts=(1, 2), ins=[4096, 8192, 12288, 16384, 20480, 0], numels=[100, 10, 20]) == -1
    assert b"task 1, tensor 1: null input" in lib.dlsim_last_error()
    assert _batched(d2s=[0]) == -1 and b"null distance matrix" in lib.dlsim_last_error()
    for acc in (2, -1):
        assert _batched(acc=acc) == -1 and b"accumulate" in lib.dlsim_last_error()
    assert _batched(dtype=7) == -2 and _batched(dtype=-1) == -2
    assert _batched(fan=(0,), dtype=7) == -2  # the dtype first, as the flat entry
    # the whole list is judged before anything runs: the last task's error, whatever the first ones are
    assert _batched(fan=(2, 2, 2), nts=(1, 1, 1), ins=[4096, 8192, 12288, 16384, 20480, 0]) == -1
    assert b"task 2, tensor 0: null input" in lib.dlsim_last_error()
    assert lib.dlsim_version() > 0


def test_batched_entry_overlaps_down_to_one_byte():
    """A matrix of n = 2 is 32 bytes, an fp32 input of 100 elements 400."""
    lib = _native.load()
    two = dict(fan=(2, 2), nts=(1, 1))
    # on its own input: the first and the last shared byte
    assert _batched(d2s=[4096]) == -1 and b"overlaps input 0" in lib.dlsim_last_error()
    assert _batched(d2s=[8192 + 399]) == -1 and b"overlaps input 1" in lib.dlsim_last_error()
    assert _batched(d2s=[4096 - 31]) == -1
    assert _batched(d2s=[4096 - 31], dtype=3, numels=[1]) == -1  # one fp64 element
    # on another task's input (task 1 reads 12288 and 16384), in both directions of the list
    assert _batched(**two, d2s=[16384 + 399, D2]) == -1
    assert b"task 1, tensor 0: the distance matrix of task 0 overlaps input 1" in lib.dlsim_last_error()
    assert _batched(**two, d2s=[D2, 4096 - 31]) == -1
    assert b"task 0, tensor 0: the distance matrix of task 1 overlaps input 0" in lib.dlsim_last_error()
    # on another matrix
    assert _batched(**two, d2s=[D2, D2 + 31]) == -1 and b"matrices of tasks 0 and 1 overlap" in lib.dlsim_last_error()
    assert _batched(**two, d2s=[D2 + 31, D2]) == -1 and b"overlap" in lib.dlsim_last_error()
    assert _batched(**two, d2s=[D2, D2]) == -1
    # one byte further none of them is an argument error: the call reaches the GPU (or fails there)
    assert lib.dlsim_version() > 0


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_batch_geometry_per_class_and_dtype(dtype):
    dt = eu.DTYPES[dtype]
    for n in (1, 2, 4, 5, 8, 9, 16, 17, 32):
        assert _native.pairdist_batch_geometry(n, dt) == (32, 192)
    lib = _native.load()
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.dlsim_pairdist_batch_geometry(0, 0, ctypes.byref(a), ctypes.byref(b)) == -1
    assert lib.dlsim_pairdist_batch_geometry(33, 0, ctypes.byref(a), ctypes.byref(b)) == -1
    assert lib.dlsim_pairdist_batch_geometry(2, 5, ctypes.byref(a), ctypes.byref(b)) == -2
    assert lib.dlsim_pairdist_batch_geometry(2, 0, None, ctypes.byref(b)) == -1
    assert lib.dlsim_pairdist_batch_geometry(2, 0, ctypes.byref(a), None) == -1


def test_python_wrapper_checks():
    x = [torch.zeros(10) for _ in range(3)]
    out = torch.zeros(9, dtype=torch.float64)
    assert _native.pairwise_sqdist_batched([]) == []
    with pytest.raises(IndexError):
        _native.pairwise_sqdist_batched([([], out)])
    with pytest.raises(ValueError, match="at most 32"):
        _native.pairwise_sqdist_batched([([x[0]] * 33, out)])
    with pytest.raises(ValueError, match="device tensor"):  # no CPU path
        _native.pairwise_sqdist_batched([(x, out)])
    with pytest.raises(IndexError):
        model_distances_batch([[]])
    with pytest.raises(ValueError, match="at most 32"):
        model_distances_batch([[nn.Linear(2, 2)] * 33])
    assert model_distances_batch([]) == []


def _net(seed=0, width=3):
    torch.manual_seed(seed)
    return nn.Linear(width, 2)


@pytest.mark.parametrize("method", [M.KRUM, M.MULTI_KRUM])
def test_aggregate_batch_raises_what_the_plugins_raise(method):
    ms = [_net(i) for i in range(7)]
    with pytest.raises(AssertionError):
        batch.aggregate_batch([(ms, [0.5, 0.5])], method=method)
    with pytest.raises(ValueError, match="unweighted"):
        batch.aggregate_batch([(ms[:3], [0.2, 0.3, 0.5])], method=method)
    with pytest.raises(IndexError):
        batch.aggregate_batch([([], None)], method=method)
    with pytest.raises(ValueError, match="at most 32 models"):
        batch.aggregate_batch([([ms[0]] * 33, None), (ms, None)], method=method)
    with pytest.raises(ValueError, match=r"n = 4 .*f = 1"):  # n < 2f + 3
        batch.aggregate_batch([(ms[:4], None)], method=method)
    with pytest.raises(ValueError, match=r"n = 6 .*f = 2"):
        batch.aggregate_batch([(ms[:6], None)], method=method, settings=types.SimpleNamespace(aggregation_byzantine=2))
    with pytest.raises(ValueError):  # parameter lists differ
        batch.aggregate_batch([(ms[:4] + [_net(1, width=4)], None)], method=method)
    assert batch.aggregate_batch([], method=method) == []


def test_aggregate_batch_m_out_of_range():
    ms = [_net(i) for i in range(5)]
    with pytest.raises(ValueError, match="m = 5"):  # m <= n - f = 4
        batch.aggregate_batch([(ms, None)], method=M.MULTI_KRUM,
                              settings=types.SimpleNamespace(aggregation_multi_krum_m=5))


def test_krum_rule_reads_the_class():
    assert batch.krum_rule(Krum) == ("Krum", 1, None)
    assert batch.krum_rule(Krum.with_params(2)) == ("Krum", 2, None)
    assert batch.krum_rule(MultiKrum.with_params(1, 2)) == ("MultiKrum", 1, 2)
    name, f, m = batch.krum_rule(MultiKrum.with_params(3))
    assert (name, f) == ("MultiKrum", 3) and m(10) == 7
    assert batch.krum_rule(None) is None and batch.krum_rule(nn.Linear) is None
    assert batch.krum_rule(Krum()) is None  # an instance is a foreign plugin: called per task
    assert batch.method_window(M.KRUM, None) is None and batch.method_window(M.MULTI_KRUM, None) is None


def _executor(method, monkeypatch, plugin=None, **settings):
    """A RoundExecutor whose batched Krum route is recorded instead of run."""
    seen = []
    ex = rounds.RoundExecutor({}, types.SimpleNamespace(gradient_aggregation=method, **settings))
    monkeypatch.setattr(rounds, "krum_arena_tasks",
                        lambda prepared, f, m, cb=None: seen.append((f, m(9) if callable(m) else m, cb)) or [])
    monkeypatch.setattr(rounds, "robust_arena_tasks", lambda *a: pytest.fail("not an order statistic"))
    monkeypatch.setattr(rounds, "aggregate_arena_tasks", lambda *a: pytest.fail("not FedAvg"))
    monkeypatch.setattr(ex, "_upload_host_models", lambda *a: None)
    monkeypatch.setattr(ex, "_arena_of", lambda *a: pytest.fail("no model is resolved in this test"))
    if plugin is not None:
        monkeypatch.setattr(rounds.ModelManager, "get_aggregation_method", lambda self: plugin)
    return ex, seen


def test_round_executor_takes_the_batched_route_for_krum_classes(monkeypatch):
    ex, seen = _executor(M.KRUM, monkeypatch, plugin=Krum.with_params(2))
    assert ex._aggregate_wave([]) == []
    assert seen == [(2, None, None)]
    ex, seen = _executor(M.MULTI_KRUM, monkeypatch, plugin=MultiKrum.with_params(1, 2))
    cb = lambda: None  # noqa: E731
    assert ex._aggregate_wave([], cb) == []
    assert seen == [(1, 2, cb)]


def test_round_executor_honours_the_settings(monkeypatch):
    ex, seen = _executor(M.KRUM, monkeypatch, aggregation_byzantine=3)
    ex._aggregate_wave([])
    assert seen == [(3, None, None)]
    ex, seen = _executor(M.MULTI_KRUM, monkeypatch, aggregation_byzantine=2, aggregation_multi_krum_m=3)
    ex._aggregate_wave([])
    assert seen == [(2, 3, None)]
    ex, seen = _executor(M.MULTI_KRUM, monkeypatch, aggregation_byzantine=2)  # m defaults to n - f
    ex._aggregate_wave([])
    assert seen == [(2, 7, None)]


def test_round_executor_checks_every_task_before_anything_is_queued(monkeypatch):
    ms = [_net(i) for i in range(5)]
    for method, name in ((M.KRUM, "Krum"), (M.MULTI_KRUM, "MultiKrum")):
        ex, seen = _executor(method, monkeypatch)
        good = ("t0", "aggregate", {"models": ms})
        with pytest.raises(ValueError, match=name + " is unweighted"):
            ex._aggregate_wave([good, ("t1", "aggregate", {"models": ms, "weights": [0.2] * 5})])
        with pytest.raises(AssertionError):
            ex._aggregate_wave([good, ("t1", "aggregate", {"models": ms, "weights": [1.0]})])
        with pytest.raises(IndexError):
            ex._aggregate_wave([good, ("t1", "aggregate", {"models": []})])
        with pytest.raises(ValueError, match="at most 32"):
            ex._aggregate_wave([good, ("t1", "aggregate", {"models": [ms[0]] * 33})])
        with pytest.raises(ValueError, match=r"n = 4 .*f = 1"):
            ex._aggregate_wave([good, ("t1", "aggregate", {"models": ms[:4]})])
        assert seen == []


def test_krum_arena_tasks_checks_before_any_device_work():
    """(n, f, m) outside the rule and more than 32 models: ValueError before a
    distance is asked for (the views are never touched)."""
    entry = lambda n: ArenaTask(None, None, {torch.float32: [None] * n}, None, [None] * n)  # noqa: E731
    with pytest.raises(ValueError, match=r"n = 4 .*f = 1"):
        model_inputs.krum_arena_tasks([entry(5), entry(4)], 1, None)
    with pytest.raises(ValueError, match="m = 5"):
        model_inputs.krum_arena_tasks([entry(5)], 1, 5)
    with pytest.raises(ValueError, match="m = 6"):
        model_inputs.krum_arena_tasks([entry(5)], 0, lambda n: n + 1)
    with pytest.raises(ValueError, match="at most 32"):
        model_inputs.krum_arena_tasks([entry(33)], 1, None)


def test_models_without_parameters_have_a_zero_matrix():
    """model_distances gives n x n zeros for models without parameters; the batched form reads n from
    `rows` (no dtype group states it), checks it, and needs no device for such a task."""
    from dasklearn_amd.arena import input_arenas
    ms = [nn.ReLU() for _ in range(3)]
    layout, params, views = input_arenas(ms)
    assert not layout.groups and views == {} and params == [[], [], []]
    d2, = model_inputs.distances_arena_tasks([ArenaTask(ms[0], layout, views, None, params)])
    assert d2.shape == (3, 3) and d2.dtype == torch.float64 and not d2.is_cuda and not d2.any()
    with pytest.raises(ValueError, match="does not state its fan-in"):
        model_inputs.distances_arena_tasks([ArenaTask(ms[0], layout, views, None)])
    with pytest.raises(ValueError, match="at most 32"):
        model_inputs.distances_arena_tasks([ArenaTask(ms[0], layout, views, None, [[]] * 33)])
