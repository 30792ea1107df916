"""The batched reduce-and-measure entry and the batched geometric-median /
centered-clipping route without a GPU: every argument error of
dlsim_wreduce_dist_batched with its code and before any HIP call, the
launch-limit diagnostic, the Python wrapper's checks, method_route's choice,
RoundExecutor's call of the lockstep launcher with the rule read from the
settings, and the exceptions of both dispatchers against the plugins'."""
from __future__ import annotations

import ctypes
import types

import pytest
import torch
from torch import nn

import _edge_util as eu
from dasklearn_amd import _native, batch, model_inputs, rounds
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M
from dasklearn_amd.gradient_aggregation import geomed
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian
from dasklearn_amd.wave_tasks import ArenaTask

D2 = 1 << 20   # vectors: far from every input below
OUT = 1 << 24  # outputs: far from both


def _arr(ct, values):
    return (ct * max(len(values), 1))(*values)


def _batched(fan=(2,), nts=(1,), ins=None, numels=None, offs=None, ws=None, outs=None, dtype=0, d2s=None, acc=0,
             b=None):
    """dlsim_wreduce_dist_batched on made-up addresses: inputs 4096 apart from 4096 on, 100 elements each,
    vectors 4096 apart from D2 on, no outputs, weights 0.5."""
    lib = _native.load()
    count = sum(n * t for n, t in zip(fan, nts))
    ins = ins if ins is not None else [4096 * (q + 1) for q in range(count)]
    numels = numels if numels is not None else [100] * sum(max(t, 0) for t in nts)
    offs = offs if offs is not None else [0] * len(numels)
    ws = ws if ws is not None else [0.5] * sum(max(n, 0) for n in fan)
    outs = outs if outs is not None else [None] * len(fan)
    d2s = d2s if d2s is not None else [D2 + 4096 * k for k in range(len(fan))]
    return lib.dlsim_wreduce_dist_batched(
        len(fan) if b is None else b, _arr(ctypes.c_int, fan), _arr(ctypes.c_int, nts), _arr(ctypes.c_void_p, ins),
        _arr(ctypes.c_size_t, numels), _arr(ctypes.c_size_t, offs), _arr(ctypes.c_double, ws),
        _arr(ctypes.c_void_p, outs), dtype, _arr(ctypes.c_void_p, d2s), acc, None)


def _err():
    return _native.load().dlsim_last_error()


def test_batched_entry_counts_and_null_arrays():
    lib = _native.load()
    assert _batched(b=-1) == -1 and b"b must be" in _err()
    assert _batched(fan=(), nts=(), b=0) == 0  # a no-op
    assert lib.dlsim_wreduce_dist_batched(0, None, None, None, None, None, None, None, 0, None, 0, None) == 0
    one, vp, sz = (ctypes.c_int * 1)(2), (ctypes.c_void_p * 2)(4096, 8192), (ctypes.c_size_t * 1)(100)
    off, w = (ctypes.c_size_t * 1)(0), (ctypes.c_double * 2)(0.5, 0.5)
    none, out, d2 = (ctypes.c_void_p * 1)(None), (ctypes.c_void_p * 1)(OUT), (ctypes.c_void_p * 1)(D2)
    for args in ((None, one, vp, sz, off, w, none, 0, d2), (one, None, vp, sz, off, w, none, 0, d2),
                 (one, one, None, sz, off, w, none, 0, d2), (one, one, vp, None, off, w, none, 0, d2),
                 (one, one, vp, sz, None, w, out, 0, d2), (one, one, vp, sz, off, w, None, 0, d2),
                 (one, one, vp, sz, off, w, none, 0, None)):
        assert lib.dlsim_wreduce_dist_batched(1, *args, 0, None) == -1
        assert b"null array" in _err()
    assert lib.dlsim_wreduce_dist_batched(1, one, one, vp, sz, off, None, none, 0, d2, 0, None) == -1
    assert b"null weights array" in _err()
    assert lib.dlsim_version() > 0  # none of them reached a HIP call: the next call still works


def test_batched_entry_task_errors():
    lib = _native.load()
    assert _batched(fan=(2, 0), nts=(1, 1), ins=[4096, 8192]) == -1 and b"task 1: n must be >= 1" in _err()
    assert _batched(fan=(33,), ins=[4096] * 33) == -1 and b"<= 32" in _err() and b"held in registers" in _err()
    assert _batched(fan=(2, 2), nts=(1, -1), ins=[4096, 8192], numels=[100]) == -1
    assert b"task 1: n_tensors" in _err()
    assert _batched(ins=[4096, 0]) == -1 and b"null input pointer at index 1" in _err()
    assert _batched(fan=(2, 2), nts=(1, 2), ins=[4096, 8192, 12288, 16384, 20480, 0], numels=[100, 10, 20]) == -1
    assert b"task 1, tensor 1: null input" in _err()
    assert _batched(d2s=[0]) == -1 and b"null distance vector" in _err()
    for acc in (2, -1):
        assert _batched(acc=acc) == -1 and b"accumulate" in _err()
    assert _batched(dtype=7) == -2 and _batched(dtype=-1) == -2
    assert _batched(fan=(0,), dtype=7) == -2  # the dtype first, as the flat entry
    # the weight rule: (double)(float)w == w unless the buffers are fp64
    assert _batched(fan=(2, 2), nts=(1, 1), ws=[0.5, 0.25, 0.5, 0.1]) == -1
    assert b"task 1: weight 1 (0.1" in _err() and b"not representable in fp32" in _err()
    assert _batched(ws=[float("nan"), 0.5]) == -1 and b"task 0: weight 0" in _err()
    assert _batched(ws=[0.1, 0.5], dtype=3, ins=[4096, 0]) == -1 and b"null input pointer" in _err()  # fp64 takes 0.1
    # a zero-length tensor is never read: any pointer will do
    assert _batched(fan=(2, 2), nts=(1, 1), ins=[0, 0, 4096, 0], numels=[0, 100]) == -1
    assert b"task 1, tensor 0: null input pointer at index 1" in _err()
    # the whole list is judged before anything runs: the last task's error, whatever the first ones are
    assert _batched(fan=(2, 2, 2), nts=(1, 1, 1), ins=[4096, 8192, 12288, 16384, 20480, 0]) == -1
    assert b"task 2, tensor 0: null input" in _err()
    assert _batched(fan=(2, 2, 2), nts=(1, 1, 1), ws=[0.5] * 5 + [1e-50]) == -1 and b"task 2: weight 1" in _err()
    assert lib.dlsim_version() > 0


def test_batched_entry_overlaps_down_to_one_byte():
    """A vector of n = 2 is 16 bytes, an fp32 input or output of 100 elements 400."""
    two = dict(fan=(2, 2), nts=(1, 1))
    # a vector on its own input: the first and the last shared byte
    assert _batched(d2s=[4096]) == -1 and b"the distance vector of task 0 overlaps input 0" in _err()
    assert _batched(d2s=[8192 + 399]) == -1 and b"overlaps input 1" in _err()
    assert _batched(d2s=[4096 - 15]) == -1
    assert _batched(d2s=[4096 - 15], dtype=3, numels=[1]) == -1  # one fp64 element
    # on another task's input (task 1 reads 12288 and 16384), in both directions of the list
    assert _batched(**two, d2s=[16384 + 399, D2]) == -1
    assert b"task 1, tensor 0: the distance vector of task 0 overlaps input 1" in _err()
    assert _batched(**two, d2s=[D2, 4096 - 15]) == -1
    assert b"task 0, tensor 0: the distance vector of task 1 overlaps input 0" in _err()
    # on another vector
    assert _batched(**two, d2s=[D2, D2 + 15]) == -1
    assert b"the distance vector of task 0 overlaps the distance vector of task 1" in _err()
    assert _batched(**two, d2s=[D2 + 15, D2]) == -1 and b"overlaps" in _err()
    assert _batched(**two, d2s=[D2, D2]) == -1
    # an output on its own input, on another task's input, on a vector, on another output, on its own tensors
    assert _batched(outs=[8192 - 399]) == -1
    assert b"task 0, tensor 0: the output of task 0, tensor 0 overlaps input 1" in _err()
    assert _batched(**two, outs=[None, 4096 + 399]) == -1
    assert b"task 0, tensor 0: the output of task 1, tensor 0 overlaps input 0" in _err()
    assert _batched(**two, outs=[D2 + 4096 + 15, None]) == -1
    assert b"the distance vector of task 1 overlaps the output of task 0, tensor 0" in _err()
    assert _batched(**two, outs=[OUT, OUT + 399]) == -1
    assert b"the output of task 0, tensor 0 overlaps the output of task 1, tensor 0" in _err()
    assert _batched(fan=(2,), nts=(2,), ins=[4096, 8192, 12288, 16384], numels=[100, 100], offs=[0, 399],
                    outs=[OUT]) == -1
    assert b"the output of task 0, tensor 0 overlaps the output of task 0, tensor 1" in _err()
    # an empty tensor's output range shares nothing; a task without an output ignores its offsets
    assert _batched(fan=(2,), nts=(2,), ins=[4096, 0, 8192, 0], numels=[100, 0], offs=[0, 8], outs=[OUT], d2s=[0]) == -1
    assert b"null distance vector" in _err()
    # one byte further none of them is an argument error: the call reaches the GPU (or fails there)
    assert _native.load().dlsim_version() > 0


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_batch_geometry_per_class_and_dtype(dtype):
    dt = eu.DTYPES[dtype]
    for n in (1, 2, 4, 5, 8, 9, 16, 17, 32):
        assert _native.reducedist_batch_geometry(n, dt) == (32, 128 if dtype == "f64" else 192)
    lib = _native.load()
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.dlsim_reducedist_batch_geometry(0, 0, ctypes.byref(a), ctypes.byref(b)) == -1
    assert lib.dlsim_reducedist_batch_geometry(33, 0, ctypes.byref(a), ctypes.byref(b)) == -1
    assert lib.dlsim_reducedist_batch_geometry(2, 5, ctypes.byref(a), ctypes.byref(b)) == -2
    assert lib.dlsim_reducedist_batch_geometry(2, 0, None, ctypes.byref(b)) == -1
    assert lib.dlsim_reducedist_batch_geometry(2, 0, ctypes.byref(a), None) == -1


def test_python_wrapper_checks():
    x = [torch.zeros(10) for _ in range(3)]
    d2 = torch.zeros(3, dtype=torch.float64)
    assert _native.wreduce_dist_batched([]) == []
    with pytest.raises(IndexError):
        _native.wreduce_dist_batched([([], [], None, d2)])
    with pytest.raises(ValueError, match="at most 32"):
        _native.wreduce_dist_batched([([x[0]] * 33, [0.0] * 33, None, d2)])
    with pytest.raises(AssertionError):
        _native.wreduce_dist_batched([(x, [0.5, 0.5], None, d2)])
    with pytest.raises(ValueError, match="device tensor"):  # no CPU path
        _native.wreduce_dist_batched([(x, [0.5, 0.25, 0.25], None, d2)])
    with pytest.raises(IndexError):
        geomed.consensus_distance_batch([([], None)])
    with pytest.raises(AssertionError):
        geomed.consensus_distance_batch([([nn.Linear(2, 2)] * 3, [1.0])])
    with pytest.raises(ValueError, match="at most 32"):
        geomed.consensus_distance_batch([([nn.Linear(2, 2)] * 33, None)])
    assert geomed.consensus_distance_batch([]) == []


# ---- the route -----------------------------------------------------------------------------------
def test_geomed_rule_reads_the_class():
    assert batch.geomed_rule(GeometricMedian) == ("GeometricMedian", 3, 1e-6)
    assert batch.geomed_rule(GeometricMedian.with_params(5, 0.25)) == ("GeometricMedian", 5, 0.25)
    assert batch.geomed_rule(CenteredClip) == ("CenteredClip", 3, None)
    assert batch.geomed_rule(CenteredClip.with_params(1.5, 0)) == ("CenteredClip", 0, 1.5)
    assert batch.geomed_rule(None) is None and batch.geomed_rule(nn.Linear) is None
    assert batch.geomed_rule(GeometricMedian()) is None  # an instance is a foreign plugin: called per task

    class Own(GeometricMedian):  # a subclass with its own aggregate is not the rule any more
        @classmethod
        def aggregate(cls, models, weights=None, to_host=None, trace=False):
            return None
    assert batch.geomed_rule(Own) is None


def test_method_route_gives_the_new_kind():
    for method, name in ((M.GEOMETRIC_MEDIAN, "GeometricMedian"), (M.CENTERED_CLIP, "CenteredClip")):
        r = batch.method_route(method, None)
        assert r.kind == batch.GEOMED and r.rule[0] == name and issubclass(r.plugin, getattr(geomed, name))
    s = types.SimpleNamespace(aggregation_gm_iters=7, aggregation_gm_nu=0.25, aggregation_clip_tau=1.5,
                              aggregation_clip_iters=0)
    assert batch.method_route(M.GEOMETRIC_MEDIAN, s).rule == ("GeometricMedian", 7, 0.25)
    assert batch.method_route(M.CENTERED_CLIP, s).rule == ("CenteredClip", 0, 1.5)

    class Foreign:
        @staticmethod
        def aggregate(models, weights=None, to_host=None):
            return "out"
    for method in (M.GEOMETRIC_MEDIAN, M.CENTERED_CLIP):
        r = batch.method_route(method, None, lambda m, s: Foreign)
        assert r.kind == batch.PLUGIN and r.per_task([([1], None)]) == ["out"]
    assert batch.method_route(M.KRUM, None).kind == batch.KRUM and batch.method_route(M.MEDIAN, None).kind == batch.WINDOW


def test_method_route_run_takes_three_or_four_launchers():
    r = batch.method_route(M.CENTERED_CLIP, None)
    seen = []
    fail = lambda *a: pytest.fail("another kind's launcher")  # noqa: E731
    own = lambda prepared, rule, cb=None: seen.append((rule, cb)) or ["x"]  # noqa: E731
    assert r.run([], None, launchers=(fail, fail, fail, own)) == ["x"] and seen == [(("CenteredClip", 3, None), None)]
    assert r.run([], launchers=(fail, fail, fail)) == []  # the three-tuple of before: this module's own fourth
    k = batch.method_route(M.KRUM, None)
    assert k.run([], launchers=(fail, fail, lambda p, f, m, cb=None: ["k"], fail)) == ["k"]


def _net(seed=0, width=3):
    torch.manual_seed(seed)
    return nn.Linear(width, 2)


def _executor(method, monkeypatch, plugin=None, **settings):
    """A RoundExecutor whose lockstep route is recorded instead of run."""
    seen = []
    ex = rounds.RoundExecutor({}, types.SimpleNamespace(gradient_aggregation=method, **settings))
    monkeypatch.setattr(rounds, "geomed_arena_tasks",
                        lambda prepared, rule, cb=None: seen.append((rule, [t.weights for t in prepared], cb)) or
                        ["out"] * len(prepared))
    for name in ("krum_arena_tasks", "robust_arena_tasks", "aggregate_arena_tasks"):
        monkeypatch.setattr(rounds, name, lambda *a: pytest.fail("another method's launcher"))
    monkeypatch.setattr(ex, "_upload_host_models", lambda *a: None)
    monkeypatch.setattr(ex, "_wave_task", lambda models, ws, cache, walked: ArenaTask(models[0], None, {}, ws))
    if plugin is not None:
        monkeypatch.setattr(rounds.ModelManager, "get_aggregation_method", lambda self: plugin)
    return ex, seen


def test_round_executor_calls_the_lockstep_launcher_with_the_settings_rule(monkeypatch):
    ex, seen = _executor(M.GEOMETRIC_MEDIAN, monkeypatch)
    assert ex._aggregate_wave([]) == [] and seen == [(("GeometricMedian", 3, 1e-6), [], None)]
    ex, seen = _executor(M.GEOMETRIC_MEDIAN, monkeypatch, aggregation_gm_iters=7, aggregation_gm_nu=0.25)
    cb = lambda: None  # noqa: E731
    assert ex._aggregate_wave([], cb) == [] and seen == [(("GeometricMedian", 7, 0.25), [], cb)]
    ex, seen = _executor(M.CENTERED_CLIP, monkeypatch, aggregation_clip_tau=1.5, aggregation_clip_iters=2)
    ms = [_net(i) for i in range(4)]
    outs = ex._aggregate_wave([("t0", "aggregate", {"models": ms}),
                               ("t1", "aggregate", {"models": ms[:2], "weights": [0.25, 0.75]})])
    # the tasks keep their weights, settled as the plugins settle them
    assert outs == ["out", "out"] and seen == [(("CenteredClip", 2, 1.5), [[0.25] * 4, [0.25, 0.75]], None)]
    with pytest.raises(ValueError, match="nu must be"):  # with_params' checks, as the per-task path
        _executor(M.GEOMETRIC_MEDIAN, monkeypatch, aggregation_gm_nu=0.0)[0]._aggregate_wave([])
    ex, seen = _executor(M.CENTERED_CLIP, monkeypatch, plugin=CenteredClip.with_params(None, 1))
    ex._aggregate_wave([])
    assert seen == [(("CenteredClip", 1, None), [], None)]


def _raised(fn):
    with pytest.raises(Exception) as e:
        fn()
    return type(e.value), str(e.value)


@pytest.mark.parametrize("method,cls", [(M.GEOMETRIC_MEDIAN, GeometricMedian), (M.CENTERED_CLIP, CenteredClip)])
def test_both_dispatchers_raise_what_the_plugins_raise(method, cls, monkeypatch):
    ms = [_net(i) for i in range(7)]
    good = ("t0", "aggregate", {"models": ms})
    cases = {
        "weights of another length": (ms, [0.5, 0.5]),
        "an empty task": ([], None),
        "33 models": ([ms[0]] * 33, None),
        "mismatched parameter lists": (ms[:4] + [_net(1, width=4)], None),
    }
    if cls is CenteredClip:
        cases["32 models under centered clipping"] = ([ms[0]] * 32, None)
    for what, (models, weights) in cases.items():
        want = _raised(lambda: cls.aggregate(models, weights))
        assert issubclass(want[0], (AssertionError, IndexError, ValueError)), what
        assert _raised(lambda: batch.aggregate_batch([(models, weights)], method=method)) == want, what
        if what != "mismatched parameter lists":  # (the executor finds those while it resolves the wave's models)
            ex, seen = _executor(method, monkeypatch)
            assert _raised(lambda: ex._aggregate_wave([good, ("t1", "aggregate", {"models": models,
                                                                                   "weights": weights})])) == want, what
            assert seen == []
    if cls is GeometricMedian:
        assert "at most 32 models" in _raised(lambda: cls.aggregate([ms[0]] * 33))[1]
    else:
        assert "at most 31 models" in _raised(lambda: cls.aggregate([ms[0]] * 32))[1]
    assert batch.aggregate_batch([], method=method) == []


def test_geomed_arena_tasks_checks_before_any_device_work():
    """More than 32 models (31 under centered clipping): ValueError before a pass is queued (the views are
    never touched)."""
    entry = lambda n: ArenaTask(None, None, {torch.float32: [None] * n}, None, [None] * n)  # noqa: E731
    with pytest.raises(ValueError, match="at most 32"):
        model_inputs.geomed_arena_tasks([entry(5), entry(33)], ("GeometricMedian", 3, 1e-6))
    with pytest.raises(ValueError, match="at most 31"):
        model_inputs.geomed_arena_tasks([entry(5), entry(32)], ("CenteredClip", 3, None))
    assert model_inputs.geomed_arena_tasks([], ("CenteredClip", 3, None)) == []
