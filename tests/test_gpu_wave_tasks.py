"""One wave of aggregate tasks through the three dispatchers, per method: RoundExecutor (the wave as
wave_tasks.ArenaTask records behind batch.method_route), aggregate_batch (every model device-resident) and
functions.aggregate task by task give the same bits, and the batched dispatchers make exactly the library
calls they made before the tasks became records: one per dtype and device, not one per task."""
from __future__ import annotations

import copy
import types

import pytest
import torch
from torch import nn

import _robust_util as ru

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.batch import aggregate_batch  # noqa: E402
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M  # noqa: E402
from dasklearn_amd.rounds import RoundExecutor  # noqa: E402

DEV = "cuda"
COUNTED = ("robust_reduce_batched_raw", "pairwise_sqdist_batched_raw", "wreduce_batched", "wreduce_rows_multi",
           "wreduce_rows", "wreduce")


class Net(nn.Module):
    """Two non-empty dtype groups and a parameter without elements. It has a dtype of its own, so it is a dtype
    group without elements, which every batched launch leaves out; inside a non-empty group its null address
    would keep an aggregate's output from counting as a registered arena, and the wave needs that form."""

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(5, 3)
        self.scale = nn.Parameter((torch.randn(7) * 0.05).to(torch.bfloat16))
        self.none = nn.Parameter(torch.empty(0, dtype=torch.float16))


def settings(method):
    return types.SimpleNamespace(gradient_aggregation=method, aggregate_on_device=True, aggregation_byzantine=1,
                                 aggregation_trim=1)


@pytest.fixture(scope="module")
def wave():
    """Three tasks of fan-in 5 (Krum's minimum for f = 1) over models in three forms: registered arenas
    (an earlier aggregate's output), separate contiguous device tensors (a deepcopy of one) and host models.
    Tasks 0 and 1 hold separate-tensor models, so their groups are read in place; task 2 holds none and is
    read from arenas (the host models' are uploaded). Returns ({name: model}, [the tasks' model names])."""
    torch.manual_seed(11)
    host = [Net() for _ in range(15)]

    def earlier(i):
        return aggregate_batch([([arena.to_device_arena(m, DEV) for m in host[2 * i:2 * i + 2]], None)])[0]
    pool = {f"ar{i}": earlier(i) for i in range(3)}
    pool.update({f"te{i}": copy.deepcopy(earlier(3 + i)) for i in range(3)})
    pool.update({f"ho{i}": host[12 + i] for i in range(3)})
    assert all(arena.registered_arenas(pool[f"ar{i}"]) is not None for i in range(3))
    assert all(arena.registered_arenas(pool[f"te{i}"]) is None and all(q.is_cuda for q in pool[f"te{i}"].parameters())
               for i in range(3))
    names = [["ar0", "te0", "ho0", "ar1", "te1"], ["te1", "ho1", "ar1", "ho0", "te2"],
             ["ho2", "ar0", "ho1", "ar2", "ar1"]]
    return pool, names


class Counter:
    """Counts the calls of the library wrappers and of torch._foreach_copy_, and calls through."""

    def __init__(self, monkeypatch):
        self.n = {name: 0 for name in COUNTED + ("_foreach_copy_",)}
        for name in COUNTED:
            self._wrap(monkeypatch, _native, name)
        self._wrap(monkeypatch, torch, "_foreach_copy_")

    def _wrap(self, monkeypatch, owner, name):
        inner = getattr(owner, name)

        def counted(*a, **k):
            self.n[name] += 1
            return inner(*a, **k)
        monkeypatch.setattr(owner, name, counted)

    def take(self):
        """The non-zero counts since the last take."""
        got = {k: v for k, v in self.n.items() if v}
        self.n = dict.fromkeys(self.n, 0)
        return got


def bits(m):
    return [ru.bits_of(q) for q in m.parameters()]


def same_model(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(bits(a), bits(b)))


# The calls of one wave on one device, counted at the commit before the tasks became records. The model has two
# non-empty dtype groups (fp32, bf16) and an empty one (fp16): "one call per dtype and device" is 2 for the
# entries that leave empty groups out and 3 for the weighted reduce, which does not; never one per task.
#   RoundExecutor: tasks 0 and 1 are read in place, task 2 from arenas.
#     FedAvg: the in-place tasks share one wreduce_rows_multi per dtype group (3), the arena task is one
#       wreduce_batched per dtype group (3); wreduce_rows_multi takes them all, so no wreduce_rows, no wreduce.
#     Median, trimmed mean: one robust_reduce_batched_raw per non-empty dtype over all three tasks (2), the
#       in-place tasks as one sub-task per non-empty tensor of the same call.
#     Krum: the distance calls go in rounds, round r every task's r-th non-empty group: two rounds of one dtype
#       each (2); then one _foreach_copy_ for the device.
#     Multi-Krum (m = n - f = 4 of 5): the same 2 distance calls, then one aggregate_arena_tasks: tasks 0 and 1
#       hold two separate-tensor models each, so one is among their 4 and they stay in place: FedAvg's counts.
#   aggregate_batch, every model a device arena: all three tasks from arenas, so no wreduce_rows_multi.
EXPECTED = {
    M.FEDAVG: ({"wreduce_rows_multi": 3, "wreduce_batched": 3}, {"wreduce_batched": 3}),
    M.MEDIAN: ({"robust_reduce_batched_raw": 2}, {"robust_reduce_batched_raw": 2}),
    M.TRIMMED_MEAN: ({"robust_reduce_batched_raw": 2}, {"robust_reduce_batched_raw": 2}),
    M.KRUM: ({"pairwise_sqdist_batched_raw": 2, "_foreach_copy_": 1},
             {"pairwise_sqdist_batched_raw": 2, "_foreach_copy_": 1}),
    M.MULTI_KRUM: ({"pairwise_sqdist_batched_raw": 2, "wreduce_rows_multi": 3, "wreduce_batched": 3},
                   {"pairwise_sqdist_batched_raw": 2, "wreduce_batched": 3}),
}


def _check(method, wave, monkeypatch):
    pool, names = wave
    s = settings(method)
    want = [functions.aggregate(s, {"models": [pool[n] for n in task], "round": 1, "peer": k})[0]
            for k, task in enumerate(names)]
    resident = {n: m if arena.registered_arenas(m) is not None else arena.to_device_arena(m, DEV)
                for n, m in pool.items()}
    dag = [(f"agg{k}", "aggregate", {"models": [(n, 0) for n in task], "round": 1, "peer": k})
           for k, task in enumerate(names)]
    counter = Counter(monkeypatch)
    ex = RoundExecutor({}, s)
    results = ex.run(dag, seed={n: [m] for n, m in pool.items()})
    in_wave = counter.take()
    batched = aggregate_batch([([resident[n] for n in task], None) for task in names], method=method, settings=s)
    in_batch = counter.take()
    monkeypatch.undo()
    print(f"{method}: RoundExecutor {in_wave}, aggregate_batch {in_batch}")
    assert ex.waves == [["agg0", "agg1", "agg2"]]
    for k in range(3):
        got = results[f"agg{k}"][0]
        assert all(q.is_cuda for q in got.parameters()) and all(q.is_cuda for q in batched[k].parameters())
        assert same_model(got, want[k]), f"task {k}: RoundExecutor and functions.aggregate disagree"
        assert same_model(batched[k], want[k]), f"task {k}: aggregate_batch and functions.aggregate disagree"
    assert (in_wave, in_batch) == EXPECTED[method]


def test_fedavg_wave(wave, monkeypatch):
    _check(M.FEDAVG, wave, monkeypatch)


def test_median_wave(wave, monkeypatch):
    _check(M.MEDIAN, wave, monkeypatch)


def test_trimmed_mean_wave(wave, monkeypatch):
    _check(M.TRIMMED_MEAN, wave, monkeypatch)


def test_krum_wave(wave, monkeypatch):
    _check(M.KRUM, wave, monkeypatch)


def test_multi_krum_wave(wave, monkeypatch):
    _check(M.MULTI_KRUM, wave, monkeypatch)


class NetInGroup(nn.Module):
    """The parameter without elements inside the fp32 group: the tensor that ArenaTask.tensor_rows leaves out of
    a group read in place. Such a model is never a registered arena (the empty tensor's address is null), so
    this wave holds separate device tensors and host models only."""

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(5, 3)
        self.none = nn.Parameter(torch.empty(0))
        self.scale = nn.Parameter((torch.randn(7) * 0.05).to(torch.bfloat16))


@pytest.mark.parametrize("method", [M.FEDAVG, M.MEDIAN, M.TRIMMED_MEAN, M.KRUM, M.MULTI_KRUM])
def test_zero_size_tensor_inside_a_group_read_in_place(method):
    """Two tasks of fan-in 5, one over separate device tensors alone, one with host models among them:
    RoundExecutor equals functions.aggregate task by task, bit for bit, and the empty parameter stays empty."""
    torch.manual_seed(23)
    host = [NetInGroup() for _ in range(8)]
    pool = {f"te{i}": copy.deepcopy(host[i]).to(DEV) for i in range(5)}
    pool.update({f"ho{i}": host[5 + i] for i in range(3)})
    names = [["te0", "te1", "te2", "te3", "te4"], ["te4", "ho0", "te1", "ho1", "ho2"]]
    s = settings(method)
    want = [functions.aggregate(s, {"models": [pool[n] for n in task], "round": 1, "peer": k})[0]
            for k, task in enumerate(names)]
    dag = [(f"agg{k}", "aggregate", {"models": [(n, 0) for n in task], "round": 1, "peer": k})
           for k, task in enumerate(names)]
    results = RoundExecutor({}, s).run(dag, seed={n: [m] for n, m in pool.items()})
    for k in range(2):
        got = results[f"agg{k}"][0]
        assert all(q.is_cuda for q in got.parameters()) and got.none.numel() == 0
        assert same_model(got, want[k]), f"task {k}: RoundExecutor and functions.aggregate disagree"
