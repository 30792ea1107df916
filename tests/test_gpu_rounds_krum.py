"""RoundExecutor and aggregate_batch under KRUM and MULTI_KRUM: a D-PSGD DAG
run in waves (every wave's distance matrices in batched launches, one
synchronisation per wave, the copies or reduces batched: model_inputs.
krum_arena_tasks) equals, bit for bit, the same DAG run task by task through
functions.aggregate (ModelManager's plugins, aggregate_on_device), on
host-trained, arena and separate-tensor models of two dtype groups; and the
batched route never calls the per-task distance entries."""
from __future__ import annotations

import copy
import types

import numpy as np
import pytest
import torch
from torch import nn

import _krum_util as ku
import _robust_util as ru
from _sgd_util import BnNet

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.batch import aggregate_batch  # noqa: E402
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Krum, MultiKrum  # noqa: E402
from dasklearn_amd.rounds import RoundExecutor  # noqa: E402

DEV = "cuda"
PEERS, ROUNDS = 6, 3
# a 10-element bias in front of larger tensors (the next one is off alignment in an arena), two dtype groups
SHAPES = [((10,), torch.float32), ((37, 29), torch.float32), ((4100,), torch.float32), ((33, 5), torch.bfloat16),
          ((7,), torch.bfloat16)]
# fan-in 5 allows f = 1; Multi-Krum with its default m = n - f = 4, and with m = 2
CONFIGS = {"krum": (M.KRUM, {}), "multi": (M.MULTI_KRUM, {}), "multi2": (M.MULTI_KRUM, {"aggregation_multi_krum_m": 2})}


class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter((torch.randn(*s) * 0.05).to(dt)) for s, dt in SHAPES])


def settings(method, **kw):
    kw.setdefault("aggregation_byzantine", 1)
    return types.SimpleNamespace(gradient_aggregation=method, aggregate_on_device=True, **kw)


def build_dag(rounds=ROUNDS, weights_on=None):
    """Round r: every peer trains its model, then aggregates its own and its four ring neighbours'
    trained models (fan-in 5); round 1 trains the seed."""
    tasks = []
    for r in range(1, rounds + 1):
        for p in range(PEERS):
            model = ("init", 0) if r == 1 else (f"agg_{p}_{r - 1}", 0)
            tasks.append((f"train_{p}_{r}", "train", {"model": model, "round": r, "peer": p}))
        for p in range(PEERS):
            models = [(f"train_{(p + d) % PEERS}_{r}", 0) for d in (-2, -1, 0, 1, 2)]
            data = {"models": models, "round": r, "peer": p}
            if weights_on == (p, r):
                data["weights"] = [0.2] * 5
            tasks.append((f"agg_{p}_{r}", "aggregate", data))
    return tasks


def _trained(params, poison=None):
    """The train stub's arithmetic on the host (the same bits wherever the model lives). poison: {peer: value}
    fills that peer's trained model."""
    out = copy.deepcopy(params["model"]).cpu()
    g = torch.Generator().manual_seed(1000 * params["round"] + params["peer"])
    with torch.no_grad():
        for q in out.parameters():
            q.add_((torch.randn(q.shape, generator=g) * 0.01).to(q.dtype))
            if poison is not None and params["peer"] in poison:
                q.fill_(poison[params["peer"]])
    return out


TRAINS = {
    "host": lambda s, p: [_trained(p)],  # the reference's CPU training
    "arena": lambda s, p: [arena.to_device_arena(_trained(p), DEV)],
    "tensors": lambda s, p: [_trained(p).to(DEV)],  # a device model with one allocation per parameter
}


def replay(tasks, train, s, init):
    """The worker's way: one task at a time, aggregates through functions.aggregate."""
    results = {"init": [init]}

    def resolve(v):
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str):
            return results[v[0]][v[1]]
        return [resolve(x) for x in v] if isinstance(v, list) else v
    for name, func, data in tasks:
        f = functions.aggregate if func == "aggregate" else train
        results[name] = f(s, {k: resolve(v) for k, v in data.items()})
    return results


def bits(m):
    return [ru.bits_of(q) for q in m.parameters()]


def same_model(a, b):
    return all((x == y).all() for x, y in zip(bits(a), bits(b)))


def _init():
    torch.manual_seed(5)
    return Small()


def final(results, rounds=ROUNDS):
    return [results[f"agg_{p}_{rounds}"][0] for p in range(PEERS)]


def _refuse(*a, **k):
    raise AssertionError("a per-task distance call on the batched route")


@pytest.mark.parametrize("place,release_early", [("host", True), ("arena", True), ("arena", False), ("tensors", True),
                                                 ("tensors", False)])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_round_executor_equals_the_per_task_path(config, place, release_early, monkeypatch):
    method, extra = CONFIGS[config]
    init, tasks = _init(), build_dag()
    s = settings(method, **extra)
    want = final(replay(tasks, TRAINS[place], s, init))
    # the batched route never asks for one task's distances: with the flat entries gone the run still passes
    monkeypatch.setattr(_native, "pairwise_sqdist", _refuse)
    monkeypatch.setattr(_native, "pairwise_sqdist_tensors_raw", _refuse)
    ex = RoundExecutor({"train": TRAINS[place]}, s, release_early=release_early)
    got = final(ex.run(tasks, seed={"init": [init]}))
    monkeypatch.undo()
    assert len(ex.waves) == 2 * ROUNDS and all(len(w) == PEERS for w in ex.waves)
    for p, (a, b) in enumerate(zip(got, want)):
        assert all(q.is_cuda for q in a.parameters())  # stayed resident
        assert same_model(a, b), f"peer {p}: the executor and functions.aggregate disagree"
        assert all(x.stride() == y.stride() and x.requires_grad == y.requires_grad
                   for x, y in zip(a.parameters(), b.parameters()))
    # and it is the configured method, not FedAvg
    fed = final(RoundExecutor({"train": TRAINS[place]}, settings(M.FEDAVG)).run(tasks, seed={"init": [init]}))
    assert not any(same_model(a, f) for a, f in zip(got, fed))


def test_the_three_configurations_differ():
    init, tasks = _init(), build_dag(rounds=1)
    outs = {}
    for config, (method, extra) in CONFIGS.items():
        outs[config] = final(RoundExecutor({"train": TRAINS["arena"]}, settings(method, **extra)).run(
            tasks, seed={"init": [init]}), 1)
    for a, b in (("krum", "multi"), ("krum", "multi2"), ("multi", "multi2")):
        assert not any(same_model(x, y) for x, y in zip(outs[a], outs[b])), (a, b)


@pytest.mark.parametrize("config", ["krum", "multi2"])
def test_an_all_nan_peer_and_an_all_inf_peer_are_never_selected(config):
    """Peer 0 sends NaN, peer 3 Inf. Every neighbourhood holds at least one of them and three finite models: a
    finite model has two finite neighbours, so a finite score (n - f - 2 = 2), the others an infinite one; Krum
    and Multi-Krum(2) select among the finite ones."""
    method, extra = CONFIGS[config]
    init, tasks = _init(), build_dag(rounds=1)
    train = lambda s, p: [_trained(p, poison={0: float("nan"), 3: float("inf")}).to(DEV)]  # noqa: E731
    s = settings(method, **extra)
    got = final(RoundExecutor({"train": train}, s).run(tasks, seed={"init": [init]}), 1)
    want = final(replay(tasks, train, s, init), 1)
    fed = final(RoundExecutor({"train": train}, settings(M.FEDAVG)).run(tasks, seed={"init": [init]}), 1)
    for p in range(PEERS):
        assert same_model(got[p], want[p])
        assert all(bool(torch.isfinite(q.float()).all()) for q in got[p].parameters()), f"{config}, peer {p}"
        assert not any(bool(torch.isfinite(q.float()).all()) for q in fed[p].parameters()), f"FedAvg, peer {p}"


@pytest.mark.parametrize("place", ["arena", "tensors", "host"])
def test_buffers_and_strides_are_those_of_model_zero_even_when_it_is_byzantine(place):
    def bn():
        m = BnNet()
        with torch.no_grad():
            m.bn.running_mean.uniform_(-1, 1)
            m.bn.num_batches_tracked.fill_(int(torch.randint(1, 99, ()).item()))
            m.fc.weight.data = m.fc.weight.data.t().contiguous().t()  # a transposed weight: not contiguous
        return m
    n, f = 8, 2
    rows, byz, want, _ = ku.plugin_case(n, f, shapes=([5, 7], [5], [5], [5]), byz=(0, 5))
    torch.manual_seed(3)
    # (the arena form of a device model: its buffers are on the device too)
    put = {"arena": lambda m: arena.to_device_arena(m.to(DEV)), "tensors": lambda m: m.to(DEV), "host": lambda m: m}[place]
    models = [put(ku.model_of(r, None, "f32", make=bn)) for r in rows]
    want64 = want.astype(np.float64)
    dag = [("agg", "aggregate", {"models": [(f"m{i}", 0) for i in range(n)]})]
    for method, plugin, m, extra in ((M.KRUM, Krum.with_params(f), 1, {}),
                                     (M.MULTI_KRUM, MultiKrum.with_params(f), n - f, {}),
                                     (M.MULTI_KRUM, MultiKrum.with_params(f, 2), 2, {"aggregation_multi_krum_m": 2})):
        chosen = ku.ref_select(want64, f, m)
        assert 0 not in chosen
        s = settings(method, aggregation_byzantine=f, **extra)
        out = RoundExecutor({}, s).run(dag, seed={f"m{i}": [mod] for i, mod in enumerate(models)})["agg"][0]
        ref = plugin.aggregate(models, to_host=False)
        assert isinstance(out, BnNet) and same_model(out, ref)
        if m == 1:
            assert same_model(out, models[chosen[0]])
        bufs, bufs0 = list(out.buffers()), list(models[0].buffers())
        assert len(bufs) == len(bufs0) == 3
        for b, b0 in zip(bufs, bufs0):
            assert torch.equal(b.cpu(), b0.cpu()) and b.data_ptr() != b0.data_ptr()
        assert not torch.equal(out.bn.running_mean.cpu(), models[chosen[0]].bn.running_mean.cpu())
        for q, q0, r in zip(out.parameters(), models[0].parameters(), ref.parameters()):
            assert q.stride() == r.stride() and q.shape == q0.shape and q.requires_grad == q0.requires_grad
        assert not out.fc.weight.is_contiguous() or place == "arena"  # to_device_arena makes contiguous views
        if place != "host":  # (a host model's buffers stay on the host, as deepcopy leaves them)
            y = out.bn(out.fc(torch.ones(4, 7, device=DEV)))  # working submodules
            assert y.shape == (4, 5)


@pytest.mark.parametrize("config", ["krum", "multi"])
def test_a_task_with_weights_raises_as_the_plugin_does(config):
    method, extra = CONFIGS[config]
    init = _init()
    s = settings(method, **extra)
    tasks = build_dag(rounds=1, weights_on=(3, 1))
    with pytest.raises(ValueError, match="is unweighted") as mine:
        RoundExecutor({"train": TRAINS["arena"]}, s).run(tasks, seed={"init": [init]})
    with pytest.raises(ValueError, match="is unweighted") as theirs:
        replay(tasks, TRAINS["arena"], s, init)
    assert str(mine.value) == str(theirs.value)


@pytest.mark.parametrize("method", [M.KRUM, M.MULTI_KRUM])
def test_aggregate_batch_over_mixed_fan_ins(method, monkeypatch):
    """Device arenas, fan-ins 5, 8 and 17 (the distance kernel's three classes) in one call, against the plugin
    per task; the batched call itself asks for no single task's distances."""
    torch.manual_seed(9)
    pool = [arena.to_device_arena(Small(), DEV) for _ in range(17)]
    fans = (5, 8, 17)
    s = types.SimpleNamespace(aggregation_byzantine=1)
    plugin = (Krum if method == M.KRUM else MultiKrum).with_params(1)
    want = [plugin.aggregate(pool[:n], to_host=False) for n in fans]
    monkeypatch.setattr(_native, "pairwise_sqdist", _refuse)
    monkeypatch.setattr(_native, "pairwise_sqdist_tensors_raw", _refuse)
    outs = aggregate_batch([(pool[:n], None) for n in fans], method=method, settings=s)
    monkeypatch.undo()
    for n, out, ref in zip(fans, outs, want):
        assert all(q.is_cuda for q in out.parameters())
        assert same_model(out, ref), f"n = {n}"
