"""RoundExecutor and aggregate_batch under settings.gradient_aggregation: a
D-PSGD DAG run in waves equals, bit for bit, the same DAG run task by task
through functions.aggregate (ModelManager's plugins, aggregate_on_device), for
the batched methods (MEDIAN, TRIMMED_MEAN) on host-trained, arena and
separate-tensor models and for the per-task methods; and it is not FedAvg."""
from __future__ import annotations

import copy
import types

import pytest
import torch
from torch import nn

import _robust_util as ru

pytestmark = pytest.mark.gpu

from dasklearn_amd import arena, functions  # noqa: E402
from dasklearn_amd.batch import aggregate_batch  # noqa: E402
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M  # noqa: E402
from dasklearn_amd.rounds import RoundExecutor  # noqa: E402

DEV = "cuda"
PEERS, ROUNDS = 6, 3
# a 10-element bias in front of larger tensors (the next one is off alignment in an arena), two dtype groups
SHAPES = [((10,), torch.float32), ((37, 29), torch.float32), ((4100,), torch.float32), ((33, 5), torch.bfloat16),
          ((7,), torch.bfloat16)]


class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter((torch.randn(*s) * 0.05).to(dt)) for s, dt in SHAPES])


def settings(method, **kw):
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
    """The train stub's arithmetic on the host (the same bits wherever the model lives)."""
    out = copy.deepcopy(params["model"]).cpu()
    g = torch.Generator().manual_seed(1000 * params["round"] + params["peer"])
    with torch.no_grad():
        for q in out.parameters():
            q.add_((torch.randn(q.shape, generator=g) * 0.01).to(q.dtype))
            if poison is not None and params["peer"] == poison:
                q.fill_(float("inf"))
    return out


TRAINS = {
    "host": lambda s, p: [_trained(p)],  # the reference's CPU training
    "arena": lambda s, p: [arena.to_device_arena(_trained(p), DEV)],
    "tensors": lambda s, p: [_trained(p).to(DEV)],  # a device model with one allocation per parameter
}


def poisoned(s, p):
    return [_trained(p, poison=0).to(DEV)]


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


@pytest.mark.parametrize("place,release_early", [("host", True), ("arena", True), ("arena", False), ("tensors", True),
                                                 ("tensors", False)])
@pytest.mark.parametrize("method", [M.MEDIAN, M.TRIMMED_MEAN])
def test_round_executor_equals_the_per_task_path(method, place, release_early):
    init, tasks = _init(), build_dag()
    s = settings(method, aggregation_trim=1)
    ex = RoundExecutor({"train": TRAINS[place]}, s, release_early=release_early)
    got = final(ex.run(tasks, seed={"init": [init]}))
    want = final(replay(tasks, TRAINS[place], s, init))
    assert len(ex.waves) == 2 * ROUNDS and all(len(w) == PEERS for w in ex.waves)
    for p, (a, b) in enumerate(zip(got, want)):
        assert all(q.is_cuda for q in a.parameters())  # stayed resident
        assert same_model(a, b), f"peer {p}: the executor and functions.aggregate disagree"
    # and it is the configured method, not FedAvg (what the executor computed before it read the setting)
    fed = final(RoundExecutor({"train": TRAINS[place]}, settings(M.FEDAVG)).run(tasks, seed={"init": [init]}))
    assert not any(same_model(a, f) for a, f in zip(got, fed))


def test_trim_is_read_from_the_settings():
    init, tasks = _init(), build_dag(rounds=1)
    outs = {}
    for trim in (1, 2):
        s = settings(M.TRIMMED_MEAN, aggregation_trim=trim)
        got = final(RoundExecutor({"train": TRAINS["arena"]}, s).run(tasks, seed={"init": [init]}), 1)
        want = final(replay(tasks, TRAINS["arena"], s, init), 1)
        assert all(same_model(a, b) for a, b in zip(got, want))
        outs[trim] = got
    assert not any(same_model(a, b) for a, b in zip(outs[1], outs[2]))
    # trim 2 of five models is their median
    s = settings(M.MEDIAN)
    med = final(RoundExecutor({"train": TRAINS["arena"]}, s).run(tasks, seed={"init": [init]}), 1)
    assert all(same_model(a, b) for a, b in zip(outs[2], med))


@pytest.mark.parametrize("method", [M.KRUM, M.GEOMETRIC_MEDIAN])
def test_per_task_methods_equal_the_per_task_path(method):
    init, tasks = _init(), build_dag(rounds=1)
    s = settings(method)
    got = final(RoundExecutor({"train": TRAINS["tensors"]}, s).run(tasks, seed={"init": [init]}), 1)
    want = final(replay(tasks, TRAINS["tensors"], s, init), 1)
    for a, b in zip(got, want):
        assert all(q.is_cuda for q in a.parameters()) and same_model(a, b)


def test_an_all_inf_peer_breaks_fedavg_but_not_the_median():
    init, tasks = _init(), build_dag(rounds=1)
    med = final(RoundExecutor({"train": poisoned}, settings(M.MEDIAN)).run(tasks, seed={"init": [init]}), 1)
    fed = final(RoundExecutor({"train": poisoned}, settings(M.FEDAVG)).run(tasks, seed={"init": [init]}), 1)
    readers = [p for p in range(PEERS) if any((p + d) % PEERS == 0 for d in (-2, -1, 0, 1, 2))]
    assert len(readers) == 5
    for p in range(PEERS):
        assert all(bool(torch.isfinite(q.float()).all()) for q in med[p].parameters()), f"median, peer {p}"
    for p in readers:
        assert not any(bool(torch.isfinite(q.float()).all()) for q in fed[p].parameters()), f"FedAvg, peer {p}"


@pytest.mark.parametrize("method", [M.MEDIAN, M.TRIMMED_MEAN])
def test_a_task_with_weights_raises_as_the_plugin_does(method):
    init = _init()
    s = settings(method)
    tasks = build_dag(rounds=1, weights_on=(3, 1))
    with pytest.raises(ValueError, match="is unweighted") as mine:
        RoundExecutor({"train": TRAINS["arena"]}, s).run(tasks, seed={"init": [init]})
    with pytest.raises(ValueError, match="is unweighted") as theirs:
        replay(tasks, TRAINS["arena"], s, init)
    assert str(mine.value) == str(theirs.value)


def test_aggregate_batch_median_over_mixed_fan_ins():
    """Device arenas, fan-ins 3, 8 and 17 (three capacity classes) in one call, against the CPU contract."""
    torch.manual_seed(9)
    pool = [Small() for _ in range(17)]
    dev = [arena.to_device_arena(m, DEV) for m in pool]
    fans = (3, 8, 17)
    outs = aggregate_batch([(dev[:n], None) for n in fans], method=M.MEDIAN)
    trimmed = aggregate_batch([(dev[:n], None) for n in fans], method=M.TRIMMED_MEAN,
                              settings=types.SimpleNamespace(aggregation_trim=1))
    for n, out, tm in zip(fans, outs, trimmed):
        assert all(q.is_cuda for q in out.parameters())
        for k, (q, t) in enumerate(zip(out.parameters(), tm.parameters())):
            xs = [list(m.parameters())[k].detach() for m in pool[:n]]
            assert ru.same_bits(q.detach().cpu(), ru.median(xs)), f"median, n={n}, parameter {k}"
            assert ru.same_bits(t.detach().cpu(), ru.trimmed_mean(xs, 1)), f"trimmed mean, n={n}, parameter {k}"
