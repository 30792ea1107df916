"""The mean around the median and Bulyan on the MI355X: the flat and tensors
entries against the CPU restatement (tests/_nearest_util.py) bit for bit, the
MeanAroundMedian and Bulyan plugins from host models, device arenas and
separate device tensors, and their selection through functions.aggregate and
RoundExecutor (settings.aggregation_trim_rule / aggregation_krum_rule)."""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

import _nearest_util as nu
import _robust_util as ru
from sgd_inputs import GNLENET_SHAPES
from test_gpu_robust import MAKERS, PLACES, _filled, _shifted, _tensor_case
from test_gpu_rounds_krum import TRAINS, Small, replay, same_model

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation import GradientAggregationMethod as M  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Bulyan, bulyan_select, model_distances  # noqa: E402
from dasklearn_amd.gradient_aggregation.robust import MeanAroundMedian, TrimmedMean  # noqa: E402
from dasklearn_amd.rounds import RoundExecutor  # noqa: E402

DEV = "cuda"
FAN_INS = (3, 8, 16, 17, 32)
DTYPES = ["f32", "bf16", "f16", "f64"]


def _check(got: torch.Tensor, want: torch.Tensor, what: str):
    got = got.detach().cpu().reshape(-1)
    assert ru.same_bits(got, want.reshape(-1)), f"{what}: {ru.diff_report(got, want.reshape(-1))}"


def _run(xs_dev, keep):
    out = torch.empty_like(xs_dev[0])
    _native.robust_nearest_reduce(xs_dev, keep, out)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (1, 2) + FAN_INS)
def test_specials_in_every_row_position(n, dtype):
    dt = ru.DTYPES[dtype]
    xs = ru.special_rows(dt, n)
    sb = ru.sorted_bits(xs, dt)
    xd = [x.to(DEV) for x in xs]
    for keep in nu.keeps(n):
        _check(_run(xd, keep), nu.nearest_mean_sorted(sb, dt, keep), f"{dtype} n={n} keep={keep}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", FAN_INS)
def test_keep_one_and_keep_n_equal_the_rank_window_entry(n, dtype):
    dt = ru.DTYPES[dtype]
    xd = [x.to(DEV) for x in ru.random_rows(dt, n, 4099, seed=60 + n)]
    lo = (n - 1) // 2
    for keep, (a, b) in ((1, (lo, lo + 1)), (n, (0, n))):
        want = torch.empty_like(xd[0])
        _native.robust_reduce(xd, a, b, want)
        assert ru.same_bits(_run(xd, keep).cpu(), want.cpu()), f"keep {keep}"


def test_the_window_moves_with_the_values():
    """Not the rank window of the same kept count (the CPU suite checks that
    these inputs tell the two apart)."""
    xs = ru.random_rows(torch.float32, 8, 20_000, seed=7, special_frac=0)
    xd = [x.to(DEV) for x in xs]
    got = _run(xd, 4)
    _check(got, nu.nearest_mean(xs, 4), "n=8 keep=4")
    assert not ru.same_bits(got.cpu(), ru.window_mean(xs, 2, 6))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
@pytest.mark.parametrize("n", (3, 8, 17, 32))
def test_row_order_does_not_matter(n, dtype):
    dt = ru.DTYPES[dtype]
    xs = ru.random_rows(dt, n, 4099, seed=77 + n)
    perm = np.random.default_rng(n).permutation(n)
    a = [x.to(DEV) for x in xs]
    b = [a[i] for i in perm]
    for keep in nu.keeps(n):
        ga, gb = _run(a, keep), _run(b, keep)
        assert ru.same_bits(ga.cpu(), gb.cpu()), f"keep {keep}"
    _check(ga, nu.nearest_mean(xs, keep), "the last kept count against the restatement")


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_input_then_output(dtype):
    dt = ru.DTYPES[dtype]
    n, p = 5, 4097
    xs = ru.random_rows(dt, n, p, seed=5)
    want = nu.nearest_mean(xs, 3)
    xd = [x.to(DEV) for x in xs]
    one_off = list(xd)
    one_off[3] = _shifted(xs[3], 1)
    _check(_run(one_off, 3), want, "one input off alignment")
    out = torch.empty(p + 16, dtype=dt, device=DEV)[1:p + 1]
    _native.robust_nearest_reduce(xd, 3, out)
    _check(out, want, "the output off alignment")


def test_overlapping_output_and_a_bad_keep_are_refused_and_nothing_runs():
    p = 1000
    buf = torch.zeros(3 * p, device=DEV)
    xs = [buf[:p], buf[p:2 * p]]
    buf[:2 * p] = 1.0
    torch.cuda.synchronize()
    for out in (buf[:p], buf[p // 2:p // 2 + p], buf[2 * p - 1:3 * p - 1]):
        with pytest.raises(_native.DlsimError) as e:
            _native.robust_nearest_reduce(xs, 1, out)
        assert e.value.rc == _native.DLSIM_E_ARG and "overlap" in str(e.value)
    for keep in (0, 3):
        with pytest.raises(_native.DlsimError) as e:
            _native.robust_nearest_reduce(xs, keep, buf[2 * p:])
        assert e.value.rc == _native.DLSIM_E_ARG and "keep" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf[:2 * p] == 1.0).all()) and bool((buf[2 * p:] == 0.0).all())


def _tensors_call(tensors, n, numels, offs, esz, keep, dt):
    out = torch.zeros(sum(numels), dtype=dt, device=DEV)
    _native.robust_nearest_reduce_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels,
                                              [int(o) * esz for o in offs], keep, out.data_ptr(),
                                              _native.dtype_code(dt, single_task=True),
                                              torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
def test_tensors_entry_on_the_gnlenet_shapes_equals_t_flat_calls(dtype):
    n = 8
    dt, numels, rows, offs, tensors = _tensor_case(GNLENET_SHAPES, dtype, n, seed=11)
    assert sum(numels) == 85_354
    for keep in (1, 4, 6):
        out = _tensors_call(tensors, n, numels, offs, rows[0].element_size(), keep, dt)
        _check(out, nu.nearest_mean(rows, keep), f"{dtype} keep {keep}")
        for k, (o, size) in enumerate(zip(offs, numels)):
            flat = _run([row[k].reshape(-1) for row in tensors], keep)
            assert ru.same_bits(out[int(o):int(o) + size].cpu(), flat.cpu()), f"tensor {k}"


def test_tensors_entry_skips_a_zero_element_tensor():
    n = 3
    dt, numels, rows, offs, tensors = _tensor_case([[5], [0], [3, 7]], "f32", n, seed=12)
    out = _tensors_call(tensors, n, numels, offs, 4, 2, dt)
    _check(out, nu.nearest_mean(rows, 2), "keep 2 over three tensors, one empty")


# ---- the plugins, end to end -----------------------------------------------------------
def _expect(models_cpu, keep):
    return [nu.nearest_mean([p.detach().reshape(-1) for p in ps], keep)
            for ps in zip(*[list(m.parameters()) for m in models_cpu])]


def _check_module(out, want, models, what):
    got = list(out.parameters())
    assert type(out) is type(models[0]) and len(got) == len(want)
    for k, (g, w, p0) in enumerate(zip(got, want, models[0].parameters())):
        assert g.device == p0.device and g.shape == p0.shape and g.dtype == p0.dtype
        assert g.requires_grad == p0.requires_grad and g.stride() == p0.stride()
        _check(g, w, f"{what} parameter {k}")
    bufs, bufs0 = list(out.buffers()), list(models[0].buffers())
    assert len(bufs) == len(bufs0)
    for b, b0 in zip(bufs, bufs0):
        assert b.device == b0.device and torch.equal(b, b0) and b.data_ptr() != b0.data_ptr()


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_mean_around_median_end_to_end(maker, place):
    n = 7
    cpu = _filled(MAKERS[maker], n, seed=510)
    models = [PLACES[place](m) for m in cpu]
    before = [[p.detach().clone() for p in m.parameters()] for m in models]
    for agg, kw, keep in ((MeanAroundMedian, {}, 5), (MeanAroundMedian.with_trim(2), {}, 3),
                          (MeanAroundMedian.with_trim(0), {}, 7), (MeanAroundMedian, {"keep": 4}, 4)):
        out = agg.aggregate(models, **kw)
        _check_module(out, _expect(cpu, keep), models, f"{agg.__name__} {maker}/{place}")
    for m, saved in zip(models, before):
        for p, s in zip(m.parameters(), saved):
            assert ru.same_bits(p.detach().cpu(), s.cpu()), "an input model changed"
    out = MeanAroundMedian.aggregate(models, to_host=(place != "host"))
    assert all(p.is_cuda == (place == "host") for p in out.parameters())
    for g, w in zip(out.parameters(), _expect(cpu, 5)):
        _check(g, w, "to_host overridden")
    # keep = 1 and keep = n are the median and the trim-0 mean of the rank-window plugins
    for keep, ref in ((1, TrimmedMean.with_trim(3)), (n, TrimmedMean.with_trim(0))):
        a, b = MeanAroundMedian.aggregate(models, keep=keep), ref.aggregate(models)
        assert same_model(a, b), f"keep {keep}"


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("n,f", [(7, 1), (11, 2)])
def test_bulyan_end_to_end(n, f, place):
    """Peer 0 sends NaNs and the last peer a scaled model: neither is selected,
    the result is finite, equal to MeanAroundMedian over the selected models
    bit for bit, and wears models[0]'s buffers although models[0] is left out.

    (Two broken peers are one more than f = 1 promises to survive at n = 7:
    the last of the five selections is made among the NaN peer, the scaled
    peer and one honest peer, where the scaled and the honest one are each
    other's nearest neighbour and score the same; the tie goes to the lower
    index, the honest peer's. Hence the scaled peer's place at the end.)"""
    cpu = _filled(MAKERS["bn"], n, seed=520 + n, special_frac=0.0)
    with torch.no_grad():
        for p in cpu[0].parameters():
            p.fill_(float("nan"))
        for p in cpu[n - 1].parameters():
            p.mul_(100.0)
    models = [PLACES[place](m) for m in cpu]
    theta = n - 2 * f
    sel = bulyan_select(model_distances(models).tolist(), f)
    assert len(sel) == theta and 0 not in sel and n - 1 not in sel
    plugin = Bulyan.with_params(f)
    out = plugin.aggregate(models)
    want = _expect([cpu[i] for i in sel], theta - 2 * f)
    _check_module(out, want, models, f"Bulyan n={n} f={f} {place}")
    assert all(bool(torch.isfinite(p).all()) for p in out.parameters())
    ref = MeanAroundMedian.aggregate([models[i] for i in sel], keep=theta - 2 * f)
    assert same_model(out, ref)
    assert not torch.equal(out.bn.running_mean.cpu(), models[sel[0]].bn.running_mean.cpu())
    dev_out = plugin.aggregate(models, to_host=False)
    assert all(p.is_cuda for p in dev_out.parameters()) and same_model(dev_out, out)
    with pytest.raises(ValueError, match="4\\*f \\+ 3"):
        Bulyan.with_params(f + 1).aggregate(models[:4 * f + 6])


def test_bulyan_with_no_byzantine_peer_is_the_sorted_mean_of_everyone():
    cpu = _filled(MAKERS["mixed"], 5, seed=530)
    out = Bulyan.with_params(0).aggregate(cpu)
    for g, w in zip(out.parameters(), _expect(cpu, 5)):
        _check(g, w, "f = 0")


CONFIGS = {"median": (M.TRIMMED_MEAN, {"aggregation_trim_rule": "median", "aggregation_trim": 2}),
           "bulyan": (M.MULTI_KRUM, {"aggregation_krum_rule": "bulyan", "aggregation_byzantine": 1})}


def _plugin(config):
    return MeanAroundMedian.with_trim(2) if config == "median" else Bulyan.with_params(1)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_functions_aggregate_through_model_manager(config):
    n = 8
    method, extra = CONFIGS[config]
    cpu = _filled(MAKERS["gnlenet"], n, seed=800)
    settings = types.SimpleNamespace(gradient_aggregation=method, **extra)
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0})
    assert isinstance(res, list) and len(res) == 1
    want = _plugin(config).aggregate(cpu)
    assert all(not p.is_cuda for p in res[0].parameters()) and same_model(res[0], want)
    if config == "median":
        for g, w in zip(res[0].parameters(), _expect(cpu, 4)):
            _check(g, w, "the restatement")
    settings.aggregate_on_device = True
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": None})
    assert all(p.is_cuda for p in res[0].parameters()) and same_model(res[0], want)
    with pytest.raises(ValueError, match="unweighted"):
        functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0, "weights": [1 / n] * n})
    # the rank rule and Multi-Krum compute something else on the same models
    plain = types.SimpleNamespace(gradient_aggregation=method, aggregation_trim=2, aggregation_byzantine=1)
    assert not same_model(functions.aggregate(plain, {"models": cpu, "round": 1, "peer": 0})[0], want)


PEERS, ROUNDS = 9, 2


def _dag():
    """Round r: every one of nine peers trains, then aggregates its own and
    its six nearest ring neighbours' trained models (fan-in 7)."""
    tasks = []
    for r in range(1, ROUNDS + 1):
        for p in range(PEERS):
            model = ("init", 0) if r == 1 else (f"agg_{p}_{r - 1}", 0)
            tasks.append((f"train_{p}_{r}", "train", {"model": model, "round": r, "peer": p}))
        for p in range(PEERS):
            models = [(f"train_{(p + d) % PEERS}_{r}", 0) for d in (-3, -2, -1, 0, 1, 2, 3)]
            tasks.append((f"agg_{p}_{r}", "aggregate", {"models": models, "round": r, "peer": p}))
    return tasks


@pytest.mark.parametrize("place", ["host", "arena", "tensors"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_round_executor_equals_the_per_task_replay(config, place):
    method, extra = CONFIGS[config]
    torch.manual_seed(5)
    init, tasks = Small(), _dag()
    s = types.SimpleNamespace(gradient_aggregation=method, aggregate_on_device=True, **extra)
    want = replay(tasks, TRAINS[place], s, init)
    got = RoundExecutor({"train": TRAINS[place]}, s).run(tasks, seed={"init": [init]})
    fed = RoundExecutor({"train": TRAINS[place]}, types.SimpleNamespace(
        gradient_aggregation=M.FEDAVG, aggregate_on_device=True)).run(tasks, seed={"init": [init]})
    for p in range(PEERS):
        a, b = got[f"agg_{p}_{ROUNDS}"][0], want[f"agg_{p}_{ROUNDS}"][0]
        assert all(q.is_cuda for q in a.parameters())
        assert same_model(a, b), f"peer {p}: the executor and functions.aggregate disagree"
        assert all(x.stride() == y.stride() for x, y in zip(a.parameters(), b.parameters()))
        assert not same_model(a, fed[f"agg_{p}_{ROUNDS}"][0])
