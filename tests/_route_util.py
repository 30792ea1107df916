"""TEST INFRASTRUCTURE for the layer between a list of nn.Modules and the
kernels of the aggregates over n <= 32 models (dasklearn_amd/model_inputs.py;
tests/test_route_util_cpu.py, tests/test_gpu_model_routes.py,
tests/test_gpu_step_streams.py): the routes, builders that turn a list of CPU
models into the list handed to a plugin, the modules with two dtype groups and
with empty parameters, and the checks every result must pass whatever the
route.

A route never changes a value: the oracle of a case is the oracle of its CPU
models on every route.
"""
from __future__ import annotations

import copy
import functools

import numpy as np
import torch
from torch import nn

import _edge_util as eu
import _geomed_util as gu
import _krum_util as ku
import _robust_util as ru
from _sgd_util import BnNet, Net
from sgd_inputs import GNLENET_SHAPES
from dasklearn_amd import arena


# ---- modules ---------------------------------------------------------------------------
class Mixed(nn.Module):
    """Two dtype groups: fp32 231 + 5 elements, bf16 129 + 36 (layout order fp32, bf16)."""

    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(33, 7))
        self.b = nn.Parameter(torch.zeros(129, dtype=torch.bfloat16))
        self.c = nn.Parameter(torch.zeros(5))
        self.d = nn.Parameter(torch.zeros(4, 9, dtype=torch.bfloat16))


class ZeroNet(nn.Module):
    """One empty tensor inside a dtype group and one group that is empty altogether."""

    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(7, 3))
        self.e = nn.Parameter(torch.zeros(0))
        self.c = nn.Parameter(torch.zeros(5))
        self.z = nn.Parameter(torch.zeros(0, dtype=torch.bfloat16))


class EmptyNet(nn.Module):
    """Nothing but one empty parameter."""

    def __init__(self):
        super().__init__()
        self.e = nn.Parameter(torch.zeros(0))


def filled(make, n: int, seed: int, special_frac: float = 0.05):
    """n models from make() whose parameters hold _robust_util.random_rows
    (specials included), every model another draw."""
    models = [make() for _ in range(n)]
    for k, ps in enumerate(zip(*[list(m.parameters()) for m in models])):
        rows = ru.random_rows(ps[0].dtype, n, ps[0].numel(), seed + k, special_frac=special_frac)
        with torch.no_grad():
            for p, r in zip(ps, rows):
                p.copy_(r.reshape(p.shape))
    return models


def mixed_models(f32_rows, bf16_rows):
    """Mixed modules holding the storage rows of the two groups (_edge_util storage)."""
    out = []
    for r32, r16 in zip(f32_rows, bf16_rows):
        m = Mixed()
        with torch.no_grad():
            m.a.copy_(eu.to_torch(r32[:231], "f32").reshape(33, 7))
            m.c.copy_(eu.to_torch(r32[231:], "f32"))
            m.b.copy_(eu.to_torch(r16[:129], "bf16"))
            m.d.copy_(eu.to_torch(r16[129:], "bf16").reshape(4, 9))
        out.append(m)
    return out


# ---- routes ------------------------------------------------------------------------------
BASELINE = ("host", "arena", "tensors")
MIXED_PLACEMENT = ("arena0_host_peers", "host0_device_peers")  # host and device models in one list
TRANSPOSED = ("transposed", "transposed_host")
# one 16-byte aligned row per model reaches the kernel: its bits are the flat entry's on separately placed rows
ONE_ROW_PER_MODEL = ("host", "arena", "arena0_host_peers", "host0_device_peers", "transposed_host")
NAMES = BASELINE + MIXED_PLACEMENT + ("arena_and_tensors",) + TRANSPOSED + ("fed_back",)


def transpose_first_matrix(model: nn.Module) -> nn.Module:
    """The first 2-D parameter re-laid with transposed strides, in place: the
    same shape and values, no longer contiguous."""
    for p in model.parameters():
        if p.dim() == 2:
            p.data = p.data.t().contiguous().t()
            assert not p.is_contiguous(), "a matrix with a unit dimension has no transposed layout"
            return model
    raise AssertionError("the model has no 2-D parameter")


def _place(kind: str, m: nn.Module, dev) -> nn.Module:
    if kind == "host":
        return m
    if kind == "arena":
        return arena.to_device_arena(m, dev)
    assert kind == "tensors"
    return copy.deepcopy(m).to(dev)


_KIND = {
    "host": lambda i: "host",
    "arena": lambda i: "arena",
    "tensors": lambda i: "tensors",
    "arena0_host_peers": lambda i: "arena" if i == 0 else "host",
    "host0_device_peers": lambda i: "host" if i == 0 else "arena" if i % 2 else "tensors",
    "arena_and_tensors": lambda i: "tensors" if i % 2 else "arena",
}


def kinds(name: str, n: int, host=(), device=()):
    """Where each of n models goes under a placement route: "host", "arena" or
    "tensors". `host` / `device`: indices that must be a host model / a device
    model whatever the route says (a device one then is an arena)."""
    assert not set(host) & set(device)
    out = []
    for i in range(n):
        k = _KIND[name](i)
        if i in host:
            k = "host"
        elif i in device and k == "host":
            k = "arena"
        out.append(k)
    return out


def _transposed(cpu, dev):
    models = [copy.deepcopy(m) if dev is None else copy.deepcopy(m).to(dev) for m in cpu]
    for i in sorted({0, len(models) // 2}):
        transpose_first_matrix(models[i])
    return models


def _default_feed(models):
    from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian
    return CoordinateMedian.aggregate(models, to_host=False)


def _fed_back(cpu, dev, feed):
    models = [arena.to_device_arena(m, dev) for m in cpu]
    fed = feed(models[:3])  # the output of an earlier aggregate: a registered arena
    with torch.no_grad():
        for q, p in zip(fed.parameters(), cpu[1].parameters()):
            q.copy_(p)
        for b, s in zip(fed.buffers(), cpu[1].buffers()):
            b.copy_(s)
    assert arena.registered_arenas(fed) is not None, "the fed-back model is no registered arena"
    models[1] = fed
    return models


def routes(dev="cuda", feed=None):
    """name -> build(cpu_models, host=(), device=()): the list handed to a
    plugin. The CPU models are never changed (host routes pass them on as they
    are). `feed`: what makes the fed-back model from the first three arenas
    (default CoordinateMedian.aggregate(..., to_host=False))."""
    feed = _default_feed if feed is None else feed
    out = {}
    for name in _KIND:
        out[name] = (lambda cpu, host=(), device=(), name=name:
                     [_place(k, m, dev) for k, m in zip(kinds(name, len(cpu), host, device), cpu)])
    out["transposed"] = lambda cpu, host=(), device=(): _transposed(cpu, dev)
    out["transposed_host"] = lambda cpu, host=(), device=(): _transposed(cpu, None)
    out["fed_back"] = lambda cpu, host=(), device=(): _fed_back(cpu, dev, feed)
    assert tuple(out) == NAMES
    return out


# ---- what every result must satisfy ----------------------------------------------------------
def storage_of(t: torch.Tensor):
    """(storage address, bytes) of a tensor."""
    s = t.untyped_storage()
    return s.data_ptr(), s.nbytes()


def result_problems(out: nn.Module, models, route: str, to_host=None):
    """What is wrong with a plugin's result module against models[0]: its
    class, every parameter's device (to_host overriding), shape, dtype and
    requires_grad, under the transposed routes its strides, and the buffers:
    equal to models[0]'s, on their device, in storage of their own."""
    m0 = models[0]
    problems = []
    if type(out) is not type(m0):
        problems.append(f"the result is a {type(out).__name__}, models[0] a {type(m0).__name__}")
    got, want = list(out.parameters()), list(m0.parameters())
    if len(got) != len(want):
        return problems + [f"{len(got)} parameters, models[0] has {len(want)}"]
    for k, (g, p0) in enumerate(zip(got, want)):
        on_gpu = p0.is_cuda if to_host is None else not to_host
        if g.is_cuda != on_gpu or (to_host is None and g.device != p0.device):
            problems.append(f"parameter {k} on {g.device}")
        if g.shape != p0.shape or g.dtype != p0.dtype or g.requires_grad != p0.requires_grad:
            problems.append(f"parameter {k}: {tuple(g.shape)} {g.dtype} requires_grad={g.requires_grad}")
        if route in TRANSPOSED and g.stride() != p0.stride():
            problems.append(f"parameter {k}: strides {g.stride()}, models[0]'s {p0.stride()}")
    bufs, bufs0 = list(out.buffers()), list(m0.buffers())
    if len(bufs) != len(bufs0):
        problems.append(f"{len(bufs)} buffers, models[0] has {len(bufs0)}")
    for k, (b, b0) in enumerate(zip(bufs, bufs0)):
        if b.device != b0.device or b.dtype != b0.dtype or not torch.equal(b, b0):
            problems.append(f"buffer {k} differs from models[0]'s")
        (a, na), (c, nc) = storage_of(b), storage_of(b0)
        if b.device == b0.device and na and nc and a < c + nc and c < a + na:
            problems.append(f"buffer {k} shares storage with models[0]'s")
    return problems


def param_bits(model: nn.Module):
    """Per parameter the unsigned bit patterns of its elements in logical (row-major) order."""
    return [ru.bits_of(p.detach().reshape(-1)) for p in model.parameters()]


def same_params(model: nn.Module, want) -> bool:
    """`model`'s parameters against a list of bit-pattern arrays (param_bits)."""
    got = param_bits(model)
    return len(got) == len(want) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def split_bits(row, model: nn.Module):
    """An fp32 storage row as the per-parameter bit arrays of `model` (param_bits' form)."""
    bits, out, off = eu.bits_of(np.asarray(row), "f32"), [], 0
    for p in model.parameters():
        out.append(bits[off:off + p.numel()])
        off += p.numel()
    assert off == bits.size
    return out


# ---- the cases of the route tests: CPU models and what the oracles say, computed once ----------------
def bn_model() -> nn.Module:
    m = BnNet()
    with torch.no_grad():
        m.bn.running_mean.uniform_(-1, 1)
        m.bn.num_batches_tracked.fill_(int(torch.randint(1, 99, ()).item()))
    return m


MAKERS = {"gnlenet": lambda: Net(GNLENET_SHAPES, "f32"), "mixed": Mixed, "bn": bn_model}
BN_SHAPES = gu.BN_SHAPES


def robust_windows(n: int):
    """(name, (lo, hi)): the median, trim 1 and trim 0."""
    lo = (n - 1) // 2
    return (("median", (lo, lo + 1)), ("trim1", (1, n - 1)), ("trim0", (0, n)))


@functools.lru_cache(maxsize=None)
def robust_case(maker: str, n: int):
    """(CPU models, window -> the expected bits of every parameter by
    _robust_util): one sort per parameter serves the three windows."""
    torch.manual_seed(5)
    cpu = filled(MAKERS[maker], n, seed=700 + n, special_frac=0.05)
    want = {w: [] for _, w in robust_windows(n)}
    for ps in zip(*[list(m.parameters()) for m in cpu]):
        sb = ru.sorted_bits([p.detach().reshape(-1) for p in ps], ps[0].dtype)
        for lo, hi in want:
            want[(lo, hi)].append(ru.bits_of(ru.window_mean_sorted(sb, ps[0].dtype, lo, hi)))
    return cpu, want


@functools.lru_cache(maxsize=None)
def krum_case(n: int, f: int, bn: bool = False):
    """_krum_util.plugin_case, or the same on BnNets whose model 0 is Byzantine:
    (rows, Byzantine indices, oracle matrix, CPU models)."""
    if not bn:
        return ku.plugin_case(n, f)
    rows, byz, want, _ = ku.plugin_case(n, f, shapes=BN_SHAPES, byz=(0, 5))
    torch.manual_seed(3)
    return rows, byz, want, [ku.model_of(r, None, "f32", make=bn_model) for r in rows]


@functools.lru_cache(maxsize=None)
def trajectory_case(name: str):
    """A _geomed_util.CASES entry: (case, rows, Byzantine indices, alphas,
    final row, passes, CPU models)."""
    case = gu.CASES[name]
    rows, byz, alphas, want, passes = gu.case_trajectory(case)
    torch.manual_seed(3)
    if case["shapes"] is gu.BN_SHAPES:
        cpu = [ku.model_of(r, None, "f32", make=bn_model) for r in rows]
    else:
        cpu = [ku.model_of(r, case["shapes"], "f32") for r in rows]
    return case, rows, byz, alphas, want, passes, cpu
