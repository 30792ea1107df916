"""The fresh-SGD step on the MI355X (dlsim_sgd_step, dlsim_sgd_step_tensors,
functions.gradient_update) against the reference's fixtures (tests/golden/sgd/)
and against torch.optim.SGD on CPU tensors, bit for bit (oracle.same_bits).

The CPU reference runs at the reference worker's 4 torch threads: PyTorch's
bf16 result depends on where each thread's vector loop ends, and
that is the layout the kernel reproduces."""
from __future__ import annotations

import os
import types

import numpy as np
import pytest
import torch

from _sgd_util import (TORCH_DTYPES, Net, fixture_gradients, fixture_model, flat_params, settings_of, to_array,
                       to_tensor, torch_flat_step, torch_sgd_step)
from oracle import fedavg_torch
from oracle import oracle as orc
from sgd_inputs import GNLENET_SHAPES, NP_DTYPES, load_sgd, seeded_pair, sgd_paths, split

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.sgd import sgd_step_module  # noqa: E402

FIXTURES = {os.path.basename(p)[:-4]: p for p in sgd_paths()}
DEV = "cuda"
LR = 0.1
# elements of one full tile of the flat kernel at these sizes (dispatch.hpp
# fixed_shape, class 0: 256 lanes x VPT 16-byte vectors; VPT 2, bf16 VPT 1)
TILE = {"f32": 2048, "bf16": 2048, "f64": 1024}
SIZES = (1, 3, 4, 5, 1023, 1024, 1025)
CASES = [(d, wd) for d in ("f32", "bf16", "f64") for wd in (0.0, 5e-4)]


def _skip_unless_pinned(meta):
    cap = torch.backends.cpu.get_cpu_capability()
    if meta["torch_version"] != torch.__version__ or meta["cpu_capability"] != cap:
        pytest.skip(f"fixture made with torch {meta['torch_version']} / {meta['cpu_capability']}, "
                    f"this is {torch.__version__} / {cap}")


def _shifted(t: torch.Tensor, shift: int) -> torch.Tensor:
    """A device copy of flat `t` whose base is `shift` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()]
    v.copy_(t)
    return v


_REF = {}


def _pair(dtype, n, wd):
    """Seeded (param, grad) CPU tensors of n elements and torch's result, computed once."""
    key = (dtype, n, wd)
    if key not in _REF:
        if n > 1_000_000:  # the launch-shape sizes, drawn the quick way
            rng = np.random.Generator(np.random.PCG64(n))
            if dtype == "bf16":  # random bits with the exponent kept in 2^-15 .. 1
                a, g = [(rng.integers(0, 1 << 16, n, dtype=np.uint16) & 0x87ff) | 0x3800 for _ in range(2)]
            else:
                x = rng.standard_normal((2, n), dtype=np.float32)
                a, g = [(x[i] * np.float32(s)).astype(NP_DTYPES[dtype]) for i, s in ((0, 0.05), (1, 0.01))]
        else:
            a, g = seeded_pair(n, 1000 + n % 997, dtype)
        p, g = to_tensor(a, dtype), to_tensor(g, dtype)
        _REF[key] = (p, g, to_array(torch_flat_step(p, g, LR, wd)))
    return _REF[key]


# ---- the flat entry ----------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(c for c in FIXTURES if c.startswith("specials_")))
def test_flat_entry_matches_the_specials_fixtures(case):
    fx = load_sgd(FIXTURES[case])
    meta = fx["meta"]
    _skip_unless_pinned(meta)
    p, g = to_tensor(fx["params"], meta["dtype"]).to(DEV), to_tensor(fx["grads"], meta["dtype"]).to(DEV)
    out = torch.empty_like(p)
    _native.sgd_step(p, g, out, meta["lr"], meta["weight_decay"])
    assert orc.same_bits(to_array(out), fx["expected"])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_flat_entry_matches_the_gnlenet_fixtures(dtype):
    """fp32 / fp64 round per element whatever the tensor boundaries, so the
    model's 14 tensors are one flat buffer (bf16: the tensors entry below)."""
    for case in (f"gnlenet_{dtype}_wd", f"gnlenet_{dtype}_nowd"):
        if case not in FIXTURES:
            continue
        fx = load_sgd(FIXTURES[case])
        meta = fx["meta"]
        p, g = to_tensor(fx["params"], dtype).to(DEV), to_tensor(fx["grads"], dtype).to(DEV)
        out = torch.empty_like(p)
        _native.sgd_step(p, g, out, meta["lr"], meta["weight_decay"])
        assert orc.same_bits(to_array(out), fx["expected"]), case


@pytest.mark.parametrize("dtype,wd", CASES)
def test_flat_entry_sizes_alignments_and_in_place(dtype, wd):
    t = TILE[dtype]
    for n in SIZES + (t - 1, t, t + 1, 85_354):
        p, g, expect = _pair(dtype, n, wd)
        for shifts in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
            dp, dg = _shifted(p, shifts[0]), _shifted(g, shifts[1])
            out = _shifted(torch.zeros_like(p), shifts[2])
            _native.sgd_step(dp, dg, out, LR, wd)
            assert orc.same_bits(to_array(out), expect), (n, shifts)
            assert orc.same_bits(to_array(dp), to_array(p)) and orc.same_bits(to_array(dg), to_array(g))
        for shift in (0, 1):
            dp, dg = _shifted(p, shift), _shifted(g, shift)
            _native.sgd_step(dp, dg, dp, LR, wd)  # in place on the parameter
            assert orc.same_bits(to_array(dp), expect), (n, shift, "param")
            dp = _shifted(p, shift)
            _native.sgd_step(dp, dg, dg, LR, wd)  # in place on the gradient
            assert orc.same_bits(to_array(dg), expect), (n, shift, "grad")


# the sizes at which the flat entry changes its launch shape (8 MB and 20 MB per
# stream for 4/8-byte elements, 96 MB for bf16), a few elements past each
@pytest.mark.parametrize("dtype,n", [("f32", 2_000_003), ("f32", 5_000_003), ("f64", 1_000_003),
                                     ("f64", 2_500_003), ("bf16", 48_000_005)])
def test_flat_entry_launch_shapes(dtype, n):
    p, g, expect = _REF.pop((dtype, n, 5e-4), None) or _pair(dtype, n, 5e-4)
    _REF.pop((dtype, n, 5e-4), None)  # large: not kept
    dp, dg = p.to(DEV), g.to(DEV)
    out = torch.empty_like(dp)
    _native.sgd_step(dp, dg, out, LR, 5e-4)
    assert orc.same_bits(to_array(out), expect)


def test_rejected_arguments_raise():
    p = torch.zeros(64, device=DEV)
    big = torch.zeros(128, device=DEV)
    with pytest.raises(_native.DlsimError, match="overlaps"):
        _native.sgd_step(big[:64], p, big[8:72], 0.1, 0.0)
    with pytest.raises(_native.DlsimError):
        _native.sgd_step(p, p.clone(), p.clone(), -0.1, 0.0)
    h = torch.zeros(64, device=DEV, dtype=torch.float16)
    with pytest.raises(_native.DlsimError):
        _native.sgd_step(h, h.clone(), h.clone(), 0.1, 0.0)


# ---- the tensors entry ---------------------------------------------------------------

def _run_tensors(ps, gs, lr, wd):
    dps, dgs = [p.to(DEV) for p in ps], [g.to(DEV) for g in gs]
    outs = [torch.empty_like(p) for p in dps]
    _native.sgd_step_tensors(dps, dgs, outs, lr, wd)
    singles = [torch.empty_like(p) for p in dps]
    for p, g, o in zip(dps, dgs, singles):
        _native.sgd_step(p, g, o, lr, wd)
    return outs, singles


@pytest.mark.parametrize("case", sorted(c for c in FIXTURES if c.startswith("gnlenet_")))
def test_tensors_entry_matches_the_gnlenet_fixtures(case):
    fx = load_sgd(FIXTURES[case])
    meta = fx["meta"]
    _skip_unless_pinned(meta)
    ps = [to_tensor(a.reshape(-1), meta["dtype"]) for a in split(fx["params"], meta["shapes"])]
    gs = [to_tensor(a.reshape(-1), meta["dtype"]) for a in split(fx["grads"], meta["shapes"])]
    outs, singles = _run_tensors(ps, gs, meta["lr"], meta["weight_decay"])
    assert orc.same_bits(np.concatenate([to_array(o) for o in outs]), fx["expected"])
    assert orc.same_bits(np.concatenate([to_array(o) for o in singles]), fx["expected"])


@pytest.mark.parametrize("dtype,wd", CASES)
def test_tensors_entry_many_small_tensors(dtype, wd):
    """70 tensors of 1 .. 3000 elements: more than one launch's 64 slots; bases
    as torch's allocator gives them and, for every third, one element off."""
    rng = np.random.Generator(np.random.PCG64(7))
    sizes = [1, 2, 3, 7, 8, 9, 10, 31, 32, 33, 2047, 2048, 2049, 3000] + [int(s) for s in rng.integers(1, 3001, 56)]
    assert len(sizes) == 70
    ps, gs, expect = zip(*[_pair(dtype, n, wd) for n in sizes])
    dps = [_shifted(p, 1 if k % 3 == 2 else 0) for k, p in enumerate(ps)]
    dgs = [g.to(DEV) for g in gs]
    outs = [torch.empty_like(g) for g in dgs]
    _native.sgd_step_tensors(dps, dgs, outs, LR, wd)
    for k, (p, g, o, e) in enumerate(zip(dps, dgs, outs, expect)):
        single = torch.empty_like(o)
        _native.sgd_step(p, g, single, LR, wd)
        assert orc.same_bits(to_array(o), to_array(single)), (k, sizes[k])
        assert orc.same_bits(to_array(o), e), (k, sizes[k])
    # in place on the parameters, one call
    _native.sgd_step_tensors(dps, dgs, dps, LR, wd)
    for k, (p, e) in enumerate(zip(dps, expect)):
        assert orc.same_bits(to_array(p), e), (k, sizes[k])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tensors_entry_with_a_large_tensor(dtype):
    """A tensor above 1 MiB moves the batch to 4 vectors per lane; bf16 at this
    size also crosses torch's parallel split (>= 32768 elements)."""
    sizes = [600_001, 10, 4096, 70_000]
    ps, gs, expect = zip(*[_pair(dtype, n, 5e-4) for n in sizes])
    outs, singles = _run_tensors(ps, gs, LR, 5e-4)
    for o, s, e, n in zip(outs, singles, expect, sizes):
        assert orc.same_bits(to_array(o), to_array(s)), n
        assert orc.same_bits(to_array(o), e), n


def test_tensors_entry_overlapping_list_runs_in_order():
    """Tensor 1 reads what tensor 0 writes: the list runs as two launches in
    order, as two single calls would."""
    p0, g0, _ = _pair("f32", 1025, 5e-4)
    dp0, dg0 = p0.to(DEV), g0.to(DEV)
    mid = torch.empty_like(dp0)
    outs = [mid, torch.empty_like(dp0)]
    _native.sgd_step_tensors([dp0, mid], [dg0, dg0], outs, LR, 5e-4)
    first = torch_flat_step(p0, g0, LR, 5e-4)
    assert orc.same_bits(to_array(outs[1]), to_array(torch_flat_step(first, g0, LR, 5e-4)))


# ---- the task ------------------------------------------------------------------------

def _task(model, grads, meta):
    gm = types.SimpleNamespace(gradient=grads)
    return functions.gradient_update(settings_of(meta["lr"], meta["momentum"], meta["weight_decay"]),
                                     {"model": model, "gradient_model": gm})[0]


@pytest.mark.parametrize("case", sorted(c for c in FIXTURES if not c.startswith("specials_")))
def test_task_host_model_gives_host_model(case):
    fx = load_sgd(FIXTURES[case])
    meta = fx["meta"]
    _skip_unless_pinned(meta)
    model, grads = fixture_model(fx), fixture_gradients(fx)
    model.gradient = ["stale"]
    before, gbefore = flat_params(model), [to_array(g) for g in grads]
    out = _task(model, grads, meta)
    assert type(out) is type(model) and out is not model and not hasattr(out, "gradient")
    assert all(not p.is_cuda and p.requires_grad and p.grad is None for p in out.parameters())
    assert [tuple(p.shape) for p in out.parameters()] == [tuple(p.shape) for p in model.parameters()]
    assert orc.same_bits(flat_params(out), fx["expected"])
    for a, b in zip(model.buffers(), out.buffers()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    assert orc.same_bits(flat_params(model), before)  # the inputs are only read
    assert all(orc.same_bits(to_array(g), b) for g, b in zip(grads, gbefore))
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("case", ["gnlenet_f32_wd", "gnlenet_bf16_wd", "gnlenet_f64_wd", "buffers_bn_f32",
                                  "short_f32", "short_bf16"])
def test_task_device_arena_model_gives_device_model(case):
    fx = load_sgd(FIXTURES[case])
    meta = fx["meta"]
    _skip_unless_pinned(meta)
    host = fixture_model(fx)
    model = arena.to_device_arena(host, DEV)
    grads = [g.to(DEV) for g in fixture_gradients(fx)]
    before = flat_params(model)
    out = _task(model, grads, meta)
    assert type(out) is type(host) and all(p.is_cuda and p.requires_grad for p in out.parameters())
    assert orc.same_bits(flat_params(out), fx["expected"])
    assert arena.registered_arenas(out) is not None  # again a module over one device arena
    for a, b in zip(model.buffers(), out.buffers()):
        assert torch.equal(a, b) and a.device == b.device and a.data_ptr() != b.data_ptr()
    assert orc.same_bits(flat_params(model), before)
    # separate device tensors (no arena) take the same kernels
    plain = fixture_model(fx).to(DEV)
    assert orc.same_bits(flat_params(_task(plain, grads, meta)), fx["expected"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_aggregate_then_gradient_update_matches_the_cpu_chain(dtype):
    """AD-PSGD's passive peer: the fan-in-2 aggregate's output (one device
    arena) is stepped with a gradient; against oracle.fedavg_torch + torch SGD."""
    hosts = []
    for seed in (31, 32):
        a, _ = seeded_pair(sum(int(np.prod(s)) for s in GNLENET_SHAPES), seed, dtype)
        m = Net(GNLENET_SHAPES, dtype)
        with torch.no_grad():
            for p, x in zip(m.parameters(), split(a, GNLENET_SHAPES)):
                p.copy_(to_tensor(x, dtype).reshape(p.shape))
        hosts.append(m)
    _, g = seeded_pair(sum(int(np.prod(s)) for s in GNLENET_SHAPES), 33, dtype)
    grads = [to_tensor(x, dtype).reshape(s) for x, s in zip(split(g, GNLENET_SHAPES), GNLENET_SHAPES)]
    agg = FedAvg.aggregate([arena.to_device_arena(m, DEV) for m in hosts], None)
    out = sgd_step_module(agg, [x.to(DEV) for x in grads], 0.05, 0.9, 1e-3)
    cpu = torch_sgd_step(fedavg_torch.aggregate_modules(hosts, None), grads, 0.05, 0.9, 1e-3)
    assert all(p.is_cuda for p in out.parameters())
    assert orc.same_bits(flat_params(out), flat_params(cpu))


def test_mixed_dtype_model_steps_per_group():
    """fp32, bf16 and fp16 parameters in one model: a kernel launch per kernel
    dtype, torch's CPU ops for the fp16 group."""
    shapes = [[40, 3], [40], [129], [7]]
    dts = ["f32", "bf16", "f16", "f32"]
    g = torch.Generator().manual_seed(9)
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(TORCH_DTYPES[d]))
                                       for s, d in zip(shapes, dts)])
    grads = [(torch.randn(s, generator=g) * 0.01).to(TORCH_DTYPES[d]) for s, d in zip(shapes, dts)]
    cpu = torch_sgd_step(model, grads, 0.1, 0.9, 5e-4, threads=torch.get_num_threads())
    for m, gs in ((model, grads), (arena.to_device_arena(model, DEV), [x.to(DEV) for x in grads])):
        out = sgd_step_module(m, gs, 0.1, 0.9, 5e-4)
        for q, e in zip(out.parameters(), cpu.parameters()):
            assert q.dtype == e.dtype and q.is_cuda == next(m.parameters()).is_cuda
            assert orc.same_bits(to_array(q), to_array(e)), q.dtype
