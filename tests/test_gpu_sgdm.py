"""The stateful momentum-SGD step on the MI355X (dlsim_sgd_momentum_step,
dlsim_sgd_momentum_step_tensors, dasklearn_amd.optimizer) against the
reference's fixtures (tests/golden/sgdm/) and against
torch.optim.SGD(foreach=False) on CPU copies at the reference worker's 4 torch
threads, bit for bit (oracle.same_bits): parameters and momentum buffers."""
from __future__ import annotations

import copy
import os

import numpy as np
import pytest
import torch

from _sgd_util import Net, flat_params, to_array, to_tensor, torch_threads
from _sgdm_util import fixture_model, fixture_steps, flat_buffers, run_rounds, torch_rounds
from oracle import fedavg_torch
from oracle import oracle as orc
from sgd_inputs import GNLENET_SHAPES, NP_DTYPES, seeded_pair, split
from sgdm_inputs import load_sgdm, sgdm_paths

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.optimizer import ArenaSGD, SGDOptimizer  # noqa: E402

FIXTURES = {os.path.basename(p)[:-4]: p for p in sgdm_paths()}
DEV = "cuda"
LR, MOM = 0.1, 0.9
SIZES = (1, 7, 31, 32, 33, 1023, 1024, 1025, 4097, 85_354)
BF16_SIZES = (32_767, 32_768, 32_801, 131_077)  # where ATen's range split and vector tails move
CASES = [(d, wd) for d in ("f32", "f64", "bf16") for wd in (0.0, 5e-4)]
PER_LAUNCH = _native.SGD_MOMENTUM_TENSORS_PER_LAUNCH


def _sizes(dtype):
    return SIZES + (BF16_SIZES if dtype == "bf16" else ())


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


def _torch_step(p, g, buf, wd, lr=LR, mom=MOM):
    """One torch.optim.SGD(foreach=False) step on flat CPU tensors, `buf` the
    momentum buffer it holds (None: a fresh optimizer). Returns (param, buffer)."""
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd, foreach=False)
    if buf is not None:
        opt.state[q]["momentum_buffer"] = buf.detach().clone()
    with torch_threads(4):
        opt.step()
    return q.detach(), opt.state[q]["momentum_buffer"]


def _draw(dtype, n, seed):
    if n > 1_000_000:  # the launch-shape sizes, drawn the quick way
        rng = np.random.Generator(np.random.PCG64(seed))
        if dtype == "bf16":  # random bits with the exponent kept in 2^-15 .. 1
            return [(rng.integers(0, 1 << 16, n, dtype=np.uint16) & 0x87ff) | 0x3800 for _ in range(2)]
        x = rng.standard_normal((2, n), dtype=np.float32)
        return [(x[i] * np.float32(s)).astype(NP_DTYPES[dtype]) for i, s in ((0, 0.05), (1, 0.01))]
    return seeded_pair(n, seed, dtype)


_REF = {}


def _chain(dtype, n, wd, steps=3):
    """Seeded CPU tensors and torch's three steps from a fresh optimizer,
    computed once: (p0, [g_s], [(p after step s, buffer after step s)])."""
    key = (dtype, n, wd, steps)
    if key not in _REF:
        a, g0 = _draw(dtype, n, 2000 + n % 997)
        gs = [g0] + [_draw(dtype, n, 3000 + 7 * s + n % 997)[1] for s in range(1, steps)]
        p0, gs = to_tensor(a, dtype), [to_tensor(g, dtype) for g in gs]
        after, p, b = [], p0, None
        for g in gs:
            p, b = _torch_step(p, g, b, wd)
            after.append((p, b))
        _REF[key] = (p0, gs, after)
    return _REF[key]


def _same(t, e):
    return orc.same_bits(to_array(t), to_array(e))


# ---- the flat entry ----------------------------------------------------------------

@pytest.mark.parametrize("dtype,wd", CASES)
def test_flat_entry_first_and_later_steps(dtype, wd):
    """A first step and two later steps at every size, in place and into
    separate outputs (inputs then unchanged)."""
    for n in _sizes(dtype):
        p0, gs, after = _chain(dtype, n, wd)
        dp, db = p0.to(DEV), torch.zeros_like(p0, device=DEV)
        for s, (g, (ep, eb)) in enumerate(zip(gs, after)):
            dg = g.to(DEV)
            # separate outputs, from the state before this step
            po, bo = torch.empty_like(dp), torch.empty_like(dp)
            pin, bin_ = dp.clone(), db.clone()
            _native.sgd_momentum_step(pin, dg, None if s == 0 else bin_, po, bo, LR, MOM, wd)
            assert _same(po, ep) and _same(bo, eb), (n, s, "separate")
            assert _same(pin, dp) and _same(bin_, db) and _same(dg, g), (n, s, "inputs written")
            # in place
            _native.sgd_momentum_step(dp, dg, None if s == 0 else db, dp, db, LR, MOM, wd)
            assert _same(dp, ep) and _same(db, eb), (n, s, "in place")
            assert _same(dg, g)


@pytest.mark.parametrize("dtype,wd", CASES)
def test_flat_entry_each_buffer_off_alignment(dtype, wd):
    """Each of the five buffers in turn one element off a 16-byte boundary
    (a later step; and the four of a first step)."""
    for n in _sizes(dtype):
        p0, gs, after = _chain(dtype, n, wd)
        (p1, b1), (p2, b2) = after[0], after[1]
        for off in range(5):
            sh = [1 if k == off else 0 for k in range(5)]
            dp, dg, db = _shifted(p1, sh[0]), _shifted(gs[1], sh[1]), _shifted(b1, sh[2])
            po, bo = _shifted(torch.zeros_like(p1), sh[3]), _shifted(torch.zeros_like(p1), sh[4])
            _native.sgd_momentum_step(dp, dg, db, po, bo, LR, MOM, wd)
            assert _same(po, p2) and _same(bo, b2), (n, off, "later")
            if off != 2:
                dp, dg = _shifted(p0, sh[0]), _shifted(gs[0], sh[1])
                po, bo = _shifted(torch.zeros_like(p1), sh[3]), _shifted(torch.zeros_like(p1), sh[4])
                _native.sgd_momentum_step(dp, dg, None, po, bo, LR, MOM, wd)
                assert _same(po, p1) and _same(bo, b1), (n, off, "first")
        # in place with parameter and buffer both misaligned
        dp, db = _shifted(p1, 1), _shifted(b1, 1)
        _native.sgd_momentum_step(dp, gs[1].to(DEV), db, dp, db, LR, MOM, wd)
        assert _same(dp, p2) and _same(db, b2), (n, "in place, misaligned")


# the first size of each launch-shape class of the flat kernel (dispatch.hpp
# fixed_shape by bytes per stream: 8 MB and 20 MB for 4/8-byte elements, 96 MB
# for bf16; class 0 is every size above), a few elements past each: a first
# step and a later step
@pytest.mark.parametrize("dtype,n", [("f32", 2_000_003), ("f32", 5_000_003), ("f64", 1_000_003),
                                     ("f64", 2_500_003), ("bf16", 48_000_005)])
def test_flat_entry_launch_shapes(dtype, n):
    p0, gs, after = _chain(dtype, n, 5e-4, steps=2)
    _REF.pop((dtype, n, 5e-4, 2), None)  # large: not kept
    dp, db = p0.to(DEV), torch.empty_like(p0, device=DEV)
    _native.sgd_momentum_step(dp, gs[0].to(DEV), None, dp, db, LR, MOM, 5e-4)
    assert _same(dp, after[0][0]) and _same(db, after[0][1])
    _native.sgd_momentum_step(dp, gs[1].to(DEV), db, dp, db, LR, MOM, 5e-4)
    assert _same(dp, after[1][0]) and _same(db, after[1][1])


def test_rejected_arguments_raise():
    p, g, b = (torch.zeros(64, device=DEV) for _ in range(3))
    big = torch.zeros(128, device=DEV)
    with pytest.raises(_native.DlsimError, match="overlaps"):
        _native.sgd_momentum_step(big[:64], g, b, big[8:72], b, 0.1, 0.9, 0.0)
    with pytest.raises(_native.DlsimError, match="overlaps"):
        _native.sgd_momentum_step(p, g, b, g, b, 0.1, 0.9, 0.0)  # the gradient is never written
    with pytest.raises(_native.DlsimError, match="momentum"):
        _native.sgd_momentum_step(p, g, b, p, b, 0.1, 0.0, 0.0)
    with pytest.raises(_native.DlsimError):
        _native.sgd_momentum_step(p, g, b, p, b, -0.1, 0.9, 0.0)
    h = [torch.zeros(64, device=DEV, dtype=torch.float16) for _ in range(3)]
    with pytest.raises(_native.DlsimError):
        _native.sgd_momentum_step(h[0], h[1], h[2], h[0], h[2], 0.1, 0.9, 0.0)
    assert float(p.abs().sum() + g.abs().sum() + b.abs().sum()) == 0.0


# ---- fixtures through both entries ---------------------------------------------------

def _fixture_through_entries(fx, flat: bool):
    """The fixture's steps on one device buffer of parameters and one of
    buffers: the flat entry, or the tensors entry with per-tensor first flags."""
    meta = fx["meta"]
    dt, shapes = meta["dtype"], meta["shapes"]
    none = {tuple(x) for x in meta["none"]}
    esz = to_tensor(fx["params"][:1], dt).element_size()
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])]).tolist()
    P = to_tensor(fx["params"], dt).to(DEV)
    B = torch.zeros_like(P) if fx["buf0"] is None else to_tensor(fx["buf0"], dt).to(DEV)
    has = [fx["buf0"] is not None] * len(shapes)
    code = _native.dtype_code(P.dtype, single_task=True)
    for s, row in enumerate(fx["grads"]):
        G = to_tensor(row, dt).to(DEV)
        if flat:
            assert not none and len(set(has)) == 1
            _native.sgd_momentum_step(P, G, B if has[0] else None, P, B, meta["lr"], meta["momentum"],
                                      meta["weight_decay"])
            has = [True] * len(shapes)
            continue
        ks = [k for k in range(len(shapes)) if (s, k) not in none]
        at = lambda t, k: t.data_ptr() + offs[k] * esz  # noqa: E731
        _native.sgd_momentum_step_tensors_raw(
            [at(P, k) for k in ks], [at(G, k) for k in ks], [at(B, k) if has[k] else None for k in ks],
            [at(P, k) for k in ks], [at(B, k) for k in ks], [offs[k + 1] - offs[k] for k in ks], meta["lr"],
            meta["momentum"], meta["weight_decay"], code, torch.cuda.current_stream().cuda_stream)
        for k in ks:
            has[k] = True
    return to_array(P), to_array(B)


@pytest.mark.parametrize("case", sorted(c for c in FIXTURES if c.startswith(("specials_", "gnlenet_"))
                                        and "bf16" not in c))
def test_flat_entry_matches_the_fixtures(case):
    """fp32 / fp64 round per element whatever the tensor boundaries, so a
    model's tensors are one flat buffer (bf16: the tensors entry below)."""
    fx = load_sgdm(FIXTURES[case])
    _skip_unless_pinned(fx["meta"])
    p, b = _fixture_through_entries(fx, flat=True)
    assert orc.same_bits(p, fx["expected"]) and orc.same_bits(b, fx["expected_buf"])


def test_flat_entry_matches_the_bf16_specials():
    for case in ("specials_bf16_wd", "specials_bf16_nowd"):  # one tensor: the flat buffer is its own extent
        fx = load_sgdm(FIXTURES[case])
        _skip_unless_pinned(fx["meta"])
        p, b = _fixture_through_entries(fx, flat=True)
        assert orc.same_bits(p, fx["expected"]) and orc.same_bits(b, fx["expected_buf"]), case


@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_tensors_entry_matches_the_fixtures(case):
    fx = load_sgdm(FIXTURES[case])
    _skip_unless_pinned(fx["meta"])
    p, b = _fixture_through_entries(fx, flat=False)
    assert orc.same_bits(p, fx["expected"]) and orc.same_bits(b, fx["expected_buf"])


# ---- the tensors entry ---------------------------------------------------------------

def _tensors_call(ps, gs, bs, pos, bos, wd):
    _native.sgd_momentum_step_tensors_raw(
        [t.data_ptr() for t in ps], [t.data_ptr() for t in gs], [None if t is None else t.data_ptr() for t in bs],
        [t.data_ptr() for t in pos], [t.data_ptr() for t in bos], [t.numel() for t in ps], LR, MOM, wd,
        _native.dtype_code(ps[0].dtype, single_task=True), torch.cuda.current_stream().cuda_stream)


def _list_case(dtype, sizes, wd, first_of):
    """Per tensor k: a first step (first_of(k)) or the second step of its chain."""
    ps, gs, bs, eps, ebs = [], [], [], [], []
    for k, n in enumerate(sizes):
        p0, g, after = _chain(dtype, n, wd)
        if first_of(k):
            ps.append(p0), gs.append(g[0]), bs.append(None), eps.append(after[0][0]), ebs.append(after[0][1])
        else:
            ps.append(after[0][0]), gs.append(g[1]), bs.append(after[0][1])
            eps.append(after[1][0]), ebs.append(after[1][1])
    return ps, gs, bs, eps, ebs


@pytest.mark.parametrize("dtype,wd", CASES)
def test_tensors_entry_many_small_tensors_with_mixed_first_flags(dtype, wd):
    """70 tensors of 1 .. 3000 elements: more than one launch's 64 slots, every
    other one on its first step; bases as torch's allocator gives them and, for
    every third, the parameter one element off."""
    rng = np.random.Generator(np.random.PCG64(7))
    sizes = [1, 2, 3, 7, 8, 9, 10, 31, 32, 33, 2047, 2048, 2049, 3000] + [int(s) for s in rng.integers(1, 3001, 56)]
    assert len(sizes) == 70 > PER_LAUNCH
    ps, gs, bs, eps, ebs = _list_case(dtype, sizes, wd, lambda k: k % 2 == 0)
    dps = [_shifted(p, 1 if k % 3 == 2 else 0) for k, p in enumerate(ps)]
    dgs = [g.to(DEV) for g in gs]
    dbs = [None if b is None else b.to(DEV) for b in bs]
    pos, bos = [torch.empty_like(g) for g in dgs], [torch.empty_like(g) for g in dgs]
    _tensors_call(dps, dgs, dbs, pos, bos, wd)
    for k in range(70):
        sp, sb = torch.empty_like(pos[k]), torch.empty_like(pos[k])
        _native.sgd_momentum_step(dps[k], dgs[k], dbs[k], sp, sb, LR, MOM, wd)
        assert _same(pos[k], sp) and _same(bos[k], sb), (k, sizes[k], "batch != single")
        assert _same(pos[k], eps[k]) and _same(bos[k], ebs[k]), (k, sizes[k])
        assert _same(dgs[k], gs[k])
    # in place, one call (a first step writes into a fresh buffer)
    inb = [torch.empty_like(g) if b is None else b for g, b in zip(dgs, dbs)]
    _tensors_call(dps, dgs, dbs, dps, inb, wd)
    for k in range(70):
        assert _same(dps[k], eps[k]) and _same(inb[k], ebs[k]), (k, sizes[k], "in place")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tensors_entry_with_a_large_tensor(dtype):
    """A tensor above 1 MiB moves the batch to 4 vectors per lane; bf16 at this
    size also crosses torch's parallel split (>= 32768 elements)."""
    sizes = [600_001, 10, 4096, 70_000]
    ps, gs, bs, eps, ebs = _list_case(dtype, sizes, 5e-4, lambda k: k == 2)
    dps, dgs = [p.to(DEV) for p in ps], [g.to(DEV) for g in gs]
    dbs = [None if b is None else b.to(DEV) for b in bs]
    pos, bos = [torch.empty_like(g) for g in dgs], [torch.empty_like(g) for g in dgs]
    _tensors_call(dps, dgs, dbs, pos, bos, 5e-4)
    for k, n in enumerate(sizes):
        sp, sb = torch.empty_like(pos[k]), torch.empty_like(pos[k])
        _native.sgd_momentum_step(dps[k], dgs[k], dbs[k], sp, sb, LR, MOM, 5e-4)
        assert _same(pos[k], sp) and _same(bos[k], sb), n
        assert _same(pos[k], eps[k]) and _same(bos[k], ebs[k]), n


def test_tensors_entry_overlapping_list_runs_in_order():
    """Tensor 1 reads (as its parameter and buffer) what tensor 0 writes: the
    list runs as two launches in order, as two single calls would."""
    p0, gs, after = _chain("f32", 1025, 5e-4)
    dp0, dg0, dg1 = p0.to(DEV), gs[0].to(DEV), gs[1].to(DEV)
    midp, midb = torch.empty_like(dp0), torch.empty_like(dp0)
    outp, outb = torch.empty_like(dp0), torch.empty_like(dp0)
    _tensors_call([dp0, midp], [dg0, dg1], [None, midb], [midp, outp], [midb, outb], 5e-4)
    assert _same(midp, after[0][0]) and _same(midb, after[0][1])
    assert _same(outp, after[1][0]) and _same(outb, after[1][1])


# ---- ArenaSGD ------------------------------------------------------------------------

def _arena_make():
    return lambda m: SGDOptimizer(m, LR, MOM, 5e-4)


@pytest.mark.parametrize("case", ["gnlenet_f32_wd", "gnlenet_bf16_wd", "gnlenet_f64_wd", "none_f32", "none_bf16"])
def test_arena_sgd_three_rounds_with_the_trainers_hand_over(case):
    """A to_device_arena model, gradients assigned as separate device tensors:
    the tensors path, ceil(14 / per-launch) launches; a fresh optimizer plus
    load_state_dict per round (model_trainer.py:89-92)."""
    fx = load_sgdm(FIXTURES[case])
    meta = fx["meta"]
    _skip_unless_pinned(meta)
    model = arena.to_device_arena(fixture_model(fx), DEV)
    seen = []

    def make(m):
        o = SGDOptimizer(m, meta["lr"], meta["momentum"], meta["weight_decay"])
        assert type(o.optimizer) is ArenaSGD
        seen.append(o.optimizer)
        return o
    opt = run_rounds(model, make, fixture_steps(fx, DEV), meta["rounds"])
    assert orc.same_bits(flat_params(model), fx["expected"])
    assert orc.same_bits(flat_buffers(opt, model), fx["expected_buf"])
    assert len(seen) == 3 and all(o.last_launches == -(-14 // PER_LAUNCH) for o in seen)
    assert all(set(o.last_paths.values()) == {"tensors"} for o in seen)
    # after load_state_dict the buffers live in the optimizer's one arena
    last = seen[-1]
    base = last._buf_arenas[next(model.parameters()).dtype]
    for k, p in enumerate(model.parameters()):
        b = last.state[p]["momentum_buffer"]
        assert b.data_ptr() == base.data_ptr() + last._layout.offsets[k] * base.element_size()
    assert arena.registered_arenas(model) is not None  # stepped in place: still one device arena


@pytest.mark.parametrize("case", ["gnlenet_f32_wd", "gnlenet_f64_wd", "gnlenet_bf16_wd"])
def test_arena_sgd_grad_arena_takes_the_flat_path(case):
    fx = load_sgdm(FIXTURES[case])
    meta = fx["meta"]
    _skip_unless_pinned(meta)
    model = arena.to_device_arena(fixture_model(fx), DEV)
    seen = []

    def make(m):
        o = SGDOptimizer(m, meta["lr"], meta["momentum"], meta["weight_decay"], grad_arena=True)
        seen.append(o.optimizer)
        return o
    opt = run_rounds(model, make, fixture_steps(fx, DEV), meta["rounds"])
    assert orc.same_bits(flat_params(model), fx["expected"])
    assert orc.same_bits(flat_buffers(opt, model), fx["expected_buf"])
    want = "tensors" if meta["dtype"] == "bf16" else "flat"  # bf16 rounds per tensor extent
    assert all(o.last_launches == 1 and set(o.last_paths.values()) == {want} for o in seen)
    g0 = next(model.parameters()).grad
    assert all(p.grad is not None and p.grad.is_contiguous() for p in model.parameters())
    assert g0.data_ptr() == seen[-1]._grad_arenas[g0.dtype].data_ptr()


def _small_model(dtypes=("f32",) * 4, seed=9):
    shapes = [[40, 3], [40], [129], [7]]
    g = torch.Generator().manual_seed(seed)
    from _sgd_util import TORCH_DTYPES
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(TORCH_DTYPES[d]))
                                       for s, d in zip(shapes, dtypes)])
    steps = [[(torch.randn(s, generator=g) * 0.01).to(TORCH_DTYPES[d]) for s, d in zip(shapes, dtypes)]
             for _ in range(3)]
    return model, steps


def _dev_steps(steps):
    return [[None if g is None else g.to(DEV) for g in row] for row in steps]


def test_arena_sgd_state_dict_round_trips_through_cpu_torch_sgd():
    host, steps = _small_model()
    cpu3, cpu_opt3 = torch_rounds(host, steps, (3,), LR, MOM, 5e-4)
    # device for two steps, then a CPU torch.optim.SGD takes the state over
    dev = arena.to_device_arena(host, DEV)
    opt = run_rounds(dev, _arena_make(), _dev_steps(steps[:2]), (2,))
    sd = opt.optimizer.state_dict()
    rd = torch.optim.SGD(host.parameters(), lr=LR, momentum=MOM, weight_decay=5e-4).state_dict()
    assert sd["param_groups"] == rd["param_groups"]  # torch's keys and values
    assert set(sd["state"]) == set(cpu_opt3.optimizer.state_dict()["state"])
    assert all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    back = copy.deepcopy(host)
    with torch.no_grad():
        for q, p in zip(back.parameters(), dev.parameters()):
            q.copy_(p.cpu())
    out, oopt = torch_rounds(back, steps[2:], (1,), LR, MOM, 5e-4, state0=sd)
    assert orc.same_bits(flat_params(out), flat_params(cpu3))
    assert orc.same_bits(flat_buffers(oopt, out), flat_buffers(cpu_opt3, cpu3))
    # and the other way round: two CPU steps, the device takes the state over
    cpu2, cpu_opt2 = torch_rounds(host, steps[:2], (2,), LR, MOM, 5e-4)
    dev = arena.to_device_arena(cpu2, DEV)
    opt = run_rounds(dev, _arena_make(), _dev_steps(steps[2:]), (1,), state0=cpu_opt2.optimizer.state_dict())
    assert orc.same_bits(flat_params(dev), flat_params(cpu3))
    assert orc.same_bits(flat_buffers(opt, dev), flat_buffers(cpu_opt3, cpu3))
    assert all(opt.optimizer.state[p]["momentum_buffer"].is_cuda for p in dev.parameters())


def test_arena_sgd_parameter_without_a_gradient_for_two_steps():
    host, steps = _small_model()
    steps[0][2] = steps[1][2] = None
    cpu, cpu_opt = torch_rounds(host, steps, (2, 1), LR, MOM, 5e-4)
    dev = arena.to_device_arena(host, DEV)
    o = SGDOptimizer(dev, LR, MOM, 5e-4)
    run_rounds(dev, lambda m: o, _dev_steps(steps[:2]), (2,))
    p2 = list(dev.parameters())[2]
    assert "momentum_buffer" not in o.optimizer.state.get(p2, {})  # no buffer until its first gradient
    assert _same(p2, list(host.parameters())[2])
    run_rounds(dev, lambda m: o, _dev_steps(steps[2:]), (1,))
    assert orc.same_bits(flat_params(dev), flat_params(cpu))
    assert orc.same_bits(flat_buffers(o, dev), flat_buffers(cpu_opt, cpu))


class _Holder:
    def __init__(self, optimizer):
        self.optimizer = optimizer


def test_arena_sgd_without_momentum_keeps_no_state():
    host, steps = _small_model()
    m = copy.deepcopy(host)
    opt = torch.optim.SGD(m.parameters(), lr=LR, momentum=0.0, weight_decay=5e-4, foreach=False)
    with torch_threads(4):
        for row in steps:
            for p, g in zip(m.parameters(), row):
                p.grad = g.clone()
            opt.step()
    for grad_arena, path in ((False, "tensors"), (True, "flat")):
        dev = arena.to_device_arena(host, DEV)
        o = ArenaSGD(dev.parameters(), lr=LR, momentum=0.0, weight_decay=5e-4, grad_arena=grad_arena)
        run_rounds(dev, lambda mm: _Holder(o), _dev_steps(steps), (3,))
        assert orc.same_bits(flat_params(dev), flat_params(m))
        assert o.state_dict()["state"] == {} == opt.state_dict()["state"]
        assert o.last_launches == 1 and set(o.last_paths.values()) == {path}


def test_arena_sgd_mixed_dtype_model_steps_per_group():
    host, steps = _small_model(("f32", "bf16", "bf16", "f32"))
    cpu, cpu_opt = torch_rounds(host, steps, (1, 2), LR, MOM, 5e-4)
    dev = arena.to_device_arena(host, DEV)
    seen = []

    def make(m):
        o = SGDOptimizer(m, LR, MOM, 5e-4)
        seen.append(o.optimizer)
        return o
    opt = run_rounds(dev, make, _dev_steps(steps), (1, 2))
    for q, e in zip(dev.parameters(), cpu.parameters()):
        assert q.dtype == e.dtype and _same(q, e), q.dtype
    for p, e in zip(dev.parameters(), cpu.parameters()):
        assert _same(opt.optimizer.state[p]["momentum_buffer"], cpu_opt.optimizer.state[e]["momentum_buffer"])
    assert all(o.last_launches == 2 and len(o.last_paths) == 2 for o in seen)
    # an fp16 parameter in the model: the reference's plain torch.optim.SGD
    half = copy.deepcopy(host).to(DEV)
    half.ps[3].data = half.ps[3].data.half()
    assert type(SGDOptimizer(half, LR, MOM, 5e-4).optimizer) is torch.optim.SGD
    with pytest.raises(TypeError):
        ArenaSGD(half.parameters(), lr=LR, momentum=MOM)


def test_arena_sgd_separate_device_tensors_and_hyper_parameter_checks():
    """`model.to(device)` (model_trainer.py:85) gives separate tensors: the
    tensors entry, buffers arena-resident all the same."""
    host, steps = _small_model()
    cpu, cpu_opt = torch_rounds(host, steps, (3,), LR, MOM, 5e-4)
    dev = copy.deepcopy(host).to(DEV)
    o = SGDOptimizer(dev, LR, MOM, 5e-4)
    assert (o.learning_rate, o.momentum, o.weight_decay) == (LR, MOM, 5e-4)
    run_rounds(dev, lambda m: o, _dev_steps(steps), (3,))
    assert orc.same_bits(flat_params(dev), flat_params(cpu))
    assert orc.same_bits(flat_buffers(o, dev), flat_buffers(cpu_opt, cpu))
    assert set(o.optimizer.last_paths.values()) == {"tensors"} and o.optimizer.last_launches == 1
    assert o.optimizer.step() is None and o.optimizer.step(lambda: 1.5) == 1.5
    for kw in ({"lr": -0.1}, {"momentum": -0.5}, {"weight_decay": -1e-4}):
        with pytest.raises(ValueError, match="Invalid"):
            ArenaSGD(dev.parameters(), **kw)


def test_aggregate_then_two_steps_then_aggregate_matches_the_cpu_chain():
    """aggregate -> two ArenaSGD steps -> aggregate, against
    oracle.fedavg_torch plus torch SGD on the CPU."""
    hosts = []
    total = sum(int(np.prod(s)) for s in GNLENET_SHAPES)
    for seed in (31, 32):
        a, _ = seeded_pair(total, seed, "f32")
        m = Net(GNLENET_SHAPES, "f32")
        with torch.no_grad():
            for p, x in zip(m.parameters(), split(a, GNLENET_SHAPES)):
                p.copy_(to_tensor(x, "f32").reshape(p.shape))
        hosts.append(m)
    steps = [[to_tensor(x, "f32").reshape(s) for x, s in zip(split(seeded_pair(total, seed, "f32")[1], GNLENET_SHAPES),
                                                              GNLENET_SHAPES)] for seed in (33, 34)]
    devs = [arena.to_device_arena(m, DEV) for m in hosts]
    agg = FedAvg.aggregate(devs, None)
    for grad_arena in (False, True):
        model = FedAvg.aggregate(devs, None)
        o = SGDOptimizer(model, 0.05, MOM, 1e-3, grad_arena=grad_arena)
        run_rounds(model, lambda m: o, _dev_steps(steps), (2,))
        assert set(o.optimizer.last_paths.values()) == {"flat" if grad_arena else "tensors"}
        out = FedAvg.aggregate([model, devs[0]], None)
        cpu, _ = torch_rounds(fedavg_torch.aggregate_modules(hosts, None), steps, (2,), 0.05, MOM, 1e-3)
        expect = fedavg_torch.aggregate_modules([cpu, hosts[0]], None)
        assert all(p.is_cuda for p in out.parameters())
        assert orc.same_bits(flat_params(model), flat_params(cpu))
        assert orc.same_bits(flat_params(out), flat_params(expect))
    assert orc.same_bits(flat_params(agg), flat_params(fedavg_torch.aggregate_modules(hosts, None)))
