"""The stateful momentum-SGD step (reference optimizer/sgd.py stepped by
model_trainer.py:89-92,126) — CPU checks: the fixtures pin what torch computes
here, the fp32 fixture tells an unfused buffer update from a fused one, both C
entries report argument errors without a GPU, and the SGDOptimizer drop-in
builds the reference's plain torch.optim.SGD for CPU and fp16 models."""
from __future__ import annotations

import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _sgd_util import Net, flat_params, torch_threads
from _sgdm_util import (fixture_model, fixture_state0, fixture_steps, flat_buffers, run_rounds, torch_rounds)
from conftest import ROOT
from dasklearn_amd import _native
from dasklearn_amd.optimizer import ArenaSGD, SGDOptimizer
from oracle import oracle as orc
from sgd_inputs import split
from sgdm_inputs import BUF_SUFFIX, MAX_BYTES, SGDM_DIR, load_sgdm, sgdm_paths

sys.path.insert(0, os.path.join(ROOT, "scripts", "probes"))
import probe_sgd_momentum_rule as rule  # noqa: E402

FIXTURES = {os.path.basename(p)[:-4]: p for p in sgdm_paths()}


def test_fixture_set_is_complete():
    want = {"gnlenet_f32_wd", "gnlenet_f32_nowd", "gnlenet_bf16_wd", "gnlenet_bf16_nowd", "gnlenet_f64_wd",
            "none_f32", "none_bf16"} | {f"specials_{d}_{w}" for d in ("f32", "bf16", "f64") for w in ("wd", "nowd")}
    assert want <= set(FIXTURES)
    for f in os.listdir(SGDM_DIR):
        assert os.path.getsize(os.path.join(SGDM_DIR, f)) < MAX_BYTES, f
        assert f.endswith(".npz") and (f[:-4] in FIXTURES or f[:-4 - len(BUF_SUFFIX)] in FIXTURES), f
    for case, p in FIXTURES.items():
        meta = load_sgdm(p)["meta"]
        if case.startswith(("gnlenet_", "none_")):
            assert len(meta["rounds"]) == 3 and all(1 <= r <= 2 for r in meta["rounds"]) and meta["momentum"] > 0
        if case.startswith("none_"):
            assert len(meta["none"]) == 2 and all(s == 0 for s, _ in meta["none"])
        if case.startswith("specials_"):
            assert load_sgdm(p)["params"].size == 729


@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_fixture_equals_live_torch_sgd(case):
    fx = load_sgdm(FIXTURES[case])
    meta = fx["meta"]
    cap = torch.backends.cpu.get_cpu_capability()
    if meta["torch_version"] != torch.__version__ or meta["cpu_capability"] != cap:
        pytest.skip(f"fixture made with torch {meta['torch_version']} / {meta['cpu_capability']}, "
                    f"this is {torch.__version__} / {cap}")
    model = fixture_model(fx)
    before = flat_params(model)
    out, opt = torch_rounds(model, fixture_steps(fx), meta["rounds"], meta["lr"], meta["momentum"],
                            meta["weight_decay"], fixture_state0(fx, model), meta["torch_threads"])
    assert orc.same_bits(flat_params(out), fx["expected"])
    assert orc.same_bits(flat_buffers(opt, out), fx["expected_buf"])
    assert not orc.same_bits(before, fx["expected"])
    assert orc.same_bits(flat_params(model), before)


def _emulate_fixture(fx, **wrong):
    """The fixture's rounds through the probe's emulation, tensor by tensor."""
    meta = fx["meta"]
    none = {tuple(x) for x in meta["none"]}
    ps = [a.reshape(-1).copy() for a in split(fx["params"], meta["shapes"])]
    bufs = [None] * len(ps) if fx["buf0"] is None else [a.reshape(-1) for a in split(fx["buf0"], meta["shapes"])]
    for s, row in enumerate(fx["grads"]):
        for k, g in enumerate(split(row, meta["shapes"])):
            if (s, k) in none:
                continue
            ps[k], bufs[k] = rule.emulate_step(meta["dtype"], ps[k], g.reshape(-1), bufs[k], meta["lr"],
                                               meta["momentum"], meta["weight_decay"], meta["torch_threads"], **wrong)
    return np.concatenate(ps), np.concatenate(bufs)


def test_f32_fixture_pins_the_unfused_buffer_update():
    """buf' = f32(f32(m) * buf) + g': a kernel that fuses the product into the
    sum fails against the fixture; the unfused emulation equals it everywhere."""
    fx = load_sgdm(FIXTURES["gnlenet_f32_wd"])
    p, b = _emulate_fixture(fx)
    assert orc.same_bits(p, fx["expected"]) and orc.same_bits(b, fx["expected_buf"])
    p, b = _emulate_fixture(fx, fused_buffer=True)
    differ = int((b.view(np.uint32) != fx["expected_buf"].view(np.uint32)).sum())
    print("buffer elements a fused update changes:", differ, "of", b.size)
    assert differ >= 1


@pytest.mark.parametrize("case", ["gnlenet_bf16_wd", "none_bf16", "none_f32", "specials_f32_wd", "specials_bf16_wd",
                                  "specials_bf16_nowd", "specials_f32_nowd"])
def test_emulated_rule_equals_the_fixtures(case):
    fx = load_sgdm(FIXTURES[case])
    p, b = _emulate_fixture(fx)
    assert orc.same_bits(p, fx["expected"]) and orc.same_bits(b, fx["expected_buf"])
    if case == "gnlenet_bf16_wd":  # momentum rounded to bf16 first is another result
        p, b = _emulate_fixture(fx, bf16_momentum=True)
        assert not orc.same_bits(b, fx["expected_buf"])


# ---- the C entries' argument checks (no GPU) -----------------------------------------

def _step(p=4096, g=8192, b=12288, po=None, bo=None, n=100, lr=0.1, mom=0.9, wd=0.0, dtype=0):
    po = p if po is None else po
    bo = (b if b else 16384) if bo is None else bo
    return _native.load().dlsim_sgd_momentum_step(p, g, b or None, po, bo, n, lr, mom, wd, dtype, None)


def test_momentum_step_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _step(n=0) == 0
    assert _step(n=0, p=0, g=0, b=0, po=0, bo=0) == 0
    assert _step(dtype=_native.DLSIM_F16) == -2 and b"F16" in lib.dlsim_last_error()
    assert _step(dtype=7) == -2
    assert _step(lr=-0.1) == -1 and b"lr" in lib.dlsim_last_error()
    assert _step(lr=float("nan")) == -1
    assert _step(wd=-1e-3) == -1 and b"weight_decay" in lib.dlsim_last_error()
    assert _step(wd=float("nan")) == -1
    for mom in (0.0, -0.5, float("nan")):
        assert _step(mom=mom) == -1 and b"momentum" in lib.dlsim_last_error()
    for null in ("p", "g", "po", "bo"):
        assert _step(**{null: 0}) == -1 and b"null" in lib.dlsim_last_error(), null
    # forbidden overlaps: anything but param_out == param and buf_out == buf
    assert _step(po=4096 + 64) == -1 and b"overlaps the parameter" in lib.dlsim_last_error()
    assert _step(bo=12288 - 4) == -1 and b"overlaps" in lib.dlsim_last_error()
    assert _step(po=8192) == -1 and b"gradient" in lib.dlsim_last_error()  # the gradient is never written
    assert _step(bo=8192) == -1
    assert _step(g=4096) == -1
    assert _step(b=4096) == -1
    assert _step(po=20480, bo=20480) == -1
    assert _step(po=12288 + 8, bo=40960) == -1
    assert _step(b=8192 + 396, dtype=_native.DLSIM_F64) == -1  # 100 doubles reach it
    assert _step(b=8192 + 400, bo=8192 + 400, dtype=0, n=0) == 0


def _tensors(ps, gs, bs, pos, bos, ns, lr=0.1, mom=0.9, wd=0.0, dtype=0, t=None):
    t = len(ns) if t is None else t
    arr = ctypes.c_void_p * max(len(ns), 1)
    return _native.load().dlsim_sgd_momentum_step_tensors(
        t, arr(*ps), arr(*gs), arr(*bs), arr(*pos), arr(*bos), (ctypes.c_size_t * max(len(ns), 1))(*ns), lr, mom, wd,
        dtype, None)


def test_momentum_step_tensors_argument_errors_need_no_gpu():
    lib = _native.load()
    one = ([4096], [8192], [None], [4096], [12288])
    assert _tensors([], [], [], [], [], []) == 0
    assert _tensors(*one, [0]) == 0  # nothing to do
    assert _tensors(*one, [4], t=-1) == -1
    assert _tensors(*one, [4], dtype=_native.DLSIM_F16) == -2
    assert _tensors(*one, [4], lr=-1.0) == -1
    assert _tensors(*one, [4], wd=float("nan")) == -1
    assert _tensors(*one, [4], mom=0.0) == -1 and b"momentum" in lib.dlsim_last_error()
    assert _tensors(*one, [4], mom=float("nan")) == -1
    assert lib.dlsim_sgd_momentum_step_tensors(1, None, None, None, None, None, None, 0.1, 0.9, 0.0, 0, None) == -1
    assert _tensors([4096, 16], [8192, 0], [None, None], [4096, 16], [12288, 64], [10, 4]) == -1
    assert b"tensor 1" in lib.dlsim_last_error() and b"null" in lib.dlsim_last_error()
    assert _tensors([4096, 65536], [8192, 70000], [None, 80000], [4096, 65536 + 8], [12288, 80000], [10, 100]) == -1
    assert b"tensor 1" in lib.dlsim_last_error() and b"overlaps" in lib.dlsim_last_error()


# ---- the drop-in on models the kernel does not take ----------------------------------

def _reference_class():
    """The reference's SGDOptimizer, restated: what dasklearn/optimizer/sgd.py builds."""
    class Ref:
        def __init__(self, model, learning_rate, momentum, weight_decay):
            self.learning_rate, self.momentum, self.weight_decay = learning_rate, momentum, weight_decay
            self.optimizer = torch.optim.SGD(model.parameters(), lr=learning_rate, momentum=momentum,
                                             weight_decay=weight_decay)
    return Ref


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_cpu_and_f16_models_get_plain_torch_sgd(dtype):
    shapes = [[33, 7], [33], [129], [5]]
    g = torch.Generator().manual_seed(5)
    model = Net(shapes, dtype)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(p.dtype))
    steps = [[(torch.randn(s, generator=g) * 0.01).to(next(model.parameters()).dtype) for s in shapes]
             for _ in range(3)]
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    opt = SGDOptimizer(a, 0.1, 0.9, 5e-4)
    assert type(opt.optimizer) is torch.optim.SGD
    assert (opt.learning_rate, opt.momentum, opt.weight_decay) == (0.1, 0.9, 5e-4)
    with torch_threads(4):
        oa = run_rounds(a, lambda m: SGDOptimizer(m, 0.1, 0.9, 5e-4), steps, (1, 2))
        ob = run_rounds(b, lambda m: _reference_class()(m, 0.1, 0.9, 5e-4), steps, (1, 2))
    assert type(oa.optimizer) is torch.optim.SGD
    assert orc.same_bits(flat_params(a), flat_params(b))
    assert orc.same_bits(flat_buffers(oa, a), flat_buffers(ob, b))
    assert not orc.same_bits(flat_params(a), flat_params(model))


def test_arena_sgd_refuses_what_it_has_no_kernel_for():
    with pytest.raises(TypeError, match="device parameters"):
        ArenaSGD([torch.nn.Parameter(torch.zeros(4))], lr=0.1, momentum=0.9)
    for kw in ({"lr": -0.1}, {"momentum": -0.5}, {"weight_decay": -1e-4}):
        with pytest.raises(ValueError, match="Invalid"):
            ArenaSGD([torch.nn.Parameter(torch.zeros(4))], **kw)


def test_arena_sgd_state_dict_keys_equal_torchs():
    """ArenaSGD's param group is built from torch.optim.SGD's own defaults;
    without a GPU the optimizer base class is initialised over a CPU
    parameter with them (tests/test_gpu_sgdm.py compares a real one)."""
    p = torch.nn.Parameter(torch.zeros(4))
    ref = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=5e-4)
    opt = ArenaSGD.__new__(ArenaSGD)
    torch.optim.Optimizer.__init__(opt, [p], ArenaSGD.torch_defaults(0.1, 0.9, 5e-4))
    sd, rd = opt.state_dict(), ref.state_dict()
    assert set(sd) == set(rd) == {"state", "param_groups"}
    assert sd["param_groups"] == rd["param_groups"]
