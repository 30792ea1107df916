"""The `gradient_update` task (reference functions.py:85-86,
model_trainer.py:133-143) — CPU checks: the fixtures pin what torch computes
here, the fp32 fixture tells a fused kernel from an unfused one, both C entries
report argument errors without a GPU, and an fp16 model goes through the task
on torch's own CPU ops with the task's contract intact."""
from __future__ import annotations

import ctypes
import os
import types

import numpy as np
import pytest
import torch
from torch import nn

from _sgd_util import (Net, fixture_gradients, fixture_model, flat_params, settings_of, to_array, torch_sgd_step,
                       torch_threads)
from dasklearn_amd import _native, functions
from oracle import oracle as orc
from sgd_inputs import load_sgd, sgd_paths

FIXTURES = {os.path.basename(p)[:-4]: p for p in sgd_paths()}


def test_fixture_set_is_complete():
    want = {"gnlenet_f32_wd", "gnlenet_f32_nowd", "gnlenet_bf16_wd", "gnlenet_bf16_nowd", "gnlenet_f64_wd",
            "buffers_bn_f32", "short_f32", "short_bf16"} | {f"specials_{d}_{w}" for d in ("f32", "bf16", "f64")
                                                           for w in ("wd", "nowd")}
    assert want <= set(FIXTURES)
    for p in FIXTURES.values():
        assert os.path.getsize(p) < 700_000, p


@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_fixture_equals_live_torch_sgd(case):
    fx = load_sgd(FIXTURES[case])
    meta = fx["meta"]
    cap = torch.backends.cpu.get_cpu_capability()
    if meta["torch_version"] != torch.__version__ or meta["cpu_capability"] != cap:
        pytest.skip(f"fixture made with torch {meta['torch_version']} / {meta['cpu_capability']}, "
                    f"this is {torch.__version__} / {cap}")
    model = fixture_model(fx)
    before = flat_params(model)
    out = torch_sgd_step(model, fixture_gradients(fx), meta["lr"], meta["momentum"], meta["weight_decay"],
                         meta["torch_threads"])
    assert orc.same_bits(flat_params(out), fx["expected"])
    assert not orc.same_bits(before, fx["expected"])


def test_short_gradient_list_leaves_trailing_parameters():
    fx = load_sgd(FIXTURES["short_f32"])
    meta = fx["meta"]
    assert meta["n_grads"] == len(meta["shapes"]) - 2
    k = sum(int(np.prod(s)) for s in meta["shapes"][:meta["n_grads"]])
    assert orc.same_bits(fx["expected"][k:], fx["params"][k:])
    assert not np.array_equal(fx["expected"][:k], fx["params"][:k])


def test_f32_fixture_pins_the_fused_rounding():
    """An unfused computation (product rounded, then the sum) differs from the
    fixture: a kernel that does not fuse would fail against it."""
    fx = load_sgd(FIXTURES["gnlenet_f32_wd"])
    meta = fx["meta"]
    p, g = fx["params"], fx["grads"]
    wd, nlr = np.float32(meta["weight_decay"]), np.float32(-meta["lr"])
    unfused = p + nlr * (g + wd * p)
    assert unfused.dtype == np.float32
    differ = int((unfused.view(np.uint32) != fx["expected"].view(np.uint32)).sum())
    print("unfused elements that differ:", differ, "of", p.size)
    assert differ >= 1
    # and the fused emulation (exact in double: 24-bit products) agrees everywhere
    g2 = (wd.astype(np.float64) * p.astype(np.float64) + g.astype(np.float64)).astype(np.float32)
    fused = (nlr.astype(np.float64) * g2.astype(np.float64) + p.astype(np.float64)).astype(np.float32)
    assert int((fused.view(np.uint32) != fx["expected"].view(np.uint32)).sum()) <= 2  # double rounding at most


def test_specials_keep_infinite_parameters_without_weight_decay():
    fx = load_sgd(FIXTURES["specials_f32_nowd"])
    p, g, e = fx["params"], fx["grads"], fx["expected"]
    keep = np.isinf(p) & np.isfinite(g)
    assert keep.any() and np.array_equal(e[keep], p[keep])
    fx = load_sgd(FIXTURES["specials_f32_wd"])
    p, g, e = fx["params"], fx["grads"], fx["expected"]
    assert np.isnan(e[np.isinf(p) & np.isfinite(g)]).all()  # inf - lr * (g + wd * inf)


# ---- the C entries' argument checks (no GPU) -----------------------------------------

def _step(p=4096, g=8192, out=12288, n=100, lr=0.1, wd=0.0, dtype=0):
    return _native.load().dlsim_sgd_step(p, g, out, n, lr, wd, dtype, None)


def test_sgd_step_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _step(n=0) == 0
    assert _step(n=0, p=0, g=0, out=0) == 0
    assert _step(dtype=_native.DLSIM_F16) == -2 and b"F16" in lib.dlsim_last_error()
    assert _step(dtype=7) == -2
    assert _step(lr=-0.1) == -1 and b"lr" in lib.dlsim_last_error()
    assert _step(lr=float("nan")) == -1
    assert _step(wd=-1e-3) == -1 and b"weight_decay" in lib.dlsim_last_error()
    assert _step(wd=float("nan")) == -1
    assert _step(p=0) == -1 and b"null" in lib.dlsim_last_error()
    assert _step(out=0) == -1
    assert _step(out=4096 + 64) == -1 and b"overlaps the parameter" in lib.dlsim_last_error()
    assert _step(out=8192 - 4) == -1 and b"gradient" in lib.dlsim_last_error()
    assert _step(out=8192 + 396, dtype=_native.DLSIM_F64) == -1  # 100 doubles reach it; 100 floats do not


def _tensors(ps, gs, outs, ns, lr=0.1, wd=0.0, dtype=0, t=None):
    t = len(ns) if t is None else t
    arr = ctypes.c_void_p * max(len(ns), 1)
    return _native.load().dlsim_sgd_step_tensors(t, arr(*ps), arr(*gs), arr(*outs),
                                                 (ctypes.c_size_t * max(len(ns), 1))(*ns), lr, wd, dtype, None)


def test_sgd_step_tensors_argument_errors_need_no_gpu():
    lib = _native.load()
    assert _tensors([], [], [], []) == 0
    assert _tensors([16], [32], [48], [0]) == 0  # nothing to do
    assert _tensors([16], [32], [48], [4], t=-1) == -1
    assert _tensors([16], [32], [48], [4], dtype=_native.DLSIM_F16) == -2
    assert _tensors([16], [32], [48], [4], lr=-1.0) == -1
    assert _tensors([16], [32], [48], [4], wd=float("nan")) == -1
    assert lib.dlsim_sgd_step_tensors(1, None, None, None, None, 0.1, 0.0, 0, None) == -1
    assert _tensors([4096, 16], [8192, 0], [12288, 48], [10, 4]) == -1 and b"tensor 1" in lib.dlsim_last_error()
    assert _tensors([4096, 65536], [8192, 70000], [12288, 65536 + 8], [10, 100]) == -1
    assert b"tensor 1" in lib.dlsim_last_error() and b"overlaps" in lib.dlsim_last_error()


# ---- fp16 through the task, on torch's CPU ops -----------------------------------------

def _f16_case(n_grads=None, seed=5):
    shapes = [[33, 7], [33], [129], [5]]
    g = torch.Generator().manual_seed(seed)
    model = Net(shapes, "f16")
    with torch.no_grad():
        for p in model.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).half())
    grads = [(torch.randn(s, generator=g) * 0.01).half() for s in shapes][:n_grads]
    return model, grads


def _task(model, grads, lr=0.1, momentum=0.9, wd=5e-4):
    gm = types.SimpleNamespace(gradient=grads)
    outs = functions.gradient_update(settings_of(lr, momentum, wd), {"model": model, "gradient_model": gm})
    assert isinstance(outs, list) and len(outs) == 1
    return outs[0]


def test_f16_model_takes_torchs_cpu_ops_bit_for_bit():
    assert "gradient_update" in functions.__all__
    model, grads = _f16_case()
    model.gradient = ["stale"]  # whatever rides on the input does not reach the output
    before = flat_params(model)
    for wd in (5e-4, 0.0):
        out = _task(model, grads, wd=wd)
        with torch_threads(torch.get_num_threads()):
            expect = []
            for p, g in zip(model.parameters(), grads):
                g2 = g.add(p.detach(), alpha=wd) if wd != 0 else g
                expect.append(to_array(p.detach().add(g2, alpha=-0.1)))
        assert orc.same_bits(flat_params(out), np.concatenate(expect))
        assert orc.same_bits(flat_params(out), flat_params(torch_sgd_step(model, grads, 0.1, 0.9, wd,
                                                                            torch.get_num_threads())))
        assert type(out) is type(model) and out is not model
        assert not hasattr(out, "gradient")
        assert all(p.requires_grad and p.dtype == torch.float16 and not p.is_cuda for p in out.parameters())
        assert all(p.grad is None for p in out.parameters())
    assert orc.same_bits(flat_params(model), before)  # the input is only read
    assert all(p.grad is None for p in model.parameters())


def test_task_contract_on_the_cpu_path():
    model, grads = _f16_case(n_grads=2)
    for p in list(model.parameters())[:1]:
        p.requires_grad_(False)
    out = _task(model, grads)
    ps, qs = list(model.parameters()), list(out.parameters())
    assert all(q.requires_grad for q in qs)
    for k in (2, 3):  # past the gradient list: unchanged (zip)
        assert orc.same_bits(to_array(qs[k]), to_array(ps[k]))
    for k in (0, 1):
        assert not orc.same_bits(to_array(qs[k]), to_array(ps[k]))
    # a None in the list: torch skips that parameter
    model, grads = _f16_case()
    out = _task(model, [grads[0], None, grads[2], grads[3]])
    assert orc.same_bits(to_array(list(out.parameters())[1]), to_array(list(model.parameters())[1]))
    # shape and dtype mismatches raise as `param.grad = grad` does
    with pytest.raises(RuntimeError, match="size"):
        _task(model, [grads[0], grads[2]])
    with pytest.raises(RuntimeError, match="type"):
        _task(model, [grads[0].float()])
    # negative hyper-parameters raise as torch.optim.SGD does
    for kw in ({"lr": -0.1}, {"momentum": -0.5}, {"wd": -1e-4}):
        with pytest.raises(ValueError, match="Invalid"):
            _task(model, grads, **kw)
        with pytest.raises(ValueError, match="Invalid"):
            args = {"lr": 0.1, "momentum": 0.0, "weight_decay": 0.0}
            args.update({("weight_decay" if k == "wd" else k): v for k, v in kw.items()})
            torch.optim.SGD([nn.Parameter(torch.zeros(1))], **args)


def test_buffers_are_copied_on_the_cpu_path():
    class BnHalf(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(7, 5)
            self.bn = nn.BatchNorm1d(5)
    torch.manual_seed(3)
    model = BnHalf().half()
    model.bn.running_mean.copy_(torch.randn(5))
    model.bn.num_batches_tracked.fill_(7)
    grads = [torch.randn(p.shape).half() * 0.01 for p in model.parameters()]
    out = _task(model, grads)
    for a, b in zip(model.buffers(), out.buffers()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    assert int(out.bn.num_batches_tracked) == 7
    assert orc.same_bits(flat_params(out), flat_params(torch_sgd_step(model, grads, 0.1, 0.9, 5e-4,
                                                                        torch.get_num_threads())))
