"""Helpers shared by tests/test_sgdm_cpu.py and tests/test_gpu_sgdm.py: the
trainer's optimizer pattern (reference model_trainer.py:89-92,126) over the
momentum-SGD fixtures (tests/golden/sgdm/) and the live CPU reference,
torch.optim.SGD(foreach=False) itself."""
from __future__ import annotations

import copy

import numpy as np
import torch
from torch import nn

from _sgd_util import Net, to_array, to_tensor, torch_threads
from sgd_inputs import split


class TorchSGDOptimizer:
    """What the reference's SGDOptimizer builds, pinned to the single-tensor path."""

    def __init__(self, model, learning_rate, momentum, weight_decay):
        self.learning_rate, self.momentum, self.weight_decay = learning_rate, momentum, weight_decay
        self.optimizer = torch.optim.SGD(model.parameters(), lr=learning_rate, momentum=momentum,
                                         weight_decay=weight_decay, foreach=False)


def fixture_model(fx: dict) -> nn.Module:
    meta = fx["meta"]
    model = Net(meta["shapes"], meta["dtype"])
    with torch.no_grad():
        for p, a in zip(model.parameters(), split(fx["params"], meta["shapes"])):
            p.copy_(to_tensor(a, meta["dtype"]).reshape(p.shape))
    return model


def fixture_steps(fx: dict, device="cpu"):
    """Per step, the gradient of every parameter (None where meta["none"] says so)."""
    meta = fx["meta"]
    none = {tuple(x) for x in meta["none"]}
    return [[None if (s, k) in none else to_tensor(a, meta["dtype"]).reshape(shape).to(device)
             for k, (a, shape) in enumerate(zip(split(row, meta["shapes"]), meta["shapes"]))]
            for s, row in enumerate(fx["grads"])]


def state_with_buffers(model: nn.Module, bufs, lr, momentum, weight_decay) -> dict:
    """The state dict of a torch.optim.SGD over a CPU copy of `model` whose
    momentum buffers are `bufs` (CPU tensors, one per parameter)."""
    m = copy.deepcopy(model).cpu()
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
    for p, b in zip(m.parameters(), bufs):
        opt.state[p]["momentum_buffer"] = b.detach().clone().reshape(p.shape)
    return opt.state_dict()


def fixture_state0(fx: dict, model):
    meta = fx["meta"]
    if fx["buf0"] is None:
        return None
    bufs = [to_tensor(a, meta["dtype"]) for a in split(fx["buf0"], meta["shapes"])]
    return state_with_buffers(model, bufs, meta["lr"], meta["momentum"], meta["weight_decay"])


def run_rounds(model: nn.Module, make, steps, rounds, state0=None):
    """The trainer's pattern on `model`, in place: per round a fresh
    `make(model)` (an object with .optimizer), load_state_dict of the previous
    round's state, then zero_grad / assign gradients / step per local step.
    Returns the last optimizer object."""
    prev_state, opt, it = state0, None, iter(steps)
    for n_steps in rounds:
        opt = make(model)
        if prev_state is not None:
            opt.optimizer.load_state_dict(prev_state)
        for _ in range(n_steps):
            grads = next(it)
            opt.optimizer.zero_grad()
            for p, g in zip(model.parameters(), grads):
                if g is None:
                    continue
                if p.grad is None:
                    p.grad = g.detach().clone()
                else:  # a gradient arena: accumulate into the view, as autograd does
                    with torch.no_grad():
                        p.grad.add_(g)
            opt.optimizer.step()
        prev_state = opt.optimizer.state_dict()
    return opt


def flat_buffers(opt, model) -> np.ndarray:
    """The momentum buffers in parameters() order, zeros where a parameter has none."""
    out = []
    for p in model.parameters():
        b = opt.optimizer.state.get(p, {}).get("momentum_buffer")
        out.append(to_array(torch.zeros_like(p) if b is None else b))
    return np.concatenate(out)


def torch_rounds(model, steps, rounds, lr, momentum, weight_decay, state0=None, threads: int = 4):
    """torch.optim.SGD(foreach=False) through the same rounds on a CPU deep
    copy; returns (model, optimizer object)."""
    m = copy.deepcopy(model).cpu()
    cpu_steps = [[None if g is None else g.detach().cpu() for g in row] for row in steps]
    with torch_threads(threads):
        opt = run_rounds(m, lambda mm: TorchSGDOptimizer(mm, lr, momentum, weight_decay), cpu_steps, rounds, state0)
    return m, opt
