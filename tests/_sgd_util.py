"""Helpers shared by tests/test_sgd_cpu.py and tests/test_gpu_sgd.py: models
from the SGD-step fixtures (tests/golden/sgd/) and the live CPU reference,
torch.optim.SGD itself."""
from __future__ import annotations

import contextlib
import types

import numpy as np
import torch
from torch import nn

from sgd_inputs import split

TORCH_DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}


def to_tensor(a: np.ndarray, dtype: str) -> torch.Tensor:
    """A fixture array (bf16 as uint16 bits) as a CPU tensor."""
    a = np.ascontiguousarray(a)
    if dtype == "bf16":
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(a.copy())


def to_array(t: torch.Tensor) -> np.ndarray:
    """Flat storage array of a tensor (bf16 as uint16 bits), on the host."""
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def flat_params(model: nn.Module) -> np.ndarray:
    return np.concatenate([to_array(p) for p in model.parameters()])


@contextlib.contextmanager
def torch_threads(n: int):
    """The reference worker's intra-op thread count (broker.py:31) while the
    CPU reference runs: PyTorch's bf16 and fp16 results depend on it."""
    old = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield
    finally:
        torch.set_num_threads(old)


class Net(nn.Module):
    def __init__(self, shapes, dtype):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(torch.zeros(*s, dtype=TORCH_DTYPES[dtype])) for s in shapes])


class BnNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(7, 5)
        self.bn = nn.BatchNorm1d(5)


def fixture_model(fx: dict) -> nn.Module:
    """The fixture's model with its parameters (and buffers) loaded."""
    meta = fx["meta"]
    model = BnNet() if meta["buffer_shapes"] else Net(meta["shapes"], meta["dtype"])
    with torch.no_grad():
        for p, a in zip(model.parameters(), split(fx["params"], meta["shapes"])):
            p.copy_(to_tensor(a, meta["dtype"]).reshape(p.shape))
        for b, a in zip(model.buffers(), split(fx["buffers"], meta["buffer_shapes"])):
            b.copy_(torch.from_numpy(a.copy()).reshape(b.shape).to(b.dtype))
    return model


def fixture_gradients(fx: dict):
    meta = fx["meta"]
    shapes = meta["shapes"][:meta["n_grads"]]
    return [to_tensor(g, meta["dtype"]).reshape(s) for g, s in zip(split(fx["grads"], shapes), shapes)]


def settings_of(lr, momentum, weight_decay):
    return types.SimpleNamespace(learning=types.SimpleNamespace(learning_rate=lr, momentum=momentum,
                                                                weight_decay=weight_decay))


def torch_sgd_step(model: nn.Module, grads, lr, momentum, weight_decay, threads: int = 4) -> nn.Module:
    """The reference's op sequence (model_trainer.py:137-143) on a deep copy:
    a fresh torch.optim.SGD, param.grad = grad over the zip, one step."""
    import copy
    m = copy.deepcopy(model).cpu()
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
    for p, g in zip(m.parameters(), grads):
        p.grad = g.detach().cpu().clone()
    with torch_threads(threads):
        opt.step()
    return m


def torch_flat_step(p: torch.Tensor, g: torch.Tensor, lr: float, weight_decay: float, threads: int = 4):
    """The step on one flat CPU tensor pair through torch.optim.SGD."""
    q = nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    with torch_threads(threads):
        torch.optim.SGD([q], lr=lr, momentum=0.9, weight_decay=weight_decay).step()
    return q.detach()
