"""The fresh-SGD step on a module: the arithmetic of the `gradient_update`
task (reference dasklearn/model_trainer.py:133-143).

`ModelTrainer.gradient_update(model, gradient_model)` builds a NEW
torch.optim.SGD(lr, momentum, weight_decay), assigns `param.grad = grad` over
`zip(model.parameters(), gradient_model.gradient)` and steps once. A fresh
optimizer's momentum buffer is a clone of the gradient, so per parameter

    g' = grad.add(param, alpha=weight_decay)     # only if weight_decay != 0
    param.add_(g', alpha=-lr)

whatever the momentum. Here that runs in one HIP kernel per dtype group
(csrc/sgd_kernels.hpp, dlsim_sgd_step / dlsim_sgd_step_tensors), bit-identical
to torch's CPU ops for fp32, fp64 and bf16:

* device models (e.g. an `aggregate` output over one device arena) with device
  gradients are read in place; the result is a module over one device arena;
* host models with host gradients (the reference's case) are packed into the
  pinned staging rows by the library's pack pool, copied H2D, stepped, and come
  back as a host module;
* fp16 groups (PyTorch's CPU result depends on its thread count) and NaN
  hyper-parameters run torch's own two adds on the CPU.

Unlike the reference, the input model is left untouched: only the returned
module carries the update.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _native
from .arena import (STAGING, _elem_size, _restride, _target_device, arena_empty, arenas_to_host, layout_of,
                    module_from_arenas, module_params, registered_arenas)


def check_hyper_parameters(lr: float, momentum: float, weight_decay: float) -> None:
    """torch.optim.SGD's own checks, same messages."""
    if lr < 0.0:
        raise ValueError(f"Invalid learning rate: {lr}")
    if momentum < 0.0:
        raise ValueError(f"Invalid momentum value: {momentum}")
    if weight_decay < 0.0:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


def _paired_gradients(params: Sequence[torch.Tensor], grads: Sequence) -> List[Optional[torch.Tensor]]:
    """Gradient of every parameter under `zip(parameters(), grads)` (None past
    the shorter list, or where the list holds None), checked as
    `param.grad = grad` checks it."""
    out: List[Optional[torch.Tensor]] = [None] * len(params)
    for k, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            continue
        if not isinstance(g, torch.Tensor):
            raise TypeError(f"assigned grad expected to be a Tensor or None but got grad of type {type(g).__name__}")
        if g.shape != p.shape:
            raise RuntimeError(f"parameter {k}: assigned grad has data of a different size")
        if g.dtype != p.dtype:
            raise RuntimeError(f"parameter {k}: assigned grad has data of a different type")
        if g.device != p.device:
            raise RuntimeError(f"parameter {k}: assigned grad has data located on a different device")
        out[k] = g.detach()
    return out


def _torch_step(p: torch.Tensor, g: Optional[torch.Tensor], lr: float, weight_decay: float) -> torch.Tensor:
    """torch's own op sequence on CPU tensors (the single-tensor SGD path)."""
    p = p.cpu()
    if g is None:
        return p
    g = g.cpu()
    if weight_decay != 0:
        g = g.add(p, alpha=weight_decay)
    return p.add(g, alpha=-lr)


def _cpu_group(params, grads, idx, offsets, total, dt, lr, weight_decay) -> torch.Tensor:
    h = torch.empty(total, dtype=dt)
    for k, off in zip(idx, offsets):
        p = params[k].detach()
        h[off:off + p.numel()].copy_(_torch_step(p, grads[k], lr, weight_decay).reshape(-1))
    return h


def _flat(t: torch.Tensor, keep: list) -> torch.Tensor:
    """`t` in parameters() element order, contiguous (copied if it is not)."""
    if not t.is_contiguous():
        t = t.contiguous()
        keep.append(t)
    return t


def _device_group(layout, params, grads, dt, dev, lr, weight_decay, pview, keep) -> torch.Tensor:
    """Device parameters and gradients, read in place."""
    idx, offsets = layout.groups[dt], layout._group_offsets[dt]
    total, esz = layout.totals[dt], _elem_size(dt)
    out = arena_empty(total, dt, dev)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    if pview is not None and dt != torch.bfloat16 and all(grads[k] is not None for k in idx):
        # gradients that are one flat buffer too (fp32 / fp64: no per-tensor rule): one flat launch
        gview = layout.arena_view(grads, dt)
        if gview is not None:
            return _native.sgd_step(pview, gview, out, lr, weight_decay)
    pp, gp, op, ns = [], [], [], []
    for k, off in zip(idx, offsets):
        p = params[k].detach()
        n = p.numel()
        if n == 0:
            continue
        if grads[k] is None:  # past the gradient list: unchanged
            out[off:off + n].copy_(p.reshape(-1))
            continue
        pp.append(_flat(p, keep).data_ptr())
        gp.append(_flat(grads[k], keep).data_ptr())
        op.append(out.data_ptr() + off * esz)
        ns.append(n)
    _native.sgd_step_tensors_raw(pp, gp, op, ns, lr, weight_decay, _native.dtype_code(dt, single_task=True), stream)
    return out


def _host_group(layout, params, grads, dt, dev, lr, weight_decay, want_host: bool, keep) -> torch.Tensor:
    """Host parameters and gradients: packed into two pinned staging rows
    (parameters, gradients) by the library's pack pool, one H2D each, the step,
    and with want_host the D2H."""
    idx, offsets = layout.groups[dt], layout._group_offsets[dt]
    total, esz = layout.totals[dt], _elem_size(dt)
    out = arena_empty(total, dt, dev)
    stream = torch.cuda.current_stream(dev)
    with_grad = [(k, off) for k, off in zip(idx, offsets) if grads[k] is not None and params[k].numel()]
    dev_rows, pinned = STAGING.acquire(dev, dt, 2, total, stream)
    synced = False
    try:
        _native.host_pack([_flat(params[k].detach(), keep) for k in idx], [o * esz for o in offsets], pinned[0])
        _native.host_pack([_flat(grads[k], keep) for k, _ in with_grad], [o * esz for _, o in with_grad], pinned[1])
        with torch.cuda.stream(stream):
            dev_rows[0].copy_(pinned[0], non_blocking=True)
            dev_rows[1].copy_(pinned[1], non_blocking=True)
            if dt != torch.bfloat16 and len(with_grad) == len(idx):
                _native.sgd_step(dev_rows[0], dev_rows[1], out, lr, weight_decay, stream)
            else:
                # bf16 rounds per tensor (each is its own buffer for torch's
                # vector / scalar split); a short gradient list leaves the rest as is
                out.copy_(dev_rows[0], non_blocking=True)
                base_p, base_g = dev_rows[0].data_ptr(), dev_rows[1].data_ptr()
                _native.sgd_step_tensors_raw([base_p + o * esz for _, o in with_grad],
                                             [base_g + o * esz for _, o in with_grad],
                                             [out.data_ptr() + o * esz for _, o in with_grad],
                                             [params[k].numel() for k, _ in with_grad], lr, weight_decay,
                                             _native.dtype_code(dt, single_task=True), stream.cuda_stream)
        if want_host:
            out = arenas_to_host({dt: out}, stream)[dt]  # waits for the stream
            synced = True
    finally:
        STAGING.release(dev, dt, stream, synced)
    return out


def sgd_step_module(model: nn.Module, gradients: Sequence, lr: float, momentum: float = 0.0,
                    weight_decay: float = 0.0, device=None, to_host: Optional[bool] = None) -> nn.Module:
    """A fresh module of `model`'s class holding the parameters after the
    first step of a new torch.optim.SGD(lr, momentum, weight_decay) with
    `param.grad = grad` over zip(model.parameters(), gradients); buffers
    copied, every parameter requires_grad, no `gradient` attribute; `model`
    and `gradients` are only read.

    to_host None: the result lives where the model's parameters live."""
    check_hyper_parameters(lr, momentum, weight_decay)
    lr, weight_decay = float(lr), float(weight_decay)
    reg = registered_arenas(model)
    layout = reg[0] if reg is not None else layout_of(model)
    params = layout.params
    grads = _paired_gradients(params, gradients)
    on_host = not any(p.is_cuda for p in params)
    host_out = on_host if to_host is None else to_host
    in_kernel = not (math.isnan(lr) or math.isnan(weight_decay))

    def kernel_group(dt, idx):
        return in_kernel and _native.sgd_kernel_dtype(dt) and layout.totals[dt] > 0 \
            and any(grads[k] is not None for k in idx)
    need_device = not host_out or any(kernel_group(dt, idx) for dt, idx in layout.groups.items())
    dev = _target_device(params, device) if need_device else None
    arenas: Dict[torch.dtype, torch.Tensor] = {}
    keep: list = []  # contiguous copies, alive until the stream has read them
    with torch.no_grad():
        for dt, idx in layout.groups.items():
            if not kernel_group(dt, idx):
                arenas[dt] = _cpu_group(params, grads, idx, layout._group_offsets[dt], layout.totals[dt], dt, lr,
                                        weight_decay)
            elif params[idx[0]].is_cuda:
                pview = reg[1][dt] if reg is not None else layout.arena_view(params, dt)
                arenas[dt] = _device_group(layout, params, grads, dt, dev, lr, weight_decay, pview, keep)
            else:
                arenas[dt] = _host_group(layout, params, grads, dt, dev, lr, weight_decay, host_out, keep)
        if host_out:
            left = {dt: a for dt, a in arenas.items() if a.is_cuda}
            if left:
                arenas.update(arenas_to_host(left, torch.cuda.current_stream(dev)))
        else:
            arenas = {dt: a if a.is_cuda else a.to(dev) for dt, a in arenas.items()}
            if keep:
                torch.cuda.current_stream(dev).synchronize()
    out = module_from_arenas(model, layout, arenas)
    if any(not p.is_contiguous() for p in params):
        _restride(out, layout)
    # train() returns unserialize_model(serialize_model(model)): a model built
    # anew, so every parameter requires grad and nothing rides along
    for q in module_params(out):
        q.requires_grad_(True)
    out.__dict__.pop("gradient", None)
    return out
