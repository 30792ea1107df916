"""The reference's optimizer (dasklearn/optimizer/sgd.py) with its step on the
MI355X: every step of torch.optim.SGD(lr, momentum, weight_decay) in one HIP
launch per dtype group, bit-identical to torch's CPU step.

`ModelTrainer.train` (model_trainer.py:89-92,126) builds a new
`SGDOptimizer(model, lr, momentum, weight_decay)` every round, copies the
previous round's state in (`optimizer.optimizer.load_state_dict(...)`) and calls
`optimizer.optimizer.zero_grad()` / `.step()` once per local step.
`SGDOptimizer` here has the same attributes; its `.optimizer` is an `ArenaSGD`
when every parameter is a device tensor of a kernel dtype (fp32, fp64, bf16),
and exactly what the reference builds, a plain torch.optim.SGD, otherwise (CPU
models, fp16, a mix), so the reference's loop runs unchanged with either:

    dasklearn.model_trainer.SGDOptimizer = dasklearn_amd.optimizer.sgd.SGDOptimizer
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import _native
from ..arena import ParamLayout, _pyhost, arena_empty
from ..sgd import check_hyper_parameters

_PER_LAUNCH = _native.SGD_MOMENTUM_TENSORS_PER_LAUNCH


class ArenaSGD(torch.optim.Optimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) (dampening 0, no
    Nesterov, no maximize: what the reference's SGDOptimizer can set) for
    device parameters of the kernel dtypes, stepped by dlsim_sgd_momentum_step
    / dlsim_sgd_momentum_step_tensors (momentum == 0: dlsim_sgd_step /
    dlsim_sgd_step_tensors in place, no state, as torch keeps none).

    One param group with torch's keys; `zero_grad`, `state_dict` and
    `load_state_dict` behave as torch's, and state dicts pass between an
    ArenaSGD and a torch.optim.SGD over a CPU copy of the model in both
    directions. The momentum buffers are views into one arena per dtype, in
    parameters() order; `load_state_dict` copies loaded buffers into it once.

    Per dtype group a step is ONE flat launch when parameters, gradients and
    buffers are each one contiguous buffer in the same order (parameters of a
    device arena, gradients lined up the same way, e.g. by `grad_arena=True`)
    and the dtype is not bf16 (whose rounding follows each tensor's own
    extent); otherwise the tensors entry, one launch per 64 tensors.
    `last_launches` is the number of kernel launches of the last step(),
    `last_paths` the path each dtype group took ("flat" or "tensors").

    grad_arena=True (off by default): `zero_grad()` points every `p.grad` at a
    zeroed view of one gradient arena per dtype instead of setting it to None,
    autograd accumulates into those views, and the flat launch applies. It
    changes what an UNUSED parameter sees: a zero gradient instead of none, so
    weight decay (and its momentum) still applies to it, where torch would
    skip it. That is why it is opt-in.

    Work goes on torch's current stream of the parameters' device."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, weight_decay: float = 0.0,
                 grad_arena: bool = False):
        check_hyper_parameters(lr, momentum, weight_decay)
        super().__init__(params, self.torch_defaults(lr, momentum, weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError("ArenaSGD takes one param group (the reference's SGDOptimizer builds one)")
        ps: List[torch.Tensor] = self.param_groups[0]["params"]
        for p in ps:
            if not p.is_cuda or not _native.sgd_kernel_dtype(p.dtype):
                raise TypeError("ArenaSGD needs device parameters of dtype float32, float64 or bfloat16 "
                                f"(got {p.dtype} on {p.device}); SGDOptimizer builds torch.optim.SGD for the rest")
            if p.device != ps[0].device:
                raise ValueError("ArenaSGD needs all parameters on one device")
        self._device = ps[0].device
        self._layout = ParamLayout(None, list(ps))
        self._buf_arenas: Dict[torch.dtype, torch.Tensor] = {}
        self._buf_views: List[Optional[torch.Tensor]] = [None] * len(ps)
        self._buf_ptrs: List[int] = [0] * len(ps)
        self._has_buf: List[bool] = [False] * len(ps)  # state[p] holds a momentum buffer (kept beside the state)
        self._numels: List[int] = [p.numel() for p in ps]
        self.grad_arena = bool(grad_arena)
        self._grad_arenas: Dict[torch.dtype, torch.Tensor] = {}
        self._grad_views: List[Optional[torch.Tensor]] = [None] * len(ps)
        self.last_launches = 0
        self.last_paths: Dict[torch.dtype, str] = {}

    @staticmethod
    def torch_defaults(lr, momentum, weight_decay) -> dict:
        """torch.optim.SGD's own defaults (and so its param-group keys),
        whatever this torch's SGD has."""
        return dict(torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, weight_decay=weight_decay).defaults)

    # ---- arenas -------------------------------------------------------------------
    def _views(self, arenas: Dict[torch.dtype, torch.Tensor], views: List[Optional[torch.Tensor]]) -> None:
        L = self._layout
        for dt, idx in L.groups.items():
            if dt in arenas or L.totals[dt] == 0:
                continue
            a = arenas[dt] = arena_empty(L.totals[dt], dt, self._device)
            for k, (shape, strides, off) in zip(idx, L.view_specs[dt]):
                views[k] = torch.as_strided(a, shape, strides, off)

    def _buffers(self) -> None:
        if not self._buf_arenas:
            self._views(self._buf_arenas, self._buf_views)
            self._buf_ptrs = [0 if v is None else v.data_ptr() for v in self._buf_views]

    def _adopt_state(self) -> None:
        """Loaded momentum buffers move into the arena (one copy each)."""
        ps = self.param_groups[0]["params"]
        for k, p in enumerate(ps):
            st = self.state.get(p)
            self._has_buf[k] = bool(st) and st.get("momentum_buffer") is not None
            if not self._has_buf[k] or p.numel() == 0:
                continue
            self._buffers()
            view = self._buf_views[k]
            if st["momentum_buffer"] is not view:
                view.copy_(st["momentum_buffer"])
                st["momentum_buffer"] = view

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("ArenaSGD takes one param group")
        with torch.no_grad():
            self._adopt_state()

    def zero_grad(self, set_to_none: bool = True) -> None:
        """torch's zero_grad; with grad_arena=True every p.grad becomes a
        zeroed view of the gradient arena whatever `set_to_none` says."""
        if not self.grad_arena:
            return super().zero_grad(set_to_none)
        self._views(self._grad_arenas, self._grad_views)
        with torch.no_grad():
            for a in self._grad_arenas.values():
                a.zero_()
        for p, v in zip(self.param_groups[0]["params"], self._grad_views):
            if v is not None and (p.grad is None or p.grad.data_ptr() != v.data_ptr()
                                  or not p.grad.is_contiguous()):
                p.grad = v

    # ---- the step -----------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        if group["dampening"] != 0 or group["nesterov"] or group["maximize"]:
            raise ValueError("ArenaSGD: dampening, nesterov and maximize are not in the kernel "
                             "(the reference's SGDOptimizer sets none of them)")
        lr, momentum, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
        check_hyper_parameters(lr, momentum, wd)
        ps: List[torch.Tensor] = group["params"]
        grads = [p.grad for p in ps]
        self.last_launches = 0
        self.last_paths = {}
        dev = self._device
        if torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                self._step_groups(ps, grads, lr, momentum, wd)
        else:
            self._step_groups(ps, grads, lr, momentum, wd)
        return loss

    def _step_groups(self, ps, grads, lr, momentum, wd) -> None:
        L = self._layout
        stream = torch._C._cuda_getCurrentRawStream(self._device.index)
        numels, has = self._numels, self._has_buf
        for dt, idx in L.groups.items():
            active = [k for k in idx if grads[k] is not None and numels[k]]
            if not active:
                continue
            for k in active:
                if grads[k].is_sparse:
                    raise RuntimeError("ArenaSGD does not support sparse gradients")
            first = []
            if momentum != 0:
                self._buffers()
                first = [k for k in active if not has[k]]
            flat = (dt != torch.bfloat16 and len(active) == len(idx) and (not first or len(first) == len(active))
                    and self._flat_step(ps, grads, dt, lr, momentum, wd, bool(first)))
            self.last_paths[dt] = "flat" if flat else "tensors"
            if not flat:
                self._tensors_step(ps, grads, active, dt, lr, momentum, wd, stream)
            for k in first:
                self.state[ps[k]]["momentum_buffer"] = self._buf_views[k]
                has[k] = True

    def _flat_step(self, ps, grads, dt, lr, momentum, wd, first: bool) -> bool:
        L = self._layout
        pview = L.arena_view(ps, dt)
        if pview is None:
            return False
        gview = L.arena_view(grads, dt)
        if gview is None:
            return False
        if momentum == 0:
            _native.sgd_step(pview, gview, pview, lr, wd)
        else:
            buf = self._buf_arenas[dt]
            _native.sgd_momentum_step(pview, gview, None if first else buf, pview, buf, lr, momentum, wd)
        self.last_launches += 1
        return True

    def _tensors_step(self, ps, grads, active, dt, lr, momentum, wd, stream) -> None:
        n = len(active)
        back = []
        # the data pointers of parameters and gradients read in C (None: some tensor is not contiguous)
        ptrs = _pyhost.data_ptrs((ps, grads), active)
        if ptrs is not None:
            pp, gp = ptrs[:n], ptrs[n:]
        else:
            pp, gp = [], []
            for k in active:
                q, g = ps[k], grads[k]
                if not g.is_contiguous():
                    g = g.contiguous()
                    back.append((None, g))  # alive until the launch is queued
                if not q.is_contiguous():  # stepped on a contiguous copy, copied back
                    q = q.detach().contiguous()
                    back.append((ps[k], q))
                pp.append(q.data_ptr())
                gp.append(g.data_ptr())
        ns = [self._numels[k] for k in active]
        code = _native.dtype_code(dt, single_task=True)
        if momentum == 0:
            _native.sgd_step_tensors_raw(pp, gp, pp, ns, lr, wd, code, stream)
        else:
            bo = [self._buf_ptrs[k] for k in active]
            bp = [b if self._has_buf[k] else None for k, b in zip(active, bo)]
            _native.sgd_momentum_step_tensors_raw(pp, gp, bp, pp, bo, ns, lr, momentum, wd, code, stream)
        self.last_launches += -(-n // _PER_LAUNCH)
        for p, q in back:
            if p is not None:
                p.copy_(q)


class SGDOptimizer:
    """Drop-in for the reference's dasklearn.optimizer.sgd.SGDOptimizer: the
    same constructor and attributes; `.optimizer` is an ArenaSGD for a device
    model of kernel dtypes and the reference's torch.optim.SGD otherwise."""

    def __init__(self, model, learning_rate, momentum, weight_decay, grad_arena: bool = False):
        self.learning_rate = learning_rate
        self.momentum = momentum
        self.weight_decay = weight_decay
        params = list(model.parameters())
        on_device = bool(params) and all(p.is_cuda and p.device == params[0].device
                                         and _native.sgd_kernel_dtype(p.dtype) for p in params)
        if on_device:
            self.optimizer = ArenaSGD(params, lr=learning_rate, momentum=momentum, weight_decay=weight_decay,
                                      grad_arena=grad_arena)
        else:
            self.optimizer = torch.optim.SGD(params, lr=learning_rate, momentum=momentum, weight_decay=weight_decay)
