"""MX (OCP microscaling) model sharing on the GPU.

A peer sends every parameter as an FP8 (E4M3 or E5M2) or FP4 (E2M1) code with
one power-of-two scale byte per 32 elements (`MXSharer.share`,
dlsim_mx_quantize), optionally keeping the rounding error as a residual it
adds to its next share (error feedback); a receiver mixes its own model with
the neighbours' codes, decoded in registers by gfx950's scaled conversions
(`mix`, `mix_batch`, dlsim_mx_wreduce), or decodes one to a model for any other
aggregator (`MXModel.dequantize`). The rules are quant.py's: FedAvg's weights,
at most 31 neighbours, which may differ in format, float32 and bfloat16
parameters only, the same synchronisation points. The reference shares dense
models only, so nothing here replaces reference code.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _native
from .arena import _restride, _target_device, arena_empty, arenas_to_host, layout_of, module_from_arenas
from .batch import _resolve
from .model_inputs import ModelInputs, flat_groups
from .quant import _check_dtypes


class MXModel:
    """What a peer puts on the wire: per dtype group of its model's layout
    (codes uint8, scale bytes uint8, the group's size, the format's name)."""

    def __init__(self, groups: "Dict[torch.dtype, Tuple[torch.Tensor, torch.Tensor, int, str]]"):
        self.groups = groups

    @property
    def nbytes(self) -> int:
        """Bytes on the wire: the codes and one per scale."""
        return sum(codes.numel() + scales.numel() for codes, scales, _, _ in self.groups.values())

    def to(self, device) -> "MXModel":
        return MXModel({dt: (c.to(device), s.to(device), size, fmt) for dt, (c, s, size, fmt) in self.groups.items()})

    def dequantize(self, like_model: nn.Module, to_host: Optional[bool] = None) -> nn.Module:
        """The decoded model (dlsim_mx_dequantize, one launch per dtype group):
        a new module with copy.deepcopy(like_model) semantics whose parameters
        hold the decoded values, where like_model lives unless to_host says
        otherwise."""
        layout = layout_of(like_model)
        _check_dtypes(layout)
        dev = _target_device(layout.params, None)
        host_out = (not any(p.is_cuda for p in layout.params)) if to_host is None else to_host
        outs = {}
        with torch.no_grad(), torch.cuda.device(dev):
            for dt, total in layout.totals.items():
                if dt not in self.groups or self.groups[dt][2] != total:
                    raise ValueError("the MX model was not made from a model with these parameters")
                codes, scales, _, fmt = self.groups[dt]
                out = outs[dt] = arena_empty(total, dt, dev)
                if total:
                    _native.mx_dequantize(codes.to(dev), scales.to(dev), fmt, out)
            if host_out:
                outs = arenas_to_host(outs, torch.cuda.current_stream(dev))
            else:
                torch.cuda.current_stream(dev).synchronize()  # the moved codes may go now
        return _restride(module_from_arenas(like_model, layout, outs), layout)


class MXSharer:
    """The sender's side for one peer's model. fmt "fp8_e4m3", "fp8_e5m2" or
    "fp4"; rounding is to nearest, ties to even; with error_feedback a
    zero-initialised residual arena per dtype group, which every share adds to
    the model before quantising and replaces with the new rounding error."""

    def __init__(self, model: nn.Module, fmt: str = "fp8_e4m3", error_feedback: bool = False, device=None):
        _native.mx_format_code(fmt)
        self.layout = layout_of(model)
        _check_dtypes(self.layout)
        self.fmt, self.error_feedback, self.device = fmt, error_feedback, device
        self.resid: Optional[Dict[torch.dtype, torch.Tensor]] = None

    def share(self, model: nn.Module) -> MXModel:
        """One quantiser launch per dtype group, stream-ordered on the model's
        device; the model is read as QuantSharer.share reads it."""
        inputs = ModelInputs([model], 1, "MX sharing", self.device)
        if inputs.layout._signature != self.layout._signature:
            raise ValueError("the model's parameters differ from the ones this sharer was made for")
        dev = inputs.dev
        groups = {}
        with torch.no_grad(), torch.cuda.device(dev):
            if self.error_feedback and self.resid is None:
                self.resid = {dt: torch.zeros(self.layout.totals[dt], dtype=dt, device=dev) for dt in self.layout.groups}
            flats = flat_groups(inputs)
            for dt, size in self.layout.totals.items():
                nc, ns = _native.mx_sizes(size, self.fmt)
                codes = torch.empty(nc, dtype=torch.uint8, device=dev)
                scales = torch.empty(ns, dtype=torch.uint8, device=dev)
                if size:
                    _native.mx_quantize(flats[dt], codes, scales, self.fmt, self.resid[dt] if self.error_feedback else None)
                groups[dt] = (codes, scales, size, self.fmt)
            if any(p is not None and len(p) for p in inputs.keep):
                torch.cuda.current_stream(dev).synchronize()  # the staged copies' sources may go now
        return MXModel(groups)


def _task(own_model, mx_models, weights, to_host):
    """(inputs, host_out, outs, [(own, rows, w, out) per non-empty group]) of one mixing task."""
    models = [own_model] + list(mx_models)
    _native.check_quant_fan_in(len(mx_models))
    w = _resolve(models, weights)
    inputs = ModelInputs([own_model], 1, "MX mixing")
    layout, dev = inputs.layout, inputs.dev
    _check_dtypes(layout)
    host_out = inputs.host_out(to_host)
    outs = {dt: torch.empty(0, dtype=dt, device="cpu" if host_out else dev)
            for dt in layout.groups if not layout.totals[dt]}
    calls = []
    with torch.no_grad(), torch.cuda.device(dev):
        flats = flat_groups(inputs)
        for dt, own in flats.items():
            rows = []
            for j, qm in enumerate(mx_models):
                if dt not in qm.groups or qm.groups[dt][2] != layout.totals[dt]:
                    raise ValueError(f"MX model {j} was not made from a model with the receiver's parameters")
                codes, scales, _, fmt = qm.groups[dt]
                rows.append((codes.to(dev, non_blocking=True), scales.to(dev, non_blocking=True), fmt))
            out = outs[dt] = arena_empty(layout.totals[dt], dt, dev)
            calls.append((own, rows, _native.weights_for_dtype(w, dt), out))
    return inputs, host_out, outs, calls


def mix(own_model: nn.Module, mx_models: Sequence[MXModel], weights: Optional[Sequence[float]] = None,
        to_host: Optional[bool] = None) -> nn.Module:
    """FedAvg.aggregate([own_model] + [qm.dequantize(own_model) for each
    neighbour], weights) bit for bit, without decoding a neighbour to memory:
    one dlsim_mx_wreduce launch per dtype group. Weights, result placement,
    the limit of 31 neighbours and the cost of each kind of own_model are
    quant.mix's; the neighbours may differ in format."""
    inputs, host_out, outs, calls = _task(own_model, mx_models, weights, to_host)
    with torch.no_grad(), torch.cuda.device(inputs.dev):
        for own, rows, w, out in calls:
            _native.mx_wreduce(own, rows, w, out)
        if not host_out:
            torch.cuda.current_stream(inputs.dev).synchronize()  # staged copies' sources and moved codes may go now
    return inputs.module(outs, to_host)


def mix_batch(tasks, to_host: Optional[bool] = None) -> List[nn.Module]:
    """`mix` for the tasks of a round, [(own_model, mx_models, weights or
    None), ...], through dlsim_mx_wreduce_batched: one call per dtype and
    device over all tasks, bit-identical to per-task `mix`."""
    prepared = [_task(own, qms, w, to_host) for own, qms, w in tasks]
    calls: Dict[tuple, list] = {}
    for inputs, _, _, task_calls in prepared:
        for c in task_calls:
            calls.setdefault((c[0].dtype, inputs.dev), []).append(c)
    with torch.no_grad():
        for (_, dev), cs in calls.items():
            with torch.cuda.device(dev):
                _native.mx_wreduce_batched(cs)
        for dev in {dev for _, dev in calls}:
            torch.cuda.current_stream(dev).synchronize()
    return [inputs.module(outs, to_host) for inputs, _, outs, _ in prepared]


__all__ = ["MXModel", "MXSharer", "mix", "mix_batch"]
