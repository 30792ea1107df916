"""Block-quantised model sharing on the GPU.

A peer sends every parameter as an 8- or 4-bit code with one fp32 scale per
256 elements (`QuantSharer.share`, dlsim_quantize), optionally keeping the
rounding error as a residual it adds to its next share (error feedback); a
receiver mixes its own model with the neighbours' codes, decoded in registers
(`mix`, `mix_batch`, dlsim_quant_wreduce), or decodes one to a model for any
other aggregator (`QuantModel.dequantize`). The quantiser of QSGD- and
CHOCO-style compressed gossip. The reference shares dense models only, so
nothing here replaces reference code; `functions.quantize` and
`functions.aggregate_quantized` are the worker tasks. float32 and bfloat16
parameters only.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _native
from .arena import _restride, _target_device, arena_empty, arenas_to_host, layout_of, module_from_arenas
from .batch import _resolve
from .model_inputs import ModelInputs, flat_groups


def _check_dtypes(layout) -> None:
    for dt in layout.groups:
        if dt not in (torch.float32, torch.bfloat16):
            raise TypeError(f"quantised sharing supports float32 and bfloat16 parameters, got {dt}")


class QuantModel:
    """What a peer puts on the wire: per dtype group of its model's layout
    (codes uint8, scales float32, the group's size, bits)."""

    def __init__(self, groups: "Dict[torch.dtype, Tuple[torch.Tensor, torch.Tensor, int, int]]"):
        self.groups = groups

    @property
    def nbytes(self) -> int:
        """Bytes on the wire: the codes and 4 per scale."""
        return sum(codes.numel() + 4 * scales.numel() for codes, scales, _, _ in self.groups.values())

    def to(self, device) -> "QuantModel":
        return QuantModel({dt: (c.to(device), s.to(device), size, bits) for dt, (c, s, size, bits) in self.groups.items()})

    def dequantize(self, like_model: nn.Module, to_host: Optional[bool] = None) -> nn.Module:
        """The decoded model (dlsim_dequantize, one launch per dtype group): a
        new module with copy.deepcopy(like_model) semantics whose parameters
        hold the decoded values, where like_model lives unless to_host says
        otherwise. What any other aggregator takes in place of the sender's
        model."""
        layout = layout_of(like_model)
        _check_dtypes(layout)
        dev = _target_device(layout.params, None)
        host_out = (not any(p.is_cuda for p in layout.params)) if to_host is None else to_host
        outs = {}
        with torch.no_grad(), torch.cuda.device(dev):
            for dt, total in layout.totals.items():
                if dt not in self.groups or self.groups[dt][2] != total:
                    raise ValueError("the quantised model was not made from a model with these parameters")
                codes, scales, _, bits = self.groups[dt]
                out = outs[dt] = arena_empty(total, dt, dev)
                if total:
                    _native.dequantize(codes.to(dev), scales.to(dev), bits, out)
            if host_out:
                outs = arenas_to_host(outs, torch.cuda.current_stream(dev))
            else:
                torch.cuda.current_stream(dev).synchronize()  # the moved codes may go now
        return _restride(module_from_arenas(like_model, layout, outs), layout)


class QuantSharer:
    """The sender's side for one peer's model. bits 8 or 4; rounding "nearest"
    or "stochastic" (call c of `share` uses seed_c = mix32(seed + c), so a
    sequence of shares is reproducible from `seed`); with error_feedback a
    zero-initialised residual arena per dtype group, which every share adds to
    the model before quantising and replaces with the new rounding error."""

    def __init__(self, model: nn.Module, bits: int = 8, rounding: str = "nearest", error_feedback: bool = False,
                 seed: int = 0, device=None):
        if bits not in (4, 8):
            raise ValueError(f"bits must be 4 or 8 (got {bits})")
        if rounding not in _native.QUANT_ROUNDINGS:
            raise ValueError(f'rounding must be "nearest" or "stochastic" (got {rounding!r})')
        self.layout = layout_of(model)
        _check_dtypes(self.layout)
        self.bits, self.rounding, self.error_feedback, self.seed, self.device = bits, rounding, error_feedback, seed, device
        self.calls = 0
        self.resid: Optional[Dict[torch.dtype, torch.Tensor]] = None

    def share(self, model: nn.Module) -> QuantModel:
        """One quantiser launch per dtype group. Stream-ordered on the model's
        device (cuda:0, or `device`, for a host model, staged by the arena
        path). A device-arena model is read in place; a plain device model is
        first copied into one flat buffer per group (model_inputs.flat_groups)."""
        inputs = ModelInputs([model], 1, "quantised sharing", self.device)
        if inputs.layout._signature != self.layout._signature:
            raise ValueError("the model's parameters differ from the ones this sharer was made for")
        dev = inputs.dev
        seed = _native.mix32(self.seed + self.calls)
        self.calls += 1
        groups = {}
        with torch.no_grad(), torch.cuda.device(dev):
            if self.error_feedback and self.resid is None:
                self.resid = {dt: torch.zeros(self.layout.totals[dt], dtype=dt, device=dev) for dt in self.layout.groups}
            flats = flat_groups(inputs)
            for dt, size in self.layout.totals.items():
                codes = torch.empty((size * self.bits + 7) // 8, dtype=torch.uint8, device=dev)
                scales = torch.empty((size + _native.QUANT_BLOCK - 1) // _native.QUANT_BLOCK, dtype=torch.float32, device=dev)
                if size:
                    _native.quantize(flats[dt], codes, scales, self.bits, self.rounding, seed,
                                     self.resid[dt] if self.error_feedback else None)
                groups[dt] = (codes, scales, size, self.bits)
            if any(p is not None and len(p) for p in inputs.keep):
                torch.cuda.current_stream(dev).synchronize()  # the staged copies' sources may go now
        return QuantModel(groups)


def _task(own_model, quant_models, weights, to_host):
    """(inputs, host_out, outs, [(own, rows, w, out) per non-empty group]) of one mixing task."""
    models = [own_model] + list(quant_models)
    _native.check_quant_fan_in(len(quant_models))
    w = _resolve(models, weights)
    inputs = ModelInputs([own_model], 1, "quantised mixing")
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
            for j, qm in enumerate(quant_models):
                if dt not in qm.groups or qm.groups[dt][2] != layout.totals[dt]:
                    raise ValueError(f"quantised model {j} was not made from a model with the receiver's parameters")
                codes, scales, _, bits = qm.groups[dt]
                rows.append((codes.to(dev, non_blocking=True), scales.to(dev, non_blocking=True), bits))
            out = outs[dt] = arena_empty(layout.totals[dt], dt, dev)
            calls.append((own, rows, _native.weights_for_dtype(w, dt), out))
    return inputs, host_out, outs, calls


def mix(own_model: nn.Module, quant_models: Sequence[QuantModel], weights: Optional[Sequence[float]] = None,
        to_host: Optional[bool] = None) -> nn.Module:
    """FedAvg.aggregate([own_model] + [qm.dequantize(own_model) for each
    neighbour], weights) bit for bit, without decoding a neighbour to memory:
    one dlsim_quant_wreduce launch per dtype group. FedAvg's weight rules (None
    or []: 1/n each, else one per model, own_model's first); a new module with
    copy.deepcopy(own_model) semantics, where own_model lives unless to_host
    says otherwise. At most 31 neighbours (ValueError); they may differ in
    bits. A device-arena own_model is read in place; a plain device model costs
    one dense copy first, a host model its staging."""
    inputs, host_out, outs, calls = _task(own_model, quant_models, weights, to_host)
    with torch.no_grad(), torch.cuda.device(inputs.dev):
        for own, rows, w, out in calls:
            _native.quant_wreduce(own, rows, w, out)
        if not host_out:
            torch.cuda.current_stream(inputs.dev).synchronize()  # staged copies' sources and moved codes may go now
    return inputs.module(outs, to_host)


def mix_batch(tasks, to_host: Optional[bool] = None) -> List[nn.Module]:
    """`mix` for the tasks of a round, [(own_model, quant_models, weights or
    None), ...], through dlsim_quant_wreduce_batched: one call per dtype and
    device over all tasks, bit-identical to per-task `mix`. Meant for
    device-arena models (read in place); others are staged as in `mix`."""
    prepared = [_task(own, qms, w, to_host) for own, qms, w in tasks]
    calls: Dict[tuple, list] = {}
    for inputs, _, _, task_calls in prepared:
        for c in task_calls:
            calls.setdefault((c[0].dtype, inputs.dev), []).append(c)
    with torch.no_grad():
        for (_, dev), cs in calls.items():
            with torch.cuda.device(dev):
                _native.quant_wreduce_batched(cs)
        for dev in {dev for _, dev in calls}:
            torch.cuda.current_stream(dev).synchronize()
    return [inputs.module(outs, to_host) for inputs, _, outs, _ in prepared]


__all__ = ["QuantModel", "QuantSharer", "mix", "mix_batch"]
