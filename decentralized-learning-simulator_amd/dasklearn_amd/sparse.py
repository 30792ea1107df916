"""Top-k sparsified model sharing on the GPU.

A peer sends only the k coordinates of its model that moved most since it last
shared them (`TopKSharer.share`, dlsim_topk_select); a receiver substitutes its
own value wherever a neighbour stayed silent and averages (`mix`, `mix_batch`,
dlsim_sparse_wreduce). The rule of the CHOCO-SGD family and of partial-model
sharing. The reference shares dense models only, so nothing here replaces
reference code; `functions.sparsify` and `functions.aggregate_sparse` are the
worker tasks. float32 and bfloat16 parameters only.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _native
from .arena import arena_empty, layout_of
from .batch import _resolve
from .model_inputs import ModelInputs, flat_groups as _flat_groups


def split_k(k: int, sizes: Sequence[int]) -> List[int]:
    """k coordinates over dtype groups of `sizes` elements: group g first gets
    floor(k * sizes[g] / sum(sizes)); the coordinates the floors leave over go
    one each to the groups that still have room, in layout order, round after
    round. The shares sum to k and none exceeds its group."""
    total = sum(sizes)
    if not 0 <= k <= total:
        raise ValueError(f"k must satisfy 0 <= k <= {total} (got {k})")
    shares = [k * s // total if total else 0 for s in sizes]
    left = k - sum(shares)
    while left:
        for g, s in enumerate(sizes):
            if left and shares[g] < s:
                shares[g] += 1
                left -= 1
    return shares


def _check_dtypes(layout) -> None:
    for dt in layout.groups:
        if dt not in (torch.float32, torch.bfloat16):
            raise TypeError(f"top-k sharing supports float32 and bfloat16 parameters, got {dt}")


class SparseModel:
    """What a peer puts on the wire: per dtype group of its model's layout
    (idx int32 ascending, val in the group's dtype, the group's size)."""

    def __init__(self, groups: "Dict[torch.dtype, Tuple[torch.Tensor, torch.Tensor, int]]"):
        self.groups = groups

    @property
    def nbytes(self) -> int:
        """Bytes on the wire: 4 per index and the element size per value."""
        return sum(idx.numel() * 4 + val.numel() * val.element_size() for idx, val, _ in self.groups.values())

    def to(self, device) -> "SparseModel":
        return SparseModel({dt: (idx.to(device), val.to(device), size) for dt, (idx, val, size) in self.groups.items()})


class TopKSharer:
    """The sender's state: the last-shared copy of one peer's model, a zeroed
    device arena per dtype group laid out by ParamLayout, so the first share is
    the top-k of |x|. Give `k` (coordinates per share) or `ratio` (k =
    floor(ratio * parameters)). k is split over the dtype groups by split_k:
    floor(k * size / total) each, the remainder one each in layout order to the
    groups with room."""

    def __init__(self, model: nn.Module, k: Optional[int] = None, ratio: Optional[float] = None, device=None):
        if (k is None) == (ratio is None):
            raise ValueError("give exactly one of k and ratio")
        self.layout = layout_of(model)
        _check_dtypes(self.layout)
        self.sizes = [self.layout.totals[dt] for dt in self.layout.groups]
        total = sum(self.sizes)
        if ratio is not None:
            if not 0.0 <= ratio <= 1.0:
                raise ValueError(f"ratio must lie in [0, 1] (got {ratio})")
            k = int(ratio * total)
        self.k = int(k)
        self.shares = split_k(self.k, self.sizes)
        self.device = device
        self.ref: Optional[Dict[torch.dtype, torch.Tensor]] = None

    def share(self, model: nn.Module) -> SparseModel:
        """One selection launch per dtype group: the group's share of the k
        coordinates that moved most since they were last shared, which the
        last-shared copy then takes over. Stream-ordered on the model's device
        (cuda:0, or `device`, for a host model, staged by the arena path). A
        device-arena model is read in place; a plain device model is first
        copied into one flat buffer per group (_flat_groups), a dense copy per
        call."""
        inputs = ModelInputs([model], 1, "top-k sharing", self.device)
        if inputs.layout._signature != self.layout._signature:
            raise ValueError("the model's parameters differ from the ones this sharer was made for")
        dev = inputs.dev
        groups = {}
        with torch.no_grad(), torch.cuda.device(dev):
            if self.ref is None:
                self.ref = {dt: torch.zeros(self.layout.totals[dt], dtype=dt, device=dev) for dt in self.layout.groups}
            flats = _flat_groups(inputs)
            for (dt, size), kg in zip(self.layout.totals.items(), self.shares):
                idx = torch.empty(kg, dtype=torch.int32, device=dev)
                val = torch.empty(kg, dtype=dt, device=dev)
                if kg:
                    _native.topk_select(flats[dt], self.ref[dt], kg, idx, val)
                groups[dt] = (idx, val, size)
            if any(p is not None and len(p) for p in inputs.keep):
                torch.cuda.current_stream(dev).synchronize()  # the staged copies' sources may go now
        return SparseModel(groups)


def _task(own_model, sparse_models, weights, to_host):
    """(inputs, host_out, outs, [(own, lists, w, out) per non-empty group]) of one mixing task."""
    models = [own_model] + list(sparse_models)
    _native.check_sparse_fan_in(len(sparse_models))
    w = _resolve(models, weights)
    inputs = ModelInputs([own_model], 1, "sparse mixing")
    layout, dev = inputs.layout, inputs.dev
    _check_dtypes(layout)
    host_out = inputs.host_out(to_host)
    outs = {dt: torch.empty(0, dtype=dt, device="cpu" if host_out else dev)
            for dt in layout.groups if not layout.totals[dt]}
    calls = []
    with torch.no_grad(), torch.cuda.device(dev):
        flats = _flat_groups(inputs)
        for dt, own in flats.items():
            lists = []
            for j, sm in enumerate(sparse_models):
                if dt not in sm.groups or sm.groups[dt][2] != layout.totals[dt]:
                    raise ValueError(f"sparse model {j} was not made from a model with the receiver's parameters")
                idx, val, _ = sm.groups[dt]
                lists.append((idx.to(dev, non_blocking=True), val.to(dev, non_blocking=True)))
            out = outs[dt] = arena_empty(layout.totals[dt], dt, dev)
            calls.append((own, lists, _native.weights_for_dtype(w, dt), out))
    return inputs, host_out, outs, calls


def mix(own_model: nn.Module, sparse_models: Sequence[SparseModel], weights: Optional[Sequence[float]] = None,
        to_host: Optional[bool] = None) -> nn.Module:
    """FedAvg.aggregate([own_model] + the neighbours densified over own_model,
    weights) bit for bit, without densifying: one dlsim_sparse_wreduce launch
    per dtype group. FedAvg's weight rules (None or []: 1/n each, else one per
    model, own_model's first); a new module with copy.deepcopy(own_model)
    semantics, where own_model lives unless to_host says otherwise. At most 31
    neighbours (ValueError). A device-arena own_model is read in place; a
    plain device model costs one dense copy first (_flat_groups), a host model
    its staging."""
    inputs, host_out, outs, calls = _task(own_model, sparse_models, weights, to_host)
    with torch.no_grad(), torch.cuda.device(inputs.dev):
        for own, lists, w, out in calls:
            _native.sparse_wreduce(own, lists, w, out)
        if not host_out:
            torch.cuda.current_stream(inputs.dev).synchronize()  # staged copies' sources and moved lists may go now
    return inputs.module(outs, to_host)


def mix_batch(tasks, to_host: Optional[bool] = None) -> List[nn.Module]:
    """`mix` for the tasks of a round, [(own_model, sparse_models, weights or
    None), ...], through dlsim_sparse_wreduce_batched: one call per dtype and
    device over all tasks, bit-identical to per-task `mix`. Meant for
    device-arena models (read in place); others are staged as in `mix`."""
    prepared = [_task(own, sms, w, to_host) for own, sms, w in tasks]
    calls: Dict[tuple, list] = {}
    for inputs, _, _, task_calls in prepared:
        for c in task_calls:
            calls.setdefault((c[0].dtype, inputs.dev), []).append(c)
    with torch.no_grad():
        for (_, dev), cs in calls.items():
            with torch.cuda.device(dev):
                _native.sparse_wreduce_batched(cs)
        for dev in {dev for _, dev in calls}:
            torch.cuda.current_stream(dev).synchronize()
    return [inputs.module(outs, to_host) for inputs, _, outs, _ in prepared]


__all__ = ["SparseModel", "TopKSharer", "mix", "mix_batch", "split_k"]
