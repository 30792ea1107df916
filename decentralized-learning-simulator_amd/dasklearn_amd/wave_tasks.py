"""ArenaTask: the unit of work of every batched aggregate, and what the batched launches share.

One aggregate task, resolved for the kernels, is the record
    model0   models[0]: the result is copy.deepcopy(model0) around fresh output arenas
    layout   model0's ParamLayout (dtype groups, offsets, sizes)
    views    {dtype: [one entry per model]} in layout order: the model's flat device arena of that
             dtype, or None for a model that keeps the group in separate contiguous device tensors (a
             device train task's deepcopy). A group with a None is read in place, tensor by tensor,
             from `rows`; one without is read from the arenas.
    weights  one Python float per model (FedAvg), or None (the unweighted aggregates)
    rows     every model's parameter list, or None when no group is read in place
The producers (batch.aggregate_batch, RoundExecutor, krum.model_distances_batch) build lists of such
tasks, `prepared`; aggregate_arena_tasks here and robust_arena_tasks, distances_arena_tasks and
krum_arena_tasks in model_inputs.py run them, all tasks of a dtype and device in one library call.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch
from torch import nn

from . import _native
from .arena import _restride, arena_empty, module_from_arenas


def _device_views(views) -> Optional[torch.device]:
    """The one CUDA device every flat view lives on, or None."""
    dev = None
    if not views:
        return None
    for vs in views.values():
        if vs is None:
            return None
        for v in vs:
            if not v.is_cuda or (dev is not None and v.device != dev):
                return None
            dev = v.device
    return dev


def _row_on(params, view, idx, sizes, dev):
    """Model i's tensors of a dtype group as the rows path reads them: its
    parameters when they are on `dev` (read in place; a registered arena's
    parameters are views of it), else the pieces of its flat view (an arena
    uploaded or copied to `dev`, e.g. a host model of the wave)."""
    if view is None or params[idx[0]].device == dev:
        return params
    row = [None] * len(params)
    for k, piece in zip(idx, view.split(sizes)):
        row[k] = piece
    return row


def _rows_device(vs, rows, layout, dt) -> torch.device:
    """The task's device: that of its flat views, or (none) of the first
    model read in place (its tensors are on the target device by
    construction, RoundExecutor._arena_of)."""
    for v in vs:
        if v is not None:
            return v.device
    t = rows[0][layout.groups[dt][0]]
    if not t.is_cuda:
        raise ValueError("rows input: tensors must be on a CUDA device")
    return t.device


class ArenaTask:
    """One aggregate task as the batched launches read it (the module docstring has the fields)."""
    __slots__ = ("model0", "layout", "views", "weights", "rows")

    def __init__(self, model0, layout, views, weights=None, rows=None):
        self.model0, self.layout, self.views, self.weights, self.rows = model0, layout, views, weights, rows

    @property
    def fan_in(self) -> int:
        """The number of models: the length of a dtype group's view list, or of `rows` when the
        models have no parameters (and so no group). Without either the task does not say."""
        for vs in self.views.values():
            return len(vs)
        if self.rows is None:
            raise ValueError("a task without parameters and without rows does not state its fan-in")
        return len(self.rows)

    def groups(self, empty: bool = True):
        """(dtype, total, view list, read in place?, device) of every dtype group in layout order
        (empty=False: of the non-empty ones). The device is the views', or for a group read in place
        _rows_device's, which raises ValueError for tensors that are not on a CUDA device."""
        layout = self.layout
        for dt in layout.groups:
            total, vs = layout.totals[dt], self.views[dt]
            if total or empty:
                in_place = any(v is None for v in vs)
                yield dt, total, vs, in_place, _rows_device(vs, self.rows, layout, dt) if in_place else vs[0].device

    def rows_on(self, dt, vs, dev, models=None):
        """The tensors of a group read in place, one parameter list per model (of `models`, some
        indices, when given), on the task's device (_row_on)."""
        idx, sizes = self.layout.groups[dt], self.layout.split_sizes[dt]
        return [_row_on(self.rows[i], vs[i], idx, sizes, dev) for i in (range(len(vs)) if models is None else models)]

    def tensor_rows(self, dt, vs, dev, models=None):
        """(rows_on, the (index, size) pairs of the group's non-empty tensors), every such tensor
        checked against the layout: what the kernels that take one pointer per tensor rely on."""
        rows = self.rows_on(dt, vs, dev, models)
        live = [(k, size) for k, size in zip(self.layout.groups[dt], self.layout.split_sizes[dt]) if size]
        for r in rows:
            for k, size in live:
                t = r[k]
                if t.device != dev or t.dtype != dt or t.numel() != size or not t.is_contiguous():
                    raise ValueError("rows input: tensors must be contiguous, of the layout's dtype and size, "
                                     "on the task's device")
        return rows, live

    def select(self, indices, weights) -> "ArenaTask":
        """The task over the models `indices` alone, with `weights`: model0 and the layout stay."""
        return ArenaTask(self.model0, self.layout, {dt: [vs[j] for j in indices] for dt, vs in self.views.items()},
                         weights, None if self.rows is None else [self.rows[j] for j in indices])


def output_arenas(task: ArenaTask, outs: list):
    """task.groups() with a fresh output arena on the group's device behind each group's fields; the
    task's {dtype: arena} (the empty groups' too) is appended to `outs`."""
    o = {}
    outs.append(o)
    for g in task.groups():
        o[g[0]] = out = arena_empty(g[1], g[0], g[4])
        yield (*g, out)


def finish_modules(prepared, outs, on_launched: Optional[Callable[[], None]] = None,
                   restride: bool = False) -> List[nn.Module]:
    """The end of every batched aggregate, once all launches are queued: on_launched() first, then
    one module per task (deepcopy(model0) semantics, parameters views of its arenas outs[i]; with
    `restride`, model0's strides), the list `prepared` consumed on the way: entry i is set to None
    once its module exists. A caller that drops its own references to the input modules in
    on_launched lets them go as the outputs are made: the arenas stay alive through the launch
    views, and the stream orders any reuse of their memory after the kernels."""
    if on_launched is not None:
        on_launched()
    mods = []
    for i, o in enumerate(outs):
        task = prepared[i]
        prepared[i] = None
        mod = module_from_arenas(task.model0, task.layout, o)
        mods.append(_restride(mod, task.layout) if restride else mod)
    return mods


def aggregate_arena_tasks(prepared: List[ArenaTask], mode: int = _native.DLSIM_EXACT,
                          on_launched: Optional[Callable[[], None]] = None) -> List[nn.Module]:
    """The weighted reduce of every task of `prepared` (every task's arenas on one device) -> one
    module per task, all tasks of a dtype and device in batched launches (fp64 groups: one
    dlsim_wreduce_f64 per task). The groups read in place go, every such task's tensors, into one
    dlsim_wreduce_batched call per dtype and device (one sub-task per tensor, pointers collected
    in C), instead of copying each such model into an arena first. on_launched and the consumption
    of `prepared`: finish_modules."""
    by_dtype = {}
    by_rows = {}
    outs = []
    for task in prepared:
        layout = task.layout
        for dt, _, vs, in_place, dev, out in output_arenas(task, outs):
            w = _native.weights_for_dtype(task.weights, dt)
            if in_place:
                by_rows.setdefault((dt, dev), []).append(
                    ((task.rows_on(dt, vs, dev), layout.groups[dt], layout.split_sizes[dt], w, out.data_ptr(),
                      layout.byte_offsets[dt]), vs, out))
            else:
                by_dtype.setdefault((dt, dev), []).append((vs, w, out))
    for (dt, dev), group in by_rows.items():
        # every task read from separate tensors: one library call for all
        stream = torch.cuda.current_stream(dev)
        code = _native.dtype_code(dt)
        if _native.wreduce_rows_multi([g[0] for g in group], code, mode, stream.cuda_stream, dev.index):
            continue
        for (rows, idx, sizes, w, out_ptr, offs), vs, out in group:
            if not _native.wreduce_rows(rows, idx, sizes, w, out_ptr, offs, code, mode, stream.cuda_stream, dev.index):
                # a model's tensors are elsewhere (its arena was copied
                # here): flatten the in-place ones too, one reduce
                with torch.no_grad():
                    flat = [v if v is not None else
                            torch._C._nn.flatten_dense_tensors([rows[i][k] for k in idx]).to(dev)
                            for i, v in enumerate(vs)]
                _native.wreduce(flat, w, out, mode, stream)
    by_rows.clear()
    for (dt, dev), group in by_dtype.items():
        stream = torch.cuda.current_stream(dev)
        if dt == torch.float64:
            for vs, w, out in group:
                _native.wreduce(vs, w, out, mode, stream)
            continue
        _native.wreduce_batched(group, mode, stream)
    by_dtype.clear()
    return finish_modules(prepared, outs, on_launched)
