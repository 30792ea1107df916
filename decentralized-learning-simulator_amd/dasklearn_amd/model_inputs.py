"""The aggregates over n <= 32 models (median and trimmed mean; the mean around the median; pairwise
distances, Krum and Bulyan; the reduce-and-measure pass of the geometric median and centered clipping) and
ModelInputs, which resolves
a list of models into what their kernels read. arena.py re-exports the public names. The batched forms
(robust_arena_tasks, distances_arena_tasks, krum_arena_tasks, reduce_dist_arena_tasks, geomed_arena_tasks)
take lists of wave_tasks.ArenaTask, whose module describes the record; batch.method_route picks among them."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _native
from .arena import (ParamLayout, _arena_entry, _clone_module, _data_ptrs, _elem_size, _register_arenas, _restride,
                    _target_device, aggregate_modules, aligned_empty, arena_empty, arenas_to_host, base_align,
                    input_arenas, module_from_arenas, module_params, row_stride)
from .wave_tasks import ArenaTask, aggregate_arena_tasks, finish_modules, output_arenas


def _stage_rows(all_params, idx, total: int, dt: torch.dtype, dev: torch.device):
    """One device row per model holding its dtype group in layout order (host
    models through one page-locked block and plain copies; models on another
    device through .to). Returns (rows, page-locked block or None): the block
    must outlive the copies queued on the current stream."""
    n = len(all_params)
    esz = _elem_size(dt)
    stride = row_stride(total, esz)
    flat = aligned_empty(n * stride, dt, dev, base_align(total * esz, esz))
    rows = [flat[i * stride:i * stride + total] for i in range(n)]
    pinned = None
    for i, ps in enumerate(all_params):
        parts = [ps[k].detach().reshape(-1) for k in idx]
        if any(q.is_cuda for q in parts):
            torch.cat([q.to(dev) for q in parts], out=rows[i])
            continue
        if pinned is None:
            pinned = torch.empty(n * total, dtype=dt, pin_memory=True)
        h = pinned[i * total:(i + 1) * total]
        torch.cat(parts, out=h)
        rows[i].copy_(h, non_blocking=True)
    return rows, pinned


class ModelInputs:
    """`models` as kernel inputs on `dev` (where models[0] lives, or `device`), resolved once. Per
    non-empty dtype group of models[0]'s layout one of two routes:
      ("flat", [one flat device tensor per model])  device arenas, read in place; or, for host models
          and models on another device, one staged device row per model (copied here)
      ("tensors", [one pointer list per model])     separate device tensors, for the *_tensors
          entries (non-contiguous ones copied first)
    An empty list raises IndexError; more than `max_inputs` models ValueError (`what` names the
    kernels); then a model whose parameter list differs from models[0]'s ValueError (ZipMismatch).
    keep: the page-locked blocks and contiguous copies that the copies queued on the current stream
    read, alive as long as this object; the sources may go once the stream has been waited for.
    staged: some input is a copy, so the result module takes models[0]'s strides (_restride)."""

    def __init__(self, models, max_inputs: int, what: str, device=None):
        self.model0 = models[0]  # IndexError for an empty list, as FedAvg
        n = self.n = len(models)
        _native._check_fan_in(n, max_inputs, "the " + what + " kernels take at most {limit} models (got {n})")
        layout, all_params, in_views = input_arenas(models)  # ZipMismatch is a ValueError
        self.layout, self.all_params, self.in_views = layout, all_params, in_views
        self.dev = dev = _target_device(all_params[0], device)
        dix = dev.index
        self.keep, self.staged, self.routes = [], False, {}
        for dt, idx in layout.groups.items():
            total = layout.totals[dt]
            if total == 0:
                continue
            views = in_views[dt]
            if views is not None and all(v.get_device() == dix for v in views):
                self.routes[dt] = ("flat", views)
                continue
            with torch.no_grad(), torch.cuda.device(dev):  # the copies below run on dev's current stream
                if all(ps[k].get_device() == dix for ps in all_params for k in idx):
                    copies, ptrs = _data_ptrs(all_params, idx)
                    self.keep.append(copies)
                    self.staged = self.staged or bool(copies)
                    t = len(idx)
                    ptrs = list(ptrs)
                    self.routes[dt] = ("tensors", [ptrs[i * t:(i + 1) * t] for i in range(n)])
                else:
                    rows, pinned = _stage_rows(all_params, idx, total, dt, dev)
                    self.keep.append(pinned)
                    self.staged = True
                    self.routes[dt] = ("flat", rows)

    def __iter__(self):
        """(dtype, route kind, route data) of the non-empty groups in layout order."""
        for dt in self.layout.groups:
            if dt in self.routes:
                yield (dt, *self.routes[dt])

    def host_out(self, to_host: Optional[bool]) -> bool:
        return (not any(p.is_cuda for p in self.layout.params)) if to_host is None else to_host

    def module(self, outs: Dict[torch.dtype, torch.Tensor], to_host: Optional[bool]) -> nn.Module:
        """copy.deepcopy(models[0]) around the arenas `outs` (one per dtype
        group, the empty ones too), on the host when models[0] lives there (or
        to_host says so): the device arenas are then copied, which waits for
        the stream."""
        if self.host_out(to_host):
            outs = dict(outs)
            outs.update(arenas_to_host({dt: a for dt, a in outs.items() if a.is_cuda},
                                       torch.cuda.current_stream(self.dev)))
        out = module_from_arenas(self.model0, self.layout, outs)
        return _restride(out, self.layout) if self.staged else out


def robust_modules(models: List[nn.Module], lo_hi_fn, device=None, to_host: Optional[bool] = None) -> nn.Module:
    """The coordinate-wise order-statistic aggregate of `models` on the GPU
    (dlsim_robust_reduce): per parameter element the n models' values are
    sorted and the window [lo, hi) = lo_hi_fn(n) of them is averaged. As
    aggregate_modules: a new module with copy.deepcopy(models[0]) semantics
    (buffers and attributes are models[0]'s), the models only read, one launch
    per dtype group, the result where models[0] lives unless to_host says
    otherwise. A model whose parameter list differs from models[0]'s raises
    ValueError (no zip semantics here); more than 32 models too."""
    models[0]  # IndexError for an empty list, as FedAvg
    n = len(models)
    _native.check_robust_fan_in(n)
    lo, hi = lo_hi_fn(n)
    inputs = ModelInputs(models, _native.MAX_ROBUST_INPUTS, "median and trimmed-mean", device)
    layout, dev, host_out = inputs.layout, inputs.dev, inputs.host_out(to_host)
    outs: Dict[torch.dtype, torch.Tensor] = {dt: torch.empty(0, dtype=dt, device="cpu" if host_out else dev)
                                             for dt in layout.groups if not layout.totals[dt]}
    with torch.no_grad(), torch.cuda.device(dev):
        raw_stream = torch._C._cuda_getCurrentRawStream(dev.index)
        for dt, kind, data in inputs:
            out = outs[dt] = arena_empty(layout.totals[dt], dt, dev)
            if kind == "flat":
                _native.robust_reduce(data, lo, hi, out)
            else:
                # every tensor a sub-task of one batched dispatch, not a launch of its own
                _native.robust_reduce_tensors_batched_raw([p for ptrs in data for p in ptrs], n,
                                                          layout.split_sizes[dt], layout.byte_offsets[dt], lo, hi,
                                                          out.data_ptr(), _native.dtype_code(dt, single_task=True),
                                                          raw_stream)
        if not host_out and any(k is not None and len(k) for k in inputs.keep):
            torch.cuda.current_stream(dev).synchronize()  # the staged copies' sources may go now
    return inputs.module(outs, to_host)


def _nearest_outs(inputs: ModelInputs, idx: Sequence[int], keep: int, host_out: bool) -> Dict[torch.dtype, torch.Tensor]:
    """One arena per dtype group of inputs.layout: the mean around the median
    (dlsim_robust_nearest_reduce) with `keep` values over the models `idx` of
    `inputs`, in that order, one call per non-empty group; the empty groups'
    arenas on the host when host_out. Stream-ordered: nothing waits."""
    layout, dev = inputs.layout, inputs.dev
    idx = list(idx)
    outs: Dict[torch.dtype, torch.Tensor] = {dt: torch.empty(0, dtype=dt, device="cpu" if host_out else dev)
                                             for dt in layout.groups if not layout.totals[dt]}
    with torch.no_grad(), torch.cuda.device(dev):
        raw_stream = torch._C._cuda_getCurrentRawStream(dev.index)
        for dt, kind, data in inputs:
            out = outs[dt] = arena_empty(layout.totals[dt], dt, dev)
            if kind == "flat":
                _native.robust_nearest_reduce([data[i] for i in idx], keep, out)
            else:
                _native.robust_nearest_reduce_tensors_raw([p for i in idx for p in data[i]], len(idx),
                                                          layout.split_sizes[dt], layout.byte_offsets[dt], keep,
                                                          out.data_ptr(), _native.dtype_code(dt, single_task=True),
                                                          raw_stream)
    return outs


def nearest_modules(models: List[nn.Module], keep_fn, device=None, to_host: Optional[bool] = None) -> nn.Module:
    """The coordinate-wise mean around the median of `models` on the GPU
    (dlsim_robust_nearest_reduce): per parameter element the n models' values
    are sorted and the keep = keep_fn(n) of them closest to the lower median
    are averaged in ascending order. Everything else as robust_modules: a new
    module with copy.deepcopy(models[0]) semantics, the models only read, one
    call per dtype group, the result where models[0] lives unless to_host says
    otherwise; ValueError for a model whose parameter list differs from
    models[0]'s, for more than 32 models and for a keep outside [1, n]."""
    models[0]  # IndexError for an empty list, as FedAvg
    n = len(models)
    _native.check_robust_fan_in(n)
    keep = int(keep_fn(n))
    if not 1 <= keep <= n:
        raise ValueError(f"mean around the median of n = {n} models: keep = {keep} must satisfy 1 <= keep <= n")
    inputs = ModelInputs(models, _native.MAX_ROBUST_INPUTS, "median and trimmed-mean", device)
    host_out = inputs.host_out(to_host)
    outs = _nearest_outs(inputs, range(n), keep, host_out)
    if not host_out and any(k is not None and len(k) for k in inputs.keep):
        torch.cuda.current_stream(inputs.dev).synchronize()  # the staged copies' sources may go now
    return inputs.module(outs, to_host)


def bulyan_modules(models: List[nn.Module], f: int, to_host: Optional[bool] = None) -> nn.Module:
    """Bulyan of `models` with Byzantine count f (gradient_aggregation/krum.py
    has the rule): the distance matrix on the GPU (model_distances), the
    selection of theta = n - 2f models on the host (krum.bulyan_select), then
    the mean around the median with keep = theta - 2f over the selected models
    in ascending index order (dlsim_robust_nearest_reduce), bit-identical to
    nearest_modules(selected, lambda _: keep). The reduce reads the rows that
    were resolved or staged for the distances: no model is copied twice.
    Buffers, attributes and parameter strides are copy.deepcopy(models[0])'s,
    also when models[0] is not selected; the result lives where models[0] lives
    unless to_host says otherwise. One D2H copy of n*n doubles and one stream
    synchronisation per call, as krum_modules."""
    from dasklearn_amd.gradient_aggregation import krum as _krum
    models[0]  # IndexError for an empty list, as FedAvg
    n = len(models)
    _native.check_pairdist_fan_in(n)
    _krum.check_bulyan_params(n, f)
    inputs = ModelInputs(models, _native.MAX_PAIRDIST_INPUTS, "pairwise-distance")
    chosen = _krum.bulyan_select(_distances(inputs).tolist(), f)  # waits for the stream: the staged sources may go
    outs = _nearest_outs(inputs, chosen, len(chosen) - 2 * f, inputs.host_out(to_host))
    return inputs.module(outs, to_host)


def robust_arena_tasks(prepared: List[ArenaTask], lo_hi_fn, on_launched=None) -> List[nn.Module]:
    """wave_tasks.aggregate_arena_tasks for the coordinate-wise order statistics
    (the weights are not read: these aggregates are unweighted): every task's
    window [lo, hi) = lo_hi_fn(its fan-in), one dlsim_robust_reduce_batched
    call per dtype and device over all tasks, a group read in place one
    sub-task per tensor of the same call. on_launched and the consumption of
    `prepared`: wave_tasks.finish_modules. More than 32 models in a task raise
    ValueError before anything is queued."""
    calls: Dict[tuple, list] = {}  # (dtype, device) -> [fan-ins, pointers, los, his, out pointers, lengths, keep]
    outs = []
    for task in prepared:
        if task.views:
            n = task.fan_in
            _native.check_robust_fan_in(n)
            lo, hi = lo_hi_fn(n)
        for dt, total, vs, in_place, dev, out in output_arenas(task, outs):
            if total == 0:
                continue
            c = calls.setdefault((dt, dev), [[], [], [], [], [], [], []])
            if in_place:  # one sub-task per non-empty tensor
                rows, live = task.tensor_rows(dt, vs, dev)
                base, esz, offsets = out.data_ptr(), out.element_size(), task.layout.offsets
                subs = [([r[k].data_ptr() for r in rows], base + offsets[k] * esz, size) for k, size in live]
                c[6].append(rows)
            else:
                subs = [([v.data_ptr() for v in vs], out.data_ptr(), total)]
                c[6].append(vs)
            for ptrs, out_ptr, size in subs:
                c[0].append(n)
                c[1] += ptrs
                c[2].append(lo)
                c[3].append(hi)
                c[4].append(out_ptr)
                c[5].append(size)
    with torch.no_grad():
        for (dt, dev), (fan, ptrs, los, his, out_ptrs, numels, _) in calls.items():
            _native.robust_reduce_batched_raw(fan, ptrs, los, his, out_ptrs, numels,
                                              _native.dtype_code(dt, single_task=True),
                                              torch._C._cuda_getCurrentRawStream(dev.index))
    calls.clear()
    return finish_modules(prepared, outs, on_launched)


def _distances(inputs: ModelInputs) -> torch.Tensor:
    n, dev, layout = inputs.n, inputs.dev, inputs.layout
    with torch.no_grad(), torch.cuda.device(dev):
        raw_stream = torch._C._cuda_getCurrentRawStream(dev.index)
        d2 = torch.empty(n * n, dtype=torch.float64, device=dev)
        first = True
        for dt, kind, data in inputs:
            if kind == "flat":
                _native.pairwise_sqdist(data, d2, accumulate=not first)
            else:
                _native.pairwise_sqdist_tensors_raw([p for ptrs in data for p in ptrs], n, layout.split_sizes[dt],
                                                    _native.dtype_code(dt, single_task=True), d2.data_ptr(),
                                                    not first, raw_stream)
            first = False
        if first:
            d2.zero_()
        host = d2.cpu()  # waits for the stream: the staged copies' sources may go now
    return host.reshape(n, n)


def model_distances(models: List[nn.Module], device=None) -> torch.Tensor:
    """The [n, n] float64 host matrix of squared L2 distances between the
    models' parameters (dlsim_pairwise_sqdist): entry [i][j] is the sum over
    every parameter element of (double(x_i) - double(x_j))^2, bitwise
    symmetric, the diagonal +0.0. Parameters only, as the aggregators. The
    dtype groups of models[0]'s layout add into the one matrix in layout
    order. A model whose parameter list differs from models[0]'s raises
    ValueError; more than 32 models too; an empty list IndexError. The matrix
    comes back with one D2H copy of n*n doubles, which waits for the stream."""
    return _distances(ModelInputs(models, _native.MAX_PAIRDIST_INPUTS, "pairwise-distance", device))


def distances_arena_tasks(prepared: List[ArenaTask]) -> List[torch.Tensor]:
    """model_distances for many tasks at once: one host [n, n] float64 matrix
    per task of `prepared` (the weights are not read), bit-identical to
    model_distances on the same models. All matrices of a device live in one
    device buffer and come back with one D2H copy, which waits for the stream:
    one synchronisation per device, not one per task. Each device's calls are
    issued with that device current (the library allocates its workspace on
    the current device).

    A dtype group with arena views is one segment of
    dlsim_pairwise_sqdist_batched, a group read in place one segment per
    non-empty tensor. A model's dtype groups add into its matrix in its own
    layout order: the calls go in rounds, round r takes every task's r-th
    non-empty group, one call per (dtype, device) inside a round, accumulating
    from round 1 on. `prepared` is only read. More than 32 models in a task
    raise ValueError before anything is queued. Models without parameters give
    n x n zeros, as model_distances does, with n read from `rows`."""
    plans = []  # per task: (fan-in, device or None, [(dtype, n_tensors, pointers, lengths)])
    keep = []
    sizes: Dict[torch.device, int] = {}
    for task in prepared:
        n = task.fan_in
        _native.check_pairdist_fan_in(n)
        dev, groups = None, []
        for dt, total, vs, in_place, dev in task.groups(empty=False):
            if not in_place:
                groups.append((dt, 1, [v.data_ptr() for v in vs], [total]))
                keep.append(vs)
                continue
            rows, live = task.tensor_rows(dt, vs, dev)
            groups.append((dt, len(live), [r[k].data_ptr() for r in rows for k, _ in live], [s for _, s in live]))
            keep.append(rows)
        off = None
        if dev is not None:
            off = sizes.get(dev, 0)
            sizes[dev] = off + n * n
        plans.append((n, dev, off, groups))
    with torch.no_grad():
        bufs = {dev: torch.empty(size, dtype=torch.float64, device=dev) for dev, size in sizes.items()}
        r = 0
        while True:
            calls: Dict[tuple, list] = {}  # (dtype, device) -> [fan-ins, tensor counts, pointers, lengths, matrices]
            for n, dev, off, groups in plans:
                if r < len(groups):
                    dt, t, ptrs, lens = groups[r]
                    c = calls.setdefault((dt, dev), [[], [], [], [], []])
                    c[0].append(n)
                    c[1].append(t)
                    c[2] += ptrs
                    c[3] += lens
                    c[4].append(bufs[dev].data_ptr() + 8 * off)
            if not calls:
                break
            for (dt, dev), (fan, nts, ptrs, lens, mats) in calls.items():
                with torch.cuda.device(dev):  # the launches and the workspace allocation go to the current device
                    _native.pairwise_sqdist_batched_raw(fan, nts, ptrs, lens,
                                                        _native.dtype_code(dt, single_task=True), mats, r > 0,
                                                        torch._C._cuda_getCurrentRawStream(dev.index))
            r += 1
        hosts = {dev: buf.cpu() for dev, buf in bufs.items()}  # waits for the stream
    keep.clear()
    return [torch.zeros(n, n, dtype=torch.float64) if dev is None else hosts[dev][off:off + n * n].reshape(n, n)
            for n, dev, off, _ in plans]


def krum_arena_tasks(prepared: List[ArenaTask], f: int, m, on_launched=None) -> List[nn.Module]:
    """wave_tasks.aggregate_arena_tasks for Krum (m None) and Multi-Krum (m an
    int, or a callable fan-in -> m) with Byzantine count f (the weights are not
    read: these aggregates are unweighted), each task what krum_modules gives
    for its models, bit for bit. Two phases around one synchronisation per
    device: every task's distance matrix in batched launches and one D2H copy
    (distances_arena_tasks), the selection per task on the host
    (krum.krum_select), then
      Krum:       the selected models' values copied bit for bit into fresh
                  output arenas, all tasks in one torch._foreach_copy_ per
                  device;
      Multi-Krum: one aggregate_arena_tasks call over all tasks, each the
                  selected models in ascending index order (ArenaTask.select)
                  with float(1./m) each in DLSIM_EXACT, as
                  FedAvg.aggregate(selected).
    Buffers, attributes and strides are models[0]'s. on_launched fires once
    the second phase is queued (the inputs are read after the synchronisation,
    so they must live until then); `prepared` is consumed as in
    aggregate_arena_tasks. More than 32 models or (n, f, m) outside Krum's
    rule raise ValueError before anything is queued."""
    from dasklearn_amd.gradient_aggregation import krum as _krum
    ms = []
    for task in prepared:
        n = task.fan_in
        _native.check_pairdist_fan_in(n)
        mk = 1 if m is None else int(m(n)) if callable(m) else int(m)
        _krum.check_krum_params(n, f, mk)
        ms.append(mk)
    chosen = [_krum.krum_select(d.tolist(), f, mk) for d, mk in zip(distances_arena_tasks(prepared), ms)]
    if m is not None:
        selected = []
        for i, (task, idx, mk) in enumerate(zip(prepared, chosen, ms)):
            selected.append(task.select(idx, [float(1. / mk)] * mk))
            prepared[i] = None
        layouts = [t.layout for t in selected]
        mods = aggregate_arena_tasks(selected, _native.DLSIM_EXACT, on_launched)
        return [_restride(mod, layout) for mod, layout in zip(mods, layouts)]
    outs = []
    copies: Dict[torch.device, tuple] = {}
    for task, (w,) in zip(prepared, chosen):
        for dt, total, vs, in_place, dev, out in output_arenas(task, outs):
            if total == 0:
                continue
            dst, src = copies.setdefault(dev, ([], []))
            if vs[w] is not None:
                dst.append(out)
                src.append(vs[w])
                continue
            (params,), live = task.tensor_rows(dt, vs, dev, (w,))  # read in place
            for k, size in live:
                off = task.layout.offsets[k]
                dst.append(out[off:off + size])
                src.append(params[k].detach().reshape(-1))
    with torch.no_grad():
        for dev, (dst, src) in copies.items():
            with torch.cuda.device(dev):
                torch._foreach_copy_(dst, src)
    copies.clear()
    return finish_modules(prepared, outs, on_launched, restride=True)


class ReduceDistPlan:
    """The inputs of the fused reduce-and-measure kernel (dlsim_wreduce_dist)
    for a list of models, resolved once (ModelInputs) and run any number of
    times: the iterations of the geometric median and of centered clipping
    (gradient_aggregation/geomed.py) read the same rows with new weights."""

    def __init__(self, models: List[nn.Module], device=None):
        self.inputs = ModelInputs(models, _native.MAX_REDUCEDIST_INPUTS, "reduce-and-measure", device)
        self.n = self.inputs.n
        self.module = self.inputs.module

    def run(self, idx: Sequence[int], weights: Sequence[float], center=None, want_out: bool = True):
        """One pass over the models `idx` (behind `center`, a dict of flat
        device arenas per dtype as an earlier pass returned it, as input 0 when
        given) with one weight per input. Returns (dict dtype -> new device
        arena, or {} without want_out; the float64 device vector of squared
        distances, one per input). Dtype groups accumulate into the one vector
        in layout order. Stream-ordered: nothing waits."""
        layout, dev = self.inputs.layout, self.inputs.dev
        idx = list(idx)
        m = len(idx) + (center is not None)
        assert len(weights) == m
        outs = {dt: torch.empty(0, dtype=dt, device=dev) for dt in layout.groups if want_out and not layout.totals[dt]}
        with torch.no_grad(), torch.cuda.device(dev):
            raw_stream = torch._C._cuda_getCurrentRawStream(dev.index)
            d2 = torch.empty(m, dtype=torch.float64, device=dev)
            first = True
            for dt, kind, data in self.inputs:
                out = arena_empty(layout.totals[dt], dt, dev) if want_out else None
                if want_out:
                    outs[dt] = out
                if kind == "flat":
                    ins = ([center[dt]] if center is not None else []) + [data[i] for i in idx]
                    _native.wreduce_dist(ins, weights, out, d2, accumulate=not first)
                else:
                    ptrs = []
                    if center is not None:
                        base = center[dt].data_ptr()
                        ptrs += [base + o for o in layout.byte_offsets[dt]]
                    for i in idx:
                        ptrs += data[i]
                    _native.wreduce_dist_tensors_raw(ptrs, m, layout.split_sizes[dt], layout.byte_offsets[dt],
                                                     weights, None if out is None else out.data_ptr(),
                                                     _native.dtype_code(dt, single_task=True), d2.data_ptr(),
                                                     not first, raw_stream)
                first = False
            if first:
                d2.zero_()
        return outs, d2


def fp32_rounded(weights: Sequence[float]) -> List[float]:
    """Every weight as the Python float of its fp32 rounding: what the fused
    kernel is handed, for fp64 models too (trajectories are then reproducible
    across dtypes)."""
    return [float(np.float32(w)) for w in weights]


def reduce_with_distances(models: List[nn.Module], weights: Sequence[float], device=None,
                          to_host: Optional[bool] = None):
    """(module, d2): the exact weighted reduce of `models` with `weights`
    (rounded to fp32 first), as FedAvg.aggregate computes it, and the float64
    host tensor of every model's squared L2 distance to that result over all
    parameters: d2[i] = sum_e (double(x_i[e]) - double(out[e]))^2, from the
    same pass over the models (dlsim_wreduce_dist). Buffers and
    attributes are copy.deepcopy(models[0])'s; the module lives where models[0]
    lives unless to_host says otherwise. The distances come back with one D2H
    copy of n doubles, which waits for the stream."""
    models[0]  # IndexError for an empty list, as the aggregators
    assert len(weights) == len(models)
    plan = ReduceDistPlan(models, device)
    outs, d2 = plan.run(range(plan.n), fp32_rounded(weights))
    host = d2.cpu()  # waits for the stream: the staged copies' sources may go now
    return plan.module(outs, to_host), host


def reduce_dist_arena_tasks(prepared: List[ArenaTask], index_lists, weight_lists, centers=None,
                            want_out: bool = True):
    """One pass of ReduceDistPlan.run for many tasks at once: pass k runs over the models index_lists[k]
    of prepared[k] (behind centers[k], a dict of flat device arenas per dtype as an earlier pass returned
    it, as input 0 when given) with one weight per input, bit-identical to that call on the same models.
    An ArenaTask may stand in the list several times (the 1-way probes of one task).

    Returns (outs, slots, bufs) without waiting for anything: outs[k] the pass's fresh output arenas
    {dtype: arena} ({} without want_out); slots[k] = (device, offset, length) of its distance vector in
    bufs[device], the one float64 device buffer that holds every vector of that device (device None: the
    models have no parameters, the vector is zeros), so that one D2H copy per device brings them all back
    (vectors_to_host).

    A dtype group with arena views is one segment of dlsim_wreduce_dist_batched, a group read in place
    one segment per non-empty tensor. A model's dtype groups add into its vector in its own layout
    order: the calls go in rounds, round r takes every pass's r-th non-empty group, one call per (dtype,
    device) inside a round, accumulating from round 1 on (distances_arena_tasks). Each device's calls are
    issued with that device current. `prepared` is only read."""
    plans = []  # per pass: (length, device or None, offset, [(dtype, n_tensors, pointers, lengths, offsets, out arena)])
    keep = []
    outs: List[Dict[torch.dtype, torch.Tensor]] = []
    sizes: Dict[torch.device, int] = {}
    for j, task in enumerate(prepared):
        idx = list(index_lists[j])
        center = None if centers is None else centers[j]
        m = len(idx) + (center is not None)
        assert len(weight_lists[j]) == m
        _native.check_reducedist_fan_in(m)
        o: Dict[torch.dtype, torch.Tensor] = {}
        outs.append(o)
        dev, groups = None, []
        layout = task.layout
        for dt, total, vs, in_place, gdev in task.groups():
            out = arena_empty(total, dt, gdev) if want_out else None
            if want_out:
                o[dt] = out
            if total == 0:
                continue
            dev = gdev
            if not in_place:
                ptrs = ([center[dt].data_ptr()] if center is not None else []) + [vs[i].data_ptr() for i in idx]
                groups.append((dt, 1, ptrs, [total], [0], out))
                keep.append(vs)
                continue
            rows, live = task.tensor_rows(dt, vs, gdev, idx)
            esz = _elem_size(dt)
            offs = [layout.offsets[k] * esz for k, _ in live]
            ptrs = [center[dt].data_ptr() + b for b in offs] if center is not None else []
            ptrs += [r[k].data_ptr() for r in rows for k, _ in live]
            groups.append((dt, len(live), ptrs, [s for _, s in live], offs, out))
            keep.append(rows)
        off = None
        if dev is not None:
            off = sizes.get(dev, 0)
            sizes[dev] = off + m
        plans.append((m, dev, off, groups))
    with torch.no_grad():
        bufs = {dev: torch.empty(size, dtype=torch.float64, device=dev) for dev, size in sizes.items()}
        r = 0
        while True:
            # (dtype, device) -> [fan-ins, tensor counts, pointers, lengths, offsets, weights, outputs, vectors]
            calls: Dict[tuple, list] = {}
            for (m, dev, off, groups), ws in zip(plans, weight_lists):
                if r < len(groups):
                    dt, t, ptrs, lens, offs, out = groups[r]
                    c = calls.setdefault((dt, dev), [[], [], [], [], [], [], [], []])
                    c[0].append(m)
                    c[1].append(t)
                    c[2] += ptrs
                    c[3] += lens
                    c[4] += offs
                    c[5] += ws
                    c[6].append(None if out is None else out.data_ptr())
                    c[7].append(bufs[dev].data_ptr() + 8 * off)
            if not calls:
                break
            for (dt, dev), (fan, nts, ptrs, lens, offs, ws, out_ptrs, vecs) in calls.items():
                with torch.cuda.device(dev):  # the launches and the workspace allocation go to the current device
                    _native.wreduce_dist_batched_raw(fan, nts, ptrs, lens, offs, ws, out_ptrs,
                                                     _native.dtype_code(dt, single_task=True), vecs, r > 0,
                                                     torch._C._cuda_getCurrentRawStream(dev.index))
            r += 1
    keep.clear()
    return outs, [(dev, off, m) for m, dev, off, _ in plans], bufs


def vectors_to_host(slots, bufs) -> List[List[float]]:
    """The distance vectors of reduce_dist_arena_tasks as lists of Python floats: one D2H copy per device,
    which waits for that device's stream."""
    hosts = {dev: buf.cpu().tolist() for dev, buf in bufs.items()}
    return [[0.0] * m if dev is None else hosts[dev][off:off + m] for dev, off, m in slots]


def geomed_arena_tasks(prepared: List[ArenaTask], rule, on_launched=None) -> List[nn.Module]:
    """wave_tasks.aggregate_arena_tasks for the geometric median (rule ("GeometricMedian", iters, nu)) and
    centered clipping (("CenteredClip", iters, tau)), each task what GeometricMedian.aggregate /
    CenteredClip.aggregate gives for its models and weights (task.weights: one float per model, None: 1/n
    each), bit for bit: the same host rules (geomed.weiszfeld_weights, clip_weights, _normalised,
    fp32_rounded) on the same distances. The tasks go in lockstep, every pass of every task in the batched
    launches of reduce_dist_arena_tasks, one D2H copy and one synchronisation per device and pass instead
    of one per task and pass:
      1. pass 0 for every task;
      2. the tasks with a non-finite distance get their 1-way probes (weight 1.0, no output) in one call;
      3. those with a partial kept set repeat pass 0 together over the kept models;
      4. iteration t for every task still iterating (a geometric median whose weights come back None
         stops; a task with no finite model keeps FedAvg's arenas). Centered clipping passes the previous
         arenas as input 0 and writes fresh ones. The last iteration's distances are not fetched.
    on_launched fires once the last pass is queued (wave_tasks.finish_modules); `prepared` is consumed as
    in aggregate_arena_tasks. More than 32 models (31 under centered clipping) raise ValueError before
    anything is queued."""
    import math

    from dasklearn_amd.gradient_aggregation import geomed as _geomed
    name, iters, param = rule
    clip = name == "CenteredClip"
    alphas = []
    for task in prepared:
        n = task.fan_in
        if clip and n > _native.MAX_REDUCEDIST_INPUTS - 1:
            raise ValueError(f"CenteredClip takes at most {_native.MAX_REDUCEDIST_INPUTS - 1} models "
                             f"(got {n}): the centre is one more input of the kernel")
        _native.check_reducedist_fan_in(n)
        alphas.append([float(1. / n)] * n if task.weights is None else [float(w) for w in task.weights])
    count = len(prepared)
    everyone = [list(range(len(a))) for a in alphas]
    ws = [fp32_rounded(a) for a in alphas]
    outs, slots, bufs = reduce_dist_arena_tasks(prepared, everyone, ws)
    d2s = vectors_to_host(slots, bufs)
    kept = [list(e) for e in everyone]
    doubt = [j for j in range(count) if not all(math.isfinite(d) for d in d2s[j])]
    if doubt:
        probes = [(j, i) for j in doubt for i in everyone[j]]
        _, pslots, pbufs = reduce_dist_arena_tasks([prepared[j] for j, _ in probes], [[i] for _, i in probes],
                                                   [[1.0]] * len(probes), want_out=False)
        finite = [math.isfinite(v[0]) for v in vectors_to_host(pslots, pbufs)]
        for j in doubt:
            kept[j] = []
        for (j, i), ok in zip(probes, finite):
            if ok:
                kept[j].append(i)
        again = [j for j in doubt if kept[j] and len(kept[j]) != len(everyone[j])]
        if again:
            for j in again:
                ws[j] = fp32_rounded(_geomed._normalised(alphas[j], kept[j]))
            aouts, aslots, abufs = reduce_dist_arena_tasks([prepared[j] for j in again], [kept[j] for j in again],
                                                           [ws[j] for j in again])
            for j, o, d in zip(again, aouts, vectors_to_host(aslots, abufs)):
                outs[j], d2s[j] = o, d
    active = [j for j in range(count) if kept[j]]
    if clip:
        a = {j: _geomed._normalised(alphas[j], kept[j]) for j in active}
    else:
        a = {j: [alphas[j][i] for i in kept[j]] for j in active}
    for t in range(iters):
        if clip:
            w = {j: _geomed.clip_weights(d2s[j], a[j], param) for j in active}
        else:
            w = {j: _geomed.weiszfeld_weights(d2s[j], a[j], param) for j in active}
            active = [j for j in active if w[j] is not None]
        if not active:
            break
        pouts, pslots, pbufs = reduce_dist_arena_tasks([prepared[j] for j in active], [kept[j] for j in active],
                                                       [w[j] for j in active],
                                                       [outs[j] for j in active] if clip else None)
        for j, o in zip(active, pouts):
            outs[j] = o
        if t + 1 < iters:
            for j, d in zip(active, vectors_to_host(pslots, pbufs)):
                d2s[j] = d[1:] if clip else d
    return finish_modules(prepared, outs, on_launched)


def _copy_of_params(model0: nn.Module, layout: ParamLayout, params, views, dev: torch.device,
                    host_out: bool) -> nn.Module:
    """copy.deepcopy(model0) whose parameters hold `params`' values bit for
    bit (a plain copy, not a 1-way reduce: x*0 + 1*x is not the identity for
    Inf and NaN), in one arena per dtype on the host or on `dev`. views[dt]:
    the model's flat arena of that dtype (one copy), or None (one per tensor)."""
    arenas = {}
    with torch.no_grad():
        for dt, idx in layout.groups.items():
            total = layout.totals[dt]
            flat = torch.empty(total, dtype=dt) if host_out else arena_empty(total, dt, dev)
            if views[dt] is not None:
                flat.copy_(views[dt])
            else:
                for k in idx:
                    off = layout.offsets[k]
                    p = params[k]
                    flat[off:off + p.numel()].copy_(p.detach().reshape(-1))
            arenas[dt] = flat
    return _restride(module_from_arenas(model0, layout, arenas), layout)


def krum_modules(models: List[nn.Module], f: int, m: Optional[int], to_host: Optional[bool] = None) -> nn.Module:
    """Krum (m None) or Multi-Krum(m) of `models` with Byzantine count f
    (gradient_aggregation/krum.py has the rule): the distance matrix on the
    GPU (model_distances), the selection on the host, then Krum copies the
    selected model's parameters bit for bit and Multi-Krum runs the selected
    models, in ascending index order, through the exact weighted reduce with
    float(1./m) each, as FedAvg.aggregate(selected) does. Buffers,
    attributes and parameter strides are copy.deepcopy(models[0])'s, also when
    models[0] is not selected; the result lives where models[0] lives unless
    to_host says otherwise.

    The selection needs the matrix on the host: one D2H copy of n*n doubles
    and one stream synchronisation per call."""
    from dasklearn_amd.gradient_aggregation import krum as _krum
    model0 = models[0]  # IndexError for an empty list, as FedAvg
    n = len(models)
    _native.check_pairdist_fan_in(n)
    _krum.check_krum_params(n, f, 1 if m is None else m)
    inputs = ModelInputs(models, _native.MAX_PAIRDIST_INPUTS, "pairwise-distance")
    chosen = _krum.krum_select(_distances(inputs).tolist(), f, 1 if m is None else m)
    host_out = inputs.host_out(to_host)
    if m is None:
        w = chosen[0]
        views = {dt: None if v is None else v[w] for dt, v in inputs.in_views.items()}
        return _copy_of_params(model0, inputs.layout, inputs.all_params[w], views, inputs.dev, host_out)
    params0 = inputs.layout.params
    del inputs  # the staged rows: the reduce below resolves the selected models for itself
    out = aggregate_modules([models[i] for i in chosen], None, _native.DLSIM_EXACT, to_host=host_out)
    if chosen[0] == 0:
        return out
    # the reduce copied the first selected model's buffers, attributes and
    # parameter strides: models[0]'s they must be, around the same values
    memo = {}
    with torch.no_grad():
        for q0, q in zip(params0, module_params(out)):
            q.requires_grad_(q0.requires_grad)
            if q.stride() != q0.stride() and not (q.is_contiguous() and q0.is_contiguous()):
                fresh = torch.empty_like(q0, memory_format=torch.preserve_format, device=q.device)
                fresh.copy_(q.detach())
                q.data = fresh  # leaves the result arena, as _restride's parameters do
            memo[id(q0)] = q
    res = _clone_module(model0, memo)
    entry = _arena_entry(out)
    if entry is not None:
        _register_arenas(res, entry)
    return res
