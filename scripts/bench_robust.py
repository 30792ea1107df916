"""The order-statistic reduce (coordinate median, trimmed mean:
dlsim_robust_reduce) on the MI355X, against the weighted reduce that moves the
same bytes (for DESIGN.md §8j).

  kernel   dlsim_robust_reduce on flat device rows: fp32 at 11,181,642 elements
           (ResNet-18) with n = 4, 8, 16, 32 (one sorting-network capacity
           each), bf16 at 125,000,000 with n = 2 and 8; the median window and
           the trim-1 window. HIP events over windows of 200 back-to-back
           launches after a warm-up; inputs AND outputs rotate over >= 1 GiB
           each (none stays in the 256 MiB Infinity Cache), a
           decoy set is read first (§5f); the median window of time, with the
           fastest and slowest. Algorithmic bytes (n + 1) * P * s per launch.
  yard     the yardstick: dlsim_wreduce, exact mode, the same n, P and dtype,
           the same buffers and rotation, in the same process, run before and
           after to show its own run-to-run spread

  batch    (--batch, instead of the above) the batched entries
           against the paths that were there before them, each leg in this one
           process, the same rotation and decoy rule, a "launch" being one whole
           call: (a) 100 tasks of n = 8 GNLeNet-sized fp32 rows: one
           dlsim_robust_reduce_batched call against 100 dlsim_robust_reduce
           calls, and against dlsim_wreduce_batched on the same buffers;
           (b) n = 8 models in ResNet-18's 62 separate tensors:
           dlsim_robust_reduce_tensors_batched against
           dlsim_robust_reduce_tensors; (c) one RoundExecutor round of 100
           GNLeNet peers with MEDIAN against the same tasks one by one through
           functions.aggregate with aggregate_on_device (wall time, stream
           synchronised); (d) one fp32 task of 11,181,642 elements, n = 8,
           through the batched entry against the flat entry.

  nearest  (--nearest, instead of the above) the mean around the
           median, dlsim_robust_nearest_reduce with keep = n - 2, against
           dlsim_robust_reduce with the rank window [1, n-1) of the same kept
           count: the same buffers, rotation and decoy rule in this one
           process, the yardstick before and after; fp32 at 11,181,642
           elements with n = 4, 8, 16, 32 and bf16 at 125,000,000 with n = 8.

    python scripts/bench_robust.py [--windows 5] [--launches 200] [--skip-bf16]
    python scripts/bench_robust.py --batch [--windows 5] [--legs abcd]
    python scripts/bench_robust.py --nearest [--windows 5] [--launches 200] [--skip-bf16]
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dasklearn_amd import _native  # noqa: E402
from dasklearn_amd.arena import aligned_empty, arena_empty, base_align, row_stride  # noqa: E402


class RobustPlan:
    """One prepared dlsim_robust_reduce call (pointers resolved once, as ReducePlan)."""

    def __init__(self, inputs, lo, hi, out):
        n = len(inputs)
        self._keep = (list(inputs), out)
        self.args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs]), n, lo, hi, ctypes.c_void_p(out.data_ptr()),
                     out.numel(), _native.dtype_code(out.dtype, single_task=True))
        self.lib = _native.load()
        self.device = out.device

    def launch(self, stream=None):
        rc = self.lib.dlsim_robust_reduce(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_robust_reduce", rc)


def windows(plans, launches, nwin):
    """Mean us per launch of nwin windows of back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for pl in plans:  # warm-up: every set once
        pl.launch()
    torch.cuda.synchronize()
    out = []
    k = 0
    for _ in range(nwin):
        e0.record()
        for _ in range(launches):
            plans[k % len(plans)].launch()
            k += 1
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return sorted(out)


def kernel_lines(P, tdt, n, launches, nwin):
    dev = torch.device("cuda", 0)
    esz = torch.empty((), dtype=tdt).element_size()
    byts = (n + 1) * P * esz
    sets = max(3, -(-(1 << 30) // (n * P * esz)))
    out_sets = -(-max(sets, -(-(1 << 30) // (P * esz))) // sets) * sets
    stride = row_stride(P, esz)
    # + 1: the decoy set, read first and never timed
    rows = aligned_empty((sets + 1) * n * stride, tdt, dev, base_align(P * esz, esz)).view(sets + 1, n, stride)
    g = torch.Generator(device=dev).manual_seed(0)
    for s in range(sets + 1):
        for i in range(n):
            rows[s, i, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.05).to(tdt))
    outs = [arena_empty(P, tdt, dev) for _ in range(out_sets + 1)]
    w = np.full(n, 1.0 / n, dtype=np.float32)
    ins = [[rows[s, i, :P] for i in range(n)] for s in range(sets + 1)]
    med = ((n - 1) // 2, (n - 1) // 2 + 1)
    legs = [("yard_1", None), ("median", med)]
    if n - 2 >= 1:
        legs.append(("trim_1", (1, n - 1)))
    legs.append(("yard_2", None))
    decoy = RobustPlan(ins[sets], *med, outs[out_sets])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"params": P, "dtype": str(tdt).replace("torch.", ""), "n": n, "bytes": byts, "rotating_sets": sets,
            "rotating_outputs": out_sets, "launches_per_window": launches, "windows": nwin}
    res = {}
    for key, win in legs:
        if win is None:
            plans = [_native.ReducePlan(ins[j % sets], w, outs[j], _native.DLSIM_EXACT) for j in range(out_sets)]
        else:
            plans = [RobustPlan(ins[j % sets], *win, outs[j]) for j in range(out_sets)]
        ws = windows(plans, launches, nwin)
        res[key] = ws[len(ws) // 2]
        line = dict(base, leg=key, median_us=round(ws[len(ws) // 2], 3), min_us=round(ws[0], 3),
                    max_us=round(ws[-1], 3), GBps=round(byts / ws[len(ws) // 2] / 1e3, 1),
                    kernel=_native.kernel_name(n, P, tdt) if win is None else
                    "dlsim::k_robust_halves" if n > 16 else "dlsim::k_robust_tiles")
        if win is not None:
            line["window"] = list(win)
        print(json.dumps(line), flush=True)
    yard_us = (res["yard_1"] + res["yard_2"]) / 2
    ratio = dict(base, leg="ratio", median_over_yard=round(res["median"] / yard_us, 4),
                 yard_spread=round(abs(res["yard_1"] - res["yard_2"]) / yard_us, 4))
    if "trim_1" in res:
        ratio["trim_1_over_yard"] = round(res["trim_1"] / yard_us, 4)
    print(json.dumps(ratio), flush=True)


# ---- the mean around the median (--nearest) ------------------------------------------------
def nearest_plan(inputs, keep, out):
    n = len(inputs)
    args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs]), n, keep, ctypes.c_void_p(out.data_ptr()), out.numel(),
            _native.dtype_code(out.dtype, single_task=True))
    return Call("dlsim_robust_nearest_reduce", args, out.device, (list(inputs), out))


def nearest_lines(P, tdt, n, launches, nwin):
    """dlsim_robust_nearest_reduce with keep = n - 2 against its yardstick, dlsim_robust_reduce with the rank window
    of the same kept count ([1, n-1)): the same loads, sort, adds and stores, so the ratio is the price of the
    distances, the window choice and the predicated sum. kernel_lines' buffers, rotation and decoy rule."""
    dev = torch.device("cuda", 0)
    esz = torch.empty((), dtype=tdt).element_size()
    byts = (n + 1) * P * esz
    sets = max(3, -(-(1 << 30) // (n * P * esz)))
    out_sets = -(-max(sets, -(-(1 << 30) // (P * esz))) // sets) * sets
    stride = row_stride(P, esz)
    rows = aligned_empty((sets + 1) * n * stride, tdt, dev, base_align(P * esz, esz)).view(sets + 1, n, stride)
    g = torch.Generator(device=dev).manual_seed(0)
    for s in range(sets + 1):
        for i in range(n):
            rows[s, i, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.05).to(tdt))
    outs = [arena_empty(P, tdt, dev) for _ in range(out_sets + 1)]
    ins = [[rows[s, i, :P] for i in range(n)] for s in range(sets + 1)]
    keep, win = n - 2, (1, n - 1)
    decoy = nearest_plan(ins[sets], keep, outs[out_sets])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "robust_nearest", "params": P, "dtype": str(tdt).replace("torch.", ""), "n": n, "keep": keep,
            "bytes": byts, "rotating_sets": sets, "rotating_outputs": out_sets, "launches_per_window": launches,
            "windows": nwin}
    shape = "halves" if n > 16 else "tiles"
    res, yards = {}, []
    for leg in ("rank_1", "nearest", "rank_2"):
        if leg == "nearest":
            plans = [nearest_plan(ins[j % sets], keep, outs[j]) for j in range(out_sets)]
        else:
            plans = [RobustPlan(ins[j % sets], *win, outs[j]) for j in range(out_sets)]
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, GBps=round(byts / ws[len(ws) // 2] / 1e3, 1),
                          kernel=f"dlsim::k_nearest_{shape}" if leg == "nearest" else f"dlsim::k_robust_{shape}")
        if leg != "nearest":
            yards.append(res[leg])
    res["rank"] = sum(yards) / 2
    ratio_line(base, "ratio", res, "nearest", "rank", yards)


# ---- the batched entries (--batch) ---------------------------------------------------------
GNLENET_SHAPES = [(32, 3, 5, 5), (32,), (32,), (32,), (32, 32, 5, 5), (32,), (32,), (32,),
                  (64, 32, 5, 5), (64,), (64,), (64,), (10, 576), (10,)]
GNLENET_P = 85_354
RESNET18_P = 11_181_642


def resnet18_numels():
    """Element counts of torchvision resnet18(num_classes=10)'s 62 parameters."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    cin = 64
    for cout, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        for b in range(2):
            shapes += [(cout, cin, 3, 3), (cout,), (cout,), (cout, cout, 3, 3), (cout,), (cout,)]
            if b == 0 and (stride != 1 or cin != cout):
                shapes += [(cout, cin, 1, 1), (cout,), (cout,)]
            cin = cout
    return [int(np.prod(sh)) for sh in shapes + [(10, 512), (10,)]]


class Call:
    """One prepared library call (arguments resolved once); `keep` holds the tensors."""

    def __init__(self, symbol, args, device, keep):
        self.fn, self.symbol, self.args, self.device, self.keep = getattr(_native.load(), symbol), symbol, args, device, keep

    def launch(self, stream=None):
        rc = self.fn(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check(self.symbol, rc)


class Seq:
    def __init__(self, plans):
        self.plans = plans

    def launch(self, stream=None):
        for pl in self.plans:
            pl.launch(stream)


def batched_call(tasks, lo, hi):
    """dlsim_robust_reduce_batched over tasks = [(inputs, out)], one window for all."""
    b = len(tasks)
    fan = (ctypes.c_int * b)(*[len(ins) for ins, _ in tasks])
    ptrs = [t.data_ptr() for ins, _ in tasks for t in ins]
    out = tasks[0][1]
    args = (b, fan, (ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_int * b)(*[lo] * b), (ctypes.c_int * b)(*[hi] * b),
            (ctypes.c_void_p * b)(*[o.data_ptr() for _, o in tasks]), (ctypes.c_size_t * b)(*[o.numel() for _, o in tasks]),
            _native.dtype_code(out.dtype, single_task=True))
    return Call("dlsim_robust_reduce_batched", args, out.device, tasks)


def wreduce_batched_call(tasks):
    """The yardstick of leg (a): dlsim_wreduce_batched, exact, uniform weights, the same buffers."""
    b = len(tasks)
    fan = (ctypes.c_int * b)(*[len(ins) for ins, _ in tasks])
    ptrs = [t.data_ptr() for ins, _ in tasks for t in ins]
    w = np.concatenate([np.full(len(ins), 1.0 / len(ins), dtype=np.float32) for ins, _ in tasks])
    out = tasks[0][1]
    args = (b, fan, (ctypes.c_void_p * len(ptrs))(*ptrs), w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            (ctypes.c_void_p * b)(*[o.data_ptr() for _, o in tasks]), (ctypes.c_size_t * b)(*[o.numel() for _, o in tasks]),
            _native.dtype_code(out.dtype), _native.DLSIM_EXACT)
    return Call("dlsim_wreduce_batched", args, out.device, (tasks, w))


def tensors_call(symbol, models, numels, offs_bytes, lo, hi, out):
    """dlsim_robust_reduce_tensors[_batched]: models = [[tensor per parameter] per model]."""
    n, t = len(models), len(numels)
    ptrs = [x.data_ptr() for m in models for x in m]
    args = ((ctypes.c_void_p * len(ptrs))(*ptrs), n, t, (ctypes.c_size_t * t)(*numels), (ctypes.c_size_t * t)(*offs_bytes),
            lo, hi, ctypes.c_void_p(out.data_ptr()), _native.dtype_code(out.dtype, single_task=True))
    return Call(symbol, args, out.device, (models, out))


def report(base, leg, ws, **extra):
    print(json.dumps(dict(base, leg=leg, median_us=round(ws[len(ws) // 2], 3), min_us=round(ws[0], 3),
                          max_us=round(ws[-1], 3), **extra)), flush=True)
    return ws[len(ws) // 2]


def filled(count, P, tdt, dev, seed):
    """count rows of P elements at the arena row stride, normal * 0.05."""
    esz = torch.empty((), dtype=tdt).element_size()
    stride = row_stride(P, esz)
    rows = aligned_empty(count * stride, tdt, dev, base_align(P * esz, esz)).view(count, stride)
    g = torch.Generator(device=dev).manual_seed(seed)
    for i in range(count):
        rows[i, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.05).to(tdt))
    return [rows[i, :P] for i in range(count)]


def ratio_line(base, leg, res, num, den, yards):
    spread = (max(yards) - min(yards)) / (sum(yards) / len(yards))
    print(json.dumps(dict(base, leg=leg, **{f"{num}_over_{den}": round(res[num] / res[den], 4)},
                          yardstick_spread=round(spread, 4))), flush=True)


def leg_a(nwin, launches):
    """100 tasks x n = 8 x GNLeNet-sized fp32 rows (a 100-peer round, every peer reading 8 of the 100 models)."""
    dev, b, n, P = torch.device("cuda", 0), 100, 8, GNLENET_P
    sets = -(-(1 << 30) // (b * P * 4)) + 1  # >= 1 GiB of distinct inputs, + the decoy
    out_sets = -(-(1 << 30) // (b * P * 4))
    out_sets = -(-out_sets // (sets - 1)) * (sets - 1)
    models = [filled(b, P, torch.float32, dev, s) for s in range(sets)]
    outs = [[arena_empty(P, torch.float32, dev) for _ in range(b)] for _ in range(out_sets + 1)]
    med = ((n - 1) // 2, (n - 1) // 2 + 1)

    def tasks(s, j):
        return [([models[s][(p + d) % b] for d in range(n)], outs[j][p]) for p in range(b)]
    decoy = batched_call(tasks(sets - 1, out_sets), *med)
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "robust_batch", "case": "a", "tasks": b, "n": n, "params": P, "dtype": "float32", "window": list(med),
            "bytes": (n + 1) * P * 4 * b, "rotating_sets": sets - 1, "rotating_outputs": out_sets,
            "calls_per_window": launches, "windows": nwin}
    res, yards = {}, []
    for leg in ("per_task_1", "batched", "wreduce_batched", "per_task_2"):
        plans = []
        for j in range(out_sets):
            tk = tasks(j % (sets - 1), j)
            if leg == "batched":
                plans.append(batched_call(tk, *med))
            elif leg == "wreduce_batched":
                plans.append(wreduce_batched_call(tk))
            else:
                plans.append(Seq([RobustPlan(ins, *med, out) for ins, out in tk]))
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, us_per_task=round(ws[len(ws) // 2] / b, 3),
                          GBps=round(base["bytes"] / ws[len(ws) // 2] / 1e3, 1))
        if leg.startswith("per_task"):
            yards.append(res[leg])
    res["per_task"] = sum(yards) / 2
    ratio_line(base, "ratio", res, "batched", "per_task", yards)
    ratio_line(base, "ratio_fedavg", res, "batched", "wreduce_batched", yards)


def leg_b(nwin, launches):
    """n = 8 models whose parameters are ResNet-18's 62 separate tensors, into one output arena."""
    dev, n, numels = torch.device("cuda", 0), 8, resnet18_numels()
    P = sum(numels)
    assert P == RESNET18_P and len(numels) == 62
    offs = [int(o) * 4 for o in np.concatenate([[0], np.cumsum(numels)])[:-1]]  # an arena's byte offsets
    sets = max(3, -(-(1 << 30) // (n * P * 4))) + 1
    out_sets = -(-(-(-(1 << 30) // (P * 4))) // (sets - 1)) * (sets - 1)
    g = torch.Generator(device=dev).manual_seed(1)
    # every tensor its own allocation, as a device model's parameters are
    models = [[[(torch.randn(k, generator=g, device=dev) * 0.05) for k in numels] for _ in range(n)] for _ in range(sets)]
    outs = [arena_empty(P, torch.float32, dev) for _ in range(out_sets + 1)]
    med = (3, 4)
    decoy = tensors_call("dlsim_robust_reduce_tensors_batched", models[sets - 1], numels, offs, *med, outs[out_sets])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "robust_batch", "case": "b", "tensors": len(numels), "n": n, "params": P, "dtype": "float32",
            "window": list(med), "bytes": (n + 1) * P * 4, "rotating_sets": sets - 1, "rotating_outputs": out_sets,
            "calls_per_window": launches, "windows": nwin}
    res, yards = {}, []
    for leg, symbol in (("per_tensor_1", "dlsim_robust_reduce_tensors"), ("batched", "dlsim_robust_reduce_tensors_batched"),
                        ("per_tensor_2", "dlsim_robust_reduce_tensors")):
        plans = [tensors_call(symbol, models[j % (sets - 1)], numels, offs, *med, outs[j]) for j in range(out_sets)]
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, GBps=round(base["bytes"] / ws[len(ws) // 2] / 1e3, 1))
        if leg.startswith("per_tensor"):
            yards.append(res[leg])
    res["per_tensor"] = sum(yards) / 2
    ratio_line(base, "ratio", res, "batched", "per_tensor", yards)


def leg_c(nwin):
    """One round of 100 GNLeNet peers, every peer the median of 8 device arenas: RoundExecutor against the same
    tasks one by one through functions.aggregate (aggregate_on_device). Wall time of the round, stream synchronised."""
    import time
    import types

    from torch import nn

    from dasklearn_amd import arena, functions
    from dasklearn_amd.gradient_aggregation import GradientAggregationMethod
    from dasklearn_amd.rounds import RoundExecutor

    class Shaped(nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = nn.ParameterList([nn.Parameter(torch.randn(*sh) * 0.05) for sh in GNLENET_SHAPES])
    peers, n = 100, 8
    torch.manual_seed(0)
    pool = [arena.to_device_arena(Shaped(), "cuda") for _ in range(peers)]
    settings = types.SimpleNamespace(gradient_aggregation=GradientAggregationMethod.MEDIAN, aggregate_on_device=True)
    tasks = [(f"agg_{p}", "aggregate", {"models": [(f"m_{(p + d) % peers}", 0) for d in range(n)], "round": 1, "peer": p})
             for p in range(peers)]

    def executor():
        ex = RoundExecutor({}, settings, keep_all=True)
        return ex.run(tasks, seed={f"m_{p}": [pool[p]] for p in range(peers)})

    def per_task():
        return [functions.aggregate(settings, {"models": [pool[(p + d) % peers] for d in range(n)], "round": 1, "peer": p})
                for p in range(peers)]
    base = {"bench": "robust_batch", "case": "c", "peers": peers, "n": n, "params": GNLENET_P, "dtype": "float32",
            "method": "MEDIAN", "timing": "wall, synchronised", "reps": nwin}
    res, yards = {}, []
    for leg, fn in (("per_task_1", per_task), ("executor", executor), ("per_task_2", per_task)):
        fn()
        torch.cuda.synchronize()
        ws = []
        for _ in range(nwin):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ws.append((time.perf_counter() - t0) * 1e6)
        ws.sort()
        res[leg] = report(base, leg, ws, us_per_task=round(ws[len(ws) // 2] / peers, 2))
        if leg.startswith("per_task"):
            yards.append(res[leg])
    res["per_task"] = sum(yards) / 2
    ratio_line(base, "ratio", res, "executor", "per_task", yards)


def leg_d(nwin, launches):
    """One fp32 task of 11,181,642 elements, n = 8, alone in a batched call: what the run-time fan-in and the
    descriptor lookup cost against the flat entry."""
    dev, n, P = torch.device("cuda", 0), 8, RESNET18_P
    sets = max(3, -(-(1 << 30) // (n * P * 4))) + 1
    out_sets = -(-(-(-(1 << 30) // (P * 4))) // (sets - 1)) * (sets - 1)
    ins = [filled(n, P, torch.float32, dev, s) for s in range(sets)]
    outs = [arena_empty(P, torch.float32, dev) for _ in range(out_sets + 1)]
    med = (3, 4)
    decoy = RobustPlan(ins[sets - 1], *med, outs[out_sets])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "robust_batch", "case": "d", "tasks": 1, "n": n, "params": P, "dtype": "float32", "window": list(med),
            "bytes": (n + 1) * P * 4, "rotating_sets": sets - 1, "rotating_outputs": out_sets,
            "calls_per_window": launches, "windows": nwin}
    res, yards = {}, []
    for leg in ("flat_1", "batched", "flat_2"):
        plans = [batched_call([(ins[j % (sets - 1)], outs[j])], *med) if leg == "batched" else
                 RobustPlan(ins[j % (sets - 1)], *med, outs[j]) for j in range(out_sets)]
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, GBps=round(base["bytes"] / ws[len(ws) // 2] / 1e3, 1))
        if leg.startswith("flat"):
            yards.append(res[leg])
    res["flat"] = sum(yards) / 2
    ratio_line(base, "ratio", res, "batched", "flat", yards)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-bf16", action="store_true")
    ap.add_argument("--batch", action="store_true", help="the batched entries' legs (a)-(d) instead of the flat kernel's")
    ap.add_argument("--legs", default="abcd", help="with --batch: which of the legs a, b, c, d")
    ap.add_argument("--nearest", action="store_true",
                    help="dlsim_robust_nearest_reduce against dlsim_robust_reduce instead of the flat kernel's legs")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust.py measures on a GPU; none is visible")
    if a.nearest:
        for n in (4, 8, 16, 32):
            nearest_lines(RESNET18_P, torch.float32, n, a.launches, a.windows)
            torch.cuda.empty_cache()
        if not a.skip_bf16:
            nearest_lines(125_000_000, torch.bfloat16, 8, a.launches, a.windows)
        return
    if a.batch:
        for leg in a.legs:
            {"a": lambda: leg_a(a.windows, 20), "b": lambda: leg_b(a.windows, 40), "c": lambda: leg_c(a.windows),
             "d": lambda: leg_d(a.windows, a.launches)}[leg]()
            torch.cuda.empty_cache()
        return
    for n in (4, 8, 16, 32):
        kernel_lines(11_181_642, torch.float32, n, a.launches, a.windows)
        torch.cuda.empty_cache()
    if not a.skip_bf16:
        for n in (2, 8):
            kernel_lines(125_000_000, torch.bfloat16, n, a.launches, a.windows)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
