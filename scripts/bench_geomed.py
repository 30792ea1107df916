"""The fused reduce-and-measure kernel (dlsim_wreduce_dist, under the geometric
median and centered clipping) on the MI355X, against the two things that exist
without it (for DESIGN.md §8l).

  fused    dlsim_wreduce_dist on flat device rows: fp32 at 11,181,642 elements
           (ResNet-18) with n = 4, 8, 16, 32, bf16 at 125,000,000 with n = 8.
           HIP events over windows of 200 back-to-back calls (each the fused
           kernel and its small finish kernel) after a warm-up; the inputs and
           outputs rotate over >= 1 GiB (none stays in the 256 MiB Infinity
           Cache), a decoy set is read first (§5f); the median
           window of time, with the fastest and slowest. Algorithmic bytes
           (n + 1) * P * s per call (every row read once, the output written).
  yard     yardstick (a): dlsim_wreduce, exact mode, the same n, P and dtype on
           the same rows with the same rotation, in the same process, run
           before and after to show its own run-to-run spread. The same bytes.
  unfused  yardstick (b), the alternative that exists today: that reduce, then
           dlsim_pairwise_sqdist over the n inputs plus the output (n + 1 <= 32).
  plugin   one GeometricMedian (T = 3) and one CenteredClip (L = 3) aggregate
           on eight ResNet-18-shaped device-arena models next to FedAvg and
           Krum on the same models (wall clock, synchronised, median of 20).

  batch    (--batch, instead of the above) the batched entry
           dlsim_wreduce_dist_batched and the lockstep route on top of it, every
           leg against the path that was there before, in the same process on
           the same buffers, the older path measured before and after:
           (a) 100 GNLeNet-sized fp32 tasks of n = 8: one batched call against
               100 dlsim_wreduce_dist calls;
           (b) two tasks of eight ResNet-18-shaped models in 62 tensors: one
               batched call against two dlsim_wreduce_dist_tensors calls (a call
               of one task is forwarded to that entry, so one task would
               measure it against itself);
           (c) a 100-peer round under GEOMETRIC_MEDIAN and CENTERED_CLIP
               through RoundExecutor against the tasks one by one through
               functions.aggregate (wall clock, synchronised);
           (d) one large task (11,181,642 fp32, n = 8) inside the batched
               kernel, beside a one-element task that keeps the call from being
               forwarded, against the flat entry on both; then two large tasks
               against two flat calls;
           (e) the flat entry's fused legs at n = 4, 8, 16, 32, to set beside
               profiles/geomed/bench_geomed_lines.json.

    python scripts/bench_geomed.py [--windows 5] [--launches 200] [--skip-bf16] [--out FILE]
    python scripts/bench_geomed.py --batch [--windows 7] [--launches N] [--legs abcde] [--out FILE]
One JSON line per measurement (also written to --out).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from dasklearn_amd import _native, arena  # noqa: E402
from dasklearn_amd.arena import aligned_empty, arena_empty, base_align, row_stride  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Krum  # noqa: E402

LINES = []


def emit(line):
    LINES.append(line)
    print(json.dumps(line), flush=True)


class FusedPlan:
    """One prepared dlsim_wreduce_dist call (pointers resolved once, as ReducePlan)."""

    def __init__(self, inputs, w, out, d2):
        n = len(inputs)
        self._keep = (list(inputs), out, d2)
        self.args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs]), n, (ctypes.c_double * n)(*[float(v) for v in w]),
                     ctypes.c_void_p(out.data_ptr()), inputs[0].numel(),
                     _native.dtype_code(inputs[0].dtype, single_task=True), ctypes.c_void_p(d2.data_ptr()), 0)
        self.lib = _native.load()
        self.device = d2.device

    def launch(self, stream=None):
        rc = self.lib.dlsim_wreduce_dist(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_wreduce_dist", rc)


class UnfusedPlan:
    """The exact reduce, then dlsim_pairwise_sqdist over the inputs and the output."""

    def __init__(self, inputs, w, out, d2):
        n = len(inputs) + 1
        self.reduce = _native.ReducePlan(inputs, w, out, _native.DLSIM_EXACT)
        self._keep = (list(inputs), out, d2)
        self.args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in list(inputs) + [out]]), n, out.numel(),
                     _native.dtype_code(out.dtype, single_task=True), ctypes.c_void_p(d2.data_ptr()), 0)
        self.lib = _native.load()
        self.device = d2.device

    def launch(self, stream=None):
        self.reduce.launch(stream)
        rc = self.lib.dlsim_pairwise_sqdist(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_pairwise_sqdist", rc)


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
    d2s = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(out_sets + 1)]
    d2m = [torch.empty((n + 1) * (n + 1), dtype=torch.float64, device=dev) for _ in range(out_sets + 1)]
    w = np.full(n, 1.0 / n, dtype=np.float32)
    ins = [[rows[s, i, :P] for i in range(n)] for s in range(sets + 1)]
    decoy = FusedPlan(ins[sets], w, outs[out_sets], d2s[out_sets])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    tile, blocks = _native.reducedist_geometry(n, tdt, P)
    base = {"params": P, "dtype": str(tdt).replace("torch.", ""), "n": n, "bytes": byts, "rotating_sets": sets,
            "output_sets": out_sets, "launches_per_window": launches, "windows": nwin}
    legs = ("yard_1", "fused", "unfused", "fused_again", "yard_2") if n + 1 <= 32 else ("yard_1", "fused", "fused_again", "yard_2")
    res = {}
    for key in legs:
        if key.startswith("fused"):
            plans = [FusedPlan(ins[j % sets], w, outs[j], d2s[j]) for j in range(out_sets)]
            kernel = "dlsim::k_reducedist + dlsim::k_reducedist_finish"
        elif key == "unfused":
            plans = [UnfusedPlan(ins[j % sets], w, outs[j], d2m[j]) for j in range(out_sets)]
            kernel = _native.kernel_name(n, P, tdt) + " + dlsim::k_pairdist + dlsim::k_pairdist_finish"
        else:
            plans = [_native.ReducePlan(ins[j % sets], w, outs[j], _native.DLSIM_EXACT) for j in range(out_sets)]
            kernel = _native.kernel_name(n, P, tdt)
        ws = windows(plans, launches, nwin)
        res[key] = ws[len(ws) // 2]
        line = dict(base, leg=key, median_us=round(ws[len(ws) // 2], 3), min_us=round(ws[0], 3),
                    max_us=round(ws[-1], 3), algorithmic_bytes=byts, GBps=round(byts / ws[len(ws) // 2] / 1e3, 1),
                    kernel=kernel)
        if key.startswith("fused"):
            line.update(tile_elems=tile, blocks=blocks)
        emit(line)
    yard_us = (res["yard_1"] + res["yard_2"]) / 2
    fused_us = (res["fused"] + res["fused_again"]) / 2
    ratio = dict(base, leg="ratio", fused_over_yard=round(fused_us / yard_us, 4),
                 yard_spread=round(abs(res["yard_1"] - res["yard_2"]) / yard_us, 4),
                 fused_spread=round(abs(res["fused"] - res["fused_again"]) / fused_us, 4))
    if "unfused" in res:
        ratio.update(fused_over_unfused=round(fused_us / res["unfused"], 4),
                     unfused_over_yard=round(res["unfused"] / yard_us, 4))
    emit(ratio)


def plugin_lines(reps=20):
    sys.path.insert(0, ROOT)
    from bench import resnet18_shapes
    dev = torch.device("cuda", 0)
    shapes = resnet18_shapes()

    class Shaped(nn.Module):
        def __init__(self, seed):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.ps = nn.ParameterList([nn.Parameter(torch.randn(sh, generator=g) * 0.05) for sh in shapes])

    n = 8
    models = [arena.to_device_arena(Shaped(100 + i), dev) for i in range(n)]
    for name, agg in (("FedAvg", FedAvg), ("Krum(f=2)", Krum.with_params(2)),
                      ("GeometricMedian(T=3)", GeometricMedian.with_params(3)),
                      ("CenteredClip(L=3)", CenteredClip.with_params(None, 3)), ("FedAvg_again", FedAvg)):
        ts = []
        for k in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = agg.aggregate(models)
            torch.cuda.synchronize()
            if k >= 3:
                ts.append((time.perf_counter() - t0) * 1e6)
            del out
        ts.sort()
        emit({"leg": "plugin", "aggregator": name, "models": n, "params": sum(int(np.prod(s)) for s in shapes),
              "where": "device arenas", "median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1),
              "max_us": round(ts[-1], 1), "reps": reps})


# ---- the batched entry --------------------------------------------------
GNLENET_SHAPES = [(32, 3, 5, 5), (32,), (32,), (32,), (32, 32, 5, 5), (32,), (32,), (32,),
                  (64, 32, 5, 5), (64,), (64,), (64,), (10, 576), (10,)]
GNLENET_P = 85_354
RESNET18_P = 11_181_642


class Seq:
    def __init__(self, plans):
        self.plans = plans

    def launch(self, stream=None):
        for pl in self.plans:
            pl.launch(stream)


class TensorsPlan:
    """One prepared dlsim_wreduce_dist_tensors call: n flat rows read as the tensors of `sizes`."""

    def __init__(self, inputs, w, out, d2, sizes):
        n, t = len(inputs), len(sizes)
        esz = out.element_size()
        offs = [int(o) * esz for o in np.concatenate([[0], np.cumsum(sizes)])[:-1]]
        self._keep = (list(inputs), out, d2)
        self.args = ((ctypes.c_void_p * (n * t))(*[x.data_ptr() + o for x in inputs for o in offs]), n, t,
                     (ctypes.c_size_t * t)(*sizes), (ctypes.c_size_t * t)(*offs),
                     (ctypes.c_double * n)(*[float(v) for v in w]), ctypes.c_void_p(out.data_ptr()),
                     _native.dtype_code(out.dtype, single_task=True), ctypes.c_void_p(d2.data_ptr()), 0)
        self.lib = _native.load()
        self.device = d2.device

    def launch(self, stream=None):
        rc = self.lib.dlsim_wreduce_dist_tensors(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_wreduce_dist_tensors", rc)


class BatchedPlan:
    """One prepared dlsim_wreduce_dist_batched call over tasks = [(inputs, w, out, d2)], every task's rows
    read as the tensors of `sizes` (default: one tensor per model)."""

    def __init__(self, tasks, sizes=None):
        b = len(tasks)
        esz = tasks[0][2].element_size()
        ptrs, lens, offs, ws = [], [], [], []
        for ins, w, out, _ in tasks:
            sz = sizes or [ins[0].numel()]
            o = [int(v) * esz for v in np.concatenate([[0], np.cumsum(sz)])[:-1]]
            ptrs += [x.data_ptr() + v for x in ins for v in o]
            lens += sz
            offs += o
            ws += [float(v) for v in w]
        self._keep = tasks
        self.args = (b, (ctypes.c_int * b)(*[len(t[0]) for t in tasks]),
                     (ctypes.c_int * b)(*[len(sizes) if sizes else 1] * b), (ctypes.c_void_p * len(ptrs))(*ptrs),
                     (ctypes.c_size_t * len(lens))(*lens), (ctypes.c_size_t * len(offs))(*offs),
                     (ctypes.c_double * len(ws))(*ws), (ctypes.c_void_p * b)(*[t[2].data_ptr() for t in tasks]),
                     _native.dtype_code(tasks[0][2].dtype, single_task=True),
                     (ctypes.c_void_p * b)(*[t[3].data_ptr() for t in tasks]), 0)
        self.lib = _native.load()
        self.device = tasks[0][3].device

    def launch(self, stream=None):
        rc = self.lib.dlsim_wreduce_dist_batched(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_wreduce_dist_batched", rc)


def filled(count, P, tdt, dev, seed):
    """count rows of P elements at the arena row stride, normal * 0.05."""
    esz = torch.empty((), dtype=tdt).element_size()
    stride = row_stride(P, esz)
    rows = aligned_empty(count * stride, tdt, dev, base_align(P * esz, esz)).view(count, stride)
    g = torch.Generator(device=dev).manual_seed(seed)
    for i in range(count):
        rows[i, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.05).to(tdt))
    return [rows[i, :P] for i in range(count)]


def report(base, leg, ws, **extra):
    emit(dict(base, leg=leg, median_us=round(ws[len(ws) // 2], 3), min_us=round(ws[0], 3), max_us=round(ws[-1], 3),
              **extra))
    return ws[len(ws) // 2]


def ratio_line(base, res, num, den, yards):
    spread = (max(yards) - min(yards)) / (sum(yards) / len(yards))
    emit(dict(base, leg="ratio", **{f"{num}_over_{den}": round(res[num] / res[den], 4)},
              yardstick_spread=round(spread, 4)))


def three_legs(base, old, make_old, make_new, sets, launches, nwin):
    """The older path, the batched call, the older path again over `sets` rotating plan sets."""
    res, yards = {}, []
    for leg in (old + "_1", "batched", old + "_2"):
        plans = [make_new(j) if leg == "batched" else make_old(j) for j in range(sets)]
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, GBps=round(base["bytes"] / ws[len(ws) // 2] / 1e3, 1))
        if leg != "batched":
            yards.append(res[leg])
    res[old] = sum(yards) / 2
    ratio_line(base, res, "batched", old, yards)


def batch_leg_a(nwin, launches):
    """100 tasks of n = 8 GNLeNet-sized fp32 rows (a 100-peer round, every peer reading 8 of the 100 models):
    one batched call against 100 dlsim_wreduce_dist calls."""
    dev, b, n, P = torch.device("cuda", 0), 100, 8, GNLENET_P
    sets = -(-(1 << 30) // (b * P * 4)) + 1  # >= 1 GiB of distinct inputs, + the decoy
    models = [filled(b, P, torch.float32, dev, s) for s in range(sets)]
    outs = [filled(b, P, torch.float32, dev, 1000 + s) for s in range(sets)]
    d2s = [[torch.empty(n, dtype=torch.float64, device=dev) for _ in range(b)] for _ in range(sets)]
    w = [1.0 / n] * n

    def tasks(s):
        return [([models[s][(p + d) % b] for d in range(n)], w, outs[s][p], d2s[s][p]) for p in range(b)]
    decoy = BatchedPlan(tasks(sets - 1))
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "geomed_batch", "case": "a", "tasks": b, "n": n, "params": P, "dtype": "float32",
            "bytes": (n + 1) * P * 4 * b, "rotating_sets": sets - 1, "calls_per_window": launches, "windows": nwin}
    three_legs(base, "per_task", lambda j: Seq([FusedPlan(*t) for t in tasks(j)]), lambda j: BatchedPlan(tasks(j)),
               sets - 1, launches, nwin)


def batch_leg_b(nwin, launches):
    """Two tasks of eight ResNet-18-shaped fp32 models in 62 tensors each."""
    sys.path.insert(0, ROOT)
    from bench import resnet18_shapes
    sizes = [int(np.prod(s)) for s in resnet18_shapes()]
    dev, b, n, P = torch.device("cuda", 0), 2, 8, sum(sizes)
    sets = max(3, -(-(1 << 30) // (b * n * P * 4))) + 1
    w = [1.0 / n] * n
    tasks = [[(filled(n, P, torch.float32, dev, s * b + k), w, filled(1, P, torch.float32, dev, 500 + s * b + k)[0],
               torch.empty(n, dtype=torch.float64, device=dev)) for k in range(b)] for s in range(sets)]
    decoy = BatchedPlan(tasks[sets - 1], sizes)
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "geomed_batch", "case": "b", "tasks": b, "n": n, "tensors": len(sizes), "params": P,
            "dtype": "float32", "bytes": b * (n + 1) * P * 4, "rotating_sets": sets - 1,
            "calls_per_window": launches, "windows": nwin}
    three_legs(base, "tensors", lambda j: Seq([TensorsPlan(*t, sizes) for t in tasks[j]]),
               lambda j: BatchedPlan(tasks[j], sizes), sets - 1, launches, nwin)


def batch_leg_c(nwin):
    """One round of 100 GNLeNet peers, every peer the geometric median (then centered clipping) over 8 device
    arenas: RoundExecutor against the same tasks one by one through functions.aggregate (aggregate_on_device).
    Wall time of the round, stream synchronised."""
    import types

    from dasklearn_amd import functions
    from dasklearn_amd.gradient_aggregation import GradientAggregationMethod
    from dasklearn_amd.rounds import RoundExecutor

    class Shaped(nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = nn.ParameterList([nn.Parameter(torch.randn(*sh) * 0.05) for sh in GNLENET_SHAPES])
    peers, n = 100, 8
    torch.manual_seed(0)
    pool = [arena.to_device_arena(Shaped(), "cuda") for _ in range(peers)]
    tasks = [(f"agg_{p}", "aggregate", {"models": [(f"m_{(p + d) % peers}", 0) for d in range(n)], "round": 1, "peer": p})
             for p in range(peers)]
    for name, method in (("GEOMETRIC_MEDIAN", GradientAggregationMethod.GEOMETRIC_MEDIAN),
                         ("CENTERED_CLIP", GradientAggregationMethod.CENTERED_CLIP)):
        settings = types.SimpleNamespace(gradient_aggregation=method, aggregate_on_device=True)

        def executor():
            ex = RoundExecutor({}, settings, keep_all=True)
            return ex.run(tasks, seed={f"m_{p}": [pool[p]] for p in range(peers)})

        def per_task():
            return [functions.aggregate(settings, {"models": [pool[(p + d) % peers] for d in range(n)], "round": 1,
                                                   "peer": p}) for p in range(peers)]
        base = {"bench": "geomed_batch", "case": "c", "peers": peers, "n": n, "iters": 3, "params": GNLENET_P,
                "dtype": "float32", "method": name, "timing": "wall, synchronised", "reps": nwin}
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
        ratio_line(base, res, "executor", "per_task", yards)


def batch_leg_d(nwin, launches, large=1):
    """`large` fp32 tasks of 11,181,642 elements, n = 8, in one batched call, against as many calls of the
    flat entry. large = 1: a one-element task of n = 1 rides along (in both paths), since a call of one
    task is forwarded to the flat entry and would measure it against itself."""
    dev, n, P = torch.device("cuda", 0), 8, RESNET18_P
    sets = max(3, -(-(1 << 30) // (large * n * P * 4))) + 1
    w = [1.0 / n] * n
    tasks = [[(filled(n, P, torch.float32, dev, s * large + k), w, filled(1, P, torch.float32, dev, 900 + s * large + k)[0],
               torch.empty(n, dtype=torch.float64, device=dev)) for k in range(large)] for s in range(sets)]
    if large == 1:
        for ts in tasks:
            ts.append((filled(1, 1, torch.float32, dev, 7), [1.0], filled(1, 1, torch.float32, dev, 8)[0],
                       torch.empty(1, dtype=torch.float64, device=dev)))
    decoy = Seq([FusedPlan(*t) for t in tasks[sets - 1]])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "geomed_batch", "case": "d", "large_tasks": large, "tasks": len(tasks[0]), "n": n, "params": P,
            "dtype": "float32", "bytes": large * (n + 1) * P * 4, "rotating_sets": sets - 1,
            "calls_per_window": launches, "windows": nwin}
    three_legs(base, "flat", lambda j: Seq([FusedPlan(*t) for t in tasks[j]]), lambda j: BatchedPlan(tasks[j]),
               sets - 1, launches, nwin)


def write_out(path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=None,
                    help="calls per window: 200 by default, 20 in leg (a) of --batch (a call there is 100 tasks)")
    ap.add_argument("--skip-bf16", action="store_true")
    ap.add_argument("--batch", action="store_true", help="the batched entry's legs (a)-(e) instead of the flat kernel's")
    ap.add_argument("--legs", default="abcde", help="with --batch: which of the legs a, b, c, d, e")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geomed.py measures on a GPU; none is visible")
    if a.batch:
        def leg_d():
            batch_leg_d(a.windows, a.launches or 200)
            torch.cuda.empty_cache()
            batch_leg_d(a.windows, a.launches or 200, large=2)

        def leg_e():
            for n in (4, 8, 16, 32):
                kernel_lines(RESNET18_P, torch.float32, n, a.launches or 200, a.windows)
                torch.cuda.empty_cache()
        for leg in a.legs:
            {"a": lambda: batch_leg_a(a.windows, a.launches or 20), "b": lambda: batch_leg_b(a.windows, a.launches or 100),
             "c": lambda: batch_leg_c(a.windows), "d": leg_d, "e": leg_e}[leg]()
            torch.cuda.empty_cache()
        write_out(a.out)
        return
    a.launches = a.launches or 200
    for n in (4, 8, 16, 32):
        kernel_lines(11_181_642, torch.float32, n, a.launches, a.windows)
        torch.cuda.empty_cache()
    if not a.skip_bf16:
        kernel_lines(125_000_000, torch.bfloat16, 8, a.launches, a.windows)
        torch.cuda.empty_cache()
    plugin_lines()
    write_out(a.out)


if __name__ == "__main__":
    main()
