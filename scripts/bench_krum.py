"""The pairwise squared-distance kernel (dlsim_pairwise_sqdist, under Krum and
Multi-Krum) on the MI355X, against the weighted reduce that reads the same
rows (for DESIGN.md §8k).

  kernel   dlsim_pairwise_sqdist on flat device rows: fp32 at 11,181,642
           elements (ResNet-18) with n = 4, 8, 16, 32, bf16 at 125,000,000
           with n = 8. HIP events over windows of 200 back-to-back calls (each
           the distance kernel and its small finish kernel) after a warm-up;
           the inputs rotate over >= 1 GiB (none stays in the 256 MiB Infinity
           Cache), a decoy set is read first (§5f); the median
           window of time, with the fastest and slowest. Algorithmic bytes
           n * P * s per call (every row read once).
  yard     the yardstick: dlsim_wreduce, exact mode, the same n, P and dtype on
           the same rows with the same rotation, in the same process, run
           before and after to show its own run-to-run spread. It reads the
           same rows and writes one more ((n + 1) * P * s bytes).
  plugin   one Krum.aggregate and one MultiKrum.aggregate on eight
           ResNet-18-shaped device-arena models next to FedAvg.aggregate on
           the same models (wall clock, synchronised, median of 20).

  batch    (--batch, instead of the above) the batched entry
           against the paths that were there before it, each leg with its
           yardstick in this one process before and after, the same rotation
           and decoy rule, a "launch" being one whole call: (a) 100 matrices
           of n = 8 GNLeNet-sized fp32 rows: one dlsim_pairwise_sqdist_batched
           call against 100 dlsim_pairwise_sqdist calls; (b) one RoundExecutor
           round of 100 GNLeNet peers under KRUM, then MULTI_KRUM, against the
           same tasks one by one through functions.aggregate with
           aggregate_on_device (wall time, stream synchronised); (c) one fp32
           task of 11,181,642 elements, n = 8, through the batched entry
           against the flat entry (a call of one task is forwarded to the
           flat path since this leg was first measured); (d) two such tasks
           in one batched call against two calls of the flat entry: large
           tasks inside the batched kernel.

    python scripts/bench_krum.py [--windows 5] [--launches 200] [--skip-bf16] [--out FILE]
    python scripts/bench_krum.py --batch [--windows 7] [--launches N] [--legs abcd] [--out FILE]
One JSON line per measurement (also written to --out). --launches is the number
of whole calls per window of legs (a), (c) and (d): 20 in (a), where a call is
100 tasks, and 200 in (c) and (d) unless given; leg (b) times single rounds on the wall clock.
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
from dasklearn_amd.gradient_aggregation.krum import Krum, MultiKrum  # noqa: E402

LINES = []


def emit(line):
    LINES.append(line)
    print(json.dumps(line), flush=True)


class DistPlan:
    """One prepared dlsim_pairwise_sqdist call (pointers resolved once, as ReducePlan)."""

    def __init__(self, inputs, d2):
        n = len(inputs)
        self._keep = (list(inputs), d2)
        self.args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs]), n, inputs[0].numel(),
                     _native.dtype_code(inputs[0].dtype, single_task=True), ctypes.c_void_p(d2.data_ptr()), 0)
        self.lib = _native.load()
        self.device = d2.device

    def launch(self, stream=None):
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
    byts = n * P * esz
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
    d2s = [torch.empty(n * n, dtype=torch.float64, device=dev) for _ in range(sets + 1)]
    w = np.full(n, 1.0 / n, dtype=np.float32)
    ins = [[rows[s, i, :P] for i in range(n)] for s in range(sets + 1)]
    decoy = DistPlan(ins[sets], d2s[sets])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    tile, blocks = _native.pairdist_geometry(n, tdt, P)
    base = {"params": P, "dtype": str(tdt).replace("torch.", ""), "n": n, "bytes": byts, "rotating_sets": sets,
            "launches_per_window": launches, "windows": nwin}
    res = {}
    for key in ("yard_1", "pairdist", "yard_2"):
        if key == "pairdist":
            plans = [DistPlan(ins[j], d2s[j]) for j in range(sets)]
            moved = byts
        else:
            plans = [_native.ReducePlan(ins[j % sets], w, outs[j], _native.DLSIM_EXACT) for j in range(out_sets)]
            moved = byts + P * esz
        ws = windows(plans, launches, nwin)
        res[key] = ws[len(ws) // 2]
        line = dict(base, leg=key, median_us=round(ws[len(ws) // 2], 3), min_us=round(ws[0], 3),
                    max_us=round(ws[-1], 3), algorithmic_bytes=moved, GBps=round(moved / ws[len(ws) // 2] / 1e3, 1),
                    kernel="dlsim::k_pairdist + dlsim::k_pairdist_finish" if key == "pairdist"
                    else _native.kernel_name(n, P, tdt))
        if key == "pairdist":
            line.update(tile_elems=tile, blocks=blocks)
        emit(line)
    yard_us = (res["yard_1"] + res["yard_2"]) / 2
    emit(dict(base, leg="ratio", pairdist_over_yard=round(res["pairdist"] / yard_us, 4),
              yard_spread=round(abs(res["yard_1"] - res["yard_2"]) / yard_us, 4)))


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
    for name, agg in (("FedAvg", FedAvg), ("Krum(f=2)", Krum.with_params(2)), ("MultiKrum(f=2)", MultiKrum.with_params(2)),
                      ("FedAvg_again", FedAvg)):
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


class BatchedDistPlan:
    """One prepared dlsim_pairwise_sqdist_batched call over tasks = [(inputs, d2)], one tensor per model."""

    def __init__(self, tasks):
        b = len(tasks)
        ptrs = [t.data_ptr() for ins, _ in tasks for t in ins]
        self._keep = tasks
        self.args = (b, (ctypes.c_int * b)(*[len(ins) for ins, _ in tasks]), (ctypes.c_int * b)(*[1] * b),
                     (ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_size_t * b)(*[ins[0].numel() for ins, _ in tasks]),
                     _native.dtype_code(tasks[0][0][0].dtype, single_task=True),
                     (ctypes.c_void_p * b)(*[d2.data_ptr() for _, d2 in tasks]), 0)
        self.lib = _native.load()
        self.device = tasks[0][1].device

    def launch(self, stream=None):
        rc = self.lib.dlsim_pairwise_sqdist_batched(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_pairwise_sqdist_batched", rc)


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


def batch_leg_a(nwin, launches):
    """100 matrices of n = 8 GNLeNet-sized fp32 rows (a 100-peer round, every peer reading 8 of the 100 models):
    one batched call against 100 dlsim_pairwise_sqdist calls."""
    dev, b, n, P = torch.device("cuda", 0), 100, 8, GNLENET_P
    sets = -(-(1 << 30) // (b * P * 4)) + 1  # >= 1 GiB of distinct inputs, + the decoy
    models = [filled(b, P, torch.float32, dev, s) for s in range(sets)]
    d2s = [[torch.empty(n * n, dtype=torch.float64, device=dev) for _ in range(b)] for _ in range(sets)]

    def tasks(s):
        return [([models[s][(p + d) % b] for d in range(n)], d2s[s][p]) for p in range(b)]
    decoy = BatchedDistPlan(tasks(sets - 1))
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "krum_batch", "case": "a", "tasks": b, "n": n, "params": P, "dtype": "float32",
            "bytes": n * P * 4 * b, "rotating_sets": sets - 1, "calls_per_window": launches, "windows": nwin}
    res, yards = {}, []
    for leg in ("per_task_1", "batched", "per_task_2"):
        plans = [BatchedDistPlan(tasks(j)) if leg == "batched" else Seq([DistPlan(ins, d2) for ins, d2 in tasks(j)])
                 for j in range(sets - 1)]
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, us_per_task=round(ws[len(ws) // 2] / b, 3),
                          GBps=round(base["bytes"] / ws[len(ws) // 2] / 1e3, 1))
        if leg.startswith("per_task"):
            yards.append(res[leg])
    res["per_task"] = sum(yards) / 2
    ratio_line(base, res, "batched", "per_task", yards)


def batch_leg_b(nwin):
    """One round of 100 GNLeNet peers, every peer Krum (then Multi-Krum) over 8 device arenas: RoundExecutor
    against the same tasks one by one through functions.aggregate (aggregate_on_device). Wall time of the round,
    stream synchronised."""
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
    for name, method in (("KRUM", GradientAggregationMethod.KRUM), ("MULTI_KRUM", GradientAggregationMethod.MULTI_KRUM)):
        settings = types.SimpleNamespace(gradient_aggregation=method, aggregate_on_device=True, aggregation_byzantine=2)

        def executor():
            ex = RoundExecutor({}, settings, keep_all=True)
            return ex.run(tasks, seed={f"m_{p}": [pool[p]] for p in range(peers)})

        def per_task():
            return [functions.aggregate(settings, {"models": [pool[(p + d) % peers] for d in range(n)], "round": 1,
                                                   "peer": p}) for p in range(peers)]
        base = {"bench": "krum_batch", "case": "b", "peers": peers, "n": n, "f": 2, "params": GNLENET_P,
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


def batch_leg_c(nwin, launches, b=1, case="c"):
    """b fp32 tasks of 11,181,642 elements, n = 8, in one batched call, against b calls of the flat entry.
    b = 1 (leg (c)): measured with the task inside the batched kernel it showed what the descriptor lookup and
    the virtual grid cost; the entry has since forwarded a call of one task to the flat path,
    so the leg now shows that the forward costs nothing. b = 2 (leg (d)): the smallest call that still runs
    large tasks inside the batched kernel, so that cost stays measurable."""
    dev, n, P = torch.device("cuda", 0), 8, RESNET18_P
    sets = max(3, -(-(1 << 30) // (b * n * P * 4))) + 1
    ins = [[filled(n, P, torch.float32, dev, s * b + k) for k in range(b)] for s in range(sets)]
    d2s = [[torch.empty(n * n, dtype=torch.float64, device=dev) for _ in range(b)] for _ in range(sets)]
    decoy = Seq([DistPlan(i, d) for i, d in zip(ins[sets - 1], d2s[sets - 1])])
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"bench": "krum_batch", "case": case, "tasks": b, "n": n, "params": P, "dtype": "float32",
            "bytes": b * n * P * 4, "rotating_sets": sets - 1, "calls_per_window": launches, "windows": nwin}
    res, yards = {}, []
    for leg in ("flat_1", "batched", "flat_2"):
        plans = [BatchedDistPlan(list(zip(ins[j], d2s[j]))) if leg == "batched" else
                 Seq([DistPlan(i, d) for i, d in zip(ins[j], d2s[j])]) for j in range(sets - 1)]
        ws = windows(plans, launches, nwin)
        res[leg] = report(base, leg, ws, GBps=round(base["bytes"] / ws[len(ws) // 2] / 1e3, 1))
        if leg.startswith("flat"):
            yards.append(res[leg])
    res["flat"] = sum(yards) / 2
    ratio_line(base, res, "batched", "flat", yards)


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
    ap.add_argument("--batch", action="store_true", help="the batched entry's legs (a)-(d) instead of the flat kernel's")
    ap.add_argument("--legs", default="abcd", help="with --batch: which of the legs a, b, c, d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_krum.py measures on a GPU; none is visible")
    if a.batch:
        for leg in a.legs:
            {"a": lambda: batch_leg_a(a.windows, a.launches or 20), "b": lambda: batch_leg_b(a.windows),
             "c": lambda: batch_leg_c(a.windows, a.launches or 200),
             "d": lambda: batch_leg_c(a.windows, a.launches or 200, b=2, case="d")}[leg]()
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
