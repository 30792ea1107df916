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

    python scripts/bench_geomed.py [--windows 5] [--launches 200] [--skip-bf16] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-bf16", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geomed.py measures on a GPU; none is visible")
    for n in (4, 8, 16, 32):
        kernel_lines(11_181_642, torch.float32, n, a.launches, a.windows)
        torch.cuda.empty_cache()
    if not a.skip_bf16:
        kernel_lines(125_000_000, torch.bfloat16, 8, a.launches, a.windows)
        torch.cuda.empty_cache()
    plugin_lines()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(LINES, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
