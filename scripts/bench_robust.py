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

    python scripts/bench_robust.py [--windows 5] [--launches 200] [--skip-bf16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-bf16", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust.py measures on a GPU; none is visible")
    for n in (4, 8, 16, 32):
        kernel_lines(11_181_642, torch.float32, n, a.launches, a.windows)
        torch.cuda.empty_cache()
    if not a.skip_bf16:
        for n in (2, 8):
            kernel_lines(125_000_000, torch.bfloat16, n, a.launches, a.windows)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
