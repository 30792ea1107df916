"""Top-k sparsified sharing on the MI355X: the selection and the
sparse neighbour reduce against what exists without them, in one process on
the same buffers. Device events around every call; the buffers of a leg rotate
over sets that together exceed the 256 MiB Infinity Cache, a decoy set is read
first; the median over the timed calls, with the fastest and slowest.

  select  dlsim_topk_select, fp32 at 11,181,642 elements and bf16 at
          125,000,000, k = P/100 and P/10. The last-shared copy is restored
          between calls (outside the events), so every call sees the same
          deltas. Yardstick: torch.topk(|x - ref|, k) on the same buffers. Also
          the time as a multiple of one read of x and ref at the north star's
          rate (--rate, TB/s): the passes the selection really costs.
  mix     dlsim_sparse_wreduce, fp32, self plus 7 neighbours, k = P/100 and
          P/10. Yardstick: dlsim_wreduce over the 8 densified rows; the scatter
          that densifies them (copy of self, index_put of the values) apart.
  round   100 GNLeNet-sized tasks (85,354 fp32, 7 neighbours of k = P/10)
          through sparse.mix_batch against 100 sparse.mix calls (wall clock,
          synchronised).

    python scripts/bench_sparse.py [--calls 20] [--legs select,mix,round] [--skip-bf16] [--out FILE]
One JSON line per measurement (also written to --out).
"""
from __future__ import annotations

import argparse
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

from dasklearn_amd import _native  # noqa: E402
from dasklearn_amd.arena import to_device_arena  # noqa: E402
from dasklearn_amd.sparse import TopKSharer, mix, mix_batch  # noqa: E402

DEV = "cuda"
CACHE = 256 << 20
LINES = []


def emit(line):
    LINES.append(line)
    print(json.dumps(line), flush=True)


def timed(calls, fn, sets, before=None):
    """us of `calls` single calls fn(set), the sets in rotation; before(set) runs outside the events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for s in sets:  # warm-up, and the decoy read
        if before:
            before(s)
        fn(s)
    torch.cuda.synchronize()
    out = []
    for c in range(calls):
        s = sets[c % len(sets)]
        if before:
            before(s)
        e0.record()
        fn(s)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out)), "calls": calls}


def nsets(bytes_per_set):
    return max(2, -(-2 * CACHE // bytes_per_set))


def leg_select(args):
    for dt, p in ((torch.float32, 11_181_642),) + (() if args.skip_bf16 else ((torch.bfloat16, 125_000_000),)):
        esz = torch.empty((), dtype=dt).element_size()
        sets = []
        for _ in range(nsets(2 * p * esz)):
            x = (torch.randn(p, device=DEV) * 0.05).to(dt)
            ref0 = (torch.randn(p, device=DEV) * 0.05).to(dt)
            sets.append({"x": x, "ref0": ref0, "ref": ref0.clone()})
        for frac in (100, 10):
            k = p // frac
            idx, val = torch.empty(k, dtype=torch.int32, device=DEV), torch.empty(k, dtype=dt, device=DEV)
            ours = timed(args.calls, lambda s: _native.topk_select(s["x"], s["ref"], k, idx, val), sets,
                         before=lambda s: s["ref"].copy_(s["ref0"]))
            yard = timed(args.calls, lambda s: torch.topk((s["x"].float() - s["ref0"].float()).abs(), k, sorted=False), sets)
            one_read_us = 2 * p * esz / (args.rate * 1e12) * 1e6
            emit({"leg": "select", "dtype": str(dt), "P": p, "k": k, "kernel": _native.topk_kernel_name(sets[0]["x"], sets[0]["ref"], k),
                  "dlsim_topk_select": ours, "torch_topk": yard, "ratio_to_torch": ours["median_us"] / yard["median_us"],
                  "one_read_of_x_and_ref_us": one_read_us, "reads_equivalent": ours["median_us"] / one_read_us})
        del sets
        torch.cuda.empty_cache()


def leg_mix(args):
    p, n, dt = 11_181_642, 8, torch.float32
    w = _native.fp32_weights([1.0 / n] * n)
    for frac in (100, 10):
        k = p // frac
        sets = []
        for _ in range(nsets(2 * p * 4)):
            own = torch.randn(p, device=DEV) * 0.05
            lists = [(torch.sort(torch.randperm(p, device=DEV)[:k])[0].to(torch.int32), torch.randn(k, device=DEV) * 0.05)
                     for _ in range(n - 1)]
            sets.append({"own": own, "lists": lists, "out": torch.empty_like(own)})
        ours = timed(args.calls, lambda s: _native.sparse_wreduce(s["own"], s["lists"], w, s["out"]), sets)
        rows = [torch.empty(p, device=DEV) for _ in range(n - 1)]

        def densify(s):
            for row, (ix, vl) in zip(rows, s["lists"]):
                row.copy_(s["own"])
                row[ix.long()] = vl
        scatter = timed(args.calls, densify, sets)
        dense_sets = []
        for s in sets[:max(2, -(-2 * CACHE // (9 * p * 4)))]:
            densify(s)
            dense_sets.append({"rows": [s["own"]] + [r.clone() for r in rows], "out": s["out"]})
        yard = timed(args.calls, lambda s: _native.wreduce(s["rows"], w, s["out"]), dense_sets)
        emit({"leg": "mix", "dtype": str(dt), "P": p, "n": n, "k": k, "dlsim_sparse_wreduce": ours, "dlsim_wreduce_dense": yard,
              "densify_scatter": scatter, "ratio_to_dense": ours["median_us"] / yard["median_us"],
              "ratio_to_dense_plus_scatter": ours["median_us"] / (yard["median_us"] + scatter["median_us"])})
        del sets, dense_sets, rows
        torch.cuda.empty_cache()


class GNLeNetSized(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.randn(85_354) * 0.05)


def leg_round(args):
    peers, m = 100, 7
    models = [to_device_arena(GNLeNetSized(), DEV) for _ in range(peers)]
    sparse = [TopKSharer(q, ratio=0.1).share(q) for q in models]
    tasks = [(models[i], [sparse[(i + j) % peers] for j in range(1, m + 1)], None) for i in range(peers)]

    def wall(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6)
        return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out)), "calls": reps}
    one = wall(lambda: [mix(*t) for t in tasks])
    batch = wall(lambda: mix_batch(tasks))
    emit({"leg": "round", "tasks": peers, "P": 85_354, "neighbours": m, "k": sparse[0].groups[torch.float32][0].numel(),
          "mix_x100": one, "mix_batch": batch, "ratio": batch["median_us"] / one["median_us"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--legs", default="select,mix,round")
    ap.add_argument("--skip-bf16", action="store_true")
    ap.add_argument("--rate", type=float, default=6.55, help="the north star's rate, TB/s")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sparse.py measures on a GPU"
    for leg in args.legs.split(","):
        {"select": leg_select, "mix": leg_mix, "round": leg_round}[leg](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in LINES)


if __name__ == "__main__":
    main()
