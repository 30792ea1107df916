"""Probe: scripts/bench_rounds.py --host as it runs, with every pass of Python's cyclic collector during
every RoundExecutor.run accounted for: by generation, inside or outside the metered aggregate waves, count
and milliseconds; and the run's wall time. The bench's own line counts the passes inside the waves only;
this shows whether a pass that appears there is new work or one that moved. One RUN line per run (the
first is the warm-up round), after the bench's own lines.

    python scripts/probes/probe_gc_whole_run.py [bench_rounds.py arguments, e.g. --rounds 5]
"""
from __future__ import annotations

import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "decentralized-learning-simulator_amd")]
import torch  # noqa: E402

import bench_rounds as br  # noqa: E402
from dasklearn_amd import rounds  # noqa: E402

state = {"cur": None, "t0": 0.0}
runs = []


def cb(phase, info):
    cur = state["cur"]
    if cur is None:
        return
    if phase == "start":
        state["t0"] = time.perf_counter()
    else:
        k = "wave" if br.GC.active else "other"
        g = info["generation"]
        cur[k + "_n"][g] += 1
        cur[k + "_s"][g] += time.perf_counter() - state["t0"]


gc.callbacks.append(cb)
orig = rounds.RoundExecutor.run


def run(self, tasks, seed=None):
    torch.cuda.synchronize()
    cur = {"wave_n": [0, 0, 0], "other_n": [0, 0, 0], "wave_s": [0.0] * 3, "other_s": [0.0] * 3}
    state["cur"] = cur
    t0 = time.perf_counter()
    try:
        return orig(self, tasks, seed)
    finally:
        torch.cuda.synchronize()
        state["cur"] = None
        cur["wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        cur["tasks"] = len(tasks)
        cur["agg_ms"] = round(self.stats["aggregate"] * 1e3, 2)
        cur["other_ms"] = round(self.stats["other"] * 1e3, 2)
        cur["wave_s"] = [round(x * 1e3, 2) for x in cur["wave_s"]]
        cur["other_s"] = [round(x * 1e3, 2) for x in cur["other_s"]]
        runs.append(cur)


rounds.RoundExecutor.run = run
sys.argv = ["bench_rounds.py", "--host", "--cpu-rounds", "1"] + sys.argv[1:]
br.main()
for r in runs:
    print("RUN " + json.dumps(r))
