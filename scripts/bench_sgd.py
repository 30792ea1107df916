"""The fresh-SGD step (the `gradient_update` task, dlsim_sgd_step) on the
MI355X, against the 2-way reduce that moves the same bytes (for DESIGN.md §8h).

  kernel   dlsim_sgd_step on flat device buffers, fp32 at 11,181,642 elements
           (ResNet-18) and bf16 at 125,000,000: HIP events over windows of 200
           back-to-back launches after a warm-up; parameters, gradients AND
           outputs rotate over >= 1 GiB each (none stays in the 256 MiB
           Infinity Cache), a decoy set is read first (§5f);
           the median window, with the fastest and slowest. Algorithmic bytes
           3 * P * s per launch.
  yard     the yardstick: dlsim_wreduce, n = 2, exact mode, same P and dtype,
           the same buffers and rotation, in the same process, run twice (before
           and after the step) to show its own run-to-run spread
  task     one functions.gradient_update on GNLeNet host modules (wall, ends
           in host memory) against the reference's op sequence on the CPU
           (a fresh torch.optim.SGD, param.grad = grad, step, state_dict copy)
           at 4 threads, as scripts/bench_host.py does for the aggregate

    python scripts/bench_sgd.py [--windows 5] [--launches 200] [--skip-task]
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import copy
import ctypes
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

from dasklearn_amd import _native, functions  # noqa: E402
from dasklearn_amd.arena import aligned_empty, arena_empty, base_align, row_stride  # noqa: E402

GNLENET = [(32, 3, 5, 5), (32,), (32,), (32,), (32, 32, 5, 5), (32,), (32,), (32,), (64, 32, 5, 5),
           (64,), (64,), (64,), (10, 576), (10,)]
LR, WD = 0.1, 5e-4


class StepPlan:
    """One prepared dlsim_sgd_step call (pointers resolved once, as ReducePlan)."""

    def __init__(self, p, g, out, lr, wd):
        self._keep = (p, g, out)
        self.args = (ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                     out.numel(), float(lr), float(wd), _native.dtype_code(out.dtype, single_task=True))
        self.lib = _native.load()
        self.device = out.device

    def launch(self, stream=None):
        rc = self.lib.dlsim_sgd_step(*self.args, _native._stream_handle(self.device, stream))
        if rc:
            _native._check("dlsim_sgd_step", rc)


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


def kernel_lines(P, tdt, launches, nwin):
    dev = torch.device("cuda", 0)
    esz = torch.empty((), dtype=tdt).element_size()
    byts = 3 * P * esz
    sets = max(3, -(-(1 << 30) // (2 * P * esz)))
    out_sets = -(-max(sets, -(-(1 << 30) // (P * esz))) // sets) * sets
    stride = row_stride(P, esz)
    # + 1: the decoy set, read first and never timed
    rows = aligned_empty((sets + 1) * 2 * stride, tdt, dev, base_align(P * esz, esz)).view(sets + 1, 2, stride)
    g = torch.Generator(device=dev).manual_seed(0)
    for s in range(sets + 1):
        rows[s, 0, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.05).to(tdt))
        rows[s, 1, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.01).to(tdt))
    outs = [arena_empty(P, tdt, dev) for _ in range(out_sets + 1)]
    w = np.array([1.0, -LR], dtype=np.float32)
    step = [StepPlan(rows[j % sets, 0, :P], rows[j % sets, 1, :P], outs[j], LR, WD) for j in range(out_sets)]
    yard = [_native.ReducePlan([rows[j % sets, 0, :P], rows[j % sets, 1, :P]], w, outs[j], _native.DLSIM_EXACT)
            for j in range(out_sets)]
    decoy = StepPlan(rows[sets, 0, :P], rows[sets, 1, :P], outs[out_sets], LR, WD)
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"params": P, "dtype": str(tdt).replace("torch.", ""), "bytes": byts, "rotating_sets": sets,
            "rotating_outputs": out_sets, "launches_per_window": launches, "windows": nwin}
    res = {}
    for key, plans in (("yard_1", yard), ("sgd_step", step), ("yard_2", yard)):
        ws = windows(plans, launches, nwin)
        res[key] = ws[len(ws) // 2]
        line = dict(base, leg=key, median_us=round(ws[len(ws) // 2], 3), min_us=round(ws[0], 3),
                    max_us=round(ws[-1], 3), GBps=round(byts / ws[len(ws) // 2] / 1e3, 1),
                    kernel=_native.kernel_name(2, P, tdt) if key.startswith("yard") else "dlsim::k_sgd_tiles")
        print(json.dumps(line), flush=True)
    yard_us = (res["yard_1"] + res["yard_2"]) / 2
    print(json.dumps(dict(base, leg="ratio", sgd_over_yard=round(res["sgd_step"] / yard_us, 4),
                          yard_spread=round(abs(res["yard_1"] - res["yard_2"]) / yard_us, 4))), flush=True)


class Shaped(nn.Module):
    def __init__(self, shapes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = nn.ParameterList([nn.Parameter(torch.randn(*s, generator=g) * 0.05) for s in shapes])


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def cpu_reference_task(model, grads, fresh):
    """train()'s gradient branch (functions.py:54-55, 70): the step on the
    model in place, then unserialize_model(serialize_model(model)) restated
    as a state_dict copy into a new model."""
    opt = torch.optim.SGD(model.parameters(), lr=LR, momentum=0.9, weight_decay=WD)
    for p, g in zip(model.parameters(), grads):
        p.grad = g
    opt.step()
    out = copy.deepcopy(fresh)
    out.load_state_dict(copy.deepcopy(model.state_dict()))
    return out


def task_line(reps):
    model = Shaped(GNLENET, 1)
    g = torch.Generator().manual_seed(2)
    grads = [torch.randn(*s, generator=g) * 0.01 for s in GNLENET]
    settings = types.SimpleNamespace(learning=types.SimpleNamespace(learning_rate=LR, momentum=0.9, weight_decay=WD))
    params = {"model": model, "gradient_model": types.SimpleNamespace(gradient=grads)}
    res = {"leg": "task", "model": "gnlenet", "params": sum(int(np.prod(s)) for s in GNLENET), "tensors": len(GNLENET)}
    t = timed(lambda: functions.gradient_update(settings, params), reps)
    res["host_task_us"] = round(t * 1e6, 1)
    torch.set_num_threads(4)
    ref_model, fresh = Shaped(GNLENET, 1), Shaped(GNLENET, 3)
    t = timed(lambda: cpu_reference_task(ref_model, grads, fresh), reps)
    res["cpu_ref_4t_us"] = round(t * 1e6, 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--task-reps", type=int, default=200)
    ap.add_argument("--skip-task", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sgd.py measures on a GPU; none is visible")
    kernel_lines(11_181_642, torch.float32, a.launches, a.windows)
    torch.cuda.empty_cache()
    kernel_lines(125_000_000, torch.bfloat16, a.launches, a.windows)
    torch.cuda.empty_cache()
    if not a.skip_task:
        task_line(a.task_reps)


if __name__ == "__main__":
    main()
