"""The stateful momentum-SGD step (dlsim_sgd_momentum_step, ArenaSGD) on the
MI355X, against the fresh-SGD step on the same buffers (for DESIGN.md §8i).

  kernel   dlsim_sgd_momentum_step in place on flat device buffers, fp32 at
           11,181,642 elements (ResNet-18) and bf16 at 125,000,000: HIP events
           over windows of 200 back-to-back launches after a warm-up;
           parameters, gradients and buffers each rotate over >= 1 GiB (none
           stays in the 256 MiB Infinity Cache), a decoy set is
           read first (§5f); the median window, with the fastest and slowest.
           `later`: 5 * P * s bytes per launch (reads p, g, buf; writes p, buf);
           `first`: 4 * P * s (no buffer read).
  yard     the yardstick: dlsim_sgd_step in place (3 * P * s) on the same
           session's buffers and rotation, run before and after, to show its
           own run-to-run spread. The comparison is achieved bytes per second.
  step     one ArenaSGD.step() on a ResNet-18-shaped device model (62 tensors,
           fp32), flat path (grad_arena=True) and tensors path, against
           torch.optim.SGD on the same device tensors (foreach=True, and
           fused=True where this torch offers it): us per step including
           Python, windows of back-to-back steps closed by a synchronize.

    python scripts/bench_sgdm.py [--windows 5] [--launches 200] [--skip-step]
One JSON line per measurement.
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

import torch  # noqa: E402
from torch import nn  # noqa: E402

from dasklearn_amd import _native  # noqa: E402
from dasklearn_amd.arena import aligned_empty, base_align, row_stride, to_device_arena  # noqa: E402
from dasklearn_amd.optimizer import ArenaSGD  # noqa: E402

LR, MOM, WD = 0.1, 0.9, 5e-4


class Plan:
    """One prepared C call (pointers resolved once)."""

    def __init__(self, fn, args, keep, device):
        self.fn, self.args, self._keep, self.device = fn, args, keep, device

    def launch(self):
        rc = self.fn(*self.args, _native._stream_handle(self.device, None))
        if rc:
            _native._check("bench_sgdm", rc)


def yard_plan(p, g):
    lib = _native.load()
    vp = ctypes.c_void_p
    return Plan(lib.dlsim_sgd_step, (vp(p.data_ptr()), vp(g.data_ptr()), vp(p.data_ptr()), p.numel(), LR, WD,
                                     _native.dtype_code(p.dtype, single_task=True)), (p, g), p.device)


def momentum_plan(p, g, b, first):
    lib = _native.load()
    vp = ctypes.c_void_p
    return Plan(lib.dlsim_sgd_momentum_step,
                (vp(p.data_ptr()), vp(g.data_ptr()), None if first else vp(b.data_ptr()), vp(p.data_ptr()),
                 vp(b.data_ptr()), p.numel(), LR, MOM, WD, _native.dtype_code(p.dtype, single_task=True)),
                (p, g, b), p.device)


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
    sets = max(3, -(-(1 << 30) // (P * esz)))  # every stream rotates over >= 1 GiB
    stride = row_stride(P, esz)
    # + 1: the decoy set, read first and never timed
    rows = aligned_empty((sets + 1) * 3 * stride, tdt, dev, base_align(P * esz, esz)).view(sets + 1, 3, stride)
    g = torch.Generator(device=dev).manual_seed(0)
    for s in range(sets + 1):
        rows[s, 0, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.05).to(tdt))
        rows[s, 1, :P].copy_((torch.randn(P, generator=g, device=dev) * 0.01).to(tdt))
        rows[s, 2, :P].copy_(rows[s, 1, :P])
    trio = [(rows[s, 0, :P], rows[s, 1, :P], rows[s, 2, :P]) for s in range(sets + 1)]
    yard = [yard_plan(p, g_) for p, g_, _ in trio[:sets]]
    later = [momentum_plan(p, g_, b, False) for p, g_, b in trio[:sets]]
    first = [momentum_plan(p, g_, b, True) for p, g_, b in trio[:sets]]
    decoy = momentum_plan(*trio[sets], False)
    for _ in range(8):
        decoy.launch()
    torch.cuda.synchronize()
    base = {"params": P, "dtype": str(tdt).replace("torch.", ""), "rotating_sets": sets,
            "launches_per_window": launches, "windows": nwin}
    res = {}
    for key, plans, streams in (("yard_1", yard, 3), ("later", later, 5), ("first", first, 4), ("yard_2", yard, 3)):
        ws = windows(plans, launches, nwin)
        med = ws[len(ws) // 2]
        res[key] = streams * P * esz / med / 1e3  # GB/s
        print(json.dumps(dict(base, leg=key, bytes=streams * P * esz, median_us=round(med, 3), min_us=round(ws[0], 3),
                              max_us=round(ws[-1], 3), GBps=round(res[key], 1),
                              kernel="dlsim::k_sgd_tiles" if key.startswith("yard") else "dlsim::k_sgdm_tiles")),
              flush=True)
    yard_rate = (res["yard_1"] + res["yard_2"]) / 2
    print(json.dumps(dict(base, leg="ratio", later_rate_over_yard=round(res["later"] / yard_rate, 4),
                          first_rate_over_yard=round(res["first"] / yard_rate, 4),
                          yard_spread=round(abs(res["yard_1"] - res["yard_2"]) / yard_rate, 4))), flush=True)


def resnet18_shapes(classes=10):
    """parameters() of a ResNet-18: 62 tensors, 11,181,642 elements at 10 classes."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    cin = 64
    for cout, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        for blk in range(2):
            shapes += [(cout, cin if blk == 0 else cout, 3, 3), (cout,), (cout,), (cout, cout, 3, 3), (cout,), (cout,)]
            if blk == 0 and stride != 1:
                shapes += [(cout, cin, 1, 1), (cout,), (cout,)]
        cin = cout
    return shapes + [(classes, 512), (classes,)]


class Shaped(nn.Module):
    def __init__(self, shapes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = nn.ParameterList([nn.Parameter(torch.randn(*s, generator=g) * 0.05) for s in shapes])


def step_windows(opt, steps, nwin):
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / steps)
    return sorted(out)


def step_lines(steps, nwin):
    dev = torch.device("cuda", 0)
    shapes = resnet18_shapes()
    host = Shaped(shapes, 1)
    base = {"leg": "step", "model": "resnet18", "tensors": len(shapes), "params": sum(p.numel() for p in host.parameters()),
            "steps_per_window": steps, "windows": nwin}
    g = torch.Generator(device=dev).manual_seed(2)

    def fill(model):
        for p in model.parameters():
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(torch.randn(p.shape, generator=g, device=dev) * 0.01)

    cases = []
    m = to_device_arena(host, dev)
    o = ArenaSGD(m.parameters(), lr=LR, momentum=MOM, weight_decay=WD, grad_arena=True)
    o.zero_grad()
    cases.append(("arena_flat", m, o))
    m = to_device_arena(host, dev)
    cases.append(("arena_tensors", m, ArenaSGD(m.parameters(), lr=LR, momentum=MOM, weight_decay=WD)))
    m = to_device_arena(host, dev)
    cases.append(("torch_foreach", m, torch.optim.SGD(m.parameters(), lr=LR, momentum=MOM, weight_decay=WD,
                                                      foreach=True)))
    try:
        m = to_device_arena(host, dev)
        cases.append(("torch_fused", m, torch.optim.SGD(m.parameters(), lr=LR, momentum=MOM, weight_decay=WD,
                                                        fused=True)))
    except (RuntimeError, TypeError, ValueError) as e:
        print(json.dumps(dict(base, optimizer="torch_fused", unavailable=str(e)[:200])), flush=True)
    for name, m, o in cases:
        fill(m)
        ws = step_windows(o, steps, nwin)
        line = dict(base, optimizer=name, median_us=round(ws[len(ws) // 2], 2), min_us=round(ws[0], 2),
                    max_us=round(ws[-1], 2))
        if isinstance(o, ArenaSGD):
            line.update(launches=o.last_launches, paths=sorted(set(o.last_paths.values())))
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sgdm.py measures on a GPU; none is visible")
    if not a.skip_kernel:
        kernel_lines(11_181_642, torch.float32, a.launches, a.windows)
        torch.cuda.empty_cache()
        kernel_lines(125_000_000, torch.bfloat16, a.launches, a.windows)
        torch.cuda.empty_cache()
    if not a.skip_step:
        step_lines(a.launches, a.windows)


if __name__ == "__main__":
    main()
