"""Block-quantised sharing on the MI355X: the quantiser and the
fused decode-reduce against what exists without them, in one process on the
same buffers. Device events around every call; the buffers of a leg rotate over
sets that together exceed the 256 MiB Infinity Cache, a decoy set is read
first; the legs of a comparison alternate call by call; the median over the
timed calls, with the fastest and slowest.

  quantize  dlsim_quantize, fp32 at 11,181,642 elements and bf16 at
            125,000,000; 8 and 4 bits, both roundings, with and without a
            residual. Yardstick: the torch expression a user would run instead
            (abs, amax over a [blocks, 256] view, divide, round, clamp, cast;
            nibble packing at 4 bits; the residual update), over the whole
            blocks only, which spares it the tail.
  mix       dlsim_quant_wreduce, self plus 7 neighbours of 8 and of 4 bits,
            against (a) dlsim_wreduce over 8 rows already dense and (b) seven
            dlsim_dequantize calls plus that reduce.
  round     100 GNLeNet-sized tasks (85,354 fp32, 7 neighbours of 8 bits)
            through quant.mix_batch against 100 quant.mix calls (wall clock,
            synchronised).

  --mx      MX sharing by the same method, FP8 E4M3 and FP4
            against the integer format of the same width on the same buffers:
            mx_quantize  dlsim_mx_quantize against dlsim_quantize (nearest) and
                         against the torch expression (amax over [blocks, 32],
                         floor(log2), scale, clamp, cast to float8 or a
                         bucketize to E2M1's 8 magnitudes, nibble packing)
            mx_mix       dlsim_mx_wreduce, self plus 7 neighbours, against
                         dlsim_quant_wreduce, dlsim_wreduce over 8 dense rows,
                         and 7 dlsim_mx_dequantize calls plus that reduce
            mx_fanin     self plus 15 neighbours (above both kernels' group
                         size), fp32 only, against dlsim_quant_wreduce

    python scripts/bench_quant.py [--calls 20] [--legs quantize,mix,round] [--mx] [--skip-bf16] [--out FILE]
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
from dasklearn_amd.quant import QuantSharer, mix, mix_batch  # noqa: E402

DEV = "cuda"
CACHE = 256 << 20
SHAPES = ((torch.float32, 11_181_642), (torch.bfloat16, 125_000_000))
LINES = []


def emit(line):
    LINES.append(line)
    print(json.dumps(line), flush=True)


def stats(us):
    return {"median_us": float(np.median(us)), "min_us": float(min(us)), "max_us": float(max(us)), "calls": len(us)}


def timed(calls, fns, sets):
    """Per name of `fns`: us of `calls` single calls fn(set), the sets in rotation and the legs alternating."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for s in sets:  # warm-up, and the decoy read
        for fn in fns.values():
            fn(s)
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for c in range(calls):
        for name, fn in fns.items():
            s = sets[c % len(sets)]
            e0.record()
            fn(s)
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: stats(us) for name, us in out.items()}


def nsets(bytes_per_set):
    return max(2, -(-2 * CACHE // bytes_per_set))


def torch_quantize(x, e, bits, stochastic):
    """The expression a user would run: codes, scales and the residual update, whole blocks only."""
    qmax = 127.0 if bits == 8 else 7.0
    nb = x.numel() // 256
    t = x[:nb * 256].float().view(nb, 256)
    if e is not None:
        t = t + e[:nb * 256].float().view(nb, 256)
    a = t.abs().amax(dim=1, keepdim=True)
    y = t * (qmax / a)
    q = (torch.floor(y + torch.rand_like(y)) if stochastic else torch.round(y)).clamp_(-qmax, qmax)
    scale = a / qmax
    if e is not None:
        e[:nb * 256].view(nb, 256).copy_(t - q * scale)
    q = q.to(torch.int8)
    return (q if bits == 8 else (q[:, 0::2] & 0xf) | (q[:, 1::2] << 4)), scale


def buffers(p, bits):
    return (torch.empty((p * bits + 7) // 8, dtype=torch.uint8, device=DEV),
            torch.empty((p + 255) // 256, dtype=torch.float32, device=DEV))


def leg_quantize(args):
    for dt, p in SHAPES[:1 if args.skip_bf16 else 2]:
        esz = torch.empty((), dtype=dt).element_size()
        sets = [{"x": (torch.randn(p, device=DEV) * 0.05).to(dt), "e": torch.zeros(p, dtype=dt, device=DEV)}
                for _ in range(nsets(2 * p * esz))]
        for bits in (8, 4):
            codes, scales = buffers(p, bits)
            for rounding in ("nearest", "stochastic"):
                for resid in (False, True):
                    r = timed(args.calls, {
                        "dlsim_quantize": lambda s: _native.quantize(s["x"], codes, scales, bits, rounding, 1,
                                                                     s["e"] if resid else None),
                        "torch": lambda s: torch_quantize(s["x"], s["e"] if resid else None, bits, rounding == "stochastic")}, sets)
                    used = [sets[0]["x"], codes] + ([sets[0]["e"]] if resid else [])
                    emit({"leg": "quantize", "dtype": str(dt), "P": p, "bits": bits, "rounding": rounding, "residual": resid,
                          "kernel": _native.quant_kernel_name("quantize", used, p, dt), **r,
                          "ratio_to_torch": r["dlsim_quantize"]["median_us"] / r["torch"]["median_us"]})
        del sets
        torch.cuda.empty_cache()


def leg_mix(args):
    n = 8
    w = _native.fp32_weights([1.0 / n] * n)
    for dt, p in SHAPES[:1 if args.skip_bf16 else 2]:
        esz = torch.empty((), dtype=dt).element_size()
        for bits in (8, 4):
            sets = []
            for _ in range(nsets((n + 1) * p * esz)):
                own = (torch.randn(p, device=DEV) * 0.05).to(dt)
                rows = []
                for _ in range(n - 1):
                    codes, scales = buffers(p, bits)
                    _native.quantize((torch.randn(p, device=DEV) * 0.05).to(dt), codes, scales, bits)
                    rows.append((codes, scales, bits))
                dense = [own] + [_native.dequantize(c, s, bits, torch.empty_like(own)) for c, s, _ in rows]
                sets.append({"own": own, "rows": rows, "dense": dense, "out": torch.empty_like(own)})
            scratch = [torch.empty(p, dtype=dt, device=DEV) for _ in range(n - 1)]

            def decode_then_reduce(s):
                for (c, sc, _), row in zip(s["rows"], scratch):
                    _native.dequantize(c, sc, bits, row)
                _native.wreduce([s["own"]] + scratch, w, s["out"])
            r = timed(args.calls, {"dlsim_quant_wreduce": lambda s: _native.quant_wreduce(s["own"], s["rows"], w, s["out"]),
                                   "dlsim_wreduce_dense": lambda s: _native.wreduce(s["dense"], w, s["out"]),
                                   "dequantize_x7_plus_wreduce": decode_then_reduce}, sets)
            ours = r["dlsim_quant_wreduce"]["median_us"]
            emit({"leg": "mix", "dtype": str(dt), "P": p, "n": n, "bits": bits, **r,
                  "ratio_to_dense": ours / r["dlsim_wreduce_dense"]["median_us"],
                  "ratio_to_decode_plus_dense": ours / r["dequantize_x7_plus_wreduce"]["median_us"]})
            del sets, scratch
            torch.cuda.empty_cache()


class GNLeNetSized(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.randn(85_354) * 0.05)


def leg_round(args):
    peers, m = 100, 7
    models = [to_device_arena(GNLeNetSized(), DEV) for _ in range(peers)]
    shared = [QuantSharer(q).share(q) for q in models]
    tasks = [(models[i], [shared[(i + j) % peers] for j in range(1, m + 1)], None) for i in range(peers)]

    def wall(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6)
        return stats(out)
    one = wall(lambda: [mix(*t) for t in tasks])
    batch = wall(lambda: mix_batch(tasks))
    emit({"leg": "round", "tasks": peers, "P": 85_354, "neighbours": m, "bits": 8, "mix_x100": one, "mix_batch": batch,
          "ratio": batch["median_us"] / one["median_us"]})


# ---- MX sharing ----------------------------------------------------------------------------
MX_AT = {8: "fp8_e4m3", 4: "fp4"}  # the MX format measured against each integer width


def mx_buffers(p, fmt):
    nc, ns = _native.mx_sizes(p, fmt)
    return torch.empty(nc, dtype=torch.uint8, device=DEV), torch.empty(ns, dtype=torch.uint8, device=DEV)


def torch_mx_quantize(x, e, fmt):
    """The expression a user would run: codes, scale bytes and the residual update, whole blocks only."""
    emax, vmax = (8, 448.0) if fmt == "fp8_e4m3" else (2, 6.0)
    nb = x.numel() // 32
    t = x[:nb * 32].float().view(nb, 32)
    if e is not None:
        t = t + e[:nb * 32].float().view(nb, 32)
    ex = torch.floor(torch.log2(t.abs().amax(dim=1, keepdim=True))) - emax
    scale = torch.exp2(ex)
    y = (t / scale).clamp_(-vmax, vmax)
    if fmt == "fp8_e4m3":
        q8 = y.to(torch.float8_e4m3fn)
        xh, q = q8.float(), q8.view(torch.uint8)
    else:
        grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], device=DEV)
        mids = (grid[1:] + grid[:-1]) / 2
        mag = torch.bucketize(y.abs(), mids)
        xh = grid[mag] * torch.sign(y)
        q = (mag | ((y < 0) << 3)).to(torch.uint8)
        q = q[:, 0::2] | (q[:, 1::2] << 4)
    if e is not None:
        e[:nb * 32].view(nb, 32).copy_(t - xh * scale)
    return q, (ex + 127).to(torch.uint8)


def leg_mx_quantize(args):
    for dt, p in SHAPES[:1 if args.skip_bf16 else 2]:
        esz = torch.empty((), dtype=dt).element_size()
        sets = [{"x": (torch.randn(p, device=DEV) * 0.05).to(dt), "e": torch.zeros(p, dtype=dt, device=DEV)}
                for _ in range(nsets(2 * p * esz))]
        for bits, fmt in MX_AT.items():
            codes, scales = buffers(p, bits)
            mcodes, mscales = mx_buffers(p, fmt)
            for resid in (False, True):
                r = timed(args.calls, {
                    "dlsim_mx_quantize": lambda s: _native.mx_quantize(s["x"], mcodes, mscales, fmt, s["e"] if resid else None),
                    "dlsim_quantize": lambda s: _native.quantize(s["x"], codes, scales, bits, "nearest", 1, s["e"] if resid else None),
                    "torch": lambda s: torch_mx_quantize(s["x"], s["e"] if resid else None, fmt)}, sets)
                used = [sets[0]["x"], mcodes] + ([sets[0]["e"]] if resid else [])
                ours = r["dlsim_mx_quantize"]["median_us"]
                emit({"leg": "mx_quantize", "dtype": str(dt), "P": p, "format": fmt, "bits": bits, "residual": resid,
                      "kernel": _native.mx_kernel_name("quantize", used, p, dt), **r,
                      "ratio_to_dlsim_quantize": ours / r["dlsim_quantize"]["median_us"],
                      "ratio_to_torch": ours / r["torch"]["median_us"]})
        del sets
        torch.cuda.empty_cache()


def mx_mix_sets(dt, p, m, bits, fmt, with_dense):
    """Buffer sets of one mixing comparison: self, m neighbours in MX and in the integer format, and
    (with_dense) the MX neighbours decoded, which the dense yardstick reads."""
    esz = torch.empty((), dtype=dt).element_size()
    sets = []
    for _ in range(nsets(((m + 1) * p * esz) if with_dense else (p * esz + m * p * bits // 8))):
        own = (torch.randn(p, device=DEV) * 0.05).to(dt)
        mx_rows, int_rows = [], []
        for _ in range(m):
            x = (torch.randn(p, device=DEV) * 0.05).to(dt)
            mx_rows.append(_native.mx_quantize(x, *mx_buffers(p, fmt), fmt) + (fmt,))
            int_rows.append(_native.quantize(x, *buffers(p, bits), bits) + (bits,))
        dense = [own] + [_native.mx_dequantize(c, s, fmt, torch.empty_like(own)) for c, s, _ in mx_rows] if with_dense else None
        sets.append({"own": own, "mx": mx_rows, "int": int_rows, "dense": dense, "out": torch.empty_like(own)})
    return sets


def leg_mx_mix(args):
    n = 8
    w = _native.fp32_weights([1.0 / n] * n)
    for dt, p in SHAPES[:1 if args.skip_bf16 else 2]:
        for bits, fmt in MX_AT.items():
            sets = mx_mix_sets(dt, p, n - 1, bits, fmt, True)
            scratch = [torch.empty(p, dtype=dt, device=DEV) for _ in range(n - 1)]

            def decode_then_reduce(s):
                for (c, sc, _), row in zip(s["mx"], scratch):
                    _native.mx_dequantize(c, sc, fmt, row)
                _native.wreduce([s["own"]] + scratch, w, s["out"])
            r = timed(args.calls, {"dlsim_mx_wreduce": lambda s: _native.mx_wreduce(s["own"], s["mx"], w, s["out"]),
                                   "dlsim_quant_wreduce": lambda s: _native.quant_wreduce(s["own"], s["int"], w, s["out"]),
                                   "dlsim_wreduce_dense": lambda s: _native.wreduce(s["dense"], w, s["out"]),
                                   "mx_dequantize_x7_plus_wreduce": decode_then_reduce}, sets)
            ours = r["dlsim_mx_wreduce"]["median_us"]
            emit({"leg": "mx_mix", "dtype": str(dt), "P": p, "n": n, "format": fmt, "bits": bits, **r,
                  "ratio_to_quant_wreduce": ours / r["dlsim_quant_wreduce"]["median_us"],
                  "ratio_to_dense": ours / r["dlsim_wreduce_dense"]["median_us"],
                  "ratio_to_decode_plus_dense": ours / r["mx_dequantize_x7_plus_wreduce"]["median_us"]})
            del sets, scratch
            torch.cuda.empty_cache()


def leg_mx_fanin(args):
    n = 16
    w = _native.fp32_weights([1.0 / n] * n)
    dt, p = SHAPES[0]
    for bits, fmt in MX_AT.items():
        sets = mx_mix_sets(dt, p, n - 1, bits, fmt, False)
        r = timed(args.calls, {"dlsim_mx_wreduce": lambda s: _native.mx_wreduce(s["own"], s["mx"], w, s["out"]),
                               "dlsim_quant_wreduce": lambda s: _native.quant_wreduce(s["own"], s["int"], w, s["out"])}, sets)
        emit({"leg": "mx_fanin", "dtype": str(dt), "P": p, "n": n, "format": fmt, "bits": bits, **r,
              "ratio_to_quant_wreduce": r["dlsim_mx_wreduce"]["median_us"] / r["dlsim_quant_wreduce"]["median_us"]})
        del sets
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--legs", help="default: quantize,mix,round; with --mx: mx_quantize,mx_mix,mx_fanin")
    ap.add_argument("--mx", action="store_true", help="measure MX sharing (DESIGN.md §8t)")
    ap.add_argument("--skip-bf16", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_quant.py measures on a GPU"
    legs = args.legs or ("mx_quantize,mx_mix,mx_fanin" if args.mx else "quantize,mix,round")
    for leg in legs.split(","):
        {"quantize": leg_quantize, "mix": leg_mix, "round": leg_round, "mx_quantize": leg_mx_quantize,
         "mx_mix": leg_mx_mix, "mx_fanin": leg_mx_fanin}[leg](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in LINES)


if __name__ == "__main__":
    main()
