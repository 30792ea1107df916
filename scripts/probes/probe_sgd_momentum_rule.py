"""How PyTorch's CPU torch.optim.SGD (momentum > 0, the single-tensor path)
rounds each step, the rule csrc/sgdm_kernels.hpp reproduces.
CPU only; prints mismatch counts of an emulation against torch over three
steps from a fresh optimizer, the state resynchronised after each step.

  g'  = grad.add(param, alpha=wd)           one fused multiply-add (§8h)
  buf = buf.mul_(momentum).add_(g', alpha=1)  a rounded product, then a plain add
  param.add_(buf, alpha=-lr)                one fused multiply-add (§8h)

  fp32   scalars rounded to fp32; a fused buffer update is counted as well
  fp64   exact rational arithmetic (fractions.Fraction) on a sample
  bf16   mul_'s scalar stays fp32: product in fp32 rounded to bf16, sum in fp32
         rounded to bf16; momentum rounded to bf16 first is counted as well.
         The alpha adds keep §8h's vector-body / scalar-tail layout.

    python scripts/probes/probe_sgd_momentum_rule.py

`emulate_step` is also the emulation tests/test_sgdm_cpu.py holds the
fixtures against.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

GRAIN, VEC = 32768, 32


# ---- number formats ----------------------------------------------------------

def bf16_to_f32(u16):
    return (np.ascontiguousarray(u16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x):
    """Round to nearest even, as bf16 bits (NaN -> 0x7fc0)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7fc0), r)


def rb(x):
    """fp32 values rounded to bf16, as fp32."""
    return bf16_to_f32(f32_to_bf16(x))


def fma32(a, b, c):
    """fp32 fma(a, b, c), exactly: the product is exact in double, the sum is
    rounded to odd in double (53 >= 2 * 24 + 2 bits), then to fp32."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        prod = a * b
        s = prod + c
        bb = s - prod
        err = (prod - (s - bb)) + (c - bb)
        fix = np.isfinite(err) & (err != 0) & np.isfinite(s) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix & (err > 0), np.nextafter(s, np.inf), np.where(fix & (err < 0), np.nextafter(s, -np.inf), s))
        return s.astype(np.float32)


def fma64(a, b, c):
    """double fma(a, b, c) by exact rational arithmetic (finite inputs)."""
    out = np.empty(len(b), np.float64)
    for j in range(len(b)):
        out[j] = float(Fraction(float(a)) * Fraction(float(b[j])) + Fraction(float(c[j])))
    return out


def scalar_mask(n, threads):
    """Elements ATen's scalar loop takes (the last len mod 32 of each thread's range)."""
    m = np.zeros(n, bool)
    if n < GRAIN or threads == 1:
        chunk = max(n, 1)
    else:
        chunk = -(-n // min(threads, -(-n // GRAIN)))
    for b in range(0, n, chunk):
        ln = min(n, b + chunk) - b
        m[b + ln - ln % VEC:b + ln] = True
    return m


def _bf16_alpha_add(a, b, alpha, threads):
    """a + alpha * b on bf16 values held as fp32 (§8h): alpha rounded to bf16."""
    al = rb(np.float32(alpha)).reshape(-1)[0]
    with np.errstate(all="ignore"):
        vec = rb((np.float64(al) * b.astype(np.float64) + a.astype(np.float64)).astype(np.float32))
        sca = rb(a + rb(al * b))
    return np.where(scalar_mask(len(a), threads), sca, vec)


# ---- the step ----------------------------------------------------------------

def emulate_step(dtype, p, g, buf, lr, momentum, wd, threads=4, fused_buffer=False, bf16_momentum=False):
    """One step on flat arrays in storage form (bf16 as uint16 bits); `buf`
    None is the first step. Returns (param, buf) after the step. The two
    switches emulate the WRONG rules, for the counts the probe prints."""
    with np.errstate(all="ignore"):
        if dtype == "f32":
            nlr, m, w = np.float32(-lr), np.float32(momentum), np.float32(wd)
            g2 = fma32(w, p, g) if wd != 0 else g.copy()
            if buf is None:
                b2 = g2
            else:
                b2 = fma32(m, buf, g2) if fused_buffer else (m * buf).astype(np.float32) + g2
            return fma32(nlr, b2, p), b2
        if dtype == "f64":
            g2 = fma64(wd, p, g) if wd != 0 else g.copy()
            if buf is None:
                b2 = g2
            else:
                b2 = fma64(momentum, buf, g2) if fused_buffer else np.float64(momentum) * buf + g2
            return fma64(-lr, b2, p), b2
        P, G = bf16_to_f32(p), bf16_to_f32(g)
        g2 = _bf16_alpha_add(G, P, wd, threads) if wd != 0 else G
        if buf is None:
            b2 = g2
        else:
            m = rb(np.float32(momentum)).reshape(-1)[0] if bf16_momentum else np.float32(momentum)
            b2 = rb(rb(m * bf16_to_f32(buf)) + g2)
        return f32_to_bf16(_bf16_alpha_add(P, b2, -lr, threads)), f32_to_bf16(b2)


def _same(a, b):
    """Mismatching elements, any NaN equal to any NaN."""
    if a.dtype == np.uint16:
        fa, fb = bf16_to_f32(a), bf16_to_f32(b)
    else:
        fa, fb = a, b
    ia, ib = a.view(f"u{a.itemsize}"), b.view(f"u{b.itemsize}")
    return int(((ia != ib) & ~(np.isnan(fa) & np.isnan(fb))).sum())


def main():
    import torch

    def to_t(a, dtype):
        if dtype == "bf16":
            return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
        return torch.from_numpy(a.copy())

    def to_np(t, dtype):
        t = t.detach().reshape(-1)
        if dtype == "bf16":
            return t.view(torch.int16).numpy().view(np.uint16).copy()
        return t.numpy().copy()

    def draw(rng, n, dtype, scale):
        x = rng.standard_normal(n) * scale
        if dtype == "f64":
            return x
        x = x.astype(np.float32)
        return f32_to_bf16(x) if dtype == "bf16" else x

    print(f"torch {torch.__version__}, {torch.backends.cpu.get_cpu_capability()}")
    rng = np.random.default_rng(5)
    sizes = {"f32": (1, 10, 31, 33, 100, 4097, 32768, 85354, 200003, 1000003),
             "bf16": (1, 10, 31, 33, 100, 4097, 32767, 32768, 32801, 85354, 131077, 200003),
             "f64": (1, 33, 2500)}
    for dtype in ("f32", "bf16", "f64"):
        for threads in (1, 4):
            torch.set_num_threads(threads)
            tot = {"rule": 0, "fused buffer update": 0, "momentum rounded to bf16": 0}
            elems = 0
            for n in sizes[dtype]:
                for lr, mom, wd in ((0.1, 0.9, 5e-4), (0.05, 0.9, 0.0), (1 / 3, 0.37, 1e-2)):
                    q = torch.nn.Parameter(to_t(draw(rng, n, dtype, 0.05), dtype))
                    opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd, foreach=False)
                    buf = None
                    for _ in range(3):
                        g = draw(rng, n, dtype, 0.01)
                        p0 = to_np(q, dtype)
                        q.grad = to_t(g, dtype)
                        opt.step()
                        p1, b1 = to_np(q, dtype), to_np(opt.state[q]["momentum_buffer"], dtype)
                        ep, eb = emulate_step(dtype, p0, g, buf, lr, mom, wd, threads)
                        tot["rule"] += _same(ep, p1) + _same(eb, b1)
                        if buf is not None:
                            elems += n
                            if dtype != "bf16":
                                tot["fused buffer update"] += _same(
                                    emulate_step(dtype, p0, g, buf, lr, mom, wd, threads, fused_buffer=True)[1], b1)
                            else:
                                tot["momentum rounded to bf16"] += _same(
                                    emulate_step(dtype, p0, g, buf, lr, mom, wd, threads, bf16_momentum=True)[1], b1)
                        buf = b1  # resynchronised
            wrong = "fused buffer update" if dtype != "bf16" else "momentum rounded to bf16"
            print(f"{dtype} threads={threads}: rule mismatches {tot['rule']} (param + buffer, 3 steps, "
                  f"{len(sizes[dtype])} sizes x 3 settings); {wrong}: {tot[wrong]} of {elems} buffer elements")


if __name__ == "__main__":
    main()
