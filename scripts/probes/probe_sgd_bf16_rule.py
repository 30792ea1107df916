"""How PyTorch's CPU `a.add(b, alpha=s)` rounds, the rule csrc/sgd_kernels.hpp
reproduces. CPU only; prints mismatch counts of an emulation
against torch, at 1, 4 and 8 threads.

  fp64   exact rational arithmetic (fractions.Fraction) on a sample: a fused
         double fma matches everywhere, product-then-sum does not
  bf16   the scalar is rounded to bf16 (through fp32). Each thread's range of
         the tensor (TensorIterator: serial below 32768 elements, else
         min(threads, ceil(n / 32768)) ranges of ceil(n / ranges)) is taken 32
         elements at a time by the vector loop, which computes in fp32 and
         rounds the result to bf16 once; the remaining len mod 32 elements go
         through c10::BFloat16 arithmetic, which rounds the product to bf16 too.
         So the result depends on the thread count, like fp16's.

    python scripts/probes/probe_sgd_bf16_rule.py
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch

GRAIN, VEC = 32768, 32


def bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def bf(x32):
    return torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(torch.bfloat16)


def rb(x32):
    return bf(x32).float().numpy()


def scalar_mask(n, threads):
    m = np.zeros(n, bool)
    if n < GRAIN or threads == 1:
        chunk = max(n, 1)
    else:
        chunk = -(-n // min(threads, -(-n // GRAIN)))
    for b in range(0, n, chunk):
        ln = min(n, b + chunk) - b
        m[b + ln - ln % VEC:b + ln] = True
    return m


def emulate_add(a, b, alpha, threads):
    al = torch.tensor(alpha, dtype=torch.float64).to(torch.float32).to(torch.bfloat16).float().item()
    A, B = a.float().numpy(), b.float().numpy()
    with np.errstate(all="ignore"):
        # the product of two bf16 values is exact in fp32 (and in double), the sum exact in double
        vec = rb((np.float64(al) * B.astype(np.float64) + A.astype(np.float64)).astype(np.float32))
        sca = rb(A + rb(np.float32(al) * B))
    return np.where(scalar_mask(len(A), threads), sca, vec)


def main():
    rng = np.random.default_rng(3)
    n = 4001
    p, g = rng.standard_normal(n), rng.standard_normal(n)
    for lr, wd in ((0.1, 5e-4), (0.003, 0.0), (1 / 3, 1e-2)):
        tp, tg = torch.from_numpy(p.copy()), torch.from_numpy(g.copy())
        g2 = (tg.add(tp, alpha=wd) if wd != 0 else tg).numpy()
        out = tp.add(torch.from_numpy(g2), alpha=-lr).numpy()
        fused = unfused = 0
        for j in range(n):
            if wd != 0:
                fused += float(Fraction(wd) * Fraction(float(p[j])) + Fraction(float(g[j]))) != g2[j]
                unfused += (np.float64(wd) * p[j]) + g[j] != g2[j]
            fused += float(Fraction(-lr) * Fraction(float(g2[j])) + Fraction(float(p[j]))) != out[j]
            unfused += (np.float64(-lr) * g2[j]) + p[j] != out[j]
        print(f"fp64 lr={lr:.4g} wd={wd:.4g}: fused fma mismatches {fused}, unfused {unfused} of {n}")
    total = 0
    for threads in (1, 4, 8):
        torch.set_num_threads(threads)
        for n in (1, 3, 5, 31, 32, 33, 63, 64, 65, 1025, 4095, 32767, 32768, 32769, 85354, 131073, 1000003):
            p, g = bf(rng.standard_normal(n) * 0.05), bf(rng.standard_normal(n) * 0.01)
            for lr, wd in ((0.1, 0.1), (0.05, 5e-4)):
                g2 = g.add(p, alpha=wd)
                out = p.add(g2, alpha=-lr)
                bad = int((bits(bf(emulate_add(g, p, wd, threads))) != bits(g2)).sum())
                bad += int((bits(bf(emulate_add(p, g2, -lr, threads))) != bits(out)).sum())
                one_rule = int((bits(bf(emulate_add(p, g2, -lr, 1)[:n - n % VEC])) != bits(out)[:n - n % VEC]).sum())
                total += bad
                if bad:
                    print(f"bf16 threads={threads} n={n} lr={lr} wd={wd}: {bad} mismatches")
                if threads > 1 and one_rule and n >= GRAIN:
                    print(f"bf16 threads={threads} n={n}: {one_rule} elements differ from the 1-thread layout")
    print("bf16: total mismatches of the vector/scalar rule", total)
    for n in (85354, 1000003):
        p = torch.from_numpy((rng.standard_normal(n) * 0.05).astype(np.float32))
        g = torch.from_numpy((rng.standard_normal(n) * 0.01).astype(np.float32))
        outs = []
        for threads in (1, 4, 8):
            torch.set_num_threads(threads)
            outs.append(p.add(g.add(p, alpha=5e-4), alpha=-0.1))
        print(f"fp32 n={n}: elements that change with the thread count", int((outs[0] != outs[1]).sum()),
              int((outs[0] != outs[2]).sum()))


if __name__ == "__main__":
    main()
