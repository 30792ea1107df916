"""CPU restatement of the order-statistic aggregators' contract,
shared by tests/test_robust_cpu.py, tests/test_gpu_robust.py and the `robust`
leg of scripts/fuzz_parity.py. numpy only: integer keys, a stable argsort on the
keys, sequential adds, one division, and for bf16 / fp16 a final rounding
through torch's `.to(dtype)`.

Per element, over its n values: sort ascending in the total order
-Inf < ... < -0.0 < +0.0 < ... < +Inf < NaN (all NaNs equal), then
acc = s[lo]; acc = acc + s[j] for j = lo+1 .. hi-1; result = acc / (hi - lo);
a NaN result is the canonical quiet NaN of the dtype.
"""
from __future__ import annotations

import numpy as np
import torch

DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
# (unsigned view, bits of +Inf, canonical quiet NaN)
_FMT = {
    torch.float32: (np.uint32, 0x7F800000, 0x7FC00000),
    torch.float64: (np.uint64, 0x7FF0000000000000, 0x7FF8000000000000),
    torch.bfloat16: (np.uint16, 0x7F80, 0x7FC0),
    torch.float16: (np.uint16, 0x7C00, 0x7E00),
}
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16,
             torch.float16: torch.int16}


def bits_of(t: torch.Tensor) -> np.ndarray:
    """The storage bits of a floating tensor as an unsigned numpy array."""
    t = t.detach().cpu().contiguous()
    return t.view(_INT_VIEW[t.dtype]).numpy().view(_FMT[t.dtype][0]).copy()


def from_bits(b: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    u = np.ascontiguousarray(b, dtype=_FMT[dtype][0])
    signed = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}[_FMT[dtype][0]]
    return torch.from_numpy(u.view(signed).copy()).view(dtype)


def keys_of(b: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """Unsigned keys whose integer order is the contract's total order."""
    ut, inf, _ = _FMT[dtype]
    nbits = np.dtype(ut).itemsize * 8
    sign = ut(1 << (nbits - 1))
    allones = ut((1 << nbits) - 1)
    neg = (b & sign) != 0
    k = np.where(neg, b ^ allones, b | sign)
    nan = (b & ut(int(sign) - 1)) > ut(inf)
    return np.where(nan, ut(int(allones) - 1), k).astype(ut)


def _widen(b: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    if dtype == torch.float32:
        return b.view(np.float32)
    if dtype == torch.float64:
        return b.view(np.float64)
    if dtype == torch.bfloat16:
        return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def sorted_bits(xs, dtype: torch.dtype) -> np.ndarray:
    """(n, P) storage bits, each column sorted ascending in the total order."""
    b = np.stack([bits_of(x).reshape(-1) for x in xs])
    order = np.argsort(keys_of(b, dtype), axis=0, kind="stable")
    return np.take_along_axis(b, order, axis=0)


def window_mean(xs, lo: int, hi: int) -> torch.Tensor:
    """The contract on a list of n same-shaped CPU tensors of one dtype."""
    return window_mean_sorted(sorted_bits(xs, xs[0].dtype), xs[0].dtype, lo, hi).reshape(xs[0].shape)


def window_mean_sorted(sb: np.ndarray, dtype: torch.dtype, lo: int, hi: int) -> torch.Tensor:
    """The same from sorted_bits' result (several windows over one sort); flat."""
    assert 0 <= lo < hi <= sb.shape[0]
    ut, _, qnan = _FMT[dtype]
    s = _widen(sb, dtype)
    with np.errstate(all="ignore"):
        acc = s[lo].copy()
        for j in range(lo + 1, hi):
            acc = acc + s[j]
        res = acc / acc.dtype.type(hi - lo)
    assert res.dtype == (np.float64 if dtype == torch.float64 else np.float32)
    nan = np.isnan(res)
    out = torch.from_numpy(res.copy())
    if dtype in (torch.bfloat16, torch.float16):
        out = out.to(dtype)  # one rounding, nearest-even
    ob = bits_of(out)
    ob[nan] = ut(qnan)
    return from_bits(ob, dtype)


def median(xs) -> torch.Tensor:
    lo = (len(xs) - 1) // 2
    return window_mean(xs, lo, lo + 1)


def trimmed_mean(xs, trim: int) -> torch.Tensor:
    return window_mean(xs, trim, len(xs) - trim)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits_of(a), bits_of(b))


def diff_report(got: torch.Tensor, exp: torch.Tensor, limit: int = 5) -> str:
    g, e = bits_of(got).reshape(-1), bits_of(exp).reshape(-1)
    bad = np.nonzero(g != e)[0]
    return f"{bad.size} of {g.size} elements differ; first: " + ", ".join(
        f"[{i}] got {int(g[i]):#x} want {int(e[i]):#x}" for i in bad[:limit])


# ---- inputs -------------------------------------------------------------------------
def special_bits(dtype: torch.dtype) -> np.ndarray:
    """One value of every class: +-0, +-subnormal, +-finite, +-Inf, NaN with
    both signs and a non-canonical payload."""
    ut, inf, qnan = _FMT[dtype]
    nbits = np.dtype(ut).itemsize * 8
    sign = 1 << (nbits - 1)
    one = bits_of(torch.ones(1, dtype=dtype))[0]
    big = int(inf) - 1  # the largest finite value
    v = [0, sign, 1, sign | 1, 3, sign | 3, int(one), sign | int(one), int(one) + 5, sign | (int(one) + 5), big,
         sign | big, int(inf), sign | int(inf), int(qnan), sign | int(qnan), int(inf) + 1, sign | (int(inf) + 5)]
    return np.array(v, dtype=ut)


def random_rows(dtype: torch.dtype, n: int, p: int, seed: int, special_frac: float = 0.15):
    """n rows of p elements: unit normals (ties included: values rounded to a
    coarse grid in places) with a fraction of specials scattered in."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p))
    coarse = rng.random((n, p)) < 0.2
    x = np.where(coarse, np.round(x * 2) / 2, x)  # ties, exact zeros
    t = torch.from_numpy(x).to(dtype)
    b = bits_of(t)
    sp = special_bits(dtype)
    mask = rng.random((n, p)) < special_frac
    b[mask] = sp[rng.integers(0, sp.size, size=int(mask.sum()))]
    return [from_bits(b[i], dtype) for i in range(n)]


def special_rows(dtype: torch.dtype, n: int):
    """n rows in which every special value visits every row position: column
    block c holds special c in row r and finite fillers elsewhere, for every
    r; then columns that are all one special value; then columns ascending
    and descending across the row index."""
    ut = _FMT[dtype][0]
    sp = special_bits(dtype)
    fill = bits_of(torch.linspace(-2.0, 2.0, n, dtype=torch.float64).to(dtype))
    cols = []
    for c in range(sp.size):
        for r in range(n):
            col = np.roll(fill, r + c).copy()
            col[r] = sp[c]
            cols.append(col)
            col2 = col.copy()  # the same special in a second row too
            col2[(r + 1) % n] = sp[c]
            cols.append(col2)
    for c in range(sp.size):
        cols.append(np.full(n, sp[c], dtype=ut))  # all equal
    asc = bits_of(torch.arange(n, dtype=torch.float64).sub(n / 2).to(dtype))
    cols += [asc, asc[::-1].copy()]
    # two NaNs, two Infs and zeros of both signs in one column
    if n >= 6:
        col = fill.copy()
        col[:6] = [sp[14], sp[15], sp[12], sp[13], sp[0], sp[1]]
        cols.append(col)
    b = np.stack(cols, axis=1).astype(ut)
    return [from_bits(b[i], dtype) for i in range(n)]


def windows(n: int):
    """The windows the tests sweep: the median, trim 0 and 1, and the widest
    trims (m = 1 and m = 2 values left)."""
    lo = (n - 1) // 2
    w = {(lo, lo + 1), (0, n)}
    for b in (1, (n - 1) // 2, (n - 2) // 2):
        if b >= 0 and n - 2 * b >= 1:
            w.add((b, n - b))
    return sorted(w)
