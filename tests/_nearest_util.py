"""CPU restatement of the mean around the median, shared by
tests/test_nearest_cpu.py, tests/test_gpu_nearest.py,
tests/test_gpu_edges_nearest.py and the `robust` leg of scripts/fuzz_parity.py.
numpy only, on top of tests/_robust_util.py's keys, sort and value widening.

Per element, over its n values and 1 <= keep <= n: s = the values sorted in
the total order of _robust_util; m = (n-1)//2, p = s[m]; d[j] = +0.0 where
s[j] has p's key, else |s[j] - p| in the accumulator type, ranked
0 <= ... <= +Inf < NaN; the window starts as [m, m+1) and grows keep - 1
times, by the right neighbour iff it exists and the left one does not exist or
is strictly farther; acc = s[lo], acc = acc + s[j] in order, result
acc / keep, rounded and canonicalised as window_mean.

nearest_lo is the greedy walk (the restatement), closed_form_lo the count the
kernels use, brute_lo an independent per-column sort.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import _robust_util as ru


def _distances(sb: np.ndarray, dtype: torch.dtype):
    """(is-NaN flags, values) of d for (n, P) sorted bits: a NaN distance is the farthest."""
    n = sb.shape[0]
    m = (n - 1) // 2
    keys = ru.keys_of(sb, dtype)
    s = ru._widen(sb, dtype)
    with np.errstate(all="ignore"):
        d = np.abs(s - s[m][None, :])
    d[keys == keys[m][None, :]] = 0
    nan = np.isnan(d)
    return nan, np.where(nan, 0, d)


def _strictly_farther(an, av, bn, bv):
    """a ranked strictly above b: NaN above everything but NaN."""
    return (an & ~bn) | (~an & ~bn & (av > bv))


def nearest_lo(sb: np.ndarray, dtype: torch.dtype, keep: int) -> np.ndarray:
    """The first position of every column's window: the greedy walk."""
    n, p = sb.shape
    assert 1 <= keep <= n
    nan, val = _distances(sb, dtype)
    cols = np.arange(p)
    lo = np.full(p, (n - 1) // 2)
    hi = lo + 1
    for _ in range(keep - 1):
        has_l, has_r = lo > 0, hi < n
        li, ri = np.maximum(lo - 1, 0), np.minimum(hi, n - 1)
        left_farther = _strictly_farther(nan[li, cols], val[li, cols], nan[ri, cols], val[ri, cols])
        right = has_r & (~has_l | left_farther)
        assert (right | has_l).all()
        lo = lo - (~right)
        hi = hi + right
    assert (lo >= 0).all() and (hi <= n).all() and ((hi - lo) == keep).all()
    return lo


def closed_form_lo(sb: np.ndarray, dtype: torch.dtype, keep: int) -> np.ndarray:
    """lo = m - l, l = #{t in 1 .. min(m, keep-1): m+keep-t > n-1 or not d[m+keep-t] < d[m-t]}."""
    n, p = sb.shape
    m = (n - 1) // 2
    nan, val = _distances(sb, dtype)
    ell = np.zeros(p, dtype=np.int64)
    for t in range(1, min(m, keep - 1) + 1):
        r, left = m + keep - t, m - t
        if r > n - 1:
            ell += 1
        else:
            ell += ~_strictly_farther(nan[left], val[left], nan[r], val[r])
    return m - ell


def mean_from_lo(sb: np.ndarray, dtype: torch.dtype, lo: np.ndarray, keep: int) -> torch.Tensor:
    """acc = s[lo]; acc = acc + s[lo+j], j = 1 .. keep-1; acc / keep; flat."""
    ut, _, qnan = ru._FMT[dtype]
    s = ru._widen(sb, dtype)
    with np.errstate(all="ignore"):
        acc = np.take_along_axis(s, lo[None, :], axis=0)[0].copy()
        for j in range(1, keep):
            acc = acc + np.take_along_axis(s, (lo + j)[None, :], axis=0)[0]
        res = acc / acc.dtype.type(keep)
    assert res.dtype == (np.float64 if dtype == torch.float64 else np.float32)
    nan = np.isnan(res)
    out = torch.from_numpy(res.copy())
    if dtype in (torch.bfloat16, torch.float16):
        out = out.to(dtype)  # one rounding, nearest-even
    ob = ru.bits_of(out)
    ob[nan] = ut(qnan)
    return ru.from_bits(ob, dtype)


def nearest_mean_sorted(sb: np.ndarray, dtype: torch.dtype, keep: int) -> torch.Tensor:
    return mean_from_lo(sb, dtype, nearest_lo(sb, dtype, keep), keep)


def nearest_mean(xs, keep: int) -> torch.Tensor:
    """The contract on a list of n same-shaped CPU tensors of one dtype."""
    dt = xs[0].dtype
    return nearest_mean_sorted(ru.sorted_bits(xs, dt), dt, keep).reshape(xs[0].shape)


def brute_lo(col_bits, dtype: torch.dtype, keep: int) -> int:
    """One sorted column (n storage bit patterns): the positions ordered by
    (distance rank, side, steps from the median) with plain Python scalars; the
    first `keep` of them must be one run of positions, whose start is returned."""
    ut, inf, _ = ru._FMT[dtype]
    nbits = np.dtype(ut).itemsize * 8
    absmask = (1 << (nbits - 1)) - 1
    col = [int(b) for b in col_bits]
    n = len(col)
    m = (n - 1) // 2
    acc = np.float64 if dtype == torch.float64 else np.float32
    vals = ru._widen(np.array(col, dtype=ut), dtype)

    def is_nan(b):
        return (b & absmask) > inf

    def rank(j):
        if col[j] == col[m] or (is_nan(col[j]) and is_nan(col[m])):
            return (0, 0.0)
        with np.errstate(all="ignore"):
            d = abs(acc(vals[j]) - acc(vals[m]))
        return (1, 0.0) if math.isnan(d) else (0, float(d))

    order = sorted(range(n), key=lambda j: (rank(j), 0 if j <= m else 1, abs(j - m)))
    chosen = sorted(order[:keep])
    assert chosen == list(range(chosen[0], chosen[0] + keep)), "the nearest values are not one run of positions"
    return chosen[0]


def keeps(n: int):
    """The kept counts the tests sweep: 1, 2, 3, (n+1)//2, n-1, n."""
    return sorted({k for k in (1, 2, 3, (n + 1) // 2, n - 1, n) if 1 <= k <= n})
