"""TEST INFRASTRUCTURE for the pairwise-distance kernel and the Krum plugins
(tests/test_krum_cpu.py, tests/test_gpu_krum.py): the longdouble distance
oracle, the value-class function, a restatement of Krum's scores and
selection written independently of gradient_aggregation/krum.py, and
generators of models whose selection is well separated.

Storage convention: _edge_util's (a row is a numpy array of float32, float64
or uint16 bit patterns for "bf16" / "f16").
"""
from __future__ import annotations

import numpy as np
import torch

import _edge_util as eu
from _sgd_util import Net

DTYPES = eu.DTYPES
U = 2.0 ** -53


def bound(n_elems: int) -> float:
    """Relative error bound of a finite entry: three roundings per term and
    n_elems - 1 additions of non-negative terms, 8 units of slack."""
    return (n_elems + 8) * U


def sqdist_oracle(rows, dtype: str) -> np.ndarray:
    """(n, n) numpy.longdouble: terms and sums in longdouble (own error below
    n_elems * 2^-63 relative). Non-finite classes come out as IEEE gives them."""
    x = [eu.decode(np.asarray(r).reshape(-1), dtype) for r in rows]
    n = len(x)
    out = np.zeros((n, n), dtype=np.longdouble)
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(i + 1, n):
                d = np.subtract(x[i], x[j], dtype=np.longdouble)
                out[i, j] = out[j, i] = np.dot(d, d)
    return out


def add_oracles(parts) -> np.ndarray:
    """Oracle matrices of consecutive pieces, added in that order."""
    with np.errstate(all="ignore"):
        acc = parts[0].copy()
        for p in parts[1:]:
            acc = acc + p
    return acc


def value_class(a) -> np.ndarray:
    """Per entry 0 (finite), 1 (+Inf or -Inf) or 2 (NaN)."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), 1, 0))


def matrix_problems(got, want, n_elems: int):
    """What is wrong with the n x n float64 matrix `got` against the
    longdouble oracle `want`: bitwise symmetry, a +0.0 diagonal, the exact
    value class of every entry, the bound on every finite entry. Returns
    (list of problems, largest err / bound over the finite entries)."""
    got = np.asarray(got, dtype=np.float64)
    n = got.shape[0]
    bits = got.view(np.uint64)
    problems = []
    if not np.array_equal(bits, bits.T):
        problems.append("not bitwise symmetric")
    if np.any(bits[np.arange(n), np.arange(n)] != 0):
        problems.append(f"diagonal is not +0.0: {got.diagonal()}")
    cg, cw = value_class(got), value_class(want)
    if not np.array_equal(cg, cw):
        i, j = np.argwhere(cg != cw)[0]
        problems.append(f"value class differs at [{i}][{j}]: got {got[i, j]}, oracle {want[i, j]}")
    worst = 0.0
    fin = (cw == 0) & (cg == 0)
    if fin.any():
        w = want[fin]
        err = np.abs(got[fin].astype(np.longdouble) - w)
        rel = np.where(w > 0, err / np.where(w > 0, w, 1), np.where(err > 0, np.inf, 0))
        worst = float(rel.max() / bound(n_elems))
        if worst > 1.0:
            problems.append(f"finite entry off by {worst:.3f} x the bound ((n_elems + 8) * 2^-53, n_elems = {n_elems})")
    return problems, worst


# ---- Krum's rule, restated ---------------------------------------------------------
def ref_scores(d2, f: int):
    a = np.array(d2, dtype=np.float64)
    n = a.shape[0]
    a = np.where(np.isfinite(a), a, np.inf)
    scores = []
    for i in range(n):
        nearest = np.sort(np.delete(a[i], i))[:n - f - 2]
        s = 0.0
        for v in nearest.tolist():
            s = s + v
        scores.append(s)
    return scores


def ref_select(d2, f: int, m: int):
    """Indices of the m best by (score, index), ascending. A stable argsort
    keeps equal scores (all-Inf ones too) in index order."""
    order = np.argsort(np.array(ref_scores(d2, f)), kind="stable")
    return sorted(int(i) for i in order[:m])


# ---- well-separated inputs ---------------------------------------------------------------
def separated_models(n: int, f: int, numel: int, dtype: str, seed: int, ms=None, nan_row: bool = False,
                     inf_row: bool = False, byz=None):
    """(storage rows (n, numel), Byzantine indices, oracle matrix). Honest rows
    are base + noise of scale 1e-2, the f Byzantine rows base + an offset of
    scale 1; with nan_row / inf_row the first / last Byzantine row is all-NaN /
    all-Inf. Asserts that for every m of `ms` (default 1, 2, n - f) the
    oracle's gap between the m-th and the (m+1)-th ranked score exceeds
    1e6 x bound(numel) x the largest finite score: the oracle's selection and
    the selection from any in-bound matrix then agree."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(numel)
    x = base[None, :] + 1e-2 * rng.standard_normal((n, numel))
    byz = sorted(int(i) for i in (rng.choice(n, size=f, replace=False) if byz is None else byz))
    assert len(byz) == f
    for i in byz:
        x[i] = base + rng.standard_normal(numel)
    if nan_row:
        x[byz[0]] = np.nan
    if inf_row:
        x[byz[-1]] = np.inf
    rows = eu.encode(x, dtype).reshape(n, numel)
    want = sqdist_oracle(rows, dtype)
    scores = np.array(ref_scores(want.astype(np.float64), f))
    ranked = np.sort(scores)
    finite = ranked[np.isfinite(ranked)]
    assert finite.size, "no finite score"
    need = 1e6 * bound(numel) * finite.max()
    for m in ((1, 2, n - f) if ms is None else ms):
        if m < n:
            gap = ranked[m] - ranked[m - 1] if np.isfinite(ranked[m - 1]) else 0.0
            assert gap > need, f"n={n} f={f} m={m} seed={seed}: score gap {gap} <= {need}"
    return rows, byz, want


GPU_PLUGIN_CONFIGS = ((5, 1), (8, 2), (17, 3), (32, 8))  # (n, f) of the plugin tests
PLUGIN_SHAPES = ([37, 11], [129], [5, 3, 3], [1])  # 582 elements, an odd size per tensor


def plugin_case(n: int, f: int, dtype: str = "f32", shapes=PLUGIN_SHAPES, special: bool = False, byz=None):
    """separated_models for the plugin tests (the CPU suite asserts the
    separation of exactly these), and the rows as CPU models."""
    numel = sum(int(np.prod(s)) for s in shapes)
    rows, byz, want = separated_models(n, f, numel, dtype, seed=4000 + 10 * n + f, nan_row=special, inf_row=special,
                                       byz=byz)
    return rows, byz, want, [model_of(r, shapes, dtype) for r in rows]


def model_of(row, shapes, dtype: str, make=None) -> torch.nn.Module:
    """A Net (or make()) whose parameters hold the storage row, in order."""
    m = Net(shapes, dtype) if make is None else make()
    t = eu.to_torch(np.asarray(row), dtype)
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(t[off:off + p.numel()].reshape(p.shape))
            off += p.numel()
    assert off == t.numel()
    return m


def flat_bits(model) -> np.ndarray:
    """All parameters of a model as one array of bit patterns (per dtype group
    order does not matter to the callers: same-architecture models only)."""
    return np.concatenate([p.detach().cpu().contiguous().reshape(-1).view(
        {2: torch.int16, 4: torch.int32, 8: torch.int64}[p.element_size()]).numpy().astype(np.int64)
        for p in model.parameters()])
