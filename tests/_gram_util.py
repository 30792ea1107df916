"""TEST INFRASTRUCTURE for the Gram distance kernel (tests/test_gram_cpu.py,
tests/test_gpu_gram.py): the contract's error bound and the check of one
matrix against the longdouble oracle of tests/_krum_util.py."""
from __future__ import annotations

import numpy as np

import _edge_util as eu
import _krum_util as ku


def centred_sums(rows, dtype: str):
    """(S, bad): S[i] = sum_e (x_i[e] - c[e])^2 in longdouble around the
    sanitised centre c = x_0 with its non-finite elements at 0; bad[i]: row i
    holds a non-finite element (its S is not used)."""
    x = np.stack([eu.decode(np.asarray(r).reshape(-1), dtype) for r in rows])
    bad = ~np.isfinite(x).all(axis=1)
    c = np.where(np.isfinite(x[0]), x[0], 0.0).astype(np.longdouble)
    with np.errstate(all="ignore"):
        d = np.where(np.isfinite(x), x, 0.0).astype(np.longdouble) - c
        return np.einsum("ie,ie->i", d, d), bad


def entry_bounds(S, n_elems: int) -> np.ndarray:
    """The contract's absolute bound per entry: 2 (P + 16) 2^-53 (S_i + S_j)."""
    return 2 * (n_elems + 16) * ku.U * (S[:, None] + S[None, :])


def gram_problems(got, rows, dtype: str, want=None):
    """What is wrong with the n x n float64 matrix `got`: bitwise symmetry, a
    +0.0 diagonal, NaN in exactly the off-diagonal entries of rows with a
    non-finite element, every other entry non-negative and within the bound of
    the oracle `want` (default: sqdist_oracle(rows)). Returns (problems, the
    largest err / bound)."""
    got = np.asarray(got, dtype=np.float64)
    n, p = got.shape[0], np.asarray(rows[0]).size
    want = ku.sqdist_oracle(rows, dtype) if want is None else want
    S, bad = centred_sums(rows, dtype)
    bits, problems = got.view(np.uint64), []
    if not np.array_equal(bits, bits.T):
        problems.append("not bitwise symmetric")
    if bits.diagonal().any():
        problems.append(f"diagonal is not +0.0: {got.diagonal()}")
    nan_want = (bad[:, None] | bad[None, :]) & ~np.eye(n, dtype=bool)
    if not np.array_equal(np.isnan(got), nan_want):
        problems.append(f"NaN entries {np.argwhere(np.isnan(got)).tolist()}, flagged rows {np.flatnonzero(bad).tolist()}")
    fin = ~nan_want & ~np.isnan(got)
    if np.signbit(got[fin]).any():
        problems.append("a negative entry or -0.0")
    err = np.abs(got[fin].astype(np.longdouble) - want[fin])
    lim = entry_bounds(np.where(bad, 0, S), p)[fin]
    ratio = np.where(err > 0, err / np.where(lim > 0, lim, 1), 0.0)
    ratio = np.where((err > 0) & (lim == 0), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        problems.append(f"an entry off by {worst:.3f} x the bound 2 (P + 16) 2^-53 (S_i + S_j), P = {p}")
    return problems, worst


def cancelling_rows(n: int, p: int, seed: int = 5):
    """fp32 rows 1e3 base + 1e-3 noise: norms 10^6 times the distances."""
    rng = np.random.default_rng(seed)
    return eu.encode(1e3 * rng.standard_normal(p)[None, :] + 1e-3 * rng.standard_normal((n, p)), "f32").reshape(n, p)
