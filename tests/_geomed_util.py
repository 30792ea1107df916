"""TEST INFRASTRUCTURE for the fused reduce-and-measure kernel and the
geometric-median / centered-clipping plugins (tests/test_geomed_cpu.py,
tests/test_gpu_geomed.py): the longdouble distance-to-centre oracle on top of
the FedAvg oracle, a restatement of both weight rules and of a whole
trajectory written independently of gradient_aggregation/geomed.py (numpy
longdouble, vectorised), the separation check that makes a GPU trajectory
equal the oracle's by induction, and the inputs the GPU trajectory tests use.

Storage convention: _edge_util's (a row is a numpy array of float32, float64
or uint16 bit patterns for "bf16" / "f16").
"""
from __future__ import annotations

import functools
import operator

import numpy as np

import _edge_util as eu
import _krum_util as ku
from oracle import oracle as orc

LD = np.longdouble
bound = ku.bound  # (n_elems + 8) * 2^-53: three roundings per term, n_elems - 1 additions, 8 units of slack
value_class = ku.value_class

# Separation factor. A GPU d2 within bound(numel) of the oracle's moves a
# weight by at most about bound(numel) relative (the square root halves the
# error, the normalising sum adds at most as much again) plus a few double
# roundings of the host rule (< 16 * 2^-53). The issue asks for 1e6 x
# bound(numel); for the 582 elements of PLUGIN_SHAPES that is 6.5e-8 relative,
# more than the half-ulp of fp32 (3.0e-8 .. 6.0e-8 relative), which no value
# off the fp32 grid can be away from a rounding midpoint. 1e3 x is the largest
# power of ten that random inputs can meet (about 0.3 % of weights fall inside
# it; the seeds below are those where none does) and still leaves three
# decades over the perturbation reasoned above.
SEPARATION = 1e3


def storage(out, dtype: str) -> np.ndarray:
    """The oracle's result as _edge_util storage."""
    return eu.bits_of(out, dtype).view(eu._STORE[dtype])


def fold_oracle(rows, w, dtype: str) -> np.ndarray:
    """The FedAvg oracle's exact fold (storage). w: fp32 values for the three
    narrow dtypes, doubles for f64."""
    return storage(orc.wreduce([np.asarray(r) for r in rows], w, dtype), dtype)


def dist_oracle(rows, out, dtype: str) -> np.ndarray:
    """(n,) longdouble: sum_e (x_i[e] - out[e])^2, terms and sums in longdouble."""
    o = eu.decode(np.asarray(out).reshape(-1), dtype).astype(LD)
    res = np.zeros(len(rows), dtype=LD)
    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            d = eu.decode(np.asarray(r).reshape(-1), dtype).astype(LD) - o
            res[i] = np.dot(d, d)
    return res


def vector_problems(got, want, n_elems: int):
    """What is wrong with the float64 vector `got` against the longdouble
    oracle: the exact value class of every entry, the bound on every finite
    one. Returns (problems, largest err / bound over the finite entries)."""
    got = np.asarray(got, dtype=np.float64)
    problems = []
    cg, cw = value_class(got), value_class(want)
    if not np.array_equal(cg, cw):
        i = int(np.argwhere(cg != cw)[0][0])
        problems.append(f"value class differs at [{i}]: got {got[i]}, oracle {want[i]}")
    if np.any(np.signbit(got[cg == 0])):
        problems.append("a negative entry")
    worst = 0.0
    fin = (cw == 0) & (cg == 0)
    if fin.any():
        w = want[fin]
        err = np.abs(got[fin].astype(LD) - w)
        rel = np.where(w > 0, err / np.where(w > 0, w, 1), np.where(err > 0, np.inf, 0))
        worst = float(rel.max() / bound(n_elems))
        if worst > 1.0:
            problems.append(f"finite entry off by {worst:.3f} x the bound ((n_elems + 8) * 2^-53, n_elems = {n_elems})")
    return problems, worst


# ---- the weight rules, restated ------------------------------------------------------------
def seq_sum(values):
    """Left-to-right sum (numpy's own is pairwise)."""
    return functools.reduce(operator.add, list(values))


def _radius(d2):
    d2 = np.asarray(d2, dtype=LD)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(d2), np.sqrt(np.where(np.isfinite(d2), d2, 0)), np.inf)


def ref_weiszfeld(d2, alphas, nu):
    """longdouble weights (not yet rounded), or None when the iteration stops."""
    r = _radius(d2)
    a = np.asarray(alphas, dtype=LD)
    beta = np.where(np.isfinite(r), a / np.maximum(LD(nu), r), LD(0))
    total = seq_sum(beta)
    if total == 0 or not np.isfinite(total):
        return None
    return beta / total


def lower_median(values):
    v = np.sort(np.asarray(values))
    return v[(len(v) - 1) // 2]


def ref_clip(d2, alphas, tau):
    """longdouble weights [centre, peers...] (not yet rounded) and the tau used."""
    r = _radius(d2)
    a = np.asarray(alphas, dtype=LD)
    t = lower_median(r) if tau is None else LD(tau)
    with np.errstate(all="ignore"):
        c = np.where(np.isinf(r), LD(0), np.where(r == 0, LD(1), np.minimum(LD(1), t / np.where(r == 0, 1, r))))
    terms = c * a
    return np.concatenate([[LD(1) - seq_sum(terms)], terms]), t


def r32(w) -> np.ndarray:
    return np.asarray(w, dtype=LD).astype(np.float32)


def midpoint_margin(w) -> float:
    """The least relative distance of a (longdouble) weight to the two fp32
    rounding midpoints next to it, over the non-zero entries of w."""
    w = np.asarray(w, dtype=LD).reshape(-1)
    w = w[w != 0]
    f = w.astype(np.float32)
    up = (f.astype(LD) + np.nextafter(f, np.float32(np.inf)).astype(LD)) / 2
    dn = (f.astype(LD) + np.nextafter(f, np.float32(-np.inf)).astype(LD)) / 2
    return float(np.min(np.minimum(np.abs(w - up), np.abs(w - dn)) / np.abs(w)))


# ---- a whole trajectory, restated -----------------------------------------------------------
def trajectory(rows, dtype: str, alphas, rule: str, iters: int, nu: float = 1e-6, tau=None):
    """The aggregate of rule "gm" / "clip" over storage rows, every pass by the
    oracles. Returns (final storage row, passes): per pass a dict of kept
    indices, fp32 `weights`, longdouble `exact` weights (None for pass 0),
    longdouble `d2` of the inputs of that pass (clip: the centre first) and
    the `tau` used."""
    outs, passes = trajectory_groups([(rows, dtype)], alphas, rule, iters, nu=nu, tau=tau)
    return outs[0], passes


def _pass_over_groups(ins, dtypes, w):
    """One pass over a model's dtype groups: every group folded by the FedAvg
    oracle with the same weights, d2 the longdouble sum of the groups'
    dist_oracle in that (layout) order."""
    outs = [fold_oracle(x, w.astype(np.float64 if dt == "f64" else np.float32), dt) for x, dt in zip(ins, dtypes)]
    with np.errstate(all="ignore"):
        d2 = seq_sum(dist_oracle(x, o, dt) for x, o, dt in zip(ins, outs, dtypes))
    return outs, d2


def trajectory_groups(groups, alphas, rule: str, iters: int, nu: float = 1e-6, tau=None):
    """trajectory() for models of several dtype groups: `groups` is the list of
    (storage rows, dtype) of one model list in layout order, row i of every
    group belonging to model i. Returns (final storage row per group, passes);
    a model is kept when it is finite in every group."""
    dtypes = [dt for _, dt in groups]
    n = len(groups[0][0])
    assert all(len(rows) == n for rows, _ in groups)
    alphas = [float(1. / n)] * n if not alphas else [float(a) for a in alphas]
    kept = [i for i in range(n) if all(np.isfinite(eu.decode(np.asarray(rows[i]), dt)).all() for rows, dt in groups)]
    if len(kept) in (0, n):
        w = np.asarray(alphas, dtype=np.float64).astype(np.float32)
        use = list(range(n))
    else:
        total = seq_sum(alphas[i] for i in kept)
        w = np.asarray([alphas[i] / total for i in kept], dtype=np.float64).astype(np.float32)
        use = kept
    xs = [[rows[i] for i in use] for rows, _ in groups]
    outs, d2 = _pass_over_groups(xs, dtypes, w)
    passes = [dict(kept=use, weights=w, exact=None, d2=d2, tau=None)]
    if not kept:
        return outs, passes
    a = [alphas[i] for i in kept]
    if rule == "clip":
        total = seq_sum(a)
        a = [v / total for v in a]
    for _ in range(iters):
        if rule == "gm":
            exact = ref_weiszfeld(d2, a, nu)
            if exact is None:
                break
            w, t, ins = r32(exact), None, xs
        else:
            exact, t = ref_clip(d2, a, tau)
            w, ins = r32(exact), [[o] + x for o, x in zip(outs, xs)]
        outs, full = _pass_over_groups(ins, dtypes, w)
        d2 = full if rule == "gm" else full[1:]
        passes.append(dict(kept=use, weights=w, exact=exact, d2=full, tau=t))
    return outs, passes


def separation_problems(passes, rule: str, numel: int, nu: float = 1e-6):
    """Why a run whose d2 are within bound(numel) of this trajectory's might
    take other fp32 weights: a weight too close to a rounding midpoint, a
    distance too close to tau (or nu), neighbours of the median too close, a
    centre weight lost to cancellation."""
    need = SEPARATION * bound(numel)
    problems = []
    for t, (prev, p) in enumerate(zip(passes, passes[1:]), start=1):
        m = midpoint_margin(p["exact"])
        if m < need:
            problems.append(f"pass {t}: a weight is {m:.3e} relative from a midpoint (< {need:.3e})")
        d2 = prev["d2"] if (rule == "gm" or t == 1) else prev["d2"][1:]
        r = _radius(d2)
        r = r[np.isfinite(r)]
        if rule == "gm":
            if np.any(np.abs(r - nu) < need * np.maximum(r, nu)):
                problems.append(f"pass {t}: a distance within {need:.3e} of nu")
            continue
        if float(p["exact"][0]) < 1e-2:
            problems.append(f"pass {t}: centre weight {float(p['exact'][0]):.3e} < 1e-2 (cancellation in 1 - sum)")
        tau = p["tau"]
        gaps = np.sort(np.abs(r - tau) / np.maximum(r, tau))
        # under tau = None one distance is tau itself (gap 0); every other one,
        # its neighbours in the median ordering among them, must be clear
        first_other = 1 if np.any(r == tau) else 0
        if len(gaps) > first_other and gaps[first_other] < need:
            problems.append(f"pass {t}: a distance {gaps[first_other]:.3e} relative from tau (< {need:.3e})")
    return problems


# ---- the inputs of the GPU trajectory tests ---------------------------------------------------
NUMEL = sum(int(np.prod(s)) for s in ku.PLUGIN_SHAPES)
GM_ITERS, GM_NU = 3, 1e-6
CLIP_ITERS = 3
BN_SHAPES = ([5, 7], [5], [5], [5])  # _sgd_util.BnNet's parameters


def _case(rule, n, f, seed, tau=None, special=False, weighted=False, shapes=ku.PLUGIN_SHAPES, byz=None):
    return dict(rule=rule, n=n, f=f, seed=seed, tau=tau, special=special, weighted=weighted, shapes=shapes, byz=byz)


# Seeds are those whose trajectories pass separation_problems
# (tests/test_geomed_cpu.py asserts it for every case).
CASES = {
    "gm-5": _case("gm", 5, 1, 7000),
    "gm-8": _case("gm", 8, 2, 7100),
    "gm-8-weighted": _case("gm", 8, 2, 7200, weighted=True),
    "gm-17": _case("gm", 17, 3, 7300),
    "gm-32": _case("gm", 32, 8, 7400),
    "gm-8-nan-inf": _case("gm", 8, 2, 7500, special=True),
    "gm-8-bn": _case("gm", 8, 2, 7600, special=True, shapes=BN_SHAPES, byz=(0, 5)),
    "clip-5": _case("clip", 5, 1, 7700),
    "clip-8": _case("clip", 8, 2, 7800),
    "clip-8-tau": _case("clip", 8, 2, 7900, tau=8.0),
    "clip-8-weighted": _case("clip", 8, 2, 8000, weighted=True),
    "clip-17": _case("clip", 17, 3, 8100),
    "clip-17-tau": _case("clip", 17, 3, 8200, tau=8.0),
    "clip-31": _case("clip", 31, 7, 8300),
    "clip-8-nan-inf": _case("clip", 8, 2, 8401, special=True),
    "clip-8-bn": _case("clip", 8, 2, 8500, special=True, shapes=BN_SHAPES, byz=(0, 5)),
}


def dirichlet(n: int, seed: int):
    """Python-float weights summing to about 1, none tiny."""
    return [float(v) for v in np.random.default_rng(seed).dirichlet(np.full(n, 8.0))]


def case_inputs(case):
    """(fp32 storage rows (n, numel), Byzantine indices, alphas or None):
    honest rows base + 1e-2 noise, Byzantine rows base + N(0, 1); with
    `special` the first Byzantine row all-NaN and the last all-Inf."""
    numel = sum(int(np.prod(s)) for s in case["shapes"])
    rows, byz, _ = ku.separated_models(case["n"], case["f"], numel, "f32", seed=case["seed"], ms=(),
                                       nan_row=case["special"], inf_row=case["special"], byz=case["byz"])
    return rows, byz, dirichlet(case["n"], case["seed"]) if case["weighted"] else None


# ---- two dtype groups through the whole iteration ----------------------------------------------
# The `Mixed` module of the GPU tests: fp32 [33, 7] and [5], bf16 [129] and [4, 9]; layout order fp32, bf16.
MIXED_GROUPS = (("f32", 33 * 7 + 5), ("bf16", 129 + 36))
MIXED_NUMEL = sum(p for _, p in MIXED_GROUPS)
# Seeds picked as CASES' were: the first from the start value whose trajectory passes separation_problems.
MIXED_CASES = {
    "gm-mixed-6": dict(rule="gm", n=6, f=1, seed=8600, tau=None),
    "clip-mixed-6": dict(rule="clip", n=6, f=1, seed=8700, tau=None),
}


def mixed_case_trajectory(case):
    """(groups [(storage rows, dtype) ...], Byzantine indices, final row per
    group, passes) of a MIXED_CASES entry: separated_models' recipe (honest
    rows base + 1e-2 noise, Byzantine rows base + N(0, 1)) over all 401
    elements, split and rounded into the two groups."""
    rng = np.random.default_rng(case["seed"])
    n = case["n"]
    base = rng.standard_normal(MIXED_NUMEL)
    x = base[None, :] + 1e-2 * rng.standard_normal((n, MIXED_NUMEL))
    byz = sorted(int(i) for i in rng.choice(n, size=case["f"], replace=False))
    for i in byz:
        x[i] = base + rng.standard_normal(MIXED_NUMEL)
    groups, off = [], 0
    for dt, p in MIXED_GROUPS:
        groups.append((eu.encode(x[:, off:off + p], dt).reshape(n, p), dt))
        off += p
    iters = GM_ITERS if case["rule"] == "gm" else CLIP_ITERS
    outs, passes = trajectory_groups(groups, None, case["rule"], iters, nu=GM_NU, tau=case["tau"])
    return groups, byz, outs, passes


def case_trajectory(case):
    rows, byz, alphas = case_inputs(case)
    iters = GM_ITERS if case["rule"] == "gm" else CLIP_ITERS
    out, passes = trajectory(list(rows), "f32", alphas, case["rule"], iters, nu=GM_NU, tau=case["tau"])
    return rows, byz, alphas, out, passes
