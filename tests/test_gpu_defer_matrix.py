"""Every compiled body of the deferred-store reduce (GPU), inside guard bands
and bit for bit against the oracle. The exact fp32 policy has one fully
unrolled kernel per (fan-in 3..14, even rows per block R from 4 to 32, or to
24 from fan-in 12), each with its own load bursts, odd-input leftover and
split between preloaded and kernarg pointers; FAST, mean and an odd R take
the runtime-R form, one per fan-in. The default dispatch reaches any of them
from the size alone (dispatch.hpp defer_rows), so all of them run here:

* fan-in 3..10 at every even R from 4 to 32, exact;
* the same with the output aliasing the first and the last input, at R = 4, 24
  (bursts of two inputs) and 32 (one burst): a block stores its R rows only
  after folding all of them, which is what makes d_out == d_inputs[i] safe;
* fan-in 3..10 at R = 6 and 5 with FAST and mean, and at R = 5 exact too
  (the runtime-R form, an odd R with its duplicate row);
* fan-in 11 at even R from 14 to 32 and fan-in 12..14 at even R from 12 to 24,
  the R values defer_rows can return once they defer (from 16 rows per CU:
  one round gives 16..24, two rounds at least 12, or 14 where RMAX is 32, the
  cost model RMAX / 2 .. RMAX), exact, at the smallest size that defers.

The library reads DLSIM_DEFER_R and DLSIM_DEFER_MIN_MB once per process, so
each R runs tests/_defer_matrix_child.py in a fresh interpreter. The checks a
child must report are worked out here from the lists below: a child that runs
fewer cases fails.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

NARROW_FAN_INS = tuple(range(3, 11))
EVEN_R = tuple(range(4, 33, 2))
ALIAS_R = (4, 24, 32)
RUNTIME_R = (5, 6)  # FAST and mean run here; 5 is the runtime-R form for exact too
OP_KINDS = {"exact": ("dirichlet", "zero_in_middle"), "fast": ("dirichlet", "zero_in_middle"),
            "mean": ("dirichlet",)}
# the R values defer_rows returns for the wide fan-ins (RMAX 32 for 11, 24 from 12)
WIDE_R = {11: tuple(range(14, 33, 2)), 12: tuple(range(12, 25, 2)), 13: tuple(range(12, 25, 2)),
          14: tuple(range(12, 25, 2))}


def narrow_ops(r):
    return ["exact"] + (["alias"] if r in ALIAS_R else []) + (["fast", "mean"] if r in RUNTIME_R else [])


def wide_fan_ins(r):
    return [n for n in sorted(WIDE_R) if r in WIDE_R[n]]


def expected_checks(ops, fan_ins, kinds=OP_KINDS):
    want = {"switches_seen"}
    for n in fan_ins:
        for op in ops:
            if op == "alias":
                want |= {f"alias_first_dirichlet_n{n}", f"alias_last_dirichlet_n{n}"}
            else:
                want |= {f"defers_{op}_n{n}"} | {f"{op}_{kind}_n{n}" for kind in kinds[op]}
    return want


def run_child(case, arg, r):
    env = dict(os.environ, DLSIM_AB="1", DLSIM_DEFER_MIN_MB="0", DLSIM_DEFER_R=str(r))
    out = subprocess.run([sys.executable, os.path.join(HERE, "_defer_matrix_child.py"), case, arg], env=env,
                         capture_output=True, text=True, timeout=180)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    print(lines[-1])  # the child's checks and wall time, for a run with -rA
    return json.loads(lines[-1])


def verify(res, r, want):
    assert res["r"] == str(r)
    assert res["checks"]["switches_seen"]
    failed = {k: res["problems"].get(k, False) for k, v in res["checks"].items() if v is not True}
    assert len(res["checks"]) == len(want) and set(res["checks"]) == want, sorted(set(res["checks"]) ^ want)
    assert not failed, failed


@pytest.mark.parametrize("r", sorted(EVEN_R + (5,)))
def test_narrow_fan_ins_at_every_compiled_r(r):
    """Fan-in 3..10 at P = 2 R 2048 + 2048 + 4*37 + 3 (two full blocks, a ragged
    block of one full row and a partial row, a 3-element tail), weights
    dirichlet and zero_in_middle; aliased outputs at R = 4, 24, 32; FAST and
    mean at R = 5 and 6."""
    ops = narrow_ops(r)
    want = expected_checks(ops, NARROW_FAN_INS)
    assert len(want) == 1 + len(NARROW_FAN_INS) * (3 + 2 * (r in ALIAS_R) + 5 * (r in RUNTIME_R))
    verify(run_child("narrow", ",".join(ops), r), r, want)


@pytest.mark.parametrize("r", sorted({r for rs in WIDE_R.values() for r in rs}))
def test_wide_fan_ins_at_every_r_the_dispatch_returns(r):
    """Fan-in 11..14 at 16 rows of 2048 elements per CU plus 2048 + 4*37 + 3,
    where they first defer; exact, dirichlet weights."""
    fan_ins = wide_fan_ins(r)
    want = expected_checks(["exact"], fan_ins, {"exact": ("dirichlet",)})
    assert fan_ins and len(want) == 1 + 2 * len(fan_ins)
    verify(run_child("wide", ",".join(str(n) for n in fan_ins), r), r, want)


def test_the_lists_cover_the_matrix():
    """Every (fan-in, R) the exact policy compiles and the dispatch can reach."""
    cells = {(n, r) for r in EVEN_R + (5,) for n in NARROW_FAN_INS if "exact" in narrow_ops(r)}
    cells |= {(n, r) for r in range(12, 33, 2) for n in wide_fan_ins(r)}
    assert {(n, r) for n in range(3, 11) for r in range(4, 33, 2)} <= cells
    assert {(11, r) for r in range(14, 33, 2)} | {(n, r) for n in (12, 13, 14) for r in range(12, 25, 2)} <= cells
    assert all({"fast", "mean"} <= set(narrow_ops(r)) for r in (5, 6))
    assert all("alias" in narrow_ops(r) for r in (4, 24, 32))
