"""Guard bands and special values on the deferred-store kernel's four bodies
(GPU): bursts of two inputs (compiled R up to 24), one burst (compiled R = 32),
the runtime-R form (FAST, mean, and an odd R, whose duplicate row and every
row past R are stored to vector nvec and dropped by the buffer range) and the
grouped form (fan-in 17). The library reads DLSIM_DEFER_R and
DLSIM_DEFER_MIN_MB once per process, so each case runs
tests/_edge_defer_child.py in a fresh interpreter.

The 3- and 2-element tails put live output bytes exactly where a store to
vector nvec would land; P = 2 R 2048 puts the guard band there. Specials sit
at _edge_util.edge_positions(P, R * 2048, 4).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_child(case, env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "_edge_defer_child.py"), case], env=env,
                         capture_output=True, text=True, timeout=180)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1])


def failed(res):
    return {k: res["problems"].get(k, False) for k, v in res["checks"].items() if not v}


@pytest.mark.parametrize("r", [4, 5, 24, 32])
def test_deferred_rows_guards_and_specials(r):
    """R = 4 and 24: bursts of two inputs; 5: the runtime-R form with a
    duplicate row; 32: one burst. Fan-in 3, 8 (fixed) and 17 (grouped), exact
    with every weight kind, FAST and mean, at the three sizes."""
    env = dict(os.environ, DLSIM_AB="1", DLSIM_DEFER_MIN_MB="0", DLSIM_DEFER_R=str(r))
    res = run_child("rows", env)
    assert res["r"] == str(r)
    assert res["checks"]["switches_seen"]
    assert len(res["checks"]) == 1 + 3 * 3 * (3 + 6 + 2 + 1) and not failed(res), failed(res)
    assert sum(k.startswith("defers_") for k in res["checks"]) == 27


def test_default_dispatch_defers_without_switches():
    """Fan-in 3 at 2,500,003 elements: deferred by the default dispatch."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DLSIM_")}
    res = run_child("default", env)
    assert len(res["checks"]) == 2 + 3 + 6 + 2 + 1 and not failed(res), failed(res)
