"""The deferred-store kernel's load bursts (GPU): every compiled body the row
counts below reach, both burst rules, bit for bit against the oracle. The
library reads DLSIM_DEFER_R and DLSIM_DEFER_MIN_MB once per process, so each
case runs tests/_defer_issue_child.py in a fresh interpreter.
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
    out = subprocess.run([sys.executable, os.path.join(HERE, "_defer_issue_child.py"), case], env=env,
                         capture_output=True, text=True, timeout=180)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize("r", [4, 6, 12, 22, 24, 32])
def test_compiled_rows_bit_exact_with_ragged_block_and_tail(r):
    """Fan-in 3, 8 and 10 with R rows per block (the exact policy's kernel
    compiled for that R: bursts of two inputs up to R = 24, input 0 then the
    rest at 32; FAST and mean: the runtime-R form) at
    P = 2 R 2048 + 2048 + 4*37 + 3 (two full blocks, a ragged block with one
    full row, a partial row and a 3-element tail), P = 2 R 2048 (neither) and
    P = 2 R 2048 + 2 (a tail and no ragged block)."""
    env = dict(os.environ, DLSIM_AB="1", DLSIM_DEFER_MIN_MB="0", DLSIM_DEFER_R=str(r))
    res = run_child("rows", env)
    assert res["r"] == str(r)
    assert len(res["checks"]) == 1 + 3 * 3 * 4 and all(res["checks"].values()), res


def test_wide_fan_in_bit_exact_at_the_smallest_deferring_size():
    """Fan-in 12 and 14 at 8,400,000 elements, where they first defer (R = 18)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DLSIM_")}
    res = run_child("wide", env)
    assert len(res["checks"]) == 4 and all(res["checks"].values()), res
