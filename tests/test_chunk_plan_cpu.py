"""dlsim_chunk_mean_plan (CPU): which kernel a chunk-mean call launches, with
what grid, decided by run_chunk_mean's own code and queried without a GPU
(cus = 256 stands for the device). The pointers are fabricated integers with
the alignment and spacing of real buffers; the query never reads through them.

The rule, restated here independently of dispatch.hpp: an fp32 launch whose
tasks are all 16-byte aligned defers its stores from 20,000,000 bytes per
stream in all, to k_chunk_mean_defer_m<MF> when every task has the same m in
4..15, to k_chunk_mean_defer when every task has m >= 16; everything else is
the tiled kernel, m > 192 the pointer-table kernel. A launch holds at most 32
tasks and 192 pointers. R (rows of 2048 fp32 a block folds before it stores)
is the fewest even value in 4..24 whose blocks fit the CUs, else the fewest in
4..rmax that fit twice the CUs, else rmax (24 for MF >= 12, else 32).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from dasklearn_amd import _native

CUS = 256
ROW = 2048  # fp32 columns of one row of 512 16-byte vectors
IN_BASE, OUT_BASE, ROW_STRIDE = 1 << 40, 1 << 46, 1 << 32  # 128-byte aligned, 4 GiB between rows


def flat_tasks(m, sizes, ms=None, in_shift=0, elem=4):
    """Chunks cut from m flat rows (ChunkManager's layout: task t reads every
    row at the same offset) into outputs that follow one another, as
    (input addresses, output address, columns). ms: a contributor count per
    task instead of m."""
    tasks, pos = [], 0
    for t, n in enumerate(sizes):
        mt = m if ms is None else ms[t]
        tasks.append(([IN_BASE + i * ROW_STRIDE + pos * elem + in_shift for i in range(mt)], OUT_BASE + pos * elem, n))
        pos += n
    return tasks


def plan(tasks, threads=1, dtype=None):
    return _native.chunk_mean_plan(tasks, threads, cus=CUS, dtype=dtype)


def forms(p):
    return [q["form"] for q in p]


def chunk_layout(total, k, vec=True):
    """ChunkManager.chunk_model's sizes: k chunks of total // k, the last one
    longer by the remainder. vec: the chunk size rounded down to whole 16-byte
    vectors, as it is for a model whose total // k is a multiple of 4
    (ResNet-18 at k = 10: 1,118,164); views of a flat row cut elsewhere are not
    16-byte aligned and take the tiled kernel's scalar path."""
    c = total // k // 4 * 4 if vec else total // k
    return [c] * (k - 1) + [total - c * (k - 1)]


# ---- the deferring threshold -----------------------------------------------------------
def test_defers_from_twenty_megabytes_per_stream():
    assert forms(plan(flat_tasks(8, [4_999_999]))) == ["tiled"]
    p = plan(flat_tasks(8, [5_000_000]))
    assert [(q["form"], q["mf"], q["ntasks"], q["first_task"]) for q in p] == [("defer_m", 8, 1, 0)]
    p = plan(flat_tasks(8, [1_250_000] * 4))
    assert [(q["form"], q["mf"], q["ntasks"]) for q in p] == [("defer_m", 8, 4)]
    assert forms(plan(flat_tasks(8, [1_250_000] * 3 + [1_249_996]))) == ["tiled"]
    assert forms(plan(flat_tasks(16, [4_999_999]))) == ["tiled"]
    assert forms(plan(flat_tasks(16, [2_500_000, 2_500_000]))) == ["defer_rf8"]


# ---- fan-in and form -------------------------------------------------------------------
@pytest.mark.parametrize("m", range(2, 18))
def test_form_by_fan_in(m):
    p = plan(flat_tasks(m, chunk_layout(5_000_011, 10)), threads=4)
    assert len(p) == 1 and p[0]["ntasks"] == 10
    odd = plan(flat_tasks(m, chunk_layout(5_000_011, 10, vec=False)), threads=4)  # views cut at 500,001 columns
    assert forms(odd) == ["tiled_few" if m <= 6 else "tiled"]
    if m < 4:
        assert p[0]["form"] == "tiled_few" and (p[0]["mf"], p[0]["R"], p[0]["bpt"]) == (0, 0, 0)
        big = plan(flat_tasks(m, [400_000_000]))
        assert forms(big) == ["tiled_few"]  # 1.6 GB per stream: still tiled
    elif m < 16:
        assert (p[0]["form"], p[0]["mf"]) == ("defer_m", m)
        assert 4 <= p[0]["R"] <= (24 if m >= 12 else 32) and p[0]["R"] % 2 == 0
    else:
        assert (p[0]["form"], p[0]["mf"], p[0]["bpt"]) == ("defer_rf8", 0, 0)


def test_mixed_fan_ins():
    half = [2_500_004, 2_500_004]
    assert forms(plan(flat_tasks(0, half, ms=[4, 5]))) == ["tiled_few"]
    assert forms(plan(flat_tasks(0, half, ms=[7, 8]))) == ["tiled"]
    assert forms(plan(flat_tasks(0, half, ms=[15, 16]))) == ["tiled"]
    p = plan(flat_tasks(0, half, ms=[16, 40]))
    assert [(q["form"], q["ntasks"]) for q in p] == [("defer_rf8", 2)]


# ---- alignment and dtype ---------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 16])
def test_one_pointer_four_bytes_off_makes_the_launch_tiled(m):
    tasks = flat_tasks(m, [2_500_000, 2_500_000])
    assert forms(plan(tasks))[0].startswith("defer")
    ins, out, n = tasks[1]
    for moved in ((ins[:m - 1] + [ins[m - 1] + 4], out, n), (ins, out + 4, n)):
        assert forms(plan([tasks[0], moved])) == ["tiled"]
    # every pointer 16 bytes on: still vectors, still deferred
    assert forms(plan(flat_tasks(m, [2_500_000, 2_500_000], in_shift=16)))[0].startswith("defer")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
@pytest.mark.parametrize("m", [4, 8, 16])
def test_only_fp32_defers(m, dtype):
    elem = 8 if dtype == torch.float64 else 2
    p = plan(flat_tasks(m, [20_000_000, 20_000_000], elem=elem), dtype=dtype)
    assert forms(p) == ["tiled_few" if m <= 6 else "tiled"]


# ---- bpt: the division that finds a block's task -----------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("k", [2, 3, 10])
def test_bpt_for_equal_chunks_and_a_remainder(k, threads):
    for total in (5_000_011, 6_300_001):
        sizes = chunk_layout(total, k)  # a longer last chunk
        c = sizes[0]
        assert sizes[-1] > c and 64 < c % ROW < ROW - 64  # a head or the row-order tail never costs a whole row
        lasts = [sizes[-1], c + 4 * ROW * 40] + ([c - 1000, 1000] if total - c >= 5_000_000 else [])
        for last in lasts:
            p = plan(flat_tasks(8, sizes[:-1] + [last]), threads)
            assert len(p) == 1 and p[0]["form"] == "defer_m" and p[0]["ntasks"] == k, (total, last, p)
            per_task = -(-(c // ROW) // p[0]["R"])
            assert p[0]["bpt"] == per_task > 0, p
            assert p[0]["grid"] == (k - 1) * per_task + max(-(-(last // ROW) // p[0]["R"]), 1), p
    one = plan(flat_tasks(8, [5_000_011]), threads)
    assert one[0]["bpt"] == one[0]["grid"] > 0


def test_bpt_is_zero_when_a_middle_task_differs():
    c = 500_000
    for k in (3, 10):
        sizes = [c] * k + [5_000_011 - c * k + 5_000_000]
        assert plan(flat_tasks(8, sizes))[0]["bpt"] > 0
        for j in range(1, k):
            other = list(sizes)
            other[j] += ROW * plan(flat_tasks(8, sizes))[0]["R"]  # one block more
            p = plan(flat_tasks(8, other))
            assert p[0]["form"] == "defer_m" and p[0]["bpt"] == 0, (k, j, p)
        first = list(sizes)
        first[0] += ROW * 40
        assert plan(flat_tasks(8, first))[0]["bpt"] == 0
    # the runtime-m form has no division: bpt stays 0
    assert plan(flat_tasks(16, [c] * 10 + [5_000_000]))[0]["bpt"] == 0


# ---- R -----------------------------------------------------------------------------------
def rule_rows(rows, cus, rmax, fixed):
    """The documented R, and the launch's grid at it. fixed: a task's last row
    block also does its ragged end (at least one block per task); else one
    ragged block per task beside the row blocks."""
    def blocks(R):
        if fixed:
            return sum(max(-(-r // R), 1) for r in rows)
        return sum(-(-r // R) for r in rows) + len(rows)
    for R in range(4, min(rmax, 24) + 1, 2):
        if blocks(R) <= cus:
            return R, blocks(R)
    for R in range(4, rmax + 1, 2):
        if blocks(R) <= 2 * cus:
            return R, blocks(R)
    return rmax, blocks(rmax)


def boundary_row_totals(cus, rmax, nt, fixed):
    """Row totals either side of every R boundary of a launch of nt equal
    tasks: blocks(R) == cus and cus + 1 (one round), 2 cus and 2 cus + 1."""
    out = set()
    for R in range(4, rmax + 1, 2):
        for fit in (cus, 2 * cus):
            per = (fit - (0 if fixed else nt)) // nt  # row blocks per task
            for rows in (per * R, per * R + 1, per * R - 1):
                if rows * nt * ROW >= 5_000_000 and rows * ROW * 4 < (1 << 31) - ROW * 4:
                    out.add(rows)
    return sorted(out)


@pytest.mark.parametrize("cus", [256, 1024, 8])
@pytest.mark.parametrize("m,nt", [(4, 1), (11, 1), (12, 1), (15, 1), (8, 10), (13, 10), (16, 1), (16, 10), (40, 4)])
def test_rows_per_block_follow_the_documented_rule(m, nt, cus):
    """cus = 256 reaches the boundaries from R = 10 up with one task (a launch
    under 5,000,000 columns does not defer), 1024 CUs the ones below, 8 CUs the
    rmax fall-back."""
    fixed = m < 16
    rmax = 24 if 12 <= m < 16 else 32
    totals = boundary_row_totals(cus, rmax, nt, fixed) + [2442 // nt + 1, 5000, 20000]
    seen = set()
    for rows in totals:
        n = rows * ROW + 36  # threads = 1: ilp_begin = n // 32 * 32, and a head is under 32 columns
        tasks = flat_tasks(m, [n] * nt)
        p = _native.chunk_mean_plan(tasks, 1, cus=cus)
        R, grid = rule_rows([rows] * nt, cus, rmax, fixed)
        assert len(p) == 1 and p[0]["form"] == ("defer_m" if fixed else "defer_rf8")
        assert (p[0]["R"], p[0]["grid"]) == (R, grid), (rows, p)
        seen.add(R)
    if cus == 8:
        assert seen == {rmax}
    else:
        assert len(seen) >= 6 and max(seen) == rmax, seen


def test_rule_at_the_shapes_the_gpu_tests_use():
    """5,000,011 columns as k = 10 and k = 2 chunks on 256 CUs: R = 10 and 12
    (MF < 12: 245 and 204 blocks), the README's R = 22 for ResNet-18's
    11,181,642 parameters at k = 10."""
    for total, k, want in ((5_000_011, 10, 10), (5_000_011, 2, 10), (11_181_642, 10, 22)):
        sizes = chunk_layout(total, k)
        rows = [n // 32 * 32 // ROW for n in sizes]  # threads = 1; the heads (< 32 columns) never cost a row here
        p = plan(flat_tasks(8, sizes))
        R, _ = rule_rows(rows, CUS, 32, True)
        assert p[0]["R"] == R == want, (total, k, p)


# ---- splits ------------------------------------------------------------------------------
def test_split_at_32_tasks():
    n = 160_000  # 33 tasks: 32 of them 20.48 MB, the last one alone far below
    p = plan(flat_tasks(4, [n] * 33))
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("defer_m", 32, 0), ("tiled_few", 1, 32)]
    p = plan(flat_tasks(4, [n] * 64))
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("defer_m", 32, 0), ("defer_m", 32, 32)]
    p = plan(flat_tasks(4, [1000] + [n] * 32))  # the first launch just under 20 MB
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("tiled_few", 32, 0), ("tiled_few", 1, 32)]


def test_split_at_192_pointers():
    n = 500_000
    p = plan(flat_tasks(16, [n] * 14))  # 12 x 16 = 192 pointers, then 2 tasks of 4 MB
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("defer_rf8", 12, 0), ("tiled", 2, 12)]
    p = plan(flat_tasks(15, [n] * 14))  # 12 x 15 = 180, a 13th would be 195
    assert [(q["form"], q["mf"], q["ntasks"], q["first_task"]) for q in p] == [("defer_m", 15, 12, 0),
                                                                              ("tiled", 0, 2, 12)]
    p = plan(flat_tasks(0, [100_000] + [2_500_000] * 2, ms=[190, 16, 16]))  # 190 + 16 > 192
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("tiled", 1, 0), ("defer_rf8", 2, 1)]
    p = plan(flat_tasks(192, [5_000_000]))
    assert [(q["form"], q["ntasks"]) for q in p] == [("defer_rf8", 1)]


def test_more_than_192_contributors_take_the_table():
    p = plan(flat_tasks(193, [5_000_000]))
    assert [(q["form"], q["ntasks"], q["R"]) for q in p] == [("table", 1, 0)]
    # the table task launches when it is met, the batch around it when it is flushed
    p = plan(flat_tasks(0, [2_500_000, 1000, 2_500_000], ms=[8, 193, 8]))
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("table", 1, 1), ("defer_m", 2, 0)]


def test_overlapping_tasks_run_one_launch_each():
    """A task that reads another task's output: one launch per task, in order,
    each deciding for itself."""
    a = ([IN_BASE + i * ROW_STRIDE for i in range(8)], OUT_BASE, 5_000_000)
    b = ([OUT_BASE] + [IN_BASE + (8 + i) * ROW_STRIDE for i in range(7)], OUT_BASE + ROW_STRIDE, 5_000_000)
    c = ([IN_BASE + (20 + i) * ROW_STRIDE for i in range(8)], OUT_BASE + 2 * ROW_STRIDE, 1000)
    p = plan([a, b, c])
    assert [(q["form"], q["mf"], q["ntasks"], q["first_task"]) for q in p] == [
        ("defer_m", 8, 1, 0), ("defer_m", 8, 1, 1), ("tiled", 0, 1, 2)]


def test_empty_tasks_and_bad_arguments():
    assert plan([]) == []
    p = plan(flat_tasks(8, [0, 5_000_000, 0]))
    assert [(q["form"], q["ntasks"], q["first_task"]) for q in p] == [("defer_m", 1, 1)]
    with pytest.raises(_native.DlsimError):
        _native.chunk_mean_plan(flat_tasks(8, [100]), 0, cus=CUS)
    with pytest.raises(_native.DlsimError):
        _native.chunk_mean_plan(flat_tasks(8, [100]), 1, cus=-1)
    with pytest.raises(_native.DlsimError):
        _native.chunk_mean_plan([([0] * 8, OUT_BASE, 100)], 1, cus=CUS)


# ---- the A/B switches (read once per process) ----------------------------------------------
_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from dasklearn_amd import _native
IN, OUT, STRIDE = 1 << 40, 1 << 46, 1 << 32
def one(m, n=5_000_011):
    q = _native.chunk_mean_plan([([IN + i * STRIDE for i in range(m)], OUT, n)], 1, cus=256)
    assert len(q) == 1
    return [q[0]["form"], q[0]["mf"], q[0]["R"]]
print(json.dumps({str(m): one(m) for m in (2, 3, 4, 6, 7, 11, 12, 15, 16, 40)}))
"""


def child_plans(**env):
    full = {k: v for k, v in os.environ.items() if not k.startswith("DLSIM_")}
    full.update(env)
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "decentralized-learning-simulator_amd")],
                         env=full, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return {int(k): tuple(v) for k, v in json.loads(out.stdout.splitlines()[-1]).items()}


DEFAULT_PLANS = {2: ("tiled_few", 0, 0), 3: ("tiled_few", 0, 0), 4: ("defer_m", 4, 10), 6: ("defer_m", 6, 10),
                 7: ("defer_m", 7, 10), 11: ("defer_m", 11, 10), 12: ("defer_m", 12, 10), 15: ("defer_m", 15, 10),
                 16: ("defer_rf8", 0, 10), 40: ("defer_rf8", 0, 10)}


def test_default_process_plans():
    """One task of 5,000,011 columns is 2441 rows: ceil(2441 / 10) = 245
    blocks (246 with the runtime-m form's ragged block) fit 256 CUs, 8 rows
    per block do not."""
    assert child_plans() == DEFAULT_PLANS


@pytest.mark.parametrize("r", [7, 24, 32, 50])
def test_defer_r_switch_sets_and_clamps_the_rows(r):
    got = child_plans(DLSIM_AB="1", DLSIM_DEFER_R=str(r))
    for m, (form, mf, _) in DEFAULT_PLANS.items():
        rmax = 24 if 12 <= m < 16 else 32
        assert got[m] == (form, mf, min(r, rmax) if form != "tiled_few" else 0), (m, got[m])


def test_defer_min_m_switch_reaches_the_four_row_form():
    got = child_plans(DLSIM_AB="1", DLSIM_CHUNK_DEFER_FIXED="0", DLSIM_CHUNK_DEFER_MIN_M="2")
    for m in DEFAULT_PLANS:
        assert got[m] == ("defer_rf4" if m <= 6 else "defer_rf8", 0, 10), (m, got[m])
    got = child_plans(DLSIM_AB="1", DLSIM_CHUNK_DEFER_FIXED="0")
    for m in DEFAULT_PLANS:
        assert got[m][0] == ("defer_rf8" if m >= 16 else "tiled_few" if m <= 6 else "tiled"), (m, got[m])
    got = child_plans(DLSIM_AB="1", DLSIM_CHUNK_DEFER="0")
    assert all(got[m][0] == ("tiled_few" if m <= 6 else "tiled") for m in DEFAULT_PLANS), got


def test_switches_need_dlsim_ab():
    assert child_plans(DLSIM_DEFER_R="7", DLSIM_CHUNK_DEFER_FIXED="0", DLSIM_CHUNK_DEFER_MIN_M="2",
                       DLSIM_CHUNK_DEFER="0") == DEFAULT_PLANS
