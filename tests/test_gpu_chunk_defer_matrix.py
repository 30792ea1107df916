"""Every compiled deferred-store body of the chunk mean (GPU), inside guard
bands and bit for bit against the order-exact oracle.

run_chunk_mean defers an fp32 launch of 16-byte aligned tasks from 20 MB per
stream: to k_chunk_mean_defer_m<MF> (one body per MF = 4..15, 24 results per
lane from MF = 12, else 32) when every task has the same m below 16, to
k_chunk_mean_defer (8 rows per load group; 4 under an A/B switch) from m = 16.
No switch moves the 20 MB, so every case here cuts its tasks from one shared
set of 16 rows of 5,000,011 columns (tests/_chunk_defer_child.py), and every
case first asserts through _native.chunk_mean_plan the form, MF and task
lookup (bpt > 0: a division; bpt == 0: cm_find_task's search) it is meant to
reach, so a case that would run the tiled kernel fails instead of passing.

* every MF at 1 and 4 threads: ChunkManager's layout (k equal chunks and a
  remainder: bpt > 0) for k = 10 and 2 and with a last chunk of twice the
  blocks, and unequal cuts (bpt == 0) with and without line-misaligned heads;
  MF = 4, 9 and 15 also against torch.mean on the CPU;
* the runtime-m form at m = 16, 32, 33, 48 (the level-1 flush after a full
  group of 16, then an add of +0 or of one more row) and 192 (one task filling
  the pointer table), m = 16 and 40 in one launch, and a call that splits at
  192 pointers into a deferred and a tiled launch;
* rows per block R = 4, 5, 22, 24, 31 and 32 under DLSIM_DEFER_R, one child
  process per R and thread count (the switches are read once), every MF and
  m = 16, 17: tasks
  of 0, 1, R - 1, R, R + 1 and 2 R rows, so last blocks of 1, R - 1 and R rows
  and a task with none; R = 32 is clamped to 24 for MF >= 12;
* the 4-rows-per-group body of k_chunk_mean_defer in children under
  DLSIM_CHUNK_DEFER_FIXED=0 DLSIM_CHUNK_DEFER_MIN_M=2, at the default R and at
  the six above;
* ChunkManager.reconstruct_model end to end on a flat model of 5,000,011
  parameters, device and host chunks, against torch's own CPU sequence.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _chunk_defer_child as cd
from dasklearn_amd import _native
from dasklearn_amd.chunk_manager import ChunkManager
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXED_MS = tuple(range(4, 16))
SWEEP_MS = FIXED_MS + (16, 17)
SWEEP_R = (4, 5, 22, 24, 31, 32)
TORCH_REF_MS = (4, 9, 15)


def rmax_of(m):
    return 24 if 12 <= m < 16 else 32


def spec_of(m, sizes):
    return [(m, b, e) for b, e in cd.cuts_to_bounds(sizes)]


def launch(name, spec, threads, expect, **kw):
    plan, problems, geometry = cd.run_launch(spec, threads, expect, **kw)
    print(json.dumps({"case": name, "threads": threads, "plan": plan, "rows": [g[0] for g in geometry]}))
    assert not problems, (name, problems)
    return plan, geometry


# ---- 1. every fixed-m body, default process ----------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("mf", FIXED_MS)
def test_every_fixed_m_body(mf, threads):
    ref = mf in TORCH_REF_MS
    for k in (10, 2):
        plan, _ = launch(f"chunk_model_k{k}", spec_of(mf, cd.chunk_layout(k)), threads,
                         cd.expect_one("defer_m", mf, k, "pos"), torch_ref=ref)
        assert plan[0]["grid"] == k * plan[0]["bpt"]
    # nine chunks of 450,000 columns and one of 950,011: the last task owns more blocks than bpt,
    # which is what min(bid / bpt, nt - 1) is for
    plan, geometry = launch("long_last_chunk", spec_of(mf, cd.chunk_layout(10, 450_000)), threads,
                            cd.expect_one("defer_m", mf, 10, "pos"))
    assert plan[0]["grid"] - 9 * plan[0]["bpt"] > plan[0]["bpt"], plan
    assert plan[0]["grid"] == cd.grid_of(geometry, plan[0]["R"], True)
    # unequal cuts: the search; outputs 16 bytes apart, a task of no whole row, one of exactly 40
    plan, geometry = launch("unequal", spec_of(mf, cd.UNEQUAL), threads, cd.expect_one("defer_m", mf, 4, "zero"),
                            torch_ref=ref)
    assert [g for g in geometry[:2]] == [(0, 0), (40, 0)] and all(g[1] == 0 for g in geometry), geometry
    plan, geometry = launch("unequal_heads", spec_of(mf, cd.UNEQUAL), threads,
                            cd.expect_one("defer_m", mf, 4, "zero"), match_heads=True)
    assert [g[1] for g in geometry] == [0, 24, 24, 28] and geometry[1][0] == 39, geometry
    assert plan[0]["grid"] == cd.grid_of(geometry, plan[0]["R"], True)


# ---- 2. the runtime-m form, default process ----------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("m", [16, 32, 33, 48])
def test_runtime_m_form(m, threads):
    """m = 16, 32 and 48: the last group of 16 is full, so level 0 is flushed
    and the final add is of +0; 33: one row after two flushes."""
    plan, geometry = launch("unequal_heads", spec_of(m, cd.UNEQUAL), threads,
                            cd.expect_one("defer_rf8", 0, 4, "zero"), match_heads=True)
    assert plan[0]["grid"] == cd.grid_of(geometry, plan[0]["R"], False)
    launch("chunk_model_k4", spec_of(m, cd.chunk_layout(4)), threads, cd.expect_one("defer_rf8", 0, 4, "zero"))


def test_one_task_fills_the_pointer_table():
    """m = 192 (kCmMaxPtrs): the 16 base rows, each passed 12 times."""
    launch("one_task_m192", [(192, 0, cd.P)], 4, cd.expect_one("defer_rf8", 0, 1, "zero"))


@pytest.mark.parametrize("threads", [1, 4])
def test_runtime_m_mixed_fan_ins(threads):
    spec = [(16 if k % 2 == 0 else 40, b, e) for k, (b, e) in enumerate(cd.cuts_to_bounds(cd.UNEQUAL))]
    launch("m16_m40", spec, threads, cd.expect_one("defer_rf8", 0, 4, "zero"), match_heads=True)


def test_split_at_192_pointers_leaves_a_tiled_launch():
    """14 tasks of m = 16: 12 of them (192 pointers, 5,000,000 columns) defer,
    the last two (4 and 7 columns) run the tiled kernel."""
    sizes = [1000, cd.ROW * 40] + [400_000] * 9 + [5_000_000 - 1000 - cd.ROW * 40 - 9 * 400_000, 4, 7]
    assert sum(sizes) == cd.P and len(sizes) == 14

    def expect(plan):
        got = [(q["form"], q["ntasks"], q["first_task"]) for q in plan]
        return [] if got == [("defer_rf8", 12, 0), ("tiled", 2, 12)] else [f"launches {got}"]
    launch("split_12_2", spec_of(16, sizes), 4, expect)


# ---- 3. and 4. the switches, one child process each ---------------------------------------
def run_child(case, threads, **env):
    full = dict(os.environ, DLSIM_AB="1", **env)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_chunk_defer_child.py"), case, threads], env=full,
                         capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-3000:]
    print(lines[-1])  # the child's checks, plans and wall time, for a run with -rA
    res = json.loads(lines[-1])
    failed = {k: res["problems"].get(k, False) for k, v in res["checks"].items() if v is not True}
    assert not failed, failed
    assert res["peak_device_mb"] < 1000
    return res


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("r", SWEEP_R)
def test_rows_per_block_sweep(r, threads):
    res = run_child("rsweep", str(threads), DLSIM_DEFER_R=str(r))
    assert res["r"] == str(r) and set(res["checks"]) == {f"m{m}_t{threads}" for m in SWEEP_MS} | {"switches_seen"}
    for m in SWEEP_MS:
        R = min(r, rmax_of(m))  # 32 is clamped to 24 for MF = 12..15
        plan = res["plans"][f"m{m}_t{threads}"]
        assert [(q["form"], q["mf"], q["R"], q["bpt"], q["ntasks"]) for q in plan] == [
            ("defer_m" if m < 16 else "defer_rf8", m if m < 16 else 0, R, 0, 7)], (m, plan)
        assert {0, 1, R - 1, R} <= set(res["covered"][f"m{m}_t{threads}"]), (m, res["covered"])


RF4_KEYS = {f"{c}_t{t}" for c in ("m2", "m3", "m6", "m2_m5") for t in (1, 4)} | {"switches_seen"}


def test_four_rows_per_group_body():
    res = run_child("rf4", "1,4", DLSIM_CHUNK_DEFER_FIXED="0", DLSIM_CHUNK_DEFER_MIN_M="2")
    assert set(res["checks"]) == RF4_KEYS
    assert all(q["form"] == "defer_rf4" for plan in res["plans"].values() for q in plan)


@pytest.mark.parametrize("r", SWEEP_R)
def test_four_rows_per_group_body_rows_per_block_sweep(r):
    res = run_child("rf4", "1,4", DLSIM_CHUNK_DEFER_FIXED="0", DLSIM_CHUNK_DEFER_MIN_M="2", DLSIM_DEFER_R=str(r))
    assert res["r"] == str(r) and set(res["checks"]) == RF4_KEYS
    for key in RF4_KEYS - {"switches_seen"}:
        assert [(q["form"], q["R"], q["ntasks"]) for q in res["plans"][key]] == [("defer_rf4", r, 7)], (key, res["plans"])
        assert {0, 1, r - 1, r} <= set(res["covered"][key]), (key, res["covered"])


# ---- 5. the production route ----------------------------------------------------------------
class _Flat(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(n))


@pytest.mark.parametrize("peers,where", [(4, "device"), (12, "device"), (15, "device"), (4, "host")])
def test_reconstruct_model_on_a_flat_model(peers, where):
    """ChunkManager.chunk_model cuts 5,000,011 parameters into nine chunks of
    500,001 and one of 500,002; every peer's chunk is a tensor of its own, as
    chunks received from peers are. Device chunks: one batched call, the
    fixed-m deferred kernel with the division lookup (asserted on the same
    chunks with outputs aligned as ChunkManager aligns them). Host chunks:
    dlsim_host_chunk_mean stages them and runs the same dispatch one chunk
    index at a time (2 MB launches: the tiled kernel). Compared with the
    reference's own sequence on the CPU."""
    host, _ = cd.base()
    k = 10
    models = [_Flat(cd.P) for _ in range(peers)]
    with torch.no_grad():
        for mdl, row in zip(models, host):
            mdl.w.copy_(torch.from_numpy(row))
    chunked = [ChunkManager.chunk_model(mdl, k) for mdl in models]
    assert [c.numel() for c in chunked[0]] == [500_001] * 9 + [500_002]
    by_index = [[chunked[i][c].clone() for i in range(peers)] for c in range(k)]
    want = torch.cat([torch.mean(torch.stack(cs), dim=0) for cs in by_index])
    del models, chunked
    if where == "device":
        chunks = [[c.to(cd.dev()) for c in cs] for cs in by_index]
        outs = [torch.empty(c[0].numel(), device=cd.dev()) for c in chunks]
        plan = _native.chunk_mean_plan(list(zip(chunks, outs)), torch.get_num_threads())
        assert [(q["form"], q["mf"], q["ntasks"]) for q in plan] == [("defer_m", peers, k)] and plan[0]["bpt"] > 0, plan
        del outs
        target = _Flat(cd.P).to(cd.dev())
    else:
        chunks = by_index
        one = _native.chunk_mean_plan([([cd.base()[1][i][:500_001] for i in range(peers)],
                                        torch.empty(500_001, device=cd.dev()))], torch.get_num_threads())
        assert [q["form"] for q in one] == ["tiled_few"], one
        target = _Flat(cd.P)
    kept = [list(cs) for cs in chunks]  # reconstruct_model replaces the lists' entries by the means, as the reference does
    out = ChunkManager.reconstruct_model(chunks, target)
    torch.cuda.synchronize()
    assert orc.same_bits(out.w.detach().cpu().numpy(), want.numpy())
    for c, cs in enumerate(kept):  # inputs unchanged
        lo, hi = c * 500_001, cd.P if c == k - 1 else (c + 1) * 500_001
        assert all(np.array_equal(x.cpu().numpy().view(np.uint32), host[i][lo:hi].view(np.uint32))
                   for i, x in enumerate(cs)), c
    del chunks, kept, target, out
    torch.cuda.empty_cache()
