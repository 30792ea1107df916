"""Guard bands and special values on the chunk-mean launches (GPU):
_native.chunk_mean_batched, PyTorch's CPU summation order, for fp32, bf16,
fp16 and fp64 at 1 and 4 worker threads.

The outputs of one launch are neighbours in one 0xA5-filled buffer
(_edge_util.guarded_many) with a 16-byte canary between them. Every launch is
checked three ways: guards clean, every view bit-equal to the order-exact
oracle, inputs unchanged. Each task carries the specials block of
_edge_util.special_block at column 0 and straddling chunk_mean_ilp_begin, the
column where the summation order changes from the cascade to the row sums.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
from dasklearn_amd import _native
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ALL_DTYPES = ["f32", "bf16", "f16", "f64"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def chunk_rows(dtype, m, n, threads, seed):
    """m rows of n columns with the specials block at column 0 and either side
    of the first column summed in row order."""
    ib = orc.chunk_mean_ilp_begin(m, n, threads, dtype)
    block, _ = eu.special_block(dtype, m)
    w = block.shape[1]
    pos = sorted({0, max(ib - w // 2, 0), max(min(ib, n - 1), 0)} if n > w else {0})
    return eu.special_rows(dtype, m, n, pos, seed)


def run_launch(dtype, threads, shapes, offset=0, align=16, in_offset=None, seed=0):
    """One chunk_mean_batched call over tasks of (m, n) = shapes; outputs
    `offset` bytes past an `align`-byte boundary, inputs `in_offset` bytes past
    a 128-byte one (default: the outputs' offset)."""
    rows = [chunk_rows(dtype, m, n, threads, seed + 17 * k) for k, (m, n) in enumerate(shapes)]
    h = eu.guarded_many([n for _, n in shapes], dtype, dev(), gap=16, align=align, offset=offset)
    io = offset if in_offset is None else in_offset
    xs = [eu.place(list(r), dtype, dev(), offsets=[io] * r.shape[0]) for r in rows]
    _native.chunk_mean_batched([(x, v) for x, v in zip(xs, h.views)], threads=threads)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == [], shapes
    for k, r in enumerate(rows):
        exp = orc.chunk_mean(list(r), dtype, threads)
        got = eu.from_torch(h.views[k], dtype)
        assert eu.same_bits(got, exp, dtype), (shapes[k], eu.unwritten(h, k), eu.diff_report(got, exp, dtype))
        assert eu.inputs_unchanged(xs[k], r, dtype), shapes[k]


NS = (1, 3, 7, 33, 2 * 4096 + 37 * 8 + 7, 40_001)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("threads", [1, 4])
def test_few_rows_and_default_shapes(threads, dtype):
    """m = 2 and 6: a launch whose tasks all have m <= 6 loads 4 rows per
    group; m = 7 and 16: 8 rows per group. n = 1 with m >= the vector lanes is
    the inner reduction."""
    run_launch(dtype, threads, [(m, n) for m in (2, 6) for n in NS], seed=1)
    run_launch(dtype, threads, [(m, n) for m in (7, 16) for n in NS], seed=2)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("threads", [1, 4])
def test_table_kernel(threads, dtype):
    """m = 193: more inputs than a kernel-argument batch holds."""
    for n in (1, 9, 5000):
        run_launch(dtype, threads, [(193, n)], seed=3)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("threads", [1, 4])
def test_line_misaligned_heads(threads, dtype):
    """Inputs and output share a 16 k mod 128 misalignment and the task has
    whole tiles to align: block 0 folds the leading columns. One launch per
    misalignment, with a task too short for a head beside the long ones."""
    E = eu.VEC_ELEMS[dtype]
    long = 2 * 1024 * E + 128 + 5 * E + (E - 1)
    for mis in (16, 48, 112):
        run_launch(dtype, threads, [(2, long), (7, long + E), (5, 100)], offset=mis, align=128, seed=mis)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("threads", [1, 4])
def test_misaligned_tasks_take_the_scalar_path(threads, dtype):
    esz = eu.ESIZE[dtype]
    shapes = [(3, 1), (3, 4099), (7, 2 * 4096 + 5), (20, 100)]
    run_launch(dtype, threads, shapes, offset=esz, seed=5)  # outputs and inputs one element off
    run_launch(dtype, threads, shapes, offset=0, in_offset=esz, seed=6)  # only the inputs
    run_launch(dtype, threads, shapes, offset=esz, in_offset=0, seed=7)  # only the outputs


@pytest.mark.parametrize("m", [16, 4, 12])
def test_deferred_forms_at_the_smallest_deferring_launch(m):
    """fp32, 5,000,011 columns in all (20 MB per stream, where run_chunk_mean
    starts to defer; no switch moves that) cut into 4 chunks: a tiny chunk
    with no whole row, a chunk of 40 whole rows exactly, and two ragged ones.
    m = 16: k_chunk_mean_defer; m = 4 and 12: k_chunk_mean_defer_m at both of
    its row limits (32 and 24 results per lane)."""
    P, threads = 5_000_011, 4
    cuts = [0, 1000, 1000 + 2048 * 40, 2_400_004, P]
    bounds = list(zip(cuts, cuts[1:]))
    rng = np.random.default_rng(m)
    flat = rng.standard_normal((m, P), dtype=np.float32) * np.float32(0.05)
    flat = eu.avoid_fill(flat, "f32").reshape(m, P)
    block, _ = eu.special_block("f32", m)
    w = block.shape[1]
    for b, e in bounds:
        ib = orc.chunk_mean_ilp_begin(m, e - b, threads, "f32")
        for q in {0, max(ib - w // 2, 0), (e - b) // 2 // 2048 * 2048, max(e - b - w, 0)}:
            ww = min(w, e - b - q)
            flat[:, b + q:b + q + ww] = block[:, :ww]
    flats = [torch.from_numpy(r).to(dev()) for r in flat]
    h = eu.guarded_many([e - b for b, e in bounds], "f32", dev(), gap=16)
    tasks = [([f[b:e] for f in flats], v) for (b, e), v in zip(bounds, h.views)]
    plan = _native.chunk_mean_plan(tasks, threads)
    want = ("defer_rf8", 0, 4) if m == 16 else ("defer_m", m, 4)
    assert [(q["form"], q["mf"], q["ntasks"]) for q in plan] == [want], plan
    assert plan[0]["bpt"] == 0 and 4 <= plan[0]["R"] <= (24 if m == 12 else 32), plan  # unequal tasks: the search
    _native.chunk_mean_batched(tasks, threads=threads)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == []
    for k, (b, e) in enumerate(bounds):
        exp = orc.chunk_mean([r[b:e] for r in flat], "f32", threads)
        got = eu.from_torch(h.views[k], "f32")
        assert eu.same_bits(got, exp, "f32"), ((b, e), eu.unwritten(h, k), eu.diff_report(got, exp, "f32"))
    assert eu.inputs_unchanged(flats, flat, "f32")
    del flats, h
    torch.cuda.empty_cache()
