"""Guard bands and special values on the batched launches (GPU):
_native.wreduce_batched (kernel-argument batches), _native.BatchPlan (the
descriptor table) and _native.mean_batched.

The outputs of one launch are neighbours in one 0xA5-filled buffer
(_edge_util.guarded_many) with only a 16-byte canary between them, as an arena
lays parameters out: a task's ragged end that spills lands in the canary or in
the next task's output. Every launch is checked three ways: guards clean,
every view bit-equal to the oracle (views are prefilled, so an unwritten
element shows), inputs unchanged.

One launch holds tasks of 1, 3, E, E + 1, 2048 and 3 * 2048 + ragged elements
(E = elements per 16-byte vector), each with the specials block of
_edge_util.special_block at its edge positions, so specials sit in the first,
the middle and the last task. The "large" variant adds a task just past
kBatchSmallBytes (1 MiB), which moves the whole launch from one to four vectors
per lane (and, for fp32 tables, to the wave map).
"""
from __future__ import annotations

import pytest
import torch

import _edge_util as eu
from dasklearn_amd import _native

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
FANS = {
    "uniform3": [3],  # the fixed fan-in body
    "uniform8": [8],  # the fixed fan-in body at a wider fan-in (fixed for every dtype: 2-byte types up to 9)
    "uniform16": [16],  # one fan-in above the fixed bodies: the runtime fan-in body, two groups and more
    "mixed": [2, 15, 3, 16, 1, 8, 9],  # mixed fan-in: the runtime fan-in body
}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def sizes_of(dtype, large):
    E = eu.VEC_ELEMS[dtype]
    s = [1, 3, E, E + 1, 2048, 3 * 2048 + 5 * E + 3]
    if large:
        s.insert(3, (1 << 20) // eu.ESIZE[dtype] + 2048 + 5 * E + E - 1)  # >= kBatchSmallBytes: VPT 4
    return s


_CASES = {}


def case(dtype, large, fans):
    """Per task: (rows, weights, expected exact / fast / mean), computed once."""
    key = (dtype, large, fans)
    if key not in _CASES:
        E = eu.VEC_ELEMS[dtype]
        tile = 256 * (4 if large else 1) * E
        out = []
        for k, p in enumerate(sizes_of(dtype, large)):
            n = FANS[fans][k % len(FANS[fans])]
            rows = eu.special_rows(dtype, n, p, eu.edge_positions(p, tile, E), seed=31 * k + n)
            w = eu.special_weights(n, eu.WEIGHT_KINDS[k % len(eu.WEIGHT_KINDS)], dtype)
            out.append((rows, w, {op: eu.expected_reduce(op, rows, w, dtype) for op in ("exact", "fast", "mean")}))
        _CASES[key] = out
    return _CASES[key]


def launch(entry, tasks):
    if entry == "batched_exact":
        _native.wreduce_batched(tasks, _native.DLSIM_EXACT)
    elif entry == "batched_fast":
        _native.wreduce_batched(tasks, _native.DLSIM_FAST)
    elif entry == "table_exact":
        _native.BatchPlan(tasks, _native.DLSIM_EXACT).launch()
    elif entry == "table_fast":
        _native.BatchPlan(tasks, _native.DLSIM_FAST).launch()
    else:
        _native.mean_batched([(xs, out) for xs, _, out in tasks])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("fans", sorted(FANS))
def test_batched_launch_guards_and_specials(fans, large, dtype):
    tasks_host = case(dtype, large, fans)
    sizes = [rows.shape[1] for rows, _, _ in tasks_host]
    for entry in ("batched_exact", "batched_fast", "table_exact", "table_fast", "mean"):
        h = eu.guarded_many(sizes, dtype, dev(), gap=16)
        assert all(v.data_ptr() % 16 == 0 for v in h.views)
        xs = [eu.place(list(rows), dtype, dev()) for rows, _, _ in tasks_host]
        launch(entry, [(x, w, v) for x, (_, w, _), v in zip(xs, tasks_host, h.views)])
        torch.cuda.synchronize()
        assert eu.check_guards(h) == [], entry
        op = "mean" if entry == "mean" else entry.split("_")[1]
        for k, (rows, _, exp) in enumerate(tasks_host):
            got = eu.from_torch(h.views[k], dtype)
            assert eu.same_bits(got, exp[op], dtype), (entry, k, rows.shape, eu.unwritten(h, k),
                                                       eu.diff_report(got, exp[op], dtype))
            assert eu.inputs_unchanged(xs[k], rows, dtype), (entry, k)
