"""Guard bands around the output of the mean-around-the-median entries
(dlsim_robust_nearest_reduce, dlsim_robust_nearest_reduce_tensors;
inst_robust_nearest.hip): the output is a view into the middle of a
0xA5-filled buffer (_edge_util.guarded). No byte outside it is written, none
inside is left unwritten, the result equals the CPU contract
(tests/_nearest_util.py) bit for bit and the inputs are unchanged.

The launch shapes are those of the rank-window entries
(tests/test_gpu_edges_robust.py has the table): tiles for capacities 4, 8 and
16, half vectors for capacity 32, the scalar kernel off 16-byte alignment,
block 0 on the ragged end; so the lengths are that module's, at the tile
boundaries of each capacity. Kept counts: 1, 2, 3, (n+1)//2, n-1, n.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
import _nearest_util as nu
import _robust_util as ru
from test_gpu_edges_robust import (DTYPES, FAN_INS, SCALAR_LENGTHS, lengths, make_rows, place, tile_elems, unchanged,
                                   verify)

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402

DEV = "cuda"


def case(dtype, n, p, seed):
    """(rows, {keep: expected}) of one (dtype, fan-in) over p elements; every
    shorter length is a prefix (the result is element-wise). No expected
    element may look like an unwritten one."""
    dt = ru.DTYPES[dtype]
    rows = make_rows(dtype, n, p, seed)
    sb = ru.sorted_bits(rows, dt)
    wants = {k: nu.nearest_mean_sorted(sb, dt, k) for k in nu.keeps(n)}
    for k, want in wants.items():
        assert not (ru.bits_of(want) == eu.fill_pattern(dtype)).any(), f"keep {k}: an expected element is the fill"
    return rows, wants


@pytest.mark.parametrize("n", FAN_INS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_entry_inside_guard_bands_at_the_tile_boundaries(dtype, n):
    esz = eu.ESIZE[dtype]
    lens = lengths(n, dtype)
    rows, wants = case(dtype, n, max(lens), seed=17000 + n)  # (seeds whose fp16 means miss 0xA5A5: case() checks)
    dev = place(rows, dtype)
    for p in lens:
        for keep, want in wants.items():
            h = eu.guarded(p * esz, dtype, DEV)
            xs = [d[:p] for d in dev]
            assert h.view.data_ptr() % 16 == 0 and all(x.data_ptr() % 16 == 0 for x in xs)
            _native.robust_nearest_reduce(xs, keep, h.view)
            torch.cuda.synchronize()
            verify(h, 0, want[:p], f"{dtype} n={n} P={p} keep={keep}")
    unchanged(dev, rows, f"{dtype} n={n}")


@pytest.mark.parametrize("off", ["input", "output"])
@pytest.mark.parametrize("n", FAN_INS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_kernel_inside_guard_bands(dtype, n, off):
    """One element off 16-byte alignment, one input with an aligned output,
    then the output with aligned inputs: the scalar kernel, blocks of 256
    elements."""
    esz = eu.ESIZE[dtype]
    assert SCALAR_LENGTHS == [1, 255, 256, 257, 549]
    rows, wants = case(dtype, n, max(SCALAR_LENGTHS), seed=15000 + n)
    offsets = [esz if off == "input" and i == n // 2 else 0 for i in range(n)]
    dev = place(rows, dtype, offsets)
    assert [d.data_ptr() % 16 for d in dev] == offsets
    for p in SCALAR_LENGTHS:
        for keep, want in wants.items():
            h = eu.guarded(p * esz, dtype, DEV, offset=esz if off == "output" else 0)
            assert h.view.data_ptr() % 16 == (esz if off == "output" else 0)
            _native.robust_nearest_reduce([d[:p] for d in dev], keep, h.view)
            torch.cuda.synchronize()
            verify(h, 0, want[:p], f"{dtype} n={n} P={p} {off} off alignment keep={keep}")
    unchanged(dev, rows, f"{dtype} n={n} {off} off alignment")


@pytest.mark.parametrize("n", [4, 32])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tensors_entry_inside_guard_bands(dtype, n):
    """The tensors of one model at an arena's byte offsets behind a 10-element
    bias: aligned and misaligned tensors next to each other, one element of
    guard bytes apart at the closest; a zero-element tensor among them."""
    esz = eu.ESIZE[dtype]
    T = tile_elems(n, dtype)
    numels = [10, T + 1, 0, 7, 2 * T + 9, 64]
    h = eu.guarded_many(numels, dtype, DEV, gap=esz, align=esz)
    rows = make_rows(dtype, n, sum(numels), seed=16000 + n)
    keep = n - 2
    want = nu.nearest_mean(rows, keep)
    assert not (ru.bits_of(want) == eu.fill_pattern(dtype)).any()
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(numels)])[:-1]]
    dev = place(rows, dtype)
    _native.robust_nearest_reduce_tensors_raw([d.data_ptr() + o * esz for d in dev for o in offs], n, numels,
                                              [s for s, _ in h.regions], keep, h.buf.data_ptr(),
                                              _native.dtype_code(ru.DTYPES[dtype], single_task=True),
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = f"{dtype} n={n} tensors"
    for k, (o, p) in enumerate(zip(offs, numels)):
        verify(h, k, want[o:o + p], what)
    unchanged(dev, rows, what)
