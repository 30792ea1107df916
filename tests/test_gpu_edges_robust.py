"""Guard bands around the output of the flat order-statistic entries
(dlsim_robust_reduce, dlsim_robust_reduce_tensors; inst_robust.hip): the output
is a view into the middle of a 0xA5-filled buffer (_edge_util.guarded). No
byte outside it is written, none inside is left unwritten, the result equals
the CPU contract (tests/_robust_util.py) bit for bit and the inputs are
unchanged.

One launch shape per capacity (inst_robust.hip rob_launch_cap), with
kBlock = 256 lanes per block (wreduce_kernels.hpp) and E elements per 16-byte
vector:

* capacity C = 4 / 8 / 16 (k_robust_tiles): 16 / C vectors per lane (1 at 16),
  a tile of T = kBlock * (C >= 16 ? 1 : 16 / C) * E elements;
* capacity 32 (k_robust_halves): one 8-byte unit per lane, 8-byte loads and
  stores, a tile of T = kBlock units = kBlock * 8 / element size elements;
* any base off 16-byte alignment: k_robust_scalar, kBlock elements per block.

Block 0 takes the ragged end (the last partial tile and the elements past the
last whole vector or unit), so the lengths sit at the tile boundaries of each
capacity.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
import _robust_util as ru

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402

DEV = "cuda"
KBLOCK = 256  # wreduce_kernels.hpp kBlock
DTYPES = ["f32", "bf16", "f16", "f64"]
FAN_INS = [3, 8, 16, 17, 32]  # capacities 4, 8, 16 and 32 at n < CAP and n = CAP
SCALAR_LENGTHS = [1, 255, 256, 257, 2 * 256 + 37]


def capacity(n):
    return 4 if n <= 4 else 8 if n <= 8 else 16 if n <= 16 else 32


def tile_elems(n, dtype):
    """T: the elements of one block's tile for fan-in n (the module docstring)."""
    C, E = capacity(n), eu.VEC_ELEMS[dtype]
    if C == 32:
        return KBLOCK * 8 // eu.ESIZE[dtype]
    return KBLOCK * (1 if C >= 16 else 16 // C) * E


def lengths(n, dtype):
    T, E = tile_elems(n, dtype), eu.VEC_ELEMS[dtype]
    out = [1, E - 1, E + 1, T - 1, T, T + 1, 2 * T + E + 1]
    if capacity(n) == 32:
        # whole vectors, then one whole 8-byte unit and no scalar tail (a byte
        # count of 8 mod 16): the last unit is an upper-less half vector
        half = T + E + E // 2
        assert half * eu.ESIZE[dtype] % 16 == 8
        out += [half, half + 1]
    return sorted(set(out))


def windows(n):
    lo = (n - 1) // 2
    return [(lo, lo + 1), (1, n - 1)]  # the median; trim 1


def make_rows(dtype, n, p, seed):
    """ru.random_rows (15 % specials) with no element equal to the fill pattern."""
    dt = ru.DTYPES[dtype]
    fill = eu.fill_pattern(dtype)
    rows = []
    for r in ru.random_rows(dt, n, p, seed):
        b = ru.bits_of(r)
        b[b == fill] ^= type(fill)(1)
        rows.append(ru.from_bits(b, dt))
    assert not any((ru.bits_of(r) == fill).any() for r in rows)
    return rows


def case(dtype, n, p, seed):
    """(rows, {window: expected}) of one (dtype, fan-in) over p elements; every
    shorter length is a prefix (the result is element-wise). No expected
    element may look like an unwritten one."""
    dt = ru.DTYPES[dtype]
    rows = make_rows(dtype, n, p, seed)
    sb = ru.sorted_bits(rows, dt)
    wants = {w: ru.window_mean_sorted(sb, dt, *w) for w in windows(n)}
    for w, want in wants.items():
        assert not (ru.bits_of(want) == eu.fill_pattern(dtype)).any(), f"window {w}: an expected element is the fill"
    return rows, wants


def place(rows, dtype, offsets=None):
    return eu.place([eu.from_torch(r, dtype) for r in rows], dtype, torch.device(DEV), offsets)


def verify(h, k, want, what):
    assert eu.check_guards(h) == [], f"{what}: guard bytes written (view, offset, value)"
    got = h.views[k].detach().cpu()
    assert eu.unwritten(h, k) == 0, f"{what}: {eu.unwritten(h, k)} elements of output {k} left unwritten"
    assert ru.same_bits(got, want.reshape(-1)), f"{what}: output {k}: {ru.diff_report(got, want.reshape(-1))}"


def unchanged(dev, rows, what):
    assert all(ru.same_bits(d.cpu(), r) for d, r in zip(dev, rows)), f"{what}: an input changed"


@pytest.mark.parametrize("n", FAN_INS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_entry_inside_guard_bands_at_the_tile_boundaries(dtype, n):
    esz = eu.ESIZE[dtype]
    lens = lengths(n, dtype)
    rows, wants = case(dtype, n, max(lens), seed=4000 + n)
    dev = place(rows, dtype)
    for p in lens:
        for (lo, hi), want in wants.items():
            h = eu.guarded(p * esz, dtype, DEV)
            xs = [d[:p] for d in dev]
            assert h.view.data_ptr() % 16 == 0 and all(x.data_ptr() % 16 == 0 for x in xs)
            _native.robust_reduce(xs, lo, hi, h.view)
            torch.cuda.synchronize()
            verify(h, 0, want[:p], f"{dtype} n={n} P={p} window=[{lo},{hi})")
    unchanged(dev, rows, f"{dtype} n={n}")


@pytest.mark.parametrize("off", ["output", "input"])
@pytest.mark.parametrize("n", FAN_INS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_kernel_inside_guard_bands(dtype, n, off):
    """One element off 16-byte alignment, the output with aligned inputs or
    one input with an aligned output: the scalar kernel, blocks of 256
    elements."""
    esz = eu.ESIZE[dtype]
    rows, wants = case(dtype, n, max(SCALAR_LENGTHS), seed=5000 + n)
    offsets = [esz if off == "input" and i == n // 2 else 0 for i in range(n)]
    dev = place(rows, dtype, offsets)
    assert [d.data_ptr() % 16 for d in dev] == offsets
    for p in SCALAR_LENGTHS:
        for (lo, hi), want in wants.items():
            h = eu.guarded(p * esz, dtype, DEV, offset=esz if off == "output" else 0)
            assert h.view.data_ptr() % 16 == (esz if off == "output" else 0)
            _native.robust_reduce([d[:p] for d in dev], lo, hi, h.view)
            torch.cuda.synchronize()
            verify(h, 0, want[:p], f"{dtype} n={n} P={p} {off} off alignment window=[{lo},{hi})")
    unchanged(dev, rows, f"{dtype} n={n} {off} off alignment")


@pytest.mark.parametrize("n", [4, 32])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tensors_entry_inside_guard_bands(dtype, n):
    """The tensors of one model at an arena's byte offsets behind a 10-element
    bias: aligned and misaligned tensors next to each other, four guard bytes
    (fp32; two for bf16) apart at the closest."""
    esz = eu.ESIZE[dtype]
    T = tile_elems(n, dtype)
    numels = [10, T + 1, 0, 7, 2 * T + 9, 64]
    h = eu.guarded_many(numels, dtype, DEV, gap=esz, align=esz)
    rows = make_rows(dtype, n, sum(numels), seed=6000 + n)
    lo, hi = 1, n - 1
    want = ru.window_mean(rows, lo, hi)
    assert not (ru.bits_of(want) == eu.fill_pattern(dtype)).any()
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(numels)])[:-1]]
    dev = place(rows, dtype)
    _native.robust_reduce_tensors_raw([d.data_ptr() + o * esz for d in dev for o in offs], n, numels,
                                      [s for s, _ in h.regions], lo, hi, h.buf.data_ptr(),
                                      _native.dtype_code(ru.DTYPES[dtype], single_task=True),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = f"{dtype} n={n} tensors"
    for k, (o, p) in enumerate(zip(offs, numels)):
        verify(h, k, want[o:o + p], what)
    unchanged(dev, rows, what)
