"""Guard bands around every output of a batched order-statistic call
(dlsim_robust_reduce_batched, dlsim_robust_reduce_tensors_batched): the
outputs lie in one 0xA5-filled buffer a few bytes apart
(_edge_util.guarded_many). No byte outside an output is written, none inside
is left unwritten, the result equals the CPU contract (tests/_robust_util.py)
bit for bit and the inputs are unchanged. fp32 and bf16 at capacity classes 4
and 32; sub-tasks in vectors (16-byte aligned) and element by element (one
element off)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
import _robust_util as ru

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402

DEV = "cuda"


def _lengths(n, dtype):
    T, E = _native.robust_batch_geometry(n, ru.DTYPES[dtype])[0], eu.VEC_ELEMS[dtype]
    return [1, E - 1, E + 1, T - 1, T, T + 1, 2 * T + E + 1]


def _inputs(dtype, n, p, seed):
    rows = ru.random_rows(ru.DTYPES[dtype], n, p, seed)
    fill = int(eu.fill_pattern(dtype))
    for r in rows:  # no input element may look like an unwritten output element
        assert not (ru.bits_of(r) == fill).any()
    return rows


def _verify(h, k, want, what):
    got = h.views[k].detach().cpu()
    assert eu.unwritten(h, k) == 0, f"{what}: {eu.unwritten(h, k)} elements of output {k} left unwritten"
    assert ru.same_bits(got, want.reshape(-1)), f"{what}: output {k}: {ru.diff_report(got, want.reshape(-1))}"


@pytest.mark.parametrize("offset_elems", [0, 1], ids=["vectors", "scalar"])
@pytest.mark.parametrize("fans", [(1, 4, 3), (17, 32)], ids=["class4", "class32"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batched_outputs_inside_guard_bands(dtype, fans, offset_elems):
    esz = eu.ESIZE[dtype]
    lens = _lengths(fans[-1], dtype)
    sizes = [lens[k % len(lens)] for k in range(len(lens) + 1)]
    h = eu.guarded_many(sizes, dtype, DEV, gap=16, align=16, offset=offset_elems * esz)
    tasks, wants, kept = [], [], []
    for k, p in enumerate(sizes):
        n = fans[k % len(fans)]
        rows = _inputs(dtype, n, p, seed=900 + 31 * k + n)
        lo, hi = ru.windows(n)[k % len(ru.windows(n))]
        dev = [r.to(DEV) for r in rows]
        assert (h.views[k].data_ptr() % 16 == 0) == (offset_elems == 0)
        tasks.append((dev, lo, hi, h.views[k]))
        wants.append(ru.window_mean(rows, lo, hi))
        kept.append((dev, rows))
    _native.robust_reduce_batched(tasks)
    torch.cuda.synchronize()
    what = f"{dtype} fan-ins {fans} offset {offset_elems}"
    assert eu.check_guards(h) == [], f"{what}: guard bytes written (view, offset, value)"
    for k, want in enumerate(wants):
        _verify(h, k, want, what)
    for dev, rows in kept:
        assert all(ru.same_bits(d.cpu(), r) for d, r in zip(dev, rows)), f"{what}: an input changed"


@pytest.mark.parametrize("n", [4, 32])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tensors_entry_inside_guard_bands(dtype, n):
    """The tensors of one model at an arena's byte offsets behind a 10-element
    bias: aligned and misaligned sub-tasks next to each other, four guard bytes
    (fp32; two for bf16) apart at the closest."""
    esz = eu.ESIZE[dtype]
    T = _native.robust_batch_geometry(n, ru.DTYPES[dtype])[0]
    numels = [10, T + 1, 0, 7, 2 * T + 9, 64]
    h = eu.guarded_many(numels, dtype, DEV, gap=esz, align=esz)
    rows = _inputs(dtype, n, sum(numels), seed=77 + n)
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(numels)])[:-1]]
    dev = [r.to(DEV) for r in rows]
    base = h.buf.data_ptr()
    _native.robust_reduce_tensors_batched_raw([d.data_ptr() + o * esz for d in dev for o in offs], n, numels,
                                              [s for s, _ in h.regions], 1, n - 1 if n > 2 else n, base,
                                              _native.dtype_code(ru.DTYPES[dtype], single_task=True),
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = f"{dtype} n={n} tensors"
    assert eu.check_guards(h) == [], f"{what}: guard bytes written (view, offset, value)"
    want = ru.window_mean(rows, 1, n - 1 if n > 2 else n)
    for k, (o, p) in enumerate(zip(offs, numels)):
        _verify(h, k, want[o:o + p], what)
    assert all(ru.same_bits(d.cpu(), r) for d, r in zip(dev, rows)), f"{what}: an input changed"
