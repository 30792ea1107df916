"""dlsim_robust_reduce_batched and dlsim_robust_reduce_tensors_batched on the
MI355X against the CPU restatement of the order-statistic contract
(tests/_robust_util.py), bit for bit: every capacity class and dtype, lengths on
every edge of the tile, batches past each launch limit, misaligned and empty
tasks among aligned ones."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _robust_util as ru
from sgd_inputs import GNLENET_SHAPES

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402

DEV = "cuda"
VEC = {"f32": 4, "f64": 2, "bf16": 8, "f16": 8}  # elements of a 16-byte vector
CLASS_FAN_INS = {4: (1, 4), 8: (5, 8), 16: (9, 16), 32: (17, 32)}  # CAP/2 + 1 and CAP (class 4: 1 and 4)


def edge_lengths(n, dtype):
    T, E = _native.robust_batch_geometry(n, ru.DTYPES[dtype])[0], VEC[dtype]
    return [1, E - 1, E, E + 1, T - 1, T, T + 1, 2 * T + E + 1, 3 * T]


def _check(got: torch.Tensor, want: torch.Tensor, what: str):
    got = got.detach().cpu().reshape(-1)
    assert ru.same_bits(got, want.reshape(-1)), f"{what}: {ru.diff_report(got, want)}"


def _shifted(t: torch.Tensor, shift: int = 1) -> torch.Tensor:
    """A device copy of flat `t` whose base is `shift` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()]
    v.copy_(t)
    return v


class Case:
    """One task: its host rows, window and expected result."""

    def __init__(self, dtype, n, p, seed, window=None, in_shift=None, out_shift=0):
        self.dt = ru.DTYPES[dtype]
        self.n, self.p = n, p
        self.rows = ru.random_rows(self.dt, n, p, seed) if p else [torch.empty(0, dtype=self.dt)] * n
        ws = ru.windows(n)
        self.lo, self.hi = ws[seed % len(ws)] if window is None else window
        self.want = ru.window_mean(self.rows, self.lo, self.hi) if p else torch.empty(0, dtype=self.dt)
        self.dev = [_shifted(r) if i == in_shift else r.to(DEV) for i, r in enumerate(self.rows)]
        self.out = torch.empty(p + 16, dtype=self.dt, device=DEV)[out_shift:out_shift + p]
        if p:
            assert self.out.data_ptr() % 16 == out_shift * self.out.element_size()

    def task(self):
        return (self.dev, self.lo, self.hi, self.out)


def run_and_check(cases, what, stream=None):
    outs = _native.robust_reduce_batched([c.task() for c in cases], stream)
    assert len(outs) == len(cases)
    (stream or torch.cuda.current_stream()).synchronize()
    for k, c in enumerate(cases):
        _check(c.out, c.want, f"{what}: task {k} (n={c.n}, P={c.p}, window=[{c.lo},{c.hi}))")
        for d, r in zip(c.dev, c.rows):
            assert ru.same_bits(d.cpu(), r), f"{what}: task {k}: an input changed"


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("cap", [4, 8, 16, 32])
def test_one_class_every_edge_length(cap, dtype):
    """Both ends of the class's fan-in range, the nine lengths around the
    vector and the tile, another window per task: one call."""
    small, full = CLASS_FAN_INS[cap]
    cases = [Case(dtype, (small, full)[k % 2], p, seed=100 * cap + k)
             for k, p in enumerate(edge_lengths(full, dtype))]
    assert edge_lengths(small, dtype) == edge_lengths(full, dtype)  # one class, one geometry
    assert len({(c.lo, c.hi) for c in cases}) > 2
    run_and_check(cases, f"{dtype} class {cap}")


@pytest.mark.parametrize("count,n", [(33, 3), (25, 8), (7, 32)])
def test_batches_past_a_launch_limit(count, n):
    """33 tasks (> 32 tasks), 25 x 8 = 200 pointers (> 192), 7 x 32 = 224 pointers."""
    _, max_tasks, max_ptrs = _native.robust_batch_geometry(n, torch.float32)
    assert count > max_tasks or count * n > max_ptrs
    lens = edge_lengths(n, "f32")
    picks = [lens[3], lens[6], lens[0], lens[7]]  # E + 1, T + 1, 1, 2T + E + 1
    cases = [Case("f32", n, picks[k % 4], seed=7000 + 37 * n + k) for k in range(count)]
    run_and_check(cases, f"{count} tasks of n = {n}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_classes_interleaved_in_task_order(dtype):
    """The host regroups by class; the results still belong to their tasks."""
    fans = [3, 8, 17, 32, 1, 5, 9, 20, 4, 16, 2, 31]
    cases = [Case(dtype, n, 1000 + 517 * k, seed=300 + k) for k, n in enumerate(fans)]
    run_and_check(cases, f"{dtype} classes interleaved")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("n", [3, 20])
def test_misaligned_tasks_among_aligned_ones(n, dtype):
    """One input one element off, one output one element off: those tasks run
    element by element in the same launch (several blocks each, and a ragged
    end), their neighbours in vectors."""
    lens = edge_lengths(n, dtype)
    p = lens[7]
    cases = [Case(dtype, n, p, seed=1), Case(dtype, n, p, seed=2, in_shift=n - 1), Case(dtype, n, lens[5], seed=3),
             Case(dtype, n, p, seed=4, out_shift=1), Case(dtype, n, 256, seed=5, in_shift=0),
             Case(dtype, n, 255, seed=6, out_shift=1), Case(dtype, n, lens[4], seed=7)]
    run_and_check(cases, f"{dtype} n={n} misaligned among aligned")


def test_zero_length_task_in_the_middle():
    cases = [Case("f32", 5, 4097, seed=1), Case("f32", 5, 0, seed=2), Case("f32", 9, 33, seed=3)]
    run_and_check(cases, "empty task in the middle")
    assert _native.robust_reduce_batched([Case("f32", 5, 0, seed=2).task()])[0].numel() == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("n", [5, 17])
def test_special_values_through_a_batch(n, dtype):
    """+-0, subnormals, +-Inf and NaNs in every row position: every window of
    the sweep as one task over the same inputs, in vectors and (inputs one
    element off) element by element."""
    dt = ru.DTYPES[dtype]
    xs = ru.special_rows(dt, n)
    sb = ru.sorted_bits(xs, dt)
    aligned, shifted = [x.to(DEV) for x in xs], [_shifted(x) for x in xs]
    tasks, wants = [], []
    for lo, hi in ru.windows(n):
        for rows in (aligned, shifted):
            tasks.append((rows, lo, hi, torch.empty_like(aligned[0])))
            wants.append((ru.window_mean_sorted(sb, dt, lo, hi), f"{dtype} n={n} window=[{lo},{hi})"))
    _native.robust_reduce_batched(tasks)
    for (_, _, _, out), (want, what) in zip(tasks, wants):
        _check(out, want, what)


def _tensors_both_entries(dt, n, numels, ptrs, offs_bytes, lo, hi):
    outs = []
    for entry in (_native.robust_reduce_tensors_batched_raw, _native.robust_reduce_tensors_raw):
        out = torch.zeros(sum(numels) + 8, dtype=dt, device=DEV)
        entry(ptrs, n, numels, offs_bytes, lo, hi, out.data_ptr(), _native.dtype_code(dt, single_task=True),
              torch.cuda.current_stream().cuda_stream)
        outs.append(out)
    assert ru.same_bits(outs[0].cpu(), outs[1].cpu()), "the batched tensors entry differs from the per-tensor one"
    assert not outs[0][sum(numels):].any()
    return outs[0][:sum(numels)]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
def test_tensors_entry_on_the_gnlenet_shapes(dtype):
    n, dt = 8, ru.DTYPES[dtype]
    numels = [int(np.prod(s)) for s in GNLENET_SHAPES]
    rows = ru.random_rows(dt, n, sum(numels), seed=11)
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(numels)])[:-1]]
    tensors = [[r[o:o + k].clone().to(DEV) for o, k in zip(offs, numels)] for r in rows]  # separate allocations
    esz = rows[0].element_size()
    for lo, hi in ((3, 4), (2, 6)):
        got = _tensors_both_entries(dt, n, numels, [t.data_ptr() for row in tensors for t in row],
                                    [o * esz for o in offs], lo, hi)
        _check(got, ru.window_mean(rows, lo, hi), f"{dtype} window [{lo},{hi})")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tensors_entry_behind_an_odd_sized_tensor(dtype):
    """Tensors at their offsets in one row per model, as ParamLayout.byte_offsets
    places them: everything behind the 10-element bias is off alignment, on the
    input and on the output side, and an empty tensor sits in the middle."""
    n, dt = 5, ru.DTYPES[dtype]
    numels = [10, 4099, 0, 7, 2 * 2048 + 9, 64]
    rows = ru.random_rows(dt, n, sum(numels), seed=12)
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(numels)])[:-1]]
    dev = [r.to(DEV) for r in rows]
    esz = rows[0].element_size()
    assert dev[0].data_ptr() % 16 == 0 and (offs[1] * esz) % 16 != 0
    ptrs = [d.data_ptr() + o * esz for d in dev for o in offs]
    got = _tensors_both_entries(dt, n, numels, ptrs, [o * esz for o in offs], 1, 4)
    _check(got, ru.window_mean(rows, 1, 4), dtype)
    for d, r in zip(dev, rows):
        assert ru.same_bits(d.cpu(), r)


def test_a_batch_on_a_side_stream():
    side = torch.cuda.Stream()
    cases = [Case("f32", n, 30_011 + n, seed=40 + n) for n in (3, 8, 17)]
    side.wait_stream(torch.cuda.current_stream())  # the inputs' copies
    run_and_check(cases, "side stream", stream=side)


def test_overlap_is_refused_and_nothing_runs():
    p = 1000
    buf = torch.zeros(6 * p, device=DEV)
    buf[:4 * p] = 1.0
    a, b, c, d = (buf[k * p:(k + 1) * p] for k in range(4))
    free1, free2 = buf[4 * p:5 * p], buf[5 * p:]
    torch.cuda.synchronize()
    bad = [
        [([a, b], 0, 1, a), ([c, d], 0, 1, free2)],  # a task's output is its own input
        [([a, b], 0, 1, free1), ([c, d], 0, 1, buf[p - 1:2 * p - 1])],  # ... shares bytes with another task's inputs
        [([a, b], 0, 1, free1), ([c, d], 0, 1, buf[5 * p - 1:6 * p - 1])],  # two outputs share one element
        [([a, b], 0, 1, free1), ([c, free1], 0, 1, free2)],  # a task reads what another writes
    ]
    for tasks in bad:
        with pytest.raises(_native.DlsimError) as e:
            _native.robust_reduce_batched(tasks)
        assert e.value.rc == _native.DLSIM_E_ARG and "overlap" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf[:4 * p] == 1.0).all()) and bool((buf[4 * p:] == 0.0).all())
