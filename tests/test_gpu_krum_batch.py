"""dlsim_pairwise_sqdist_batched and model_distances_batch on the MI355X.

The oracle is the flat entry's bits: every task of a batched call must hold
exactly what dlsim_pairwise_sqdist (or dlsim_pairwise_sqdist_tensors) writes
for the same buffers, so no tolerance appears here; one task per dtype is
checked against the longdouble oracle of tests/_krum_util.py as well. Every
batched matrix sits in a 0xA5-guarded buffer (_edge_util.guarded): no guard
byte written, no entry left unwritten, inputs unchanged.

Rows are slices of one pool of random device rows per dtype (inputs may be
shared between tasks), so a case costs its kernels and little else."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import _edge_util as eu
import _krum_util as ku
from sgd_inputs import GNLENET_SHAPES

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import model_distances, model_distances_batch  # noqa: E402

DEV = "cuda"
HUGE = 10 ** 10
DTYPE_NAMES = ["f32", "f64", "bf16", "f16"]
CLASSES = {"four": (2, 3, 4), "eight": (5, 8), "cross": (9, 16, 17, 32)}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_POOLS = {}


def _geometry(n, dtype):
    """(T, B): the tile and the grid cap of n aligned inputs of dtype."""
    return _native.pairdist_geometry(n, eu.DTYPES[dtype], HUGE)


def _pool(dtype):
    """(32 random rows of 2.2 M elements at a 128-byte aligned stride, a copy of their bits): made once per dtype."""
    if dtype not in _POOLS:
        g = torch.Generator(device=DEV).manual_seed(77 + len(_POOLS))
        width = 2_200_064  # a multiple of 64 elements
        rows = (torch.randn(32, width, generator=g, device=DEV, dtype=torch.float32) * 0.5).to(eu.DTYPES[dtype])
        assert rows.data_ptr() % 128 == 0
        _POOLS[dtype] = (rows, rows.view(_INT[rows.element_size()]).clone())
    return _POOLS[dtype]


def _pool_unchanged(dtype):
    rows, saved = _pool(dtype)
    return torch.equal(rows.view(saved.dtype), saved)


def _rows(dtype, n, length, first=0, off=0):
    """n pool rows (from row `first`, wrapping) of `length` elements, `off` elements into the row."""
    rows, _ = _pool(dtype)
    return [rows[(first + i) % 32, off:off + length] for i in range(n)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


def _flat(xs, accumulate=False, prefill=None):
    """The flat entry's matrix for one task, as int64 bit patterns."""
    n = len(xs)
    d2 = torch.empty(n * n, dtype=torch.float64, device=DEV) if prefill is None else prefill.clone()
    _native.pairwise_sqdist(xs, d2, accumulate=accumulate)
    return _bits(d2)


def _batched(tasks, accumulate=False, prefills=None, stream=None):
    """One batched call over tasks = [list of flat tensors], every matrix guarded. Returns the bit patterns."""
    hs = [eu.guarded(len(xs) ** 2 * 8, "f64", DEV) for xs in tasks]
    if prefills is not None:
        for h, p in zip(hs, prefills):
            h.view.copy_(p)
    _native.pairwise_sqdist_batched([(xs, h.view) for xs, h in zip(tasks, hs)], accumulate=accumulate, stream=stream)
    torch.cuda.synchronize()
    for k, h in enumerate(hs):
        assert eu.check_guards(h) == [], f"task {k}: guard bytes written"
        if prefills is None:
            assert eu.unwritten(h) == 0, f"task {k}: entries left unwritten"
    return [_bits(h.view) for h in hs]


def _assert_tasks(tasks, got, want, what):
    for k, (xs, g, w) in enumerate(zip(tasks, got, want)):
        assert np.array_equal(g, w), f"{what}: task {k} (n = {len(xs)}, {xs[0].numel()} elements) differs from the flat entry"


# ---- lengths per class and dtype -------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_lengths_per_class_and_dtype(cls, dtype):
    """Both ends of the class over {1, E-1, E, E+1, T-1, T, T+1, 2T+E+1, BT+T+3}: at the last length a task's
    virtual blocks take two tiles, one tile and the tail while its neighbours in the grid take one or none."""
    E = eu.VEC_ELEMS[dtype]
    tasks = []
    for n in (CLASSES[cls][0], CLASSES[cls][-1]):
        T, B = _geometry(n, dtype)
        assert T == 256 * E and B * T <= 2 * 1024 * 1024
        for k, length in enumerate((1, E - 1, E, E + 1, T - 1, T, T + 1, 2 * T + E + 1, B * T + T + 3)):
            tasks.append(_rows(dtype, n, length, first=3 * k))
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(xs) for xs in tasks], f"{cls} {dtype}")
    assert _pool_unchanged(dtype)
    # one task against the longdouble oracle: the smaller fan-in at 2T + E + 1
    xs = tasks[7]
    rows = np.stack([eu.from_torch(x, dtype) for x in xs])
    problems, worst = ku.matrix_problems(got[7].view(np.float64).reshape(len(xs), len(xs)),
                                         ku.sqdist_oracle(rows, dtype), xs[0].numel())
    print(f"{cls} {dtype}: max err / bound {worst:.4f}")
    assert not problems, problems


# ---- launch limits ---------------------------------------------------------------------------
@pytest.mark.parametrize("count,n", [(40, 3), (30, 8), (7, 32)])
def test_past_each_launch_limit(count, n):
    """32 segments (n = 3), 192 pointers (24 tasks of 8, 6 of 32): the list is split into launches."""
    ms, mp = _native.pairdist_batch_geometry(n, torch.float32)
    assert count > min(ms, mp // n)
    T, _ = _geometry(n, "f32")
    tasks = [_rows("f32", n, T + 5 + k, first=k) for k in range(count)]
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(xs) for xs in tasks], f"{count} tasks of n = {n}")
    assert _pool_unchanged("f32")


# ---- mixed batches ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_classes_interleaved_and_misaligned_tasks(dtype):
    """All three classes in one call, tasks at 2-, 4- and 8-byte offsets (those the dtype allows) among aligned
    ones: a misaligned task takes the scalar form, as the flat entry does."""
    esz = eu.ESIZE[dtype]
    T = 256 * eu.VEC_ELEMS[dtype]
    offs = [b // esz for b in (2, 4, 8) if b % esz == 0]
    tasks = []
    for k, n in enumerate((3, 8, 17, 2, 5, 32, 4, 9, 8, 3, 16, 5)):
        off = offs[k % len(offs)] if k % 2 else 0
        tasks.append(_rows(dtype, n, T + 300 + 7 * k, first=k, off=off))
    assert any(xs[0].data_ptr() % 16 for xs in tasks) and any(xs[0].data_ptr() % 16 == 0 for xs in tasks)
    # a task whose rows are not all aligned alike
    mixed = _rows(dtype, 6, 2 * T + 9)
    mixed[4] = _rows(dtype, 1, 2 * T + 9, first=9, off=offs[0])[0]
    tasks.insert(5, mixed)
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(xs) for xs in tasks], f"mixed {dtype}")
    assert _pool_unchanged(dtype)


def test_degenerate_tasks_in_the_middle():
    T, _ = _geometry(8, "f32")
    tasks = [_rows("f32", 8, T + 1), _rows("f32", 5, 0), _rows("f32", 1, 1000), _rows("f32", 3, 77),
             _rows("f32", 1, 0), _rows("f32", 9, 5)]
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(xs) for xs in tasks], "degenerate")
    assert not got[1].any() and not got[2].any() and not got[4].any()
    # accumulating, such a task writes nothing
    pre = [torch.rand(len(xs) ** 2, dtype=torch.float64, device=DEV) for xs in tasks]
    acc = _batched(tasks, accumulate=True, prefills=pre)
    _assert_tasks(tasks, acc, [_flat(xs, True, p) for xs, p in zip(tasks, pre)], "degenerate, accumulating")
    for k in (1, 2, 4):
        assert np.array_equal(acc[k], _bits(pre[k]))
    assert _native.pairwise_sqdist_batched([]) == []
    _native.pairwise_sqdist_batched_raw([], [], [], [], 0, [], False, None)  # b == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_accumulate_into_prefilled_matrices(dtype):
    T = 256 * eu.VEC_ELEMS[dtype]
    tasks = [_rows(dtype, n, T * 3 + 11 * n, first=n) for n in (2, 4, 7, 8, 12, 32)]
    pre = [torch.rand(len(xs) ** 2, dtype=torch.float64, device=DEV) * 100 for xs in tasks]
    got = _batched(tasks, accumulate=True, prefills=pre)
    _assert_tasks(tasks, got, [_flat(xs, True, p) for xs, p in zip(tasks, pre)], f"accumulate {dtype}")
    assert not any(np.array_equal(g, _bits(p)) for g, p in zip(got, pre))


# ---- the tensors form ------------------------------------------------------------------------
def _tensor_task(n, shapes, seed):
    """n models, each one flat fp32 buffer with its tensors packed back to back (so a tensor behind a 10-element
    one is 8 bytes off alignment). Returns (buffers, model-major pointers, lengths)."""
    sizes = [int(np.prod(s)) for s in shapes]
    g = torch.Generator(device=DEV).manual_seed(seed)
    bufs = [torch.randn(sum(sizes), generator=g, device=DEV) * 0.1 for _ in range(n)]
    ptrs = []
    for b in bufs:
        off = 0
        for s in sizes:
            ptrs.append(b.data_ptr() + 4 * off)
            off += s
    return bufs, ptrs, sizes


def test_tensors_form_on_gnlenet_shapes():
    shapes = [list(GNLENET_SHAPES), [[10]] + list(GNLENET_SHAPES), list(GNLENET_SHAPES)[:5] + [[0]] + [[3, 3]]]
    fans = (8, 5, 17)
    cases = [_tensor_task(n, sh, 40 + n) for n, sh in zip(fans, shapes)]
    assert cases[1][1][1] % 16 == 8  # the tensor behind the 10-element one
    saved = [[b.clone() for b in c[0]] for c in cases]
    code = _native.dtype_code(torch.float32, single_task=True)
    for accumulate in (False, True):
        pre = [torch.rand(n * n, dtype=torch.float64, device=DEV) for n in fans]
        want = []
        for (bufs, ptrs, sizes), n, p in zip(cases, fans, pre):
            d2 = p.clone()
            _native.pairwise_sqdist_tensors_raw(ptrs, n, sizes, code, d2.data_ptr(), accumulate, None)
            want.append(_bits(d2))
        hs = [eu.guarded(n * n * 8, "f64", DEV) for n in fans]
        if accumulate:
            for h, p in zip(hs, pre):
                h.view.copy_(p)
        torch.cuda.synchronize()
        _native.pairwise_sqdist_batched_raw(fans, [len(c[2]) for c in cases], [p for c in cases for p in c[1]],
                                            [s for c in cases for s in c[2]], code, [h.view.data_ptr() for h in hs],
                                            accumulate, None)
        torch.cuda.synchronize()
        for k, (h, w) in enumerate(zip(hs, want)):
            assert eu.check_guards(h) == [] and (accumulate or eu.unwritten(h) == 0)
            assert np.array_equal(_bits(h.view), w), f"task {k}, accumulate {accumulate}"
    assert all(torch.equal(b, s) for c, ss in zip(cases, saved) for b, s in zip(c[0], ss))


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_nans_of_several_tensors_add_as_the_flat_entry_adds_them(dtype):
    """A pair that is NaN in several tensors of a model: from a NaN in the first row, from a NaN in the second
    row (the other sign after the subtraction), from Inf - Inf, in every order, aligned and not. The sum keeps one
    of the NaNs' bits, and which one depends on the operand order of the add: the flat entry's."""
    tdt, esz = eu.DTYPES[dtype], eu.ESIZE[dtype]
    n, sizes = 5, [700, 64, 1300, 10, 2100, 64]
    code = _native.dtype_code(tdt, single_task=True)
    g = torch.Generator(device=DEV).manual_seed(5)
    tasks = []
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1]):
        bufs = [(torch.randn(sum(sizes), generator=g, device=DEV) * 0.3).to(tdt) for _ in range(n)]
        offs = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        for kind, k in zip(order, (0, 2, 4)):  # tensors 0, 2 and 4 make the pair (0, 1) NaN, each in its way
            at = int(offs[k]) + 3
            if kind == 0:
                bufs[0][at] = float("nan")
            elif kind == 1:
                bufs[1][at] = float("nan")
            else:
                bufs[0][at] = bufs[1][at] = float("inf")
        ptrs = [b.data_ptr() + esz * int(o) for b in bufs for o in offs]
        tasks.append((bufs, ptrs))
    want = []
    for bufs, ptrs in tasks:
        d2 = torch.empty(n * n, dtype=torch.float64, device=DEV)
        _native.pairwise_sqdist_tensors_raw(ptrs, n, sizes, code, d2.data_ptr(), False, None)
        want.append(_bits(d2))
    hs = [eu.guarded(n * n * 8, "f64", DEV) for _ in tasks]
    torch.cuda.synchronize()
    _native.pairwise_sqdist_batched_raw([n] * len(tasks), [len(sizes)] * len(tasks), [p for _, ps in tasks for p in ps],
                                        sizes * len(tasks), code, [h.view.data_ptr() for h in hs], False, None)
    torch.cuda.synchronize()
    for k, (h, w) in enumerate(zip(hs, want)):
        assert eu.check_guards(h) == [] and eu.unwritten(h) == 0
        got = _bits(h.view)
        assert np.isnan(got.view(np.float64).reshape(n, n)[0, 1])
        assert np.array_equal(got, w), f"task {k}: {[hex(v) for v in got[got != w]]} against {[hex(v) for v in w[got != w]]}"


# ---- sharing ---------------------------------------------------------------------------------
def test_shared_rows_and_the_same_pointer_twice():
    T, _ = _geometry(5, "f32")
    shared = _rows("f32", 1, 2 * T + 3, first=31)[0]
    tasks = []
    for k in range(5):  # a ring: one model is a row of five tasks
        xs = _rows("f32", 5, 2 * T + 3, first=4 * k)
        xs[k] = shared
        tasks.append(xs)
    twice = _rows("f32", 8, T + 9)
    twice[6] = twice[1]
    tasks.append(twice)
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(xs) for xs in tasks], "sharing")
    assert got[5].reshape(8, 8)[1, 6] == 0 and got[5].reshape(8, 8)[6, 1] == 0  # +0.0
    assert _pool_unchanged("f32")


# ---- specials --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_specials_stay_in_their_task(dtype):
    """A NaN row, a +Inf row and +Inf against -Inf at _edge_util.edge_positions of one task: exact value classes
    there, and every other task's matrix bitwise what it is without them."""
    n = 8
    T, _ = _geometry(n, dtype)
    E = eu.VEC_ELEMS[dtype]
    p = 2 * T + T // 2 + E + (E - 1)
    pos = eu.edge_positions(p, T, E)
    assert len(pos) == 5
    clean = [x.clone() for x in _rows(dtype, n, p, first=5)]
    bad = [x.clone() for x in clean]
    idx = torch.tensor(pos, device=DEV)
    bad[1][idx] = float("nan")
    bad[3][idx] = float("inf")
    bad[5][idx] = float("inf")
    bad[6][idx] = float("-inf")
    others = [_rows(dtype, 3, p, first=1), _rows(dtype, 8, T + 1, first=2), _rows(dtype, 17, 600, first=3)]
    without = _batched(others[:1] + [clean] + others[1:])
    got = _batched(others[:1] + [bad] + others[1:])
    for k in (0, 2, 3):
        assert np.array_equal(got[k], without[k]), f"task {k} changed with its neighbour's specials"
    assert np.array_equal(got[1], _flat(bad))
    m = got[1].view(np.float64).reshape(n, n)
    rows = np.stack([eu.from_torch(x, dtype) for x in bad])
    problems, _ = ku.matrix_problems(m, ku.sqdist_oracle(rows, dtype), p)
    assert not problems, problems
    assert np.isnan(np.delete(m[1], 1)).all()  # the NaN row
    assert np.isnan(m[3, 5]) and m[3, 6] == np.inf and m[5, 6] == np.inf and m[0, 3] == np.inf
    assert np.isfinite(m[np.ix_([0, 2, 4, 7], [0, 2, 4, 7])]).all()


# ---- repeatability and streams ---------------------------------------------------------------
def test_a_second_call_and_a_side_stream_give_the_same_bits():
    T, _ = _geometry(8, "bf16")
    tasks = [_rows("bf16", n, 3 * T + 17, first=n) for n in (3, 8, 20, 8, 4)]
    first = _batched(tasks)
    again = _batched(tasks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _batched(tasks, stream=side)
    for a, b, c in zip(first, again, third):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    _assert_tasks(tasks, first, [_flat(xs) for xs in tasks], "streams")


# ---- refused overlaps ------------------------------------------------------------------------
def test_refused_overlaps_leave_the_buffers_unchanged():
    xs, ys = _rows("f32", 3, 1000), _rows("f32", 3, 1000, first=3)
    h = eu.guarded(2 * 9 * 8, "f64", DEV)
    d2 = h.view
    before = _bits(d2)
    rows, _ = _pool("f32")
    on_input = rows[4].view(torch.int64).view(torch.float64)[:9]  # the first 72 bytes of task 1's row 1
    calls = {
        "its own input": [(ys, on_input), (xs, d2[:9])],
        "another task's input": [(xs, on_input), (ys, d2[:9])],
        "another matrix, one shared double": [(xs, d2[:9]), (ys, d2[8:17])],
    }
    for what, tasks in calls.items():
        with pytest.raises(_native.DlsimError, match="overlap") as e:
            _native.pairwise_sqdist_batched(tasks)
        assert e.value.rc == -1, what
    # down to one shared byte: a matrix that ends one byte into the other
    raw = [[3, 3], [1, 1], [x.data_ptr() for x in xs + ys], [1000, 1000], 0]
    base = d2.data_ptr()
    with pytest.raises(_native.DlsimError, match="overlap"):
        _native.pairwise_sqdist_batched_raw(*raw, [base, base + 71], False, None)
    with pytest.raises(_native.DlsimError, match="overlap"):
        _native.pairwise_sqdist_batched_raw(*raw, [base + 72, xs[2].data_ptr() + 3999], False, None)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d2), before) and eu.check_guards(h) == []
    assert _pool_unchanged("f32")
    # one byte further is accepted
    _native.pairwise_sqdist_batched_raw(*raw, [base, base + 72], False, None)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == [] and eu.unwritten(h) == 0


# ---- model_distances_batch -------------------------------------------------------------------
class _TwoGroups(torch.nn.Module):
    """fp32 and bf16 parameters; `bf16_first` decides which dtype group the layout meets first."""

    def __init__(self, seed, bf16_first):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        specs = [((10,), torch.float32), ((37, 29), torch.float32), ((33, 5), torch.bfloat16), ((4100,), torch.float32),
                 ((7,), torch.bfloat16)]
        if bf16_first:
            specs = [specs[2], specs[4], specs[0], specs[1], specs[3]]
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).to(dt)) for s, dt in specs])


def _same_matrix(a, b):
    return a.shape == b.shape and np.array_equal(a.numpy().view(np.int64), b.numpy().view(np.int64))


def test_model_distances_batch_on_every_route():
    hosts = {False: [_TwoGroups(i, False) for i in range(9)], True: [_TwoGroups(50 + i, True) for i in range(6)]}
    arenas = {k: [arena.to_device_arena(m, DEV) for m in v] for k, v in hosts.items()}
    separate = {k: [copy.deepcopy(m).to(DEV) for m in v] for k, v in hosts.items()}  # one allocation per parameter
    mixed = [arenas[False][0], separate[False][1], arenas[False][2], separate[False][3], separate[False][4]]
    tasks = [arenas[False], separate[True], mixed, arenas[True][:3], separate[False][:8], hosts[False][:3],
             arenas[False][:1]]
    got = model_distances_batch(tasks)
    assert len(got) == len(tasks)
    for k, (models, d2) in enumerate(zip(tasks, got)):
        want = model_distances(models)
        assert not d2.is_cuda and d2.dtype == torch.float64 and _same_matrix(d2, want), f"task {k}"
    assert float(got[0][0, 1]) > 0 and not got[6].any()
    # the two layout orders add their dtype groups in their own order: the matrices differ from the swapped order
    assert [dt for dt in arena.input_arenas(arenas[False][:2])[0].groups] == [torch.float32, torch.bfloat16]
    assert [dt for dt in arena.input_arenas(arenas[True][:2])[0].groups] == [torch.bfloat16, torch.float32]


def test_model_distances_batch_never_calls_the_per_task_entries(monkeypatch):
    """Device-resident tasks (a ring: every model a row of five tasks) go through the batched entry alone."""
    torch.manual_seed(3)
    models = [arena.to_device_arena(torch.nn.Linear(40, 30), DEV) for _ in range(12)]
    tasks = [models[k:k + 5] for k in range(6)]
    want = [model_distances(t) for t in tasks]

    def refuse(*a, **k):
        raise AssertionError("a per-task distance call")
    monkeypatch.setattr(_native, "pairwise_sqdist", refuse)
    monkeypatch.setattr(_native, "pairwise_sqdist_tensors_raw", refuse)
    got = model_distances_batch(tasks)
    assert all(_same_matrix(a, b) for a, b in zip(got, want))


def test_models_without_parameters_give_the_zeros_of_model_distances():
    """A task of parameterless models between two real ones: n x n zeros, as model_distances gives."""
    from dasklearn_amd.gradient_aggregation.krum import _resident_entry
    from dasklearn_amd.model_inputs import distances_arena_tasks
    from dasklearn_amd.wave_tasks import ArenaTask
    torch.manual_seed(5)
    bare = [torch.nn.ReLU() for _ in range(4)]
    layout, params, views = arena.input_arenas(bare)
    real = [arena.to_device_arena(torch.nn.Linear(9, 7), DEV) for _ in range(3)]
    entry = _resident_entry(real, None)
    got = distances_arena_tasks([entry, ArenaTask(bare[0], layout, views, None, params), entry])
    want = model_distances(bare, device=DEV)
    assert want.shape == (4, 4) and not want.any() and _same_matrix(got[1], want)
    assert _same_matrix(got[0], model_distances(real)) and _same_matrix(got[2], got[0])
