"""dlsim_wreduce_dist_batched and consensus_distance_batch on the MI355X.

The oracle is the flat entry's bits: every task of a batched call must hold
exactly what dlsim_wreduce_dist (or dlsim_wreduce_dist_tensors) writes for the
same buffers, output and distance vector, so no tolerance appears there; one
task per dtype and class is checked against the FedAvg oracle and the
longdouble distance oracle of tests/_geomed_util.py as well, so that the
siblings cannot agree on a wrong answer. Every batched output and vector sits
in a 0xA5-guarded buffer (_edge_util.guarded): no guard byte written, no
element left unwritten, inputs unchanged. The flat reference writes into a
buffer at the same misalignment, since the output's base selects the form,
and that buffer is prefilled with zeros: an fp16 or bf16 mean can equal the
0xA5A5 pattern by chance, so an output element counts as unwritten when it
holds the pattern where the flat entry's does not, which the comparison of
the two finds.

Rows are slices of one pool of random device rows per dtype (inputs may be
shared between tasks), so a case costs its kernels and little else."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import _edge_util as eu
import _geomed_util as gu
from sgd_inputs import GNLENET_SHAPES

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena  # noqa: E402
from dasklearn_amd.gradient_aggregation import geomed  # noqa: E402

DEV = "cuda"
HUGE = 10 ** 10
DTYPE_NAMES = ["f32", "f64", "bf16", "f16"]
CLASSES = {"cap4": (1, 4), "cap8": (5, 8), "cap16": (9, 16), "cap32": (17, 32)}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_WIDTH = {"f32": 1_100_032, "f64": 16_384, "bf16": 16_384, "f16": 16_384}  # multiples of 64 elements
_POOLS = {}


def _geometry(n, dtype):
    """(T, B): the tile and the grid cap of n aligned inputs of dtype."""
    return _native.reducedist_geometry(n, eu.DTYPES[dtype], HUGE)


def _pool(dtype):
    """(32 random rows at a 128-byte aligned stride, a copy of their bits): made once per dtype."""
    if dtype not in _POOLS:
        g = torch.Generator(device=DEV).manual_seed(91 + len(_POOLS))
        rows = (torch.randn(32, _WIDTH[dtype], generator=g, device=DEV, dtype=torch.float32) * 0.5).to(eu.DTYPES[dtype])
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


def _weights(n, dtype, seed=0):
    """Dirichlet weights as the entry takes them: fp32-representable unless the buffers are fp64."""
    w = np.random.default_rng(300 + 37 * n + seed).dirichlet(np.ones(n))
    return [float(v) if dtype == "f64" else float(np.float32(v)) for v in w]


class Task:
    """One flat task: rows, weights, and where its output goes (out_off bytes off alignment; None: no output)."""

    def __init__(self, dtype, xs, w=None, out_off=0, seed=0):
        self.dtype, self.xs, self.out_off = dtype, xs, out_off
        self.w = _weights(len(xs), dtype, seed) if w is None else w

    @property
    def nbytes(self):
        return self.xs[0].numel() * eu.ESIZE[self.dtype]


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy().copy()


def _out_bits(h):
    return eu.bits_of(eu.from_torch(h.view, h.dtype), h.dtype).copy()


def _flat(t, accumulate=False, prefill=None):
    """The flat entry's (output bits or None, vector bits) for one task, the output at the task's misalignment."""
    n = len(t.xs)
    d2 = torch.empty(n, dtype=torch.float64, device=DEV) if prefill is None else prefill.clone()
    h = None if t.out_off is None else eu.guarded(t.nbytes, t.dtype, DEV, offset=t.out_off)
    if h is not None:
        h.view.zero_()  # another prefill than the batched side's (the module docstring)
    _native.wreduce_dist(t.xs, t.w, None if h is None else h.view, d2, accumulate=accumulate)
    torch.cuda.synchronize()
    return (None if h is None else _out_bits(h)), _bits64(d2)


def _batched(tasks, accumulate=False, prefills=None, stream=None):
    """One batched call, every output and vector guarded. Returns [(output bits or None, vector bits)]."""
    outs = [None if t.out_off is None else eu.guarded(t.nbytes, t.dtype, DEV, offset=t.out_off) for t in tasks]
    vecs = [eu.guarded(len(t.xs) * 8, "f64", DEV) for t in tasks]
    if prefills is not None:
        for h, p in zip(vecs, prefills):
            h.view.copy_(p)
    torch.cuda.synchronize()
    _native.wreduce_dist_batched([(t.xs, t.w, None if o is None else o.view, v.view)
                                  for t, o, v in zip(tasks, outs, vecs)], accumulate=accumulate, stream=stream)
    torch.cuda.synchronize()
    res = []
    for k, (t, o, v) in enumerate(zip(tasks, outs, vecs)):
        assert eu.check_guards(v) == [], f"task {k}: guard bytes of the vector written"
        if prefills is None:
            assert eu.unwritten(v) == 0, f"task {k}: vector entries left unwritten"
        if o is not None:
            assert eu.check_guards(o) == [], f"task {k}: guard bytes of the output written"
        res.append((None if o is None else _out_bits(o), _bits64(v.view)))
    return res


def _assert_tasks(tasks, got, want, what):
    for k, (t, g, w) in enumerate(zip(tasks, got, want)):
        where = f"{what}: task {k} (n = {len(t.xs)}, {t.xs[0].numel()} elements)"
        assert (g[0] is None) == (w[0] is None)
        if g[0] is not None:
            assert np.array_equal(g[0], w[0]), f"{where}: output differs from the flat entry"
        assert np.array_equal(g[1], w[1]), f"{where}: vector differs from the flat entry"


def _assert_oracle(t, got, what):
    """One task against the FedAvg oracle (output bits) and the longdouble distances ((P + 8) * 2^-53)."""
    dtype = t.dtype
    rows = np.stack([eu.from_torch(x, dtype) for x in t.xs])
    w = np.asarray(t.w, dtype=np.float64 if dtype == "f64" else np.float32)
    want_out = gu.fold_oracle(rows, w, dtype)
    out = got[0].view(eu._STORE[dtype])
    assert eu.same_bits(out, want_out, dtype), f"{what}: " + eu.diff_report(out, want_out, dtype)
    problems, worst = gu.vector_problems(got[1].view(np.float64), gu.dist_oracle(rows, want_out, dtype), rows.shape[1])
    print(f"{what}: max err / bound {worst:.4f}")
    assert not problems, f"{what}: {problems}"


# ---- lengths per class and dtype -------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_lengths_per_class_and_dtype(cls, dtype):
    """Both ends of the class over {1, T-1, T, T+1, 2T+E+1, 3T}, E the elements of one lane's vector."""
    tasks = []
    for n in CLASSES[cls]:
        T, B = _geometry(n, dtype)
        E = T // 256
        assert B == 1024 and E * eu.ESIZE[dtype] in (4, 8, 16)
        for k, length in enumerate((1, T - 1, T, T + 1, 2 * T + E + 1, 3 * T)):
            tasks.append(Task(dtype, _rows(dtype, n, length, first=3 * k), seed=k))
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], f"{cls} {dtype}")
    assert _pool_unchanged(dtype)
    _assert_oracle(tasks[4], got[4], f"{cls} {dtype} n={len(tasks[4].xs)} at 2T+E+1")


@pytest.mark.parametrize("n", [2, 32])
def test_a_segment_whose_blocks_stride(n):
    """Just past 1024 tiles: block 0 of the segment takes two tiles, block 1 the partial one, the last the tail,
    between two small neighbours in the grid."""
    T, B = _geometry(n, "f32")
    tasks = [Task("f32", _rows("f32", 3, 77, first=1)), Task("f32", _rows("f32", n, B * T + T + 3)),
             Task("f32", _rows("f32", n, T + 1, first=5))]
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], f"striding n = {n}")
    assert _pool_unchanged("f32")


# ---- launch limits ---------------------------------------------------------------------------
@pytest.mark.parametrize("count,n,dtype", [(40, 3, "f32"), (7, 32, "f32"), (5, 32, "f64")])
def test_past_each_launch_limit(count, n, dtype):
    """32 segments (n = 3), 192 pointers (6 tasks of 32; fp64's double weights leave 128: 4 tasks)."""
    ms, mp = _native.reducedist_batch_geometry(n, eu.DTYPES[dtype])
    assert (ms, mp) == (32, 128 if dtype == "f64" else 192)
    assert count > min(ms, mp // n)
    T, _ = _geometry(n, dtype)
    tasks = [Task(dtype, _rows(dtype, n, T + 5 + k, first=k), seed=k) for k in range(count)]
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], f"{count} tasks of n = {n} {dtype}")
    assert _pool_unchanged(dtype)


# ---- mixed batches ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_classes_interleaved_misaligned_and_null_outputs(dtype):
    """All four classes in one call; bases one element off among aligned ones, an aligned task with a misaligned
    output, a task whose rows are not aligned alike, and tasks without an output among tasks with one."""
    esz = eu.ESIZE[dtype]
    T = 256 * eu.VEC_ELEMS[dtype]
    tasks = []
    for k, n in enumerate((3, 8, 17, 2, 5, 32, 4, 9, 8, 1, 16, 5)):
        off = 1 if k % 2 else 0  # elements
        out_off = None if k % 3 == 2 else esz if k % 4 == 1 else 0
        tasks.append(Task(dtype, _rows(dtype, n, T + 300 + 7 * k, first=k, off=off), out_off=out_off, seed=k))
    assert any(t.xs[0].data_ptr() % 16 for t in tasks) and any(t.xs[0].data_ptr() % 16 == 0 for t in tasks)
    tasks.append(Task(dtype, _rows(dtype, 6, 2 * T + 9), out_off=esz))  # aligned rows, misaligned output
    mixed = _rows(dtype, 6, 2 * T + 9)
    mixed[4] = _rows(dtype, 1, 2 * T + 9, first=9, off=1)[0]
    tasks.insert(5, Task(dtype, mixed))
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], f"mixed {dtype}")
    assert any(g[0] is None for g in got) and any(g[0] is not None for g in got)
    assert _pool_unchanged(dtype)


def test_degenerate_tasks_in_the_middle():
    """Length 0, fan-in 1 (a real reduce here: w * x and its distance), and through the raw entry a task without
    a tensor: zeros, or nothing when accumulating."""
    T, _ = _geometry(8, "f32")
    tasks = [Task("f32", _rows("f32", 8, T + 1)), Task("f32", _rows("f32", 5, 0)),
             Task("f32", _rows("f32", 1, 1000), w=[1.0]), Task("f32", _rows("f32", 3, 77)),
             Task("f32", _rows("f32", 1, 0), w=[0.5]), Task("f32", _rows("f32", 1, 333), w=[0.25], out_off=None),
             Task("f32", _rows("f32", 9, 5))]
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], "degenerate")
    assert not got[1][1].any() and not got[2][1].any() and not got[4][1].any() and got[5][1].any()
    assert np.array_equal(got[2][0], eu.bits_of(eu.from_torch(tasks[2].xs[0], "f32"), "f32"))  # 1.0 * x, finite x
    pre = [torch.rand(len(t.xs), dtype=torch.float64, device=DEV) for t in tasks]
    acc = _batched(tasks, accumulate=True, prefills=pre)
    _assert_tasks(tasks, acc, [_flat(t, True, p) for t, p in zip(tasks, pre)], "degenerate, accumulating")
    for k in (1, 4):
        assert np.array_equal(acc[k][1], _bits64(pre[k]))
    # no tensor at all, between two tasks with one
    code = _native.dtype_code(torch.float32, single_task=True)
    xs, ys = tasks[0].xs, tasks[3].xs
    for accumulate in (False, True):
        hs = [eu.guarded(n * 8, "f64", DEV) for n in (8, 4, 3)]
        for h in hs:
            h.view.fill_(3.0)
        _native.wreduce_dist_batched_raw([8, 4, 3], [1, 0, 1], [x.data_ptr() for x in xs + ys], [T + 1, 77], [0, 0],
                                         tasks[0].w + [0.25] * 4 + tasks[3].w, [None, None, None], code,
                                         [h.view.data_ptr() for h in hs], accumulate, None)
        torch.cuda.synchronize()
        assert all(eu.check_guards(h) == [] for h in hs)
        assert (hs[1].view == (3.0 if accumulate else 0.0)).all()
        for h, t in ((hs[0], tasks[0]), (hs[2], tasks[3])):
            null = Task("f32", t.xs, w=t.w, out_off=None)
            assert np.array_equal(_bits64(h.view), _flat(null, accumulate, torch.full_like(h.view, 3.0))[1])
    assert _native.wreduce_dist_batched([]) == []
    _native.wreduce_dist_batched_raw([], [], [], [], [], [], [], 0, [], False, None)  # b == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_accumulate_into_prefilled_vectors(dtype):
    T = 256 * eu.VEC_ELEMS[dtype]
    tasks = [Task(dtype, _rows(dtype, n, T * 3 + 11 * n, first=n)) for n in (2, 4, 7, 8, 12, 32)]
    pre = [torch.rand(len(t.xs), dtype=torch.float64, device=DEV) * 100 for t in tasks]
    got = _batched(tasks, accumulate=True, prefills=pre)
    _assert_tasks(tasks, got, [_flat(t, True, p) for t, p in zip(tasks, pre)], f"accumulate {dtype}")
    assert not any(np.array_equal(g[1], _bits64(p)) for g, p in zip(got, pre))


# ---- the tensors form ------------------------------------------------------------------------
def _tensor_task(n, shapes, seed, tdt=torch.float32):
    """n models, each one flat buffer with its tensors packed back to back (so a tensor behind a 10-element
    fp32 one is 8 bytes off alignment). Returns (buffers, model-major pointers, lengths, byte offsets)."""
    sizes = [int(np.prod(s)) for s in shapes]
    g = torch.Generator(device=DEV).manual_seed(seed)
    bufs = [(torch.randn(sum(sizes), generator=g, device=DEV) * 0.1).to(tdt) for _ in range(n)]
    esz = bufs[0].element_size()
    offs = [int(o) * esz for o in np.concatenate([[0], np.cumsum(sizes)])[:-1]]
    ptrs = [b.data_ptr() + o for b in bufs for o in offs]
    return bufs, ptrs, sizes, offs


def _run_tensor_tasks(cases, fans, ws, tdt, accumulate, with_out, batched):
    """The tasks through the batched entry, or one by one through dlsim_wreduce_dist_tensors: [(output bits or
    None, vector bits)], outputs and vectors guarded and prefilled alike."""
    dtype = {v: k for k, v in eu.DTYPES.items()}[tdt]
    code = _native.dtype_code(tdt, single_task=True)
    esz = eu.ESIZE[dtype]
    outs = [eu.guarded(sum(c[2]) * esz, dtype, DEV) if wo else None for c, wo in zip(cases, with_out)]
    vecs = [eu.guarded(n * 8, "f64", DEV) for n in fans]
    if accumulate:
        for k, h in enumerate(vecs):
            h.view.copy_(torch.arange(1, fans[k] + 1, dtype=torch.float64) * 0.37)
    if not batched:
        for o in outs:
            if o is not None:
                o.view.zero_()  # another prefill than the batched side's
    torch.cuda.synchronize()
    if batched:
        _native.wreduce_dist_batched_raw(fans, [len(c[2]) for c in cases], [p for c in cases for p in c[1]],
                                         [s for c in cases for s in c[2]], [o for c in cases for o in c[3]],
                                         [v for w in ws for v in w],
                                         [None if o is None else o.view.data_ptr() for o in outs], code, [h.view.data_ptr() for h in vecs], accumulate, None)
    else:
        for c, n, w, o, h in zip(cases, fans, ws, outs, vecs):
            _native.wreduce_dist_tensors_raw(c[1], n, c[2], c[3], w, None if o is None else o.view.data_ptr(), code,
                                             h.view.data_ptr(), accumulate, None)
    torch.cuda.synchronize()
    res = []
    for o, h in zip(outs, vecs):
        assert eu.check_guards(h) == [] and (accumulate or eu.unwritten(h) == 0)
        assert o is None or eu.check_guards(o) == []
        res.append((None if o is None else _out_bits(o), _bits64(h.view)))
    return res


def test_tensors_form_on_gnlenet_shapes():
    shapes = [list(GNLENET_SHAPES), [[10]] + list(GNLENET_SHAPES), list(GNLENET_SHAPES)[:5] + [[0]] + [[3, 3]],
              list(GNLENET_SHAPES)]
    fans = (8, 5, 17, 1)
    cases = [_tensor_task(n, sh, 40 + n) for n, sh in zip(fans, shapes)]
    assert cases[1][1][1] % 16 == 8  # the tensor behind the 10-element one
    ws = [_weights(n, "f32") for n in fans]
    saved = [[b.clone() for b in c[0]] for c in cases]
    for accumulate in (False, True):
        for with_out in ((True, True, True, True), (True, False, True, False)):
            want = _run_tensor_tasks(cases, fans, ws, torch.float32, accumulate, with_out, batched=False)
            got = _run_tensor_tasks(cases, fans, ws, torch.float32, accumulate, with_out, batched=True)
            for k, (g, w) in enumerate(zip(got, want)):
                assert (g[0] is None) == (w[0] is None) and (g[0] is None or np.array_equal(g[0], w[0])), f"task {k}"
                assert np.array_equal(g[1], w[1]), f"task {k}, accumulate {accumulate}"
    assert all(torch.equal(b, s) for c, ss in zip(cases, saved) for b, s in zip(c[0], ss))


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_nans_of_several_tensors_add_as_the_flat_entry_adds_them(dtype):
    """An input whose distance is NaN in several tensors of a model: from its own NaN (either sign), from a NaN
    of the output that another input's NaN made, from Inf - Inf, in every order, aligned and not. The sum keeps
    one of the NaNs' bits, and which one depends on the operand order of the add: the flat entry's."""
    tdt = eu.DTYPES[dtype]
    n, sizes = 5, [700, 64, 1300, 10, 2100, 64]
    tasks = []
    for t, order in enumerate(([0, 1, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1])):
        bufs, ptrs, _, offs = _tensor_task(n, [[s] for s in sizes], 5 + t, tdt)
        esz = bufs[0].element_size()
        for kind, k in zip(order, (0, 2, 4)):
            at = offs[k] // esz + 3
            if kind == 0:
                bufs[0][at] = float("nan")
            elif kind == 1:
                bufs[1][at] = -float("nan")
            else:
                bufs[0][at] = float("inf")
                bufs[1][at] = float("-inf")
        tasks.append((bufs, ptrs, sizes, offs))
    fans, ws = [n] * len(tasks), [_weights(n, dtype, k) for k in range(len(tasks))]
    for with_out in (True, False):
        want = _run_tensor_tasks(tasks, fans, ws, tdt, False, [with_out] * len(tasks), batched=False)
        got = _run_tensor_tasks(tasks, fans, ws, tdt, False, [with_out] * len(tasks), batched=True)
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.isnan(g[1].view(np.float64)).all()
            assert np.array_equal(g[1], w[1]), f"task {k}: {[hex(v) for v in g[1]]} against {[hex(v) for v in w[1]]}"
            assert g[0] is None or np.array_equal(g[0], w[0])


# ---- sharing ---------------------------------------------------------------------------------
def test_shared_rows_and_the_same_pointer_twice():
    T, _ = _geometry(5, "f32")
    shared = _rows("f32", 1, 2 * T + 3, first=31)[0]
    tasks = []
    for k in range(5):  # a ring: one model is a row of five tasks
        xs = _rows("f32", 5, 2 * T + 3, first=4 * k)
        xs[k] = shared
        tasks.append(Task("f32", xs, seed=k))
    twice = _rows("f32", 8, T + 9)
    twice[6] = twice[1]
    tasks.append(Task("f32", twice))
    got = _batched(tasks)
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], "sharing")
    assert got[5][1][1] == got[5][1][6]
    assert _pool_unchanged("f32")


# ---- specials --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_specials_stay_in_their_task(dtype):
    """_edge_util's block of signed zeros, Inf, NaN, subnormals and overflowing sums at the tile, partial-tile
    and tail edges of one task: the flat entry's bits and the oracle's value classes there, and every other
    task's output and vector bitwise what they are without them."""
    n = 8
    T, _ = _geometry(n, dtype)
    E = T // 256
    p = 2 * T + T // 2 + E + (E - 1)
    pos = eu.edge_positions(p, T, E)
    assert len(pos) == 5 or E == 1
    bad_rows = eu.special_rows(dtype, n, p, pos, seed=700)
    clean_rows = eu.random_rows(dtype, n, p, seed=700)
    bad, clean = eu.place(list(bad_rows), dtype, DEV), eu.place(list(clean_rows), dtype, DEV)
    w = _weights(n, dtype)
    others = [Task(dtype, _rows(dtype, 3, p, first=1)), Task(dtype, _rows(dtype, 8, T + 1, first=2)),
              Task(dtype, _rows(dtype, 17, 600, first=3))]
    without = _batched(others[:1] + [Task(dtype, clean, w=w)] + others[1:])
    tb = Task(dtype, bad, w=w)
    tasks = others[:1] + [tb] + others[1:]
    got = _batched(tasks)
    for k in (0, 2, 3):
        assert np.array_equal(got[k][0], without[k][0]) and np.array_equal(got[k][1], without[k][1]), \
            f"task {k} changed with its neighbour's specials"
    _assert_tasks(tasks, got, [_flat(t) for t in tasks], f"specials {dtype}")
    _assert_oracle(tb, got[1], f"specials {dtype}")
    assert eu.inputs_unchanged(bad, bad_rows, dtype)
    assert not np.isfinite(got[1][1].view(np.float64)).all() and np.isfinite(without[1][1].view(np.float64)).all()


# ---- repeatability and streams ---------------------------------------------------------------
def test_a_second_call_and_a_side_stream_give_the_same_bits():
    T, _ = _geometry(8, "bf16")
    tasks = [Task("bf16", _rows("bf16", n, 3 * T + 17, first=n)) for n in (3, 8, 20, 8, 4)]
    first = _batched(tasks)
    again = _batched(tasks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _batched(tasks, stream=side)
    for a, b, c in zip(first, again, third):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    _assert_tasks(tasks, first, [_flat(t) for t in tasks], "streams")


# ---- refused overlaps ------------------------------------------------------------------------
def test_refused_overlaps_leave_the_buffers_unchanged():
    xs, ys, zs = _rows("f32", 3, 1000), _rows("f32", 3, 1000, first=3), _rows("f32", 3, 4, first=6)
    w = _weights(3, "f32")
    hv = eu.guarded(2 * 3 * 8, "f64", DEV)
    ho = eu.guarded(2 * 4000, "f32", DEV)
    d2, out = hv.view, ho.view
    before = _bits64(d2)
    rows, _ = _pool("f32")
    vec_on_input = rows[4].view(torch.int64).view(torch.float64)[:3]  # the first 24 bytes of task 1's row 1
    calls = {
        "a vector on its own input": [(ys, w, None, vec_on_input), (xs, w, None, d2[:3])],
        "a vector on another task's input": [(xs, w, None, vec_on_input), (ys, w, None, d2[:3])],
        "two vectors, one shared double": [(xs, w, None, d2[:3]), (ys, w, None, d2[2:5])],
        "an output on another task's input": [(xs, w, ys[1], d2[:3]), (ys, w, None, d2[3:])],
        "two outputs, one shared element": [(xs, w, out[:1000], d2[:3]), (ys, w, out[999:1999], d2[3:])],
        "an output on another task's vector": [(zs, w, d2[4:6].view(torch.float32), d2[:3]), (ys, w, None, d2[3:])],
    }
    for what, tasks in calls.items():
        with pytest.raises(_native.DlsimError, match="overlap") as e:
            _native.wreduce_dist_batched(tasks)
        assert e.value.rc == -1, what
    # down to one shared byte, through the raw entry: a vector that ends one byte into the other, an output that
    # ends one byte into an input
    code = _native.dtype_code(torch.float32, single_task=True)
    raw = [[3, 3], [1, 1], [x.data_ptr() for x in xs + ys], [1000, 1000], [0, 0], w + w]
    base, obase = d2.data_ptr(), out.data_ptr()
    with pytest.raises(_native.DlsimError, match="overlap"):
        _native.wreduce_dist_batched_raw(*raw, [None, None], code, [base, base + 23], False, None)
    with pytest.raises(_native.DlsimError, match="overlap"):
        _native.wreduce_dist_batched_raw(*raw, [obase, ys[0].data_ptr() - 3999], code, [base, base + 24], False, None)
    torch.cuda.synchronize()
    assert np.array_equal(_bits64(d2), before) and eu.check_guards(hv) == [] and eu.check_guards(ho) == []
    assert eu.unwritten(ho) == 2000 and _pool_unchanged("f32")
    # one byte further is accepted
    _native.wreduce_dist_batched_raw(*raw, [obase, obase + 4000], code, [base, base + 24], False, None)
    torch.cuda.synchronize()
    assert eu.check_guards(hv) == [] and eu.unwritten(hv) == 0 and eu.check_guards(ho) == [] and eu.unwritten(ho) == 0


# ---- consensus_distance_batch ----------------------------------------------------------------
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


def _param_bits(m):
    return [p.detach().cpu().contiguous().view(_INT[p.element_size()]).numpy().copy() for p in m.parameters()]


def _same_result(a, b):
    (ma, da), (mb, db) = a, b
    return (da.shape == db.shape and np.array_equal(da.numpy().view(np.int64), db.numpy().view(np.int64))
            and all(np.array_equal(x, y) for x, y in zip(_param_bits(ma), _param_bits(mb)))
            and [p.device for p in ma.parameters()] == [p.device for p in mb.parameters()])


def test_consensus_distance_batch_on_every_route():
    hosts = {False: [_TwoGroups(i, False) for i in range(9)], True: [_TwoGroups(50 + i, True) for i in range(6)]}
    arenas = {k: [arena.to_device_arena(m, DEV) for m in v] for k, v in hosts.items()}
    separate = {k: [copy.deepcopy(m).to(DEV) for m in v] for k, v in hosts.items()}  # one allocation per parameter
    mixed = [arenas[False][0], separate[False][1], arenas[False][2], separate[False][3], separate[False][4]]
    tasks = [(arenas[False], None), (separate[True], [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.03125]), (mixed, None),
             (arenas[True][:3], [0.25, 0.5, 0.25]), (separate[False][:8], None), (hosts[False][:3], None),
             (arenas[False][:1], None)]
    got = geomed.consensus_distance_batch(tasks)
    assert len(got) == len(tasks)
    for k, ((models, weights), g) in enumerate(zip(tasks, got)):
        want = geomed.consensus_distance(models, weights)
        assert not g[1].is_cuda and g[1].dtype == torch.float64 and _same_result(g, want), f"task {k}"
    assert float(got[0][1][1]) > 0 and not got[6][1].any()
    with pytest.raises(AssertionError):
        geomed.consensus_distance_batch([(arenas[False][:3], [0.5, 0.5])])
    with pytest.raises(IndexError):
        geomed.consensus_distance_batch([(arenas[False][:3], None), ([], None)])


def test_consensus_distance_batch_never_calls_the_per_task_entries(monkeypatch):
    """Device-resident tasks (a ring: every model a row of five tasks) go through the batched entry alone."""
    torch.manual_seed(3)
    models = [arena.to_device_arena(torch.nn.Linear(40, 30), DEV) for _ in range(12)]
    sep = [copy.deepcopy(m).to(DEV) for m in models[:5]]
    tasks = [(models[k:k + 5], None) for k in range(6)] + [(sep, None)]
    want = [geomed.consensus_distance(*t) for t in tasks]

    def refuse(*a, **k):
        raise AssertionError("a per-task reduce-and-measure call")
    monkeypatch.setattr(_native, "wreduce_dist", refuse)
    monkeypatch.setattr(_native, "wreduce_dist_tensors_raw", refuse)
    got = geomed.consensus_distance_batch(tasks)
    assert all(_same_result(a, b) for a, b in zip(got, want))
