"""Stream order and concurrent callers of the five newer kernel families on
the MI355X: the fresh-SGD step, the momentum step, the order statistics,
pairwise distances and reduce-and-measure, flat and *_tensors entries. Every
entry says "stream-ordered"; the two distance families also allocate and free
their partial-sum workspace in stream order and take a memset shortcut for
n = 1 or zero elements.

Side-stream ordering: a side stream is kept busy, then the copies that give
the inputs their rows B, the entry itself and a second overwrite with rows C
are queued on it with no host wait in between. The result must be the oracle's
for B: a launch, memset or workspace use that left the stream reads rows A (the
inputs' first contents) or C, or races the prefill of the outputs.

The references are the kernels' own: torch.optim.SGD on the CPU, the numpy
contract of _robust_util, _krum_util's and _geomed_util's longdouble oracles.
A *_tensors entry adds its tensors' partial sums in order; with sizes
(0, 37, 2051, 5) that keeps the bound of one call over all elements (three
non-empty pieces, two more roundings, 2093 - 2051 >= 2; the argument of
tests/test_gpu_model_routes.py).
"""
from __future__ import annotations

import threading

import numpy as np
import pytest
import torch

import _edge_util as eu
import _geomed_util as gu
import _krum_util as ku
import _robust_util as ru
import _route_util as rt
from _sgd_util import torch_flat_step, torch_threads

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian  # noqa: E402
from dasklearn_amd.gradient_aggregation.krum import Krum  # noqa: E402
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian  # noqa: E402

DEV = "cuda"
LR, MOM, WD = 0.1, 0.9, 5e-4
SLEEP_CYCLES = 100_000_000  # about 50 ms: half of what tests/test_gpu_resident_alloc.py queues for 0.1 s
FLAT_SIZE = 4099
TENSOR_SIZES = (0, 37, 2051, 5)  # the first tensor empty: a *_tensors distance entry memsets, then accumulates


def _code(dtype):
    return _native.dtype_code(eu.DTYPES[dtype], single_task=True)


def _torch_momentum_step(p, g, buf):
    """One torch.optim.SGD(foreach=False) step on flat CPU tensors."""
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    opt = torch.optim.SGD([q], lr=LR, momentum=MOM, weight_decay=WD, foreach=False)
    opt.state[q]["momentum_buffer"] = buf.detach().clone()
    with torch_threads(4):
        opt.step()
    return q.detach(), opt.state[q]["momentum_buffer"]


def _clean(*guards):
    for g in guards:
        assert eu.check_guards(g) == [], "guard bytes written"


def _same(got, exp, dtype, what):
    assert eu.same_bits(got, exp, dtype), f"{what}: " + eu.diff_report(got, exp, dtype)


# ---- the entries ------------------------------------------------------------------------------
# setup(dtype, n, sizes) -> (element count of every input tensor, make); make(ins) -> (launch, check) around fresh
# guarded outputs. launch(stream, raw): the torch stream (or None: the current one) for the tensor entries, its
# handle for the raw ones. check(rows): the outputs against the oracle of the inputs' storage rows.
def _sgd(tensors):
    def setup(dtype, n, sizes):
        def make(ins):
            ps, gs = ins[0::2], ins[1::2]
            outs = eu.guarded_many(sizes, dtype, DEV)

            def launch(stream, raw):
                if tensors:
                    _native.sgd_step_tensors(ps, gs, outs.views, LR, WD, stream=stream)
                else:
                    _native.sgd_step(ps[0], gs[0], outs.view, LR, WD, stream=stream)

            def check(rows):
                _clean(outs)
                for k, s in enumerate(sizes):
                    if s:
                        exp = torch_flat_step(eu.to_torch(rows[2 * k], dtype), eu.to_torch(rows[2 * k + 1], dtype), LR, WD)
                        _same(eu.from_torch(outs.views[k], dtype), eu.from_torch(exp, dtype), dtype, f"tensor {k}")
            return launch, check
        return [s for s in sizes for _ in range(2)], make
    return setup


def _sgdm(tensors):
    def setup(dtype, n, sizes):
        def make(ins):
            ps, gs, bs = ins[0::3], ins[1::3], ins[2::3]
            po, bo = eu.guarded_many(sizes, dtype, DEV), eu.guarded_many(sizes, dtype, DEV)

            def launch(stream, raw):
                if tensors:
                    _native.sgd_momentum_step_tensors_raw(
                        [t.data_ptr() for t in ps], [t.data_ptr() for t in gs], [t.data_ptr() for t in bs],
                        [v.data_ptr() for v in po.views], [v.data_ptr() for v in bo.views], list(sizes), LR, MOM, WD,
                        _code(dtype), raw)
                else:
                    _native.sgd_momentum_step(ps[0], gs[0], bs[0], po.view, bo.view, LR, MOM, WD, stream=stream)

            def check(rows):
                _clean(po, bo)
                for k, s in enumerate(sizes):
                    if s:
                        ep, eb = _torch_momentum_step(*(eu.to_torch(rows[3 * k + j], dtype) for j in range(3)))
                        _same(eu.from_torch(po.views[k], dtype), eu.from_torch(ep, dtype), dtype, f"parameter {k}")
                        _same(eu.from_torch(bo.views[k], dtype), eu.from_torch(eb, dtype), dtype, f"buffer {k}")
            return launch, check
        return [s for s in sizes for _ in range(3)], make
    return setup


def _model_major(n, sizes):
    return [s for _ in range(n) for s in sizes]


def _robust(tensors):
    def setup(dtype, n, sizes):
        t, lo = len(sizes), (n - 1) // 2

        def make(ins):
            outs = eu.guarded_many(sizes, dtype, DEV)

            def launch(stream, raw):
                if tensors:
                    _native.robust_reduce_tensors_raw([x.data_ptr() for x in ins], n, list(sizes),
                                                      [s for s, _ in outs.regions], lo, lo + 1, outs.buf.data_ptr(),
                                                      _code(dtype), raw)
                else:
                    _native.robust_reduce(ins, lo, lo + 1, outs.view, stream=stream)

            def check(rows):
                _clean(outs)
                for k, s in enumerate(sizes):
                    if s:
                        exp = ru.window_mean([eu.to_torch(rows[i * t + k], dtype) for i in range(n)], lo, lo + 1)
                        got = eu.bits_of(eu.from_torch(outs.views[k], dtype), dtype)
                        assert np.array_equal(got, ru.bits_of(exp)), f"tensor {k}: {int((got != ru.bits_of(exp)).sum())} differ"
            return launch, check
        return _model_major(n, sizes), make
    return setup


def _model_rows(rows, n, t, dtype):
    """The storage rows of n models of t tensors each, one concatenated row per model."""
    return np.stack([np.concatenate([np.asarray(rows[i * t + k]) for k in range(t)]) for i in range(n)]) \
        if sum(np.asarray(r).size for r in rows) else np.zeros((n, 0), dtype=eu._STORE[dtype])


def _pairdist(tensors):
    def setup(dtype, n, sizes):
        t = len(sizes)

        def make(ins):
            d2 = eu.guarded(n * n * 8, "f64", DEV)

            def launch(stream, raw):
                if tensors:
                    _native.pairwise_sqdist_tensors_raw([x.data_ptr() for x in ins], n, list(sizes), _code(dtype),
                                                        d2.view.data_ptr(), False, raw)
                else:
                    _native.pairwise_sqdist(ins, d2.view, stream=stream)

            def check(rows):
                _clean(d2)
                assert eu.unwritten(d2) == 0, "matrix entries left unwritten"
                problems, _ = ku.matrix_problems(d2.view.cpu().numpy().reshape(n, n),
                                                 ku.sqdist_oracle(_model_rows(rows, n, t, dtype), dtype), sum(sizes))
                assert not problems, problems
            return launch, check
        return _model_major(n, sizes), make
    return setup


def _reducedist(tensors):
    def setup(dtype, n, sizes):
        t = len(sizes)
        w = [float(v) for v in eu.special_weights(n, "dirichlet", dtype)]

        def make(ins):
            d2, outs = eu.guarded(n * 8, "f64", DEV), eu.guarded_many(sizes, dtype, DEV)

            def launch(stream, raw):
                if tensors:
                    _native.wreduce_dist_tensors_raw([x.data_ptr() for x in ins], n, list(sizes),
                                                     [s for s, _ in outs.regions], w, outs.buf.data_ptr(), _code(dtype),
                                                     d2.view.data_ptr(), False, raw)
                else:
                    _native.wreduce_dist(ins, w, outs.view, d2.view, stream=stream)

            def check(rows):
                _clean(d2, outs)
                assert eu.unwritten(d2) == 0, "distances left unwritten"
                x = _model_rows(rows, n, t, dtype)
                fold = gu.fold_oracle(x, np.asarray(w, dtype=np.float32), dtype) if x.shape[1] else x[0]
                got = np.concatenate([eu.from_torch(v, dtype) for v in outs.views])
                _same(got, fold, dtype, "out")
                problems, _ = gu.vector_problems(d2.view.cpu().numpy(), gu.dist_oracle(x, fold, dtype), sum(sizes))
                assert not problems, problems
            return launch, check
        return _model_major(n, sizes), make
    return setup


ENTRIES = {
    "sgd_step": (_sgd(False), False), "sgd_step_tensors": (_sgd(True), True),
    "sgd_momentum_step": (_sgdm(False), False), "sgd_momentum_step_tensors_raw": (_sgdm(True), True),
    "robust_reduce": (_robust(False), False), "robust_reduce_tensors_raw": (_robust(True), True),
    "pairwise_sqdist": (_pairdist(False), False), "pairwise_sqdist_tensors_raw": (_pairdist(True), True),
    "wreduce_dist": (_reducedist(False), False), "wreduce_dist_tensors_raw": (_reducedist(True), True),
}


def _cases():
    """(entry, fan-in, zero-element call): the steps once; the order statistics
    at n = 1 and one fan-in per distance-kernel shape; the distance families
    also with no element at all (n = 1 and zero elements are their memset
    shortcuts, taken with accumulate off)."""
    out = []
    for name in ENTRIES:
        if name.startswith("sgd"):
            out.append((name, 1, False))
            continue
        out += [(name, n, False) for n in (1, 3, 9, 17)]
        if not name.startswith("robust"):
            out.append((name, 3, True))
    return out


@pytest.mark.parametrize("how", ["stream_argument", "current_stream"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("entry,n,zero", _cases())
def test_every_entry_is_ordered_on_a_side_stream(entry, n, zero, dtype, how):
    setup, tensors = ENTRIES[entry]
    sizes = tuple(TENSOR_SIZES if tensors else (FLAT_SIZE,))
    if zero:
        sizes = tuple(0 for _ in sizes)
    shapes, make = setup(dtype, n, sizes)
    a, b, c = ([eu.random_rows(dtype, 1, p, seed=seed + 13 * i)[0] for i, p in enumerate(shapes)]
               for seed in (8100, 8200, 8300))
    ins, src_b, src_c = (eu.place(rows, dtype, DEV) for rows in (a, b, c))  # 1. the inputs hold rows A
    launch, check = make(ins)                                              # 2. prefilled, guarded outputs
    torch.cuda.synchronize()                                                # 3.
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP_CYCLES)                                     # 4. the stream is busy
        for x, src in zip(ins, src_b):                                      # 5. rows B, queued behind it
            x.copy_(src, non_blocking=True)
        if how == "current_stream":                                         # 6. the entry: the path the plugins use,
            launch(None, torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))
    if how == "stream_argument":                                            # or the stream handed over
        launch(s, s.cuda_stream)
    with torch.cuda.stream(s):
        for x, src in zip(ins, src_c):                                      # 7. rows C
            x.copy_(src, non_blocking=True)
    s.synchronize()                                                         # 8.
    check(b)
    assert eu.inputs_unchanged(ins, c, dtype)


# ---- two streams at once -----------------------------------------------------------------------------
def test_two_streams_do_not_mix_their_workspaces():
    """Each stream runs pairwise distances at n = 17 and reduce-and-measure at
    n = 9 on its own inputs, queued alternately six times with nothing waited
    for until the end. The summation order is a function of the grid alone, so
    every result equals the same call run alone bit for bit, unless the two
    calls' workspaces or partial sums mix."""
    p = 300_011
    w = [float(v) for v in eu.special_weights(9, "dirichlet", "f32")]
    work = []
    for j in range(2):
        pd = eu.place(list(eu.random_rows("f32", 17, p, seed=8400 + j)), "f32", DEV)
        rd = eu.place(list(eu.random_rows("f32", 9, p, seed=8500 + j)), "f32", DEV)
        m = torch.empty(17 * 17, dtype=torch.float64, device=DEV)
        out, d2 = torch.empty(p, device=DEV), torch.empty(9, dtype=torch.float64, device=DEV)
        _native.pairwise_sqdist(pd, m)
        _native.wreduce_dist(rd, w, out, d2)
        torch.cuda.synchronize()
        work.append((pd, rd, m.cpu().numpy(), out.cpu().numpy(), d2.cpu().numpy(), torch.cuda.Stream()))
    results = []
    torch.cuda.synchronize()
    for it in range(6):
        for j, (pd, rd, *_, s) in enumerate(work):
            m = eu.guarded(17 * 17 * 8, "f64", DEV)
            d2, out = eu.guarded(9 * 8, "f64", DEV), eu.guarded(p * 4, "f32", DEV)
            _native.pairwise_sqdist(pd, m.view, stream=s)
            _native.wreduce_dist(rd, w, out.view, d2.view, stream=s)
            results.append((it, j, m, d2, out))
    for *_, s in work:
        s.synchronize()
    for it, j, m, d2, out in results:
        _, _, want_m, want_out, want_d2, _ = work[j]
        _clean(m, d2, out)
        assert np.array_equal(m.view.cpu().numpy().view(np.uint64), want_m.view(np.uint64)), f"matrix, round {it} stream {j}"
        assert np.array_equal(d2.view.cpu().numpy().view(np.uint64), want_d2.view(np.uint64)), f"d2, round {it} stream {j}"
        assert np.array_equal(out.view.cpu().numpy().view(np.uint32), want_out.view(np.uint32)), f"out, round {it} stream {j}"


# ---- caller threads -------------------------------------------------------------------------------------
def test_plugins_from_four_threads_on_their_own_streams():
    """Four host threads, each on its own stream, six iterations each of
    CoordinateMedian, Krum(2), GeometricMedian and CenteredClip on host and
    arena lists in turn; the expectations come from the oracles, computed
    before the threads start. Every result is theirs bit for bit."""
    routes = rt.routes(DEV)
    jobs = []  # (name, aggregate(models), {route: models}, expected parameter bits)
    cpu, want = rt.robust_case("mixed", 5)
    jobs.append(("median", lambda ms: CoordinateMedian.aggregate(ms), cpu, want[dict(rt.robust_windows(5))["median"]]))
    rows, _, d2, cpu = rt.krum_case(8, 2)
    best = ku.ref_select(d2.astype(np.float64), 2, 1)[0]
    jobs.append(("krum", lambda ms: Krum.with_params(2).aggregate(ms), cpu, rt.split_bits(rows[best], cpu[0])))
    for name in ("gm-8-weighted", "clip-8-tau"):
        case, rows, _, alphas, final, _, cpu = rt.trajectory_case(name)
        agg = (GeometricMedian.with_params(gu.GM_ITERS, gu.GM_NU) if case["rule"] == "gm"
               else CenteredClip.with_params(case["tau"], gu.CLIP_ITERS))
        jobs.append((name, lambda ms, agg=agg, alphas=alphas: agg.aggregate(ms, alphas), cpu, rt.split_bits(final, cpu[0])))
    jobs = [(name, call, {r: routes[r](cpu) for r in ("host", "arena")}, exp) for name, call, cpu, exp in jobs]
    torch.cuda.synchronize()
    errors = []

    def worker(tid):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for it in range(6):
                    route = ("host", "arena")[(tid + it) % 2]
                    for name, call, lists, exp in jobs:
                        out = call(lists[route])
                        s.synchronize()
                        if not rt.same_params(out, exp):
                            errors.append(f"thread {tid} iteration {it}: {name} on {route} differs")
        except Exception as ex:  # noqa: BLE001 - reported below
            errors.append(f"thread {tid}: {type(ex).__name__}: {ex}")

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=100)
    assert not any(t.is_alive() for t in threads), "a caller thread is stuck"
    assert not errors, errors[:5]
