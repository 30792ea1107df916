"""Guard bands around every output of the SGD, momentum-SGD and
order-statistic launches (GPU). These kernels have their specials tests
(tests/test_gpu_sgd.py, test_gpu_sgdm.py, test_gpu_robust.py); what no test
looked at is the memory around their outputs. The references are the existing
ones: torch.optim.SGD on the CPU (_sgd_util, _sgdm_util) and the numpy
contract of _robust_util.

Every output is a view into a 0xA5-filled buffer (_edge_util.guarded; the
tensor-list entries: _edge_util.guarded_many, neighbours 16 bytes apart). Each
case checks the guards, the output bit for bit (prefilled, so an unwritten
element shows) and that the inputs are unchanged.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
import _robust_util as ru
from _sgd_util import torch_flat_step, torch_threads
from dasklearn_amd import _native

pytestmark = pytest.mark.gpu

LR, MOM, WD = 0.1, 0.9, 5e-4
SGD_DTYPES = ["f32", "bf16", "f64"]
SIZES = (1, 3, 4099, 2_000_003)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def torch_momentum_step(p, g, buf):
    """One torch.optim.SGD(foreach=False) step on flat CPU tensors (buf None: the first)."""
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = g.detach().clone()
    opt = torch.optim.SGD([q], lr=LR, momentum=MOM, weight_decay=WD, foreach=False)
    if buf is not None:
        opt.state[q]["momentum_buffer"] = buf.detach().clone()
    with torch_threads(4):
        opt.step()
    return q.detach(), opt.state[q]["momentum_buffer"]


_REF = {}


def sgd_ref(dtype, n):
    """(p, g, b) storage rows and torch's results, once per (dtype, n):
    the fresh-SGD step, the first momentum step, a later momentum step."""
    if (dtype, n) not in _REF:
        rows = eu.random_rows(dtype, 3, n, seed=n % 1009 + 5)
        p, g, b = (eu.to_torch(r, dtype) for r in rows)
        first = torch_momentum_step(p, g, None)
        later = torch_momentum_step(p, g, b)
        _REF[dtype, n] = (rows, eu.from_torch(torch_flat_step(p, g, LR, WD), dtype),
                          tuple(eu.from_torch(t, dtype) for t in first), tuple(eu.from_torch(t, dtype) for t in later))
    return _REF[dtype, n]


def guarded_with(row, dtype, offset):
    """A guarded view holding `row` (an in-place operand)."""
    h = eu.guarded(row.size * eu.ESIZE[dtype], dtype, dev(), offset=offset)
    h.view.copy_(eu.to_torch(row, dtype))
    return h


def check(h, exp, dtype, what):
    assert eu.check_guards(h) == [], what
    got = eu.from_torch(h.view, dtype)
    assert eu.same_bits(got, exp, dtype), (what, eu.unwritten(h), eu.diff_report(got, exp, dtype))


def shifts_for(count):
    """No buffer off alignment, then each of `count` buffers one element off in turn."""
    return [(0,) * count] + [tuple(1 if k == j else 0 for k in range(count)) for j in range(count)]


@pytest.mark.parametrize("dtype", SGD_DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_sgd_step_guards(n, dtype):
    esz = eu.ESIZE[dtype]
    rows, exp, _, _ = sgd_ref(dtype, n)
    for sp, sg, so in shifts_for(3):
        dp, dg = eu.place(list(rows[:2]), dtype, dev(), offsets=[sp * esz, sg * esz])
        h = eu.guarded(n * esz, dtype, dev(), offset=so * esz)
        _native.sgd_step(dp, dg, h.view, LR, WD)
        torch.cuda.synchronize()
        check(h, exp, dtype, ("separate", sp, sg, so))
        assert eu.inputs_unchanged([dp, dg], rows[:2], dtype)
    for s in (0, 1):  # in place on the parameter
        h = guarded_with(rows[0], dtype, s * esz)
        dg = eu.place([rows[1]], dtype, dev())[0]
        _native.sgd_step(h.view, dg, h.view, LR, WD)
        torch.cuda.synchronize()
        check(h, exp, dtype, ("in place", s))
        assert eu.inputs_unchanged([dg], rows[1:2], dtype)


@pytest.mark.parametrize("dtype", SGD_DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_sgd_momentum_step_guards(n, dtype):
    esz = eu.ESIZE[dtype]
    rows, _, first, later = sgd_ref(dtype, n)
    for sh in shifts_for(5):
        for step, (ep, eb) in (("first", first), ("later", later)):
            dp, dg, db = eu.place(list(rows), dtype, dev(), offsets=[sh[0] * esz, sh[1] * esz, sh[2] * esz])
            hp = eu.guarded(n * esz, dtype, dev(), offset=sh[3] * esz)
            hb = eu.guarded(n * esz, dtype, dev(), offset=sh[4] * esz)
            _native.sgd_momentum_step(dp, dg, None if step == "first" else db, hp.view, hb.view, LR, MOM, WD)
            torch.cuda.synchronize()
            check(hp, ep, dtype, (step, "param", sh))
            check(hb, eb, dtype, (step, "buffer", sh))
            assert eu.inputs_unchanged([dp, dg, db], rows, dtype)
    for s in (0, 1):  # in place: the parameter and the buffer are the outputs
        hp, hb = guarded_with(rows[0], dtype, s * esz), guarded_with(rows[2], dtype, s * esz)
        dg = eu.place([rows[1]], dtype, dev())[0]
        _native.sgd_momentum_step(hp.view, dg, hb.view, hp.view, hb.view, LR, MOM, WD)
        torch.cuda.synchronize()
        check(hp, later[0], dtype, ("in place param", s))
        check(hb, later[1], dtype, ("in place buffer", s))
        assert eu.inputs_unchanged([dg], rows[1:2], dtype)


def list_sizes(dtype):
    """130 tensors, more than two launches of 64, of 0 to 5000 elements."""
    E = eu.VEC_ELEMS[dtype]
    rng = np.random.default_rng(130)
    sizes = [0, 1, E - 1, E, E + 1, 3, 2047, 2048, 2049, 5000, 0] + [int(s) for s in rng.integers(0, 5001, 119)]
    assert len(sizes) == 130 > 2 * _native.SGD_MOMENTUM_TENSORS_PER_LAUNCH
    return sizes


@pytest.mark.parametrize("dtype", SGD_DTYPES)
def test_sgd_step_tensors_guards(dtype):
    sizes = list_sizes(dtype)
    rows = [eu.random_rows(dtype, 2, n, seed=k) for k, n in enumerate(sizes)]
    exp = [eu.from_torch(torch_flat_step(eu.to_torch(r[0], dtype), eu.to_torch(r[1], dtype), LR, WD), dtype)
           if r.shape[1] else r[0] for r in rows]
    dps = [eu.place([r[0]], dtype, dev())[0] for r in rows]
    dgs = [eu.place([r[1]], dtype, dev())[0] for r in rows]
    h = eu.guarded_many(sizes, dtype, dev(), gap=16)
    _native.sgd_step_tensors(dps, dgs, h.views, LR, WD)
    torch.cuda.synchronize()
    assert eu.check_guards(h) == []
    for k, r in enumerate(rows):
        got = eu.from_torch(h.views[k], dtype)
        assert eu.same_bits(got, exp[k], dtype), (k, sizes[k], eu.diff_report(got, exp[k], dtype))
        assert eu.inputs_unchanged([dps[k], dgs[k]], r, dtype)


@pytest.mark.parametrize("dtype", SGD_DTYPES)
def test_sgd_momentum_step_tensors_guards_with_mixed_first_flags(dtype):
    sizes = list_sizes(dtype)
    rows = [eu.random_rows(dtype, 3, n, seed=500 + k) for k, n in enumerate(sizes)]
    is_first = [k % 2 == 0 for k in range(len(sizes))]
    exp = []
    for r, f in zip(rows, is_first):
        if r.shape[1] == 0:
            exp.append((r[0], r[0]))
            continue
        p, g, b = (eu.to_torch(x, dtype) for x in r)
        exp.append(tuple(eu.from_torch(t, dtype) for t in torch_momentum_step(p, g, None if f else b)))
    d = [eu.place(list(r), dtype, dev()) for r in rows]
    hp, hb = eu.guarded_many(sizes, dtype, dev(), gap=16), eu.guarded_many(sizes, dtype, dev(), gap=16)
    _native.sgd_momentum_step_tensors_raw(
        [x[0].data_ptr() for x in d], [x[1].data_ptr() for x in d],
        [None if f else x[2].data_ptr() for x, f in zip(d, is_first)], [v.data_ptr() for v in hp.views],
        [v.data_ptr() for v in hb.views], sizes, LR, MOM, WD, _native.dtype_code(eu.DTYPES[dtype], single_task=True),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert eu.check_guards(hp) == [] and eu.check_guards(hb) == []
    for k, r in enumerate(rows):
        for h, e, what in ((hp, exp[k][0], "param"), (hb, exp[k][1], "buffer")):
            got = eu.from_torch(h.views[k], dtype)
            assert eu.same_bits(got, e, dtype), (k, sizes[k], what, eu.diff_report(got, e, dtype))
        assert eu.inputs_unchanged(d[k], r, dtype)


# ---- the order-statistic aggregators ----------------------------------------------------
ROBUST_NS = [3, 4, 8, 16, 17, 32]  # every capacity of the sorting network, and k_robust_halves


def robust_windows(n):
    lo = (n - 1) // 2
    return [(lo, lo + 1), (1, n - 1)]  # the median, trim 1


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("n", ROBUST_NS)
def test_robust_reduce_guards(n, dtype):
    dt, esz = ru.DTYPES[dtype], eu.ESIZE[dtype]
    p = 2 * 2048 + 37 * eu.VEC_ELEMS[dtype] + eu.VEC_ELEMS[dtype] - 1
    xs = ru.random_rows(dt, n, p, seed=n)
    sb = ru.sorted_bits(xs, dt)
    host = [ru.bits_of(x) for x in xs]
    for lo, hi in robust_windows(n):
        exp = ru.bits_of(ru.window_mean_sorted(sb, dt, lo, hi))
        for out_off, in_off in ((0, 0), (16, 0), (esz, 0), (0, esz)):
            dxs = eu.place([b.view(eu._STORE[dtype]) for b in host], dtype, dev(), offsets=[0] * (n - 1) + [in_off])
            h = eu.guarded(p * esz, dtype, dev(), offset=out_off)
            _native.robust_reduce(dxs, lo, hi, h.view)
            torch.cuda.synchronize()
            assert eu.check_guards(h) == [], (lo, hi, out_off, in_off)
            got = eu.bits_of(eu.from_torch(h.view, dtype), dtype)
            assert np.array_equal(got, exp), (lo, hi, out_off, in_off, int((got != exp).sum()), eu.unwritten(h))
            assert eu.inputs_unchanged(dxs, [b.view(eu._STORE[dtype]) for b in host], dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
def test_robust_reduce_tensors_guards(dtype):
    """The tensor-list entry writing at byte offsets into one guarded buffer:
    neighbours 16 bytes apart, sizes around the vector width, an empty tensor."""
    dt, esz, E = ru.DTYPES[dtype], eu.ESIZE[dtype], eu.VEC_ELEMS[dtype]
    n = 8
    sizes = [1, E - 1, E, E + 1, 0, 2048, 3 * 2048 + 5 * E + 3, 5]
    models = [ru.random_rows(dt, n, s, seed=40 + k) if s else [torch.empty(0, dtype=dt)] * n
              for k, s in enumerate(sizes)]  # models[k][i]: tensor k of model i
    dts = [eu.place([ru.bits_of(x).view(eu._STORE[dtype]) for x in m], dtype, dev()) for m in models]
    for lo, hi in robust_windows(n):
        h = eu.guarded_many(sizes, dtype, dev(), gap=16)
        _native.robust_reduce_tensors_raw([dts[k][i].data_ptr() for i in range(n) for k in range(len(sizes))], n,
                                          sizes, [s for s, _ in h.regions], lo, hi, h.buf.data_ptr(),
                                          _native.dtype_code(dt, single_task=True),
                                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert eu.check_guards(h) == [], (lo, hi)
        for k, s in enumerate(sizes):
            if s:
                exp = ru.bits_of(ru.window_mean(models[k], lo, hi))
                got = eu.bits_of(eu.from_torch(h.views[k], dtype), dtype)
                assert np.array_equal(got, exp), (lo, hi, k, s, eu.unwritten(h, k))
