"""The wide coordinate-wise median and trimmed mean on the MI355X
(dlsim_robust_reduce_wide over 33 to 128 rows, sort "wide") against the CPU
restatement of the contract (tests/_robust_util.py), bit for bit. Lengths come
from dlsim_robust_wide_geometry (tile T, lanes per element G)."""
from __future__ import annotations

import types

import pytest
import torch

import _edge_util as eu
import _robust_util as ru
from _sgd_util import Net
from sgd_inputs import GNLENET_SHAPES
from test_gpu_robust import PLACES, Mixed, _check, _expect, _filled, _shifted, _tensor_case

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian, TrimmedMean  # noqa: E402

DEV = "cuda"
DTYPES = ["f32", "bf16", "f16", "f64"]
CROSSING = ((31, 33), (32, 64), (63, 65), (95, 97))  # windows over a lane boundary of the group


def _run(xs_dev, lo, hi, out=None):
    out = torch.empty_like(xs_dev[0]) if out is None else out
    _native.robust_reduce_wide(xs_dev, lo, hi, out)
    return out


def _windows(n):
    return sorted(set(ru.windows(n)) | {w for w in CROSSING if w[1] <= n} | {(0, n)})


def _lengths(n, dtype):
    """1, a unit less one, the tile's edges, two tiles + a partial one + an odd tail."""
    T, G = _native.robust_wide_geometry(n, ru.DTYPES[dtype])
    U = 8 // eu.ESIZE[dtype]
    assert G == (2 if n <= 64 else 4) and T == 256 // G * U
    return sorted({1, U - 1, T - 1, T, T + 1, 2 * T + T // 2 + U + max(U - 1, 1)} - {0})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (33, 64, 65, 96, 97, 128))
def test_flat_entry_over_sizes_and_windows(n, dtype):
    """Every length is a prefix of one set of rows: one sort of the oracle serves them all."""
    dt = ru.DTYPES[dtype]
    sizes = _lengths(n, dtype)
    xs = ru.random_rows(dt, n, sizes[-1], seed=2000 + n)
    sb = ru.sorted_bits(xs, dt)
    xd = [x.to(DEV) for x in xs]
    for lo, hi in _windows(n):
        want = ru.window_mean_sorted(sb, dt, lo, hi)
        for p in sizes:
            _check(_run([x[:p] for x in xd], lo, hi), want[:p], f"{dtype} n={n} P={p} window=[{lo},{hi})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (33, 65, 128))
def test_specials_in_every_row_position(n, dtype):
    """Every special value in every row, hence in every lane of a group and every slot; the
    element form too (a base one element off alignment)."""
    dt = ru.DTYPES[dtype]
    xs = ru.special_rows(dt, n)
    sb = ru.sorted_bits(xs, dt)
    xd = [x.to(DEV) for x in xs]
    for lo, hi in _windows(n):
        _check(_run(xd, lo, hi), ru.window_mean_sorted(sb, dt, lo, hi), f"{dtype} n={n} window=[{lo},{hi})")
    shifted = [_shifted(x, 1) for x in xs]
    for lo, hi in (((n - 1) // 2, (n - 1) // 2 + 1), (0, n), (31, 33)):
        _check(_run(shifted, lo, hi), ru.window_mean_sorted(sb, dt, lo, hi), f"{dtype} n={n} elements [{lo},{hi})")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
@pytest.mark.parametrize("n", (40, 100))
def test_row_order_does_not_matter(n, dtype):
    dt = ru.DTYPES[dtype]
    xs = ru.random_rows(dt, n, 777, seed=77 + n)
    a = [x.to(DEV) for x in xs]
    for lo, hi in _windows(n):
        ga = _run(a, lo, hi)
        for r in (1, 16, 32, 47):
            assert ru.same_bits(ga.cpu(), _run(a[r:] + a[:r], lo, hi).cpu()), f"rotated by {r}, window [{lo},{hi})"
    _check(ga, ru.window_mean(xs, lo, hi), "the last window against the oracle")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("n", (5, 32))
def test_up_to_32_rows_are_forwarded_to_the_register_kernels(n, dtype):
    xd = [x.to(DEV) for x in ru.random_rows(ru.DTYPES[dtype], n, 4099, seed=n)]
    assert _native.robust_wide_geometry(n, ru.DTYPES[dtype])[1] == 1
    for lo, hi in ru.windows(n):
        want = torch.empty_like(xd[0])
        _native.robust_reduce(xd, lo, hi, want)
        assert ru.same_bits(_run(xd, lo, hi).cpu(), want.cpu())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", (40, 100))
def test_guard_bands_and_alignment(n, dtype):
    """The output between 0xA5 bands, aligned, then with one input and then the output off a
    16-byte boundary (4 bytes; one element for fp64): every output byte written, no other."""
    dt = ru.DTYPES[dtype]
    T, _ = _native.robust_wide_geometry(n, dt)
    p = 2 * T + T // 2 + 3
    off = max(4, eu.ESIZE[dtype])
    xs = ru.random_rows(dt, n, p, seed=5 + n, special_frac=0.0)
    lo, hi = 3, n - 3
    want = ru.window_mean(xs, lo, hi)
    xd = [x.to(DEV) for x in xs]
    one_off = list(xd)
    one_off[n - 2] = _shifted(xs[n - 2], off // eu.ESIZE[dtype])
    for ins, out_off in ((xd, 0), (one_off, 0), (xd, off)):
        h = eu.guarded(p * eu.ESIZE[dtype], dtype, DEV, offset=out_off)
        _run(ins, lo, hi, h.view)
        torch.cuda.synchronize()
        assert eu.check_guards(h) == [] and eu.unwritten(h) == 0
        _check(h.view, want, f"{dtype} n={n} output offset {out_off}")
    assert all(ru.same_bits(d.cpu(), x) for d, x in zip(xd + [one_off[n - 2]], xs + [xs[n - 2]])), "an input changed"


@pytest.mark.parametrize("dtype,shapes", [("f32", GNLENET_SHAPES), ("bf16", GNLENET_SHAPES), ("f32", [[5], [0], [3, 7]])])
def test_tensors_entry_equals_flat_calls(dtype, shapes):
    n = 40
    dt, numels, rows, offs, tensors = _tensor_case(shapes, dtype, n, seed=11)
    esz = rows[0].element_size()
    for lo, hi in ((19, 20), (4, 36)):
        out = torch.zeros(sum(numels), dtype=dt, device=DEV)
        _native.robust_reduce_wide_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels,
                                               [int(o) * esz for o in offs], lo, hi, out.data_ptr(),
                                               _native.dtype_code(dt, single_task=True),
                                               torch.cuda.current_stream().cuda_stream)
        flat = torch.zeros_like(out)
        for k, (o, m) in enumerate(zip(offs, numels)):
            if m:
                _run([row[k] for row in tensors], lo, hi, flat[o:o + m])
        assert ru.same_bits(out.cpu(), flat.cpu())
        _check(out, ru.window_mean(rows, lo, hi), f"{dtype} window [{lo},{hi})")


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("n", (40, 100))
def test_plugins_end_to_end(n, place):
    """Host models, device arenas (the flat entry) and device tensors read in place (the tensors entry)."""
    cpu = _filled(Mixed, n, seed=500 + n)
    models = [PLACES[place](m) for m in cpu]
    lo = (n - 1) // 2
    for agg, window in ((CoordinateMedian.with_sort("wide"), (lo, lo + 1)),
                        (TrimmedMean.with_trim(3, sort="wide"), (3, n - 3))):
        out = agg.aggregate(models)
        for k, (g, w, p0) in enumerate(zip(out.parameters(), _expect(cpu, *window), models[0].parameters())):
            assert g.device == p0.device and g.dtype == p0.dtype
            _check(g, w, f"{agg.__name__} {place} n={n} parameter {k}")
    for g, w in zip(TrimmedMean.aggregate(models, trim=3, sort="wide").parameters(), _expect(cpu, 3, n - 3)):
        _check(g, w, "the sort keyword")


def test_functions_aggregate_and_a_broken_minority():
    """settings.aggregation_sort = "wide" through ModelManager; ten of 100 peers send Inf or NaN."""
    n = 100
    cpu = _filled(lambda: Net([[33, 7], [129], [5]], "f32"), n, seed=700, special_frac=0.0)
    with torch.no_grad():
        for k in range(10):
            for p in cpu[7 * k + 3].parameters():
                p.fill_(float("inf") if k % 2 else float("nan"))
    for method, window in ((2, (49, 50)), (3, (10, 90))):
        settings = types.SimpleNamespace(gradient_aggregation=method, aggregation_sort="wide", aggregation_trim=10)
        (res,) = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0})
        for g, w in zip(res.parameters(), _expect(cpu, *window)):
            assert bool(torch.isfinite(g).all()) and not g.is_cuda
            _check(g, w, f"method {method}")
