"""dlsim_mx_quantize, dlsim_mx_dequantize, dlsim_mx_wreduce (flat and batched)
and dasklearn_amd.mx on the GPU, bit for bit against a float64 numpy
restatement of the wire format (include/dlsim.h): a generic minifloat round and
a code-to-value table per format; the reduce against the committed oracle's
exact fold over rows decoded by that restatement. Every buffer is a view inside
0xA5 guard bytes (the helpers of test_gpu_quant.py)."""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _edge_util as eu
from test_gpu_quant import DEV, F32, MAXV, Mixed, clean, group_rows, guarded, row, storage, widen

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, functions  # noqa: E402
from dasklearn_amd.arena import to_device_arena  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.mx import MXSharer, mix, mix_batch  # noqa: E402
from dasklearn_amd.quant import QuantSharer  # noqa: E402

FORMATS = {"fp8_e4m3": (4, 3), "fp8_e5m2": (5, 2), "fp4": (2, 1)}  # exponent and mantissa bits
CASES = [(dt, fmt) for dt in ("f32", "bf16") for fmt in FORMATS]


# ---- the restatement ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(fmt):
    """(values of every code as float64, emin, emax, max): the OCP formats."""
    ebits, mbits = FORMATS[fmt]
    bias = 2 ** (ebits - 1) - 1
    c = np.arange(2 ** (1 + ebits + mbits))
    e, m = (c >> mbits) & (2 ** ebits - 1), (c & (2 ** mbits - 1)).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** (1 - bias - mbits), (1 + m / 2 ** mbits) * 2.0 ** (e.astype(np.float64) - bias))
    if fmt == "fp8_e4m3":
        v[(c & 0x7f) == 0x7f] = np.nan
    if fmt == "fp8_e5m2":
        v[e == 31] = np.where(m[e == 31] == 0, np.inf, np.nan)
    v = np.where(c >> (ebits + mbits), -v, v)
    return v, 1 - bias, {"fp8_e4m3": 8, "fp8_e5m2": 15, "fp4": 2}[fmt], np.nanmax(v[np.isfinite(v)])


def per_elem(v, p):
    return np.repeat(v, 32)[:p]


def pack(q, fmt):
    if fmt != "fp4":
        return q.astype(np.uint8)
    n = np.zeros(-(-q.size // 2) * 2, np.uint8)
    n[:q.size] = q
    return n[0::2] | (n[1::2] << 4)


def restate_decode(codes, scales, p, dtype, fmt):
    """The storage row that codes and scale bytes decode to."""
    q = codes[:p] if fmt != "fp4" else np.stack([codes & 0xf, codes >> 4], axis=1).reshape(-1)[:p]
    s = per_elem(scales, p).astype(np.float64)
    with np.errstate(all="ignore"):
        x = np.where(s == 255, np.nan, table(fmt)[0][q] * 2.0 ** (s - 127)).astype(F32)  # one rounding: the product is exact
        return eu.encode(x.astype(np.float64), dtype)


def restate_quantize(x, dtype, fmt, resid=None):
    """(codes uint8, scale bytes uint8, new residual storage or None) of the storage row x."""
    p, mbits = x.size, FORMATS[fmt][1]
    values, emin, emax, vmax = table(fmt)
    with np.errstate(all="ignore"):
        t = widen(x, dtype) if resid is None else widen(x, dtype) + widen(resid, dtype)
        padded = np.zeros(-(-p // 32) * 32, F32)
        padded[:p] = t
        A = (padded.view(np.uint32) & np.uint32(0x7fffffff)).reshape(-1, 32).max(axis=1)
        live = (A < 0x7f800000) & (A >= 0x1f800000)
        S = np.where(A >= 0x7f800000, 255, np.where(live, (A >> 23).astype(np.int64) - emax, 0)).astype(np.uint8)
        y = np.abs(np.where(per_elem(live, p), t, F32(0)).astype(np.float64)) / 2.0 ** (per_elem(S, p).astype(np.float64) - 127)
        e = np.maximum(np.frexp(y)[1] - 1, emin)  # floor(log2 y), exactly
        step = 2.0 ** (e - mbits)
        r = np.minimum(np.rint(y / step) * step, vmax)
        q = np.searchsorted(values[:values.size // 2][np.isfinite(values[:values.size // 2])], r)
        q = np.where(per_elem(live, p), q | (np.signbit(t) * (values.size // 2)), 0)
        codes = pack(q, fmt)
        new = None
        if resid is not None:
            new = eu.encode((t - widen(restate_decode(codes, S, p, dtype, fmt), dtype)).astype(np.float64), dtype)
    return codes, S, new


def sizes(dtype):
    tile, cap = (_native.mx_geometry(1, eu.DTYPES[dtype])[k] for k in ("tile_elems", "max_blocks"))
    return [1, 31, 32, 33, tile - 1, tile + 1, cap * tile + 1]  # the last: two passes of the grid


def check_quantize(dtype, fmt, with_resid, x, e, off, what):
    p, tdt, esz = x.size, eu.DTYPES[dtype], eu.ESIZE[dtype]
    nc, ns = _native.mx_sizes(p, fmt)
    xb, xv = guarded(p * esz, off, x)
    eb, ev = guarded(p * esz, off, e)
    cb, cv = guarded(nc, off)
    sb, sv = guarded(ns, off)
    form = "scalar" if off else "vec"
    used = [xv] + ([ev] if with_resid else []) + [cv]
    assert _native.mx_kernel_name("quantize", used, p, tdt) == f"dlsim::k_mx_quantize<{form}>"
    _native.mx_quantize(xv.view(tdt), cv, sv, fmt, ev.view(tdt) if with_resid else None)
    torch.cuda.synchronize()
    codes, scales, new = restate_quantize(x, dtype, fmt, e if with_resid else None)
    got_c, got_s = cv.cpu().numpy(), sv.cpu().numpy()
    assert all(clean(b, v) for b, v in ((xb, xv), (eb, ev), (cb, cv), (sb, sv))), f"{what}: guard bytes written"
    assert np.array_equal(got_s, scales), f"{what}: scale bytes differ at {np.nonzero(got_s != scales)[0][:5]}"
    bad = np.nonzero(got_c != codes)[0][:5]
    assert bad.size == 0, f"{what}: codes differ at {bad}: got {got_c[bad]}, expected {codes[bad]}"
    assert np.array_equal(storage(xv, dtype).view(np.uint8), x.view(np.uint8)), f"{what}: the model changed"
    want_e = new if with_resid else e
    assert eu.same_bits(storage(ev, dtype), want_e, dtype), f"{what}: residual " + eu.diff_report(storage(ev, dtype), want_e, dtype)
    return got_c, got_s


def check_dequantize(dtype, fmt, codes, scales, p, off, what):
    tdt = eu.DTYPES[dtype]
    _, cv = guarded(codes.size, off, codes)
    _, sv = guarded(scales.size, off, scales)
    ob, ov = guarded(p * eu.ESIZE[dtype], off)
    form = "scalar" if off else "vec"
    assert _native.mx_kernel_name("dequantize", [cv, ov], p, tdt) == f"dlsim::k_mx_dequantize<{form}>"
    _native.mx_dequantize(cv, sv, fmt, ov.view(tdt))
    torch.cuda.synchronize()
    exp = restate_decode(codes, scales, p, dtype, fmt)
    assert clean(ob, ov), f"{what}: guard bytes written"
    assert eu.same_bits(storage(ov, dtype), exp, dtype), f"{what}: decode " + eu.diff_report(storage(ov, dtype), exp, dtype)


@pytest.mark.parametrize("with_resid", [False, True])
@pytest.mark.parametrize("dtype,fmt", CASES)
def test_quantize_and_dequantize_at_every_length_and_form(dtype, fmt, with_resid):
    for p in sizes(dtype):
        for off in (0, 4) if p in (33, sizes(dtype)[5]) else (0,):
            what = f"{dtype} {fmt} resid={with_resid} P={p} off={off}"
            codes, scales = check_quantize(dtype, fmt, with_resid, row(dtype, p), row(dtype, p, 1), off, what)
            check_dequantize(dtype, fmt, codes, scales, p, off, what)


def special(kind, dtype, fmt, n):
    """n values of one special block, as float64."""
    values, _, emax, vmax = table(fmt)
    alt = np.where(np.arange(n) % 2, -1.0, 1.0)
    v = np.random.default_rng(5).standard_normal(n) * 0.05
    if kind == "zero":
        v[:] = 0.0
    elif kind == "signed_zero":
        v = 0.0 * alt
    elif kind == "tiny":
        v = np.where(np.arange(n) % 3, 2.0 ** -65, -2.0 ** -70)
    elif kind == "subnormal":
        v = np.where(np.arange(n) % 2, 2.0 ** -130, -2.0 ** -133)
        v[n // 2] = 1.0
    elif kind == "inf_nan":
        v[0], v[n - 1] = np.inf, np.nan
    elif kind == "inf":
        v[n // 2] = -np.inf
    elif kind == "flt_max":
        v[0], v[n - 1] = MAXV[dtype], -MAXV[dtype]
    elif kind == "ties":  # max pins S = 127; -0; a value that rounds past max; the subnormal midpoints; normal ones from the top
        pos = np.sort(values[np.isfinite(values) & (values >= 0)])
        mids = (pos[1:] + pos[:-1]) / 2
        nsub = 2 ** FORMATS[fmt][1]  # midpoints up to the least normal value
        pool = np.concatenate([[vmax, -0.0, 2.0 ** (emax + 1) * 31 / 32, mids[-1]], mids[:nsub], mids[nsub:-1][::-1]])
        v = np.resize(pool, n) * np.where(np.arange(n) < 2, 1.0, alt)
    return v


@pytest.mark.parametrize("kind", ["zero", "signed_zero", "tiny", "subnormal", "inf_nan", "inf", "flt_max", "ties"])
@pytest.mark.parametrize("dtype,fmt", CASES)
def test_special_blocks_first_middle_and_short_last(dtype, fmt, kind):
    p = 4 * 32 + 19
    x = row(dtype, p, 2).copy()
    for start in (0, 64, 128):
        n = min(32, p - start)
        x[start:start + n] = eu.encode(special(kind, dtype, fmt, n), dtype)
    what = f"{dtype} {fmt} {kind}"
    codes, scales = check_quantize(dtype, fmt, True, x, np.zeros_like(x), 0, what)
    if kind in ("inf_nan", "inf"):
        assert (scales[[0, 2, 4]] == 255).all() and not codes[:32 // (2 if fmt == "fp4" else 1)].any()
    if kind in ("zero", "signed_zero", "tiny"):
        assert not scales[[0, 2, 4]].any()
    if kind == "ties":
        assert (scales[[0, 2, 4]] == 127).all()
    check_dequantize(dtype, fmt, codes, scales, p, 0, what)


# ---- the reduce -------------------------------------------------------------------------
def neighbours(p, m, seed):
    """m neighbours of random code bytes, formats cycling, scale bytes from [48, 252] and 0xFF; the second
    neighbour's scale bytes are foreign: 0, 1, 47, 253, 254."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(m):
        fmt = list(FORMATS)[j % 3]
        nc, ns = _native.mx_sizes(p, fmt)
        scales = rng.integers(48, 253, ns, dtype=np.uint8)
        scales[rng.random(ns) < 0.1] = 255
        if j == 1:
            scales = np.resize(np.array([0, 1, 47, 253, 254], np.uint8), ns)
        out.append((rng.integers(0, 256, nc, dtype=np.uint8), scales, fmt))
    return out


def place_neighbours(nbrs, off=0):
    return [(guarded(c.size, off, c)[1], guarded(s.size, 0, s)[1], f) for c, s, f in nbrs]


def check_reduce(dtype, p, m, weights, alias=False, off=0, what=""):
    tdt, esz = eu.DTYPES[dtype], eu.ESIZE[dtype]
    own, nbrs = row(dtype, p, 3), neighbours(p, m, p + m)
    w = eu.orc.reference_weights(m + 1, None) if weights is None else eu.special_weights(m + 1, weights, dtype)
    ob, ov = guarded(p * esz, off, own if alias else None)
    xv = ov if alias else guarded(p * esz, off, own)[1]
    dn = place_neighbours(nbrs, off)
    form = "scalar" if off else "vec"
    assert _native.mx_kernel_name("wreduce", [xv, ov] + [c for c, _, _ in dn], p, tdt) == f"dlsim::k_mx_wreduce<{form}>"
    _native.mx_wreduce(xv.view(tdt), dn, w, ov.view(tdt))
    torch.cuda.synchronize()
    rows = [own] + [restate_decode(c, s, p, dtype, f) for c, s, f in nbrs]
    exp = eu.expected_reduce("exact", np.stack(rows), w, dtype)
    assert clean(ob, ov), f"{what}: guard bytes written"
    assert eu.same_bits(storage(ov, dtype), exp, dtype), f"{what}: " + eu.diff_report(storage(ov, dtype), exp, dtype)
    assert all(np.array_equal(c.cpu().numpy(), h) and np.array_equal(s.cpu().numpy(), hs)
               for (c, s, _), (h, hs, _) in zip(dn, nbrs)), f"{what}: codes or scales changed"
    if not alias:
        assert np.array_equal(storage(xv, dtype).view(np.uint8), own.view(np.uint8)), f"{what}: the dense row changed"


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("weights", ["dirichlet", None])
@pytest.mark.parametrize("m", [0, 1, 7, 31])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reduce_fan_ins_mixed_formats_weights_and_alias(dtype, m, weights, alias):
    check_reduce(dtype, 2 * 4096 + 37, m, weights, alias, what=f"{dtype} m={m} {weights} alias={alias}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reduce_at_every_length_and_in_the_scalar_form(dtype):
    for p in sizes(dtype):
        check_reduce(dtype, p, 3, "dirichlet", what=f"{dtype} P={p}")
    for p in (33, 4097):
        check_reduce(dtype, p, 9, "dirichlet", off=4, what=f"{dtype} P={p} scalar")


@pytest.mark.parametrize("shapes", [[(4096 + 3, 31, 0), (3 * 4096, 2, 4), (37, 7, 0)],
                                    [(0, 1, 0), (1, 0, 0)] + [(500 + 97 * t, t % 7, 4 * (t % 4 == 3)) for t in range(38)]])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batched_reduce_equals_the_flat_entry(dtype, shapes):
    """Three tasks of different size, fan-in and alignment; then 40 tasks with over 100 neighbours, which
    split over launches (32 tasks, 80 neighbours) and forms."""
    tdt, esz = eu.DTYPES[dtype], eu.ESIZE[dtype]
    tasks, flat, guards = [], [], []
    for t, (p, m, off) in enumerate(shapes):
        xv = guarded(p * esz, off, row(dtype, p, 4) if p else None)[1].view(tdt)
        dn = place_neighbours(neighbours(p, m, 50 + t), off)
        w = eu.special_weights(m + 1, "dirichlet", dtype)
        ob, ov = guarded(p * esz, off)
        ref = torch.empty_like(xv)
        _native.mx_wreduce(xv, dn, w, ref)
        tasks.append((xv, dn, w, ov.view(tdt)))
        flat.append(ref)
        guards.append((ob, ov))
    torch.cuda.synchronize()
    _native.mx_wreduce_batched(tasks)
    torch.cuda.synchronize()
    for t, ((ob, ov), ref) in enumerate(zip(guards, flat)):
        assert clean(ob, ov), f"task {t}: guard bytes written"
        assert np.array_equal(ov.cpu().numpy(), ref.view(torch.uint8).cpu().numpy()), f"task {t} differs from its flat call"


# ---- the Python layer -------------------------------------------------------------------
@pytest.mark.parametrize("where", ["arena", "cuda", "cpu"])
def test_mix_equals_fedavg_over_dequantised_models(where):
    torch.manual_seed(31)
    own = to_device_arena(Mixed(), DEV) if where == "arena" else Mixed().to(where)
    peers = [Mixed().to(DEV) for _ in range(3)]
    qms = [MXSharer(q, fmt=f).share(q) for q, f in zip(peers, FORMATS)]
    nf32, nbf = 67 * 33 + 33, 33 * 9 + 9  # Mixed's two dtype groups
    assert qms[0].nbytes == nf32 + -(-nf32 // 32) + nbf + -(-nbf // 32)
    assert qms[2].nbytes == -(-nf32 // 2) + -(-nf32 // 32) + -(-nbf // 2) + -(-nbf // 32)
    dense = [copy.deepcopy(own).cpu()] + [qm.dequantize(own).cpu() for qm in qms]
    for w in (None, [0.4, 0.3, 0.2, 0.1]):
        exp = FedAvg.aggregate(dense, w)
        got = mix(own, qms, w)
        batch = mix_batch([(own, qms, w), (own, qms[:1], None)])
        assert all(q.device.type == ("cpu" if where == "cpu" else "cuda") for q in got.parameters())
        for a, b, c in zip(exp.parameters(), got.parameters(), batch[0].parameters()):
            assert torch.equal(a, b.cpu()) and torch.equal(b.cpu(), c.cpu())


def test_sharer_error_feedback_and_worker_tasks():
    torch.manual_seed(32)
    models = [Mixed().to(DEV) for _ in range(3)]
    # error feedback: the residual arenas follow the restatement over three shares
    sharer = MXSharer(models[0], fmt="fp4", error_feedback=True)
    resid = {name: np.zeros_like(r) for name, r in group_rows(models[0]).items()}
    for model in models:
        qm = sharer.share(model)
        for (name, x), dt in zip(group_rows(model).items(), (torch.float32, torch.bfloat16)):
            codes, scales, resid[name] = restate_quantize(x, name, "fp4", resid=resid[name])
            assert np.array_equal(qm.groups[dt][0].cpu().numpy(), codes) and np.array_equal(qm.groups[dt][1].cpu().numpy(), scales)
            assert eu.same_bits(eu.from_torch(sharer.resid[dt], name), resid[name], name)
    # the worker tasks: `format` selects MX, the sharer registry keeps and drops the residual
    task = {"model": models[1], "peer": 3, "format": "fp8_e5m2", "error_feedback": True, "session": "mx"}
    first = functions.quantize(SimpleNamespace(), task)[0]
    x = group_rows(models[1])["f32"]
    assert np.array_equal(first.groups[torch.float32][0].cpu().numpy(), restate_quantize(x, "f32", "fp8_e5m2")[0])
    second = functions.quantize(SimpleNamespace(), task)[0]  # the residual of the first share is added
    assert not torch.equal(first.groups[torch.float32][0], second.groups[torch.float32][0])
    functions.reset_sharers("mx")
    assert torch.equal(functions.quantize(SimpleNamespace(), task)[0].groups[torch.float32][0], first.groups[torch.float32][0])
    got = functions.aggregate_quantized(SimpleNamespace(), {"model": models[0], "quant_models": [first, second]})[0]
    exp = FedAvg.aggregate([models[0]] + [qm.dequantize(models[0]) for qm in (first, second)], None)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(exp.parameters(), got.parameters()))
    integer = QuantSharer(models[0]).share(models[0])
    with pytest.raises(ValueError, match="mixes"):
        functions.aggregate_quantized(SimpleNamespace(), {"model": models[0], "quant_models": [first, integer]})
