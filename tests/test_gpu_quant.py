"""dlsim_quantize, dlsim_dequantize, dlsim_quant_wreduce (flat and batched) and
dasklearn_amd.quant on the GPU, bit for bit against a numpy restatement of the
wire format's arithmetic (include/dlsim.h: float32 operations one at a time, a
uint32 hash); the reduce against the committed oracle's exact fold over rows
decoded by that restatement. Every output is a view inside 0xA5 guard bytes."""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import _edge_util as eu

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, functions  # noqa: E402
from dasklearn_amd.arena import to_device_arena  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.quant import QuantSharer, mix, mix_batch  # noqa: E402

DEV = "cuda"
F32 = np.float32
BAND = 4096
MAXV = {"f32": float(np.finfo(F32).max), "bf16": float(np.uint32(0x7f7f0000).view(F32))}
FORMATS = [(dt, bits) for dt in ("f32", "bf16") for bits in (8, 4)]


# ---- the restatement ------------------------------------------------------------------
def mix32(h):
    h = np.atleast_1d(np.asarray(h, dtype=np.uint32))  # arrays wrap silently
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x7feb352d)
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x846ca68b)
    return h ^ (h >> np.uint32(16))


def widen(a, dtype):
    return eu.decode(a, dtype).astype(F32)  # exact: both formats are subsets of float32


def per_elem(v, p):
    return np.repeat(v, 256)[:p]


def restate_quantize(x, dtype, bits, stochastic=False, seed=0, resid=None):
    """(codes uint8, scales float32, new residual storage or None) of the storage row x."""
    p, qmax = x.size, F32(127 if bits == 8 else 7)
    with np.errstate(all="ignore"):
        t = widen(x, dtype) if resid is None else widen(x, dtype) + widen(resid, dtype)
        padded = np.zeros(-(-p // 256) * 256, F32)
        padded[:p] = t
        A = (padded.view(np.uint32) & np.uint32(0x7fffffff)).reshape(-1, 256).max(axis=1)
        a = A.view(F32)
        nan = A >= 0x7f800000
        ok = ~nan & ~(a < F32(2.0 ** -96))
        scale = np.where(nan, F32(np.nan), F32(0)).astype(F32)
        r = np.zeros_like(scale)
        scale[ok] = a[ok] / qmax
        r[ok] = qmax / a[ok]
        y = t * per_elem(r, p)
        if stochastic:
            h = mix32(np.arange(p, dtype=np.uint32) ^ mix32(np.uint32(seed)))
            z = np.floor(y + (h >> np.uint32(8)).astype(F32) * F32(2.0 ** -24))
        else:
            z = np.rint(y)
        q = np.clip(np.where(per_elem(ok, p), z, F32(0)), -qmax, qmax).astype(np.int32)
        new = None
        if resid is not None:
            xhat = widen(restate_decode(pack(q, bits), scale, p, dtype, bits), dtype)
            new = eu.encode((t - xhat).astype(np.float64), dtype)
    return pack(q, bits), scale, new


def pack(q, bits):
    if bits == 8:
        return q.astype(np.int8).view(np.uint8)
    n = np.zeros(-(-q.size // 2) * 2, np.uint8)
    n[:q.size] = q.astype(np.uint8) & 0xf
    return n[0::2] | (n[1::2] << 4)


def restate_decode(codes, scales, p, dtype, bits):
    """The storage row that codes and scales decode to."""
    if bits == 8:
        q = codes.view(np.int8).astype(F32)[:p]
    else:
        nib = np.stack([codes & 0xf, codes >> 4], axis=1).reshape(-1)[:p].astype(np.int32)
        q = ((nib ^ 8) - 8).astype(F32)
    with np.errstate(all="ignore"):
        return eu.encode((q * per_elem(scales, p)).astype(np.float64), dtype)


# ---- buffers ----------------------------------------------------------------------------
def guarded(nbytes, off=0, fill=None):
    """(0xA5 buffer, uint8 view of nbytes bytes `off` bytes past a 256-byte boundary inside it)."""
    buf = torch.full((2 * BAND + off + nbytes,), eu.FILL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[BAND + off:BAND + off + nbytes]
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)))
    return buf, view


def clean(buf, view):
    host, lo = buf.cpu().numpy(), view.data_ptr() - buf.data_ptr()
    return (host[:lo] == eu.FILL).all() and (host[lo + view.numel():] == eu.FILL).all()


def storage(view, dtype):
    return view.cpu().numpy().view(np.uint16 if dtype == "bf16" else F32)


def sizes(dtype):
    tile, cap = (_native.quant_geometry(1, eu.DTYPES[dtype])[k] for k in ("tile_elems", "max_blocks"))
    return [1, 255, 256, 257, 4095, 4097, tile - 1, tile + 1, cap * 4096 + 1]  # the last: two passes of every grid


@functools.lru_cache(maxsize=None)
def row(dtype, p, seed=0):
    return eu.random_rows(dtype, 1, p, seed)[0]  # shared: never written


def check_quantize(dtype, bits, rounding, with_resid, x, e, off, what):
    p, tdt, esz = x.size, eu.DTYPES[dtype], eu.ESIZE[dtype]
    seed = 0x9e3779b9 + p
    xb, xv = guarded(p * esz, off, x)
    eb, ev = guarded(p * esz, off, e)
    cb, cv = guarded((p * bits + 7) // 8, off)
    sb, sv = guarded(-(-p // 256) * 4, off)
    resid = ev.view(tdt) if with_resid else None
    form = "scalar" if off else "vec"
    used = [xv] + ([ev] if with_resid else []) + [cv]
    assert _native.quant_kernel_name("quantize", used, p, tdt) == f"dlsim::k_quantize<{form}>"
    _native.quantize(xv.view(tdt), cv, sv.view(torch.float32), bits, rounding, seed, resid)
    torch.cuda.synchronize()
    codes, scales, new = restate_quantize(x, dtype, bits, rounding == "stochastic", seed, e if with_resid else None)
    assert all(clean(b, v) for b, v in ((xb, xv), (eb, ev), (cb, cv), (sb, sv))), f"{what}: guard bytes written"
    assert np.array_equal(cv.cpu().numpy(), codes), f"{what}: codes differ at {np.nonzero(cv.cpu().numpy() != codes)[0][:5]}"
    assert eu.same_bits(storage(sv, "f32"), scales, "f32"), f"{what}: " + eu.diff_report(storage(sv, "f32"), scales, "f32")
    assert np.array_equal(storage(xv, dtype).view(np.uint8), x.view(np.uint8)), f"{what}: the model changed"
    want_e = new if with_resid else e
    assert eu.same_bits(storage(ev, dtype), want_e, dtype), f"{what}: residual " + eu.diff_report(storage(ev, dtype), want_e, dtype)
    return cv, sv


@pytest.mark.parametrize("with_resid", [False, True])
@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("dtype,bits", FORMATS)
def test_quantize_and_dequantize_at_every_length_and_form(dtype, bits, rounding, with_resid):
    for p in sizes(dtype):
        for off in (0, 4) if p in (257, 4097) else (0,):
            what = f"{dtype} {bits} bit {rounding} resid={with_resid} P={p} off={off}"
            cv, sv = check_quantize(dtype, bits, rounding, with_resid, row(dtype, p), row(dtype, p, 1), off, what)
            if rounding == "nearest" and not with_resid:
                check_dequantize(dtype, bits, cv.cpu().numpy(), storage(sv, "f32"), p, off, what)


def check_dequantize(dtype, bits, codes, scales, p, off, what):
    tdt = eu.DTYPES[dtype]
    _, cv = guarded(codes.size, off, codes)
    _, sv = guarded(scales.size * 4, off, scales)
    ob, ov = guarded(p * eu.ESIZE[dtype], off)
    form = "scalar" if off else "vec"
    assert _native.quant_kernel_name("dequantize", [cv, ov], p, tdt) == f"dlsim::k_dequantize<{form}>"
    _native.dequantize(cv, sv.view(torch.float32), bits, ov.view(tdt))
    torch.cuda.synchronize()
    exp = restate_decode(codes, scales, p, dtype, bits)
    assert clean(ob, ov), f"{what}: guard bytes written"
    assert eu.same_bits(storage(ov, dtype), exp, dtype), f"{what}: decode " + eu.diff_report(storage(ov, dtype), exp, dtype)


def special(kind, dtype, bits, n):
    """n values of one special block, as float64."""
    qmax, k = (127, 3) if bits == 8 else (7, -5)
    v = np.random.default_rng(5).standard_normal(n) * 0.05
    if kind == "zero":
        v[:] = 0.0
    elif kind == "signed_zero":
        v = np.where(np.arange(n) % 2, -0.0, 0.0)
    elif kind == "tiny":
        v = np.where(np.arange(n) % 3, 2.0 ** -97, -2.0 ** -100)
    elif kind == "subnormal":
        v = np.where(np.arange(n) % 2, 2.0 ** -130, -2.0 ** -133)
        v[n // 2] = 1.0
    elif kind == "inf_nan":
        v[0], v[n - 1] = np.inf, np.nan
    elif kind == "inf":
        v[n // 2] = -np.inf
    elif kind == "flt_max":
        v[0], v[n - 1] = MAXV[dtype], -MAXV[dtype]
    elif kind == "ties":  # r = 2^-k exactly, y = +-0.5, +-1.5, ...
        v = ((np.arange(n) % qmax) + 0.5) * 2.0 ** k * np.where(np.arange(n) % 2, -1.0, 1.0)
        v[0] = qmax * 2.0 ** k
    return v


@pytest.mark.parametrize("kind", ["zero", "signed_zero", "tiny", "subnormal", "inf_nan", "inf", "flt_max", "ties"])
@pytest.mark.parametrize("dtype,bits", FORMATS)
def test_special_blocks_first_middle_and_short_last(dtype, bits, kind):
    p = 4 * 256 + 99
    x = row(dtype, p, 2).copy()
    for start in (0, 512, 1024):
        n = min(256, p - start)
        x[start:start + n] = eu.encode(special(kind, dtype, bits, n), dtype)
    for rounding in ("nearest", "stochastic"):
        what = f"{dtype} {bits} bit {kind} {rounding}"
        cv, sv = check_quantize(dtype, bits, rounding, True, x, np.zeros_like(x), 0, what)
    scales = storage(sv, "f32")
    if kind in ("inf_nan", "inf"):
        assert np.isnan(scales[[0, 2, 4]]).all() and not cv.cpu().numpy()[:256 * bits // 8].any()
    if kind in ("zero", "signed_zero", "tiny"):
        assert not scales[[0, 2, 4]].view(np.uint32).any()
    check_dequantize(dtype, bits, cv.cpu().numpy(), scales, p, 0, what)


# ---- the reduce -------------------------------------------------------------------------
def neighbours(dtype, p, m, seed):
    """m neighbours of random code bytes and scales, bits alternating; NaN and zero scales in the second."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(m):
        bits = 8 if j % 2 == 0 else 4
        codes = rng.integers(0, 256, (p * bits + 7) // 8, dtype=np.uint8)
        scales = (rng.random(-(-p // 256), dtype=F32) * F32(1e-3)).astype(F32)
        if j == 1:
            scales[::3] = np.nan
            scales[1::3] = 0.0
        out.append((codes, scales, bits))
    return out


def place_neighbours(nbrs, off=0):
    return [(guarded(c.size, off, c)[1], guarded(s.size * 4, 0, s)[1].view(torch.float32), b) for c, s, b in nbrs]


def check_reduce(dtype, p, m, weights, alias=False, off=0, what=""):
    tdt, esz = eu.DTYPES[dtype], eu.ESIZE[dtype]
    own, nbrs = row(dtype, p, 3), neighbours(dtype, p, m, p + m)
    w = eu.orc.reference_weights(m + 1, None) if weights is None else eu.special_weights(m + 1, weights, dtype)
    ob, ov = guarded(p * esz, off, own if alias else None)
    xv = ov if alias else guarded(p * esz, off, own)[1]
    dn = place_neighbours(nbrs, off)
    form = "scalar" if off else "vec"
    assert _native.quant_kernel_name("wreduce", [xv, ov] + [c for c, _, _ in dn], p, tdt) == f"dlsim::k_quant_wreduce<{form}>"
    _native.quant_wreduce(xv.view(tdt), dn, w, ov.view(tdt))
    torch.cuda.synchronize()
    rows = [own] + [restate_decode(c, s, p, dtype, b) for c, s, b in nbrs]
    exp = eu.expected_reduce("exact", np.stack(rows), w, dtype)
    assert clean(ob, ov), f"{what}: guard bytes written"
    assert eu.same_bits(storage(ov, dtype), exp, dtype), f"{what}: " + eu.diff_report(storage(ov, dtype), exp, dtype)
    assert all(np.array_equal(c.cpu().numpy(), h) for (c, _, _), (h, _, _) in zip(dn, nbrs)), f"{what}: codes changed"


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("weights", ["dirichlet", None])
@pytest.mark.parametrize("m", [0, 1, 7, 31])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reduce_fan_ins_mixed_bits_weights_and_alias(dtype, m, weights, alias):
    check_reduce(dtype, 2 * 4096 + 37, m, weights, alias, what=f"{dtype} m={m} {weights} alias={alias}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reduce_at_every_length_and_in_the_scalar_form(dtype):
    for p in sizes(dtype):
        check_reduce(dtype, p, 3, "dirichlet", what=f"{dtype} P={p}")
    for p in (257, 4097):
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
        dn = place_neighbours(neighbours(dtype, p, m, 50 + t), off)
        w = eu.special_weights(m + 1, "dirichlet", dtype)
        ob, ov = guarded(p * esz, off)
        ref = torch.empty_like(xv)
        _native.quant_wreduce(xv, dn, w, ref)
        tasks.append((xv, dn, w, ov.view(tdt)))
        flat.append(ref)
        guards.append((ob, ov))
    torch.cuda.synchronize()
    _native.quant_wreduce_batched(tasks)
    torch.cuda.synchronize()
    for t, ((ob, ov), ref) in enumerate(zip(guards, flat)):
        assert clean(ob, ov), f"task {t}: guard bytes written"
        assert np.array_equal(ov.cpu().numpy(), ref.view(torch.uint8).cpu().numpy()), f"task {t} differs from its flat call"


@pytest.mark.parametrize("bits", [8, 4])
def test_stochastic_rounding_is_unbiased(bits):
    """4096 copies of one block: the per-position mean of the decoded values lies within 0.047 * scale
    of the input: 6 sigma with sigma <= scale / (2 * sqrt(4096)) for a rounding error of at most one step."""
    block = np.random.default_rng(21).standard_normal(256).astype(F32)
    x = np.tile(block, 4096)
    _, xv = guarded(x.size * 4, 0, x)
    _, cv = guarded(x.size * bits // 8)
    _, sv = guarded(4096 * 4)
    _native.quantize(xv.view(torch.float32), cv, sv.view(torch.float32), bits, "stochastic", 12345)
    scales = storage(sv, "f32")
    assert (scales == scales[0]).all()
    dec = restate_decode(cv.cpu().numpy(), scales, x.size, "f32", bits).astype(np.float64).reshape(4096, 256)
    assert np.abs(dec.mean(axis=0) - block).max() <= 0.047 * float(scales[0])


# ---- the Python layer -------------------------------------------------------------------
class Mixed(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(67, 33)
        self.b = nn.Linear(33, 9).to(torch.bfloat16)


def group_rows(model):
    """The model's dtype groups as storage rows, in layout order."""
    out = {}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        out[name] = eu.from_torch(torch.cat([q.detach().reshape(-1) for q in model.parameters() if q.dtype == dt]), name)
    return out


@pytest.mark.parametrize("where", ["arena", "cuda", "cpu"])
def test_mix_equals_fedavg_over_dequantised_models(where):
    torch.manual_seed(31)
    own = to_device_arena(Mixed(), DEV) if where == "arena" else Mixed().to(where)
    peers = [Mixed().to(DEV) for _ in range(3)]
    qms = [QuantSharer(q, bits=b, rounding=r, seed=5).share(q) for q, b, r in
           zip(peers, (8, 4, 8), ("nearest", "stochastic", "stochastic"))]
    assert qms[0].nbytes == 67 * 33 + 33 + 4 * 9 + 33 * 9 + 9 + 4 * 2
    dense = [copy.deepcopy(own).cpu()] + [qm.dequantize(own).cpu() for qm in qms]
    for w in (None, [0.4, 0.3, 0.2, 0.1]):
        exp = FedAvg.aggregate(dense, w)
        got = mix(own, qms, w)
        batch = mix_batch([(own, qms, w), (own, qms[:1], None)])
        assert all(q.device.type == ("cpu" if where == "cpu" else "cuda") for q in got.parameters())
        for a, b, c in zip(exp.parameters(), got.parameters(), batch[0].parameters()):
            assert torch.equal(a, b.cpu()) and torch.equal(b.cpu(), c.cpu())
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        mix(nn.Linear(3, 2).half().to(DEV), [])


def test_sharer_state_error_feedback_seeds_and_worker_tasks():
    torch.manual_seed(32)
    models = [Mixed().to(DEV) for _ in range(3)]
    # error feedback: the residual arenas follow the restatement over three shares
    sharer = QuantSharer(models[0], bits=4, error_feedback=True)
    resid = {name: np.zeros_like(r) for name, r in group_rows(models[0]).items()}
    for model in models:
        qm = sharer.share(model)
        for (name, x), dt in zip(group_rows(model).items(), (torch.float32, torch.bfloat16)):
            codes, scales, resid[name] = restate_quantize(x, name, 4, resid=resid[name])
            assert np.array_equal(qm.groups[dt][0].cpu().numpy(), codes)
            assert eu.same_bits(eu.from_torch(sharer.resid[dt], name), resid[name], name)
    # stochastic: share c uses mix32(seed + c)
    sharer = QuantSharer(models[0], bits=8, rounding="stochastic", seed=77)
    shares = [sharer.share(models[0]).groups[torch.float32][0].cpu().numpy() for _ in range(2)]
    x = group_rows(models[0])["f32"]
    for c, got in enumerate(shares):
        assert np.array_equal(got, restate_quantize(x, "f32", 8, True, int(mix32(77 + c)[0]))[0])
    assert not np.array_equal(shares[0], shares[1])
    # the worker tasks, and reset_sharers
    task = {"model": models[1], "peer": 3, "bits": 8, "rounding": "stochastic", "session": "q"}
    first = functions.quantize(SimpleNamespace(), task)[0]
    assert np.array_equal(first.groups[torch.float32][0].cpu().numpy(),
                          restate_quantize(group_rows(models[1])["f32"], "f32", 8, True, int(mix32(0)[0]))[0])
    second = functions.quantize(SimpleNamespace(), task)[0]
    assert not torch.equal(first.groups[torch.float32][0], second.groups[torch.float32][0])
    functions.reset_sharers("q")
    assert torch.equal(functions.quantize(SimpleNamespace(), task)[0].groups[torch.float32][0], first.groups[torch.float32][0])
    got = functions.aggregate_quantized(SimpleNamespace(), {"model": models[0], "quant_models": [first, second]})[0]
    exp = FedAvg.aggregate([models[0]] + [qm.dequantize(models[0]) for qm in (first, second)], None)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(exp.parameters(), got.parameters()))
