"""dlsim_topk_select on the GPU against a numpy restatement of its contract:
fp32 subtraction, keys as uint32 with the sign bit cleared, np.lexsort on
(index, -key), the first k taken, their indices sorted. idx, val and the
updated ref are compared bit for bit (val and ref as integers, so NaN payloads
count). x is placed on its own, ref, idx and val inside 0xA5 guard bands
(_edge_util.guarded): no byte outside idx[0:k], val[0:k] and ref is written."""
from __future__ import annotations

import threading

import numpy as np
import pytest
import torch
from torch import nn

import _edge_util as eu

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native  # noqa: E402
from dasklearn_amd.sparse import TopKSharer  # noqa: E402

DEV = "cuda"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def widen(a, dtype):
    return a.astype(np.float32) if dtype == "f32" else eu.decode(a, dtype).astype(np.float32)


def expected(xs, rs, k, dtype):
    """(idx, val bits, new ref bits) of the contract for storage rows xs, rs."""
    with np.errstate(all="ignore"):
        key = (widen(xs, dtype) - widen(rs, dtype)).view(np.uint32) & np.uint32(0x7FFFFFFF)
    order = np.lexsort((np.arange(key.size), -key.astype(np.int64)))
    sel = np.sort(order[:k]).astype(np.int32)
    xb, ref = eu.bits_of(xs, dtype), eu.bits_of(rs, dtype).copy()
    ref[sel] = xb[sel]
    return sel, xb[sel], ref.view(np.asarray(rs).dtype), (int(key[order[k - 1]]) if k else None)


def run(dtype, xs, rs, k, x_off=0, ref_off=0, stream=None, what=""):
    esz, p = eu.ESIZE[dtype], xs.size
    x = eu.place([xs], dtype, DEV, [x_off])[0]
    href = eu.guarded(p * esz, dtype, DEV, offset=ref_off)
    href.view.copy_(eu.to_torch(rs, dtype))
    hidx, hval, hthr = eu.guarded(k * 4, "f32", DEV), eu.guarded(k * esz, dtype, DEV), eu.guarded(4, "f32", DEV)
    idx = hidx.view.view(torch.int32)
    vec = x.data_ptr() % 16 == 0 and href.view.data_ptr() % 16 == 0
    assert _native.topk_kernel_name(x, href.view, k) == ("" if k == 0 else
                                                         f"dlsim::k_topk_write<{'vec' if vec else 'scalar'}>")
    torch.cuda.synchronize()  # the buffers were filled on the default stream
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        _native.topk_select(x, href.view, k, idx, hval.view, threshold=hthr.view.view(torch.int32) if k else None)
    torch.cuda.synchronize()
    want_idx, want_val, want_ref, want_thr = expected(xs, rs, k, dtype)
    for h, name in ((href, "ref"), (hidx, "idx"), (hval, "val"), (hthr, "threshold")):
        assert not eu.check_guards(h), f"{what}: bytes around {name} written: {eu.check_guards(h)[:4]}"
    got_idx = idx.cpu().numpy()
    assert np.array_equal(got_idx, want_idx), f"{what}: idx differs at {np.nonzero(got_idx != want_idx)[0][:5]}"
    assert np.array_equal(eu.bits_of(eu.from_torch(hval.view, dtype), dtype), want_val), f"{what}: val differs"
    assert np.array_equal(eu.bits_of(eu.from_torch(href.view, dtype), dtype), eu.bits_of(want_ref, dtype)), f"{what}: ref differs"
    assert eu.inputs_unchanged([x], [xs], dtype), f"{what}: x changed"
    if k:
        assert int(hthr.view.view(torch.int32).item()) == want_thr, f"{what}: threshold"


def tied_rows(dtype, p, seed):
    """x and ref whose deltas repeat (small integers over 8, signs mixed): every cut meets ties."""
    rng = np.random.default_rng(seed)
    return (eu.encode(rng.integers(-40, 41, p) / 8.0, dtype), eu.encode(rng.integers(-3, 4, p) / 8.0, dtype))


def boundaries(dtype):
    g = _native.topk_geometry(1, TDT[dtype])
    return [b + d for b in (g["vec_tile"], g["block_tile"], g["max_blocks"] * g["block_tile"]) for d in (-1, 0, 1)]


@pytest.mark.parametrize("dtype,p", [(dt, p) for dt in ("f32", "bf16") for p in [1, 2, 3] + boundaries(dt)])
def test_lengths_at_the_vector_tile_block_tile_and_grid_stride(dtype, p):
    xs, rs = tied_rows(dtype, p, seed=p)
    ks = [max(p // 7, 1)] if p > 100_000 else sorted({0, 1, p - 1, p, max(p // 7, 1)})
    for k in ks:
        run(dtype, xs, rs, k, what=f"{dtype} P={p} k={k}")


@pytest.mark.parametrize("off", ["x", "ref"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_misaligned_pointer_takes_the_scalar_form(dtype, off):
    g = _native.topk_geometry(1, TDT[dtype])
    p, esz = g["block_tile"] + g["vec_tile"] + 5, eu.ESIZE[dtype]
    xs, rs = tied_rows(dtype, p, seed=77)
    for k in (1, p // 7, p):
        run(dtype, xs, rs, k, x_off=esz if off == "x" else 0, ref_off=esz if off == "ref" else 0,
            what=f"{dtype} {off} off alignment k={k}")


def hard_rows(dtype, kind, p):
    """Data that breaks a wrong radix select; (x, ref, [k, ...])."""
    i = np.arange(p)
    zeros = eu.encode(np.zeros(p), dtype)
    if kind == "all_equal":  # the result is purely the tie rule
        return eu.encode(np.where(i % 2 == 0, 1.0, -1.0), dtype), zeros, [1, p // 3, p - 1]
    if kind == "two_values":  # the cut falls inside the lower value
        return eu.encode(np.where(i % 3 == 0, -2.0, 1.0), dtype), zeros, [p // 2, p // 3 + 1]
    if kind == "lowest_digit":  # keys that differ in the lowest 10 bits only
        if dtype == "f32":
            return (np.uint32(0x3F800000) + (i * 7 % 1024).astype(np.uint32)).view(np.float32), zeros, [p // 5, 3]
        return eu.encode(np.ones(p), dtype), eu.encode(2.0 ** -(15.0 + i % 10), dtype), [p // 5, 3]
    if kind == "highest_digit":  # keys that differ in the highest 11 bits only
        return eu.encode((1.0 + 0.125 * (i % 8)) * 2.0 ** (i * 5 % 60 - 30), dtype), zeros, [p // 5, 3]
    assert kind == "specials"  # +-0, subnormals, +-Inf and NaN deltas, Inf - Inf among them
    tiny = eu._SUBNORMALS[dtype]
    pool = np.array([0.0, -0.0, tiny[0], -tiny[1], np.inf, -np.inf, np.nan, 1.0, -2.0, np.inf, 3.0])
    refs = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, np.inf, 3.0])
    n_nan = int((i % 11 == 6).sum() + (i % 11 == 9).sum())
    return eu.encode(pool[i % 11], dtype), eu.encode(refs[i % 11], dtype), [n_nan - 1, n_nan + 3, p // 2, p - 2]


@pytest.mark.parametrize("kind", ["all_equal", "two_values", "lowest_digit", "highest_digit", "specials"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_data_that_breaks_a_wrong_radix_select(dtype, kind):
    g = _native.topk_geometry(1, TDT[dtype])
    p = 2 * g["block_tile"] + 37
    xs, rs, ks = hard_rows(dtype, kind, p)
    for k in ks:
        run(dtype, xs, rs, k, what=f"{dtype} {kind} k={k}")


def test_a_side_stream_and_two_caller_threads_own_their_workspaces():
    p = 3 * _native.topk_geometry(1, torch.float32)["block_tile"] + 11
    errors = []

    def work(seed):
        try:
            st = torch.cuda.Stream()
            xs, rs = tied_rows("f32", p, seed)
            for k in (p // 9, p // 2, 5):
                run("f32", xs, rs, k, stream=st, what=f"thread {seed} k={k}")
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(s,)) for s in (1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


class Mixed(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(67, 33)
        self.b = nn.Linear(33, 9).to(torch.bfloat16)


def test_two_consecutive_shares_of_a_model_with_fp32_and_bf16_groups():
    torch.manual_seed(3)
    model = Mixed().to(DEV)
    sharer = TopKSharer(model, ratio=0.1)
    flat = lambda dt: torch.cat([q.detach().reshape(-1) for q in model.parameters() if q.dtype == dt])  # noqa: E731
    refs = {name: eu.encode(np.zeros(flat(dt).numel()), name) for name, dt in TDT.items()}
    assert sum(sharer.shares) == sharer.k == int(0.1 * sum(q.numel() for q in model.parameters()))
    for step in range(2):
        sm = sharer.share(model)
        torch.cuda.synchronize()
        for (name, dt), kg in zip(TDT.items(), sharer.shares):
            idx, val, size = sm.groups[dt]
            want_idx, want_val, refs[name], _ = expected(eu.from_torch(flat(dt), name), refs[name], kg, name)
            assert size == refs[name].size and np.array_equal(idx.cpu().numpy(), want_idx), f"step {step} {name}"
            assert np.array_equal(eu.bits_of(eu.from_torch(val, name), name), want_val), f"step {step} {name}"
            assert np.array_equal(eu.bits_of(eu.from_torch(sharer.ref[dt], name), name), eu.bits_of(refs[name], name))
        assert sm.nbytes == sum(k * (4 + e) for k, e in zip(sharer.shares, (4, 2)))
        with torch.no_grad():  # the second share selects from the deltas the first one left
            for q in model.parameters():
                q.add_(torch.randn_like(q, dtype=torch.float32).to(q.dtype) * 0.01)
