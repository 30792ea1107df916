"""TEST INFRASTRUCTURE: guard bands around outputs and special-value inputs
for the edge tests (tests/test_edge_util_cpu.py, tests/test_gpu_edges_*.py,
scripts/fuzz_parity.py).

Storage convention (the oracle's): a row is a numpy array of float32 ("f32"),
float64 ("f64") or uint16 bit patterns ("bf16", "f16").

* guarded / guarded_many / check_guards: an output that is a typed view into
  the middle of one uint8 buffer filled with 0xA5. A kernel that writes a byte
  outside the view changes a guard byte; one that leaves an element unwritten
  leaves the 0xA5 pattern in the view, which no input generator here produces
  and no oracle result of these inputs equals.
* special_rows / special_block / special_weights / edge_positions: random rows
  with a block of special values (signed zeros, Inf, NaN, subnormals, sums
  that overflow) written where a kernel's code paths change.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import oracle as orc

FILL = 0xA5
DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
ESIZE = {"f32": 4, "f64": 8, "bf16": 2, "f16": 2}
VEC_ELEMS = {"f32": 4, "f64": 2, "bf16": 8, "f16": 8}  # elements of a 16-byte vector
_UINT = {"f32": np.uint32, "f64": np.uint64, "bf16": np.uint16, "f16": np.uint16}
_INT_VIEW = {"f32": torch.int32, "f64": torch.int64, "bf16": torch.int16, "f16": torch.int16}
_STORE = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16, "f16": np.uint16}


def group_size(dtype: str) -> int:
    """Inputs per load group of the runtime fan-in kernels (dispatch.hpp group_size)."""
    return 8 if ESIZE[dtype] >= 4 else 4


# ---- storage <-> torch ------------------------------------------------------------
def bits_of(a, dtype: str) -> np.ndarray:
    """A storage array (or the oracle's float16 result) as unsigned integers."""
    a = np.ascontiguousarray(a)
    return a.view(_UINT[dtype])


def to_torch(a, dtype: str) -> torch.Tensor:
    """A storage array as a CPU tensor of the dtype (a copy)."""
    b = bits_of(a, dtype)
    signed = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}[_UINT[dtype]]
    return torch.from_numpy(b.view(signed).copy()).view(DTYPES[dtype])


def from_torch(t: torch.Tensor, dtype: str) -> np.ndarray:
    """A tensor's elements as a storage array on the host."""
    t = t.detach().cpu().contiguous()
    return t.view(_INT_VIEW[dtype]).numpy().view(_UINT[dtype]).view(_STORE[dtype]).copy()


def encode(x64, dtype: str) -> np.ndarray:
    """float64 values rounded (nearest-even) into the dtype's storage."""
    x64 = np.asarray(x64, dtype=np.float64)
    with np.errstate(all="ignore"):
        if dtype == "f64":
            return x64.copy()
        x32 = x64.astype(np.float32)
        if dtype == "f32":
            return x32
        if dtype == "bf16":
            return orc.f32_to_bf16_bits(x32).reshape(x32.shape)
        return orc.f32_to_f16_bits(x32).view(np.uint16)


def decode(a, dtype: str) -> np.ndarray:
    """Storage as exact float64 values."""
    a = np.asarray(a)
    if dtype == "bf16":
        return orc.bf16_bits_to_f32(a).astype(np.float64)
    if dtype == "f16":
        return a.view(np.uint16).view(np.float16).astype(np.float64)
    return a.astype(np.float64)


def fill_pattern(dtype: str):
    """The element a prefilled, unwritten output holds (0xA5 in every byte)."""
    return _UINT[dtype](int.from_bytes(bytes([FILL]) * ESIZE[dtype], "little"))


def avoid_fill(a, dtype: str) -> np.ndarray:
    """No element of an input may look like an unwritten output element."""
    b = bits_of(a, dtype)
    hit = b == fill_pattern(dtype)
    if hit.any():
        b = b.copy()
        b[hit] ^= _UINT[dtype](1)
    return b.view(_STORE[dtype])


def same_bits(got, exp, dtype: str) -> bool:
    """orc.same_bits on storage of dtype (f16 compared as binary16)."""
    if dtype == "f16":
        return orc.same_bits(bits_of(got, dtype).view(np.float16), bits_of(exp, dtype).view(np.float16))
    return orc.same_bits(np.asarray(got), np.asarray(exp))


def diff_report(got, exp, dtype: str, limit: int = 6) -> str:
    g, e = bits_of(got, dtype).reshape(-1), bits_of(exp, dtype).reshape(-1)
    if g.shape != e.shape:
        return f"shapes differ: {g.shape} / {e.shape}"
    gv, ev = decode(np.asarray(got).reshape(-1), dtype), decode(np.asarray(exp).reshape(-1), dtype)
    bad = np.nonzero((g != e) & ~(np.isnan(gv) & np.isnan(ev)))[0]
    return f"{bad.size} of {g.size} elements differ; first: " + ", ".join(
        f"[{i}] got {int(g[i]):#x} want {int(e[i]):#x}" for i in bad[:limit])


# ---- guard bands --------------------------------------------------------------------
class Guarded:
    """One 0xA5-filled uint8 buffer and the typed views into it. regions[k] =
    (first byte, byte count) of views[k]; every other byte is a guard."""

    def __init__(self, buf, regions, dtype):
        self.buf, self.regions, self.dtype = buf, regions, dtype
        self.views = [buf[s:s + nb].view(DTYPES[dtype]) for s, nb in regions]

    @property
    def view(self):
        return self.views[0]


def _alloc(total: int, device) -> torch.Tensor:
    """The 0xA5-filled buffer. On a GPU its base must be 128-byte aligned: the
    views' offsets are then their misalignment, which selects the kernels'
    paths (host allocations, used by the CPU self-tests only: 64)."""
    total = (total + 255) // 256 * 256
    buf = torch.full((total,), FILL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % (128 if buf.is_cuda else 64) == 0, "guard buffer base not line-aligned"
    return buf


def guarded(nbytes: int, dtype: str, device, offset: int = 0, band: int = 4096) -> Guarded:
    """A view of `nbytes` bytes of `dtype`, `band + offset` bytes into a buffer
    of band + offset + nbytes + band bytes (rounded up to 256) filled with
    0xA5. The allocation is 128-byte aligned on a GPU (_alloc asserts it) and
    band is a multiple of 128, so `offset` is the view's misalignment: 0 / 16
    keep the vector paths, one element gives the scalar path, 16 k mod 128 the
    chunk-mean heads."""
    assert band % 128 == 0 and offset % ESIZE[dtype] == 0 and nbytes % ESIZE[dtype] == 0
    buf = _alloc(band + offset + nbytes + band, device)
    return Guarded(buf, [(band + offset, nbytes)], dtype)


def guarded_many(sizes, dtype: str, device, gap: int = 16, align: int = 16, offset: int = 0,
                 band: int = 4096) -> Guarded:
    """Views of sizes[k] elements laid out in one buffer as an arena lays out
    parameters: view k + 1 starts at the first `align`-byte boundary (plus
    `offset`) that leaves at least `gap` guard bytes after view k, so a
    neighbour is `gap` to `gap + align - 1` bytes away; full bands at both ends."""
    esz = ESIZE[dtype]
    assert band % 128 == 0 and offset % esz == 0 and align % esz == 0 and offset < align
    regions, pos = [], band
    for k, n in enumerate(sizes):
        start = pos if k == 0 else (pos + gap + align - 1) // align * align
        start += offset
        regions.append((start, int(n) * esz))
        pos = start + int(n) * esz
    return Guarded(_alloc(pos + band, device), regions, dtype)


def check_guards(h: Guarded, limit: int = 64):
    """The guard bytes that no longer hold 0xA5 (at most `limit` of them), as
    (view index k, byte offset relative to view k's first byte, value): a byte
    before the first view belongs to view 0 with a negative offset, every other
    one to the view it follows, with an offset >= that view's byte count.
    Empty when clean."""
    host = h.buf.detach().cpu().numpy()
    guard = np.ones(host.size, dtype=bool)
    for s, nb in h.regions:
        guard[s:s + nb] = False
    bad = np.nonzero(guard & (host != FILL))[0]
    starts = np.array([s for s, _ in h.regions])
    out = []
    for i in bad[:limit]:
        k = max(int(np.searchsorted(starts, i, side="right")) - 1, 0)
        out.append((k, int(i) - int(starts[k]), int(host[i])))
    return out


def unwritten(h: Guarded, k: int = 0) -> int:
    """Elements of view k that still hold the fill pattern."""
    return int((bits_of(from_torch(h.views[k], h.dtype), h.dtype) == fill_pattern(h.dtype)).sum())


def inputs_unchanged(devs, hosts, dtype: str) -> bool:
    """Byte equality of every input tensor with the host rows it was made from."""
    return all(np.array_equal(bits_of(from_torch(d, dtype), dtype), bits_of(np.asarray(x), dtype).reshape(-1))
               for d, x in zip(devs, hosts))


def place(rows, dtype: str, device, offsets=None):
    """Each storage row as its own device tensor, `offsets[i]` bytes past a
    128-byte aligned address (default 0)."""
    out = []
    for i, r in enumerate(rows):
        off = 0 if offsets is None else offsets[i]
        assert off % ESIZE[dtype] == 0
        r = np.asarray(r).reshape(-1)
        buf = torch.empty(128 + off + r.size * ESIZE[dtype], dtype=torch.uint8, device=device)
        lead = (-buf.data_ptr()) % 128 + off
        t = buf[lead:lead + r.size * ESIZE[dtype]].view(DTYPES[dtype])
        t.copy_(to_torch(r, dtype))
        out.append(t)
    return out


# ---- special values -------------------------------------------------------------------
_SUBNORMALS = {"f32": (1e-40, 1e-45), "bf16": (2.0 ** -130, 2.0 ** -133), "f16": (2.0 ** -20, 2.0 ** -24),
               "f64": (5e-324, 2.0 ** -1060)}
_TINY = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24, "f64": 5e-324}  # least subnormal
_MIN_NORMAL = {"f32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -14, "f64": 2.0 ** -1022}
_OVERFLOW = {"f32": (3e38, 3e38, -3e38), "bf16": (3e38, 3e38, -3e38), "f16": (60000.0, 60000.0, -65504.0),
             "f64": (1.7e308, 1.7e308, -1.7e308)}


def inf_inputs(dtype: str, n: int):
    """The inputs that hold an Inf in column group B: G - 1, G and n - 1 where
    the fan-in spans more than one group of G inputs, else n / 2 and n - 1."""
    g = group_size(dtype)
    return sorted({g - 1, g, n - 1} if n > g else {n // 2, n - 1})


def special_block(dtype: str, n: int):
    """(storage block of shape (n, W), names of its W columns). Which input
    holds which value is the point (column groups of the module docstring of
    tests/test_gpu_edges_reduce.py); the other inputs of a column hold small
    exact finite values. The columns a 1 to 3 element scalar tail can hold
    come first: all -0, +Inf in input 0, Inf in the first group-B input."""
    fill = np.array([0.125 * (1 + i % 5) for i in range(n)])
    cols, names = [], []

    def add(name, col):
        names.append(name)
        cols.append(np.asarray(col, dtype=np.float64))

    def only(i, v):
        c = fill.copy()
        c[i] = v
        return c

    b_in = inf_inputs(dtype, n)
    add("C_all_neg_zero", np.full(n, -0.0))
    add("A_pos_inf_in_0", only(0, np.inf))
    add(f"B_inf_in_{b_in[0]}", only(b_in[0], np.inf))
    add("A_neg_inf_in_0", only(0, -np.inf))
    for j in b_in[1:]:
        add(f"B_inf_in_{j}", only(j, np.inf))
    if n >= 2:
        j1, j2 = (b_in[0], b_in[1]) if len(b_in) > 1 else (0, n - 1)  # n > G: two different groups
        c = only(j1, np.inf)
        c[j2] = -np.inf
        add(f"B_match_{j1}_{j2}", c)
    c = np.full(n, -0.0)
    c[n - 1] = 0.0
    add("C_neg_zero_last_pos", c)
    add("C_neg_tiny_product", np.full(n, -_TINY[dtype]))
    add("D_nan_in_middle", only(n // 2, np.nan))
    s1, s2 = _SUBNORMALS[dtype]
    add("E_subnormal_a", np.full(n, s1))
    add("E_subnormal_b", np.array([s2 if i % 2 == 0 else -s2 for i in range(n)]))
    add("E_subnormal_product", np.full(n, 1.5 * _MIN_NORMAL[dtype]))
    c = np.zeros(n)
    big = _OVERFLOW[dtype]
    c[:min(n, 3)] = big[:min(n, 3)]
    add("F_overflow_and_back", c)
    if dtype == "f16":
        for name, col in f16_tie_columns(n):
            add(name, col)
    return np.stack([encode(c, dtype) for c in cols], axis=1), names


def f16_tie_value(w):
    """An fp16 value x whose product with the fp32 weight w is a
    double-rounding tie: rounding w * x to fp32 and then to fp16 (the
    reference) gives other bits than one rounding of the exact product straight
    to fp16 (what a fused multiply-and-convert computes); the largest such
    product among all positive finite fp16 x, or None (a zero or power-of-two
    weight has none: its products are exact)."""
    w = np.float32(w)
    x = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16)
    with np.errstate(all="ignore"):
        twice = (w * x.astype(np.float32)).astype(np.float16)
        exact = np.float64(w) * x.astype(np.float64)  # 24 x 11 bits: exact in a double
        once = exact.astype(np.float16)
    k = np.nonzero((twice.view(np.uint16) != once.view(np.uint16)) & np.isfinite(twice) & np.isfinite(once))[0]
    if k.size == 0:
        return None
    return float(x[k[np.argmax(np.abs(exact[k]))]])


@functools.lru_cache(maxsize=None)
def f16_tie_pool(count: int = 129):
    """`count` fp32 weights in (0.05, 1), each with an f16_tie_value (about
    one weight in ten has one), and those values: the "f16_tie" weight kind
    and column group G."""
    rng = np.random.default_rng(2011)
    ws, xs = [], []
    while len(ws) < count:
        w = np.float32(rng.uniform(0.05, 1.0))
        x = f16_tie_value(w)
        if x is not None:
            ws.append(float(w))
            xs.append(x)
    return tuple(ws), tuple(xs)


def f16_tie_inputs(n: int):
    """The inputs that get a column of group G: the first, both sides of the
    first boundary between load groups of 4, the middle and the last."""
    return sorted({0, 3, 4, n // 2, n - 1} & set(range(n)))


def f16_tie_columns(n: int):
    """Column group G: column "G_f16_tie_<i>" holds, in input i, the fp16 value
    whose product with input i's weight of the "f16_tie" kind is a
    double-rounding tie, and 0 in every other input. The exact fold's result
    is then the product itself, rounded to fp32 and then to fp16; a product
    rounded once, straight to fp16, shows in the output bits."""
    _, xs = f16_tie_pool(max(129, n))  # one seeded sequence: a longer pool extends a shorter one
    out = []
    for i in f16_tie_inputs(n):
        col = np.zeros(n)
        col[i] = xs[i]
        out.append((f"G_f16_tie_{i}", col))
    return out


def special_rows(dtype: str, n: int, p: int, positions, seed: int) -> np.ndarray:
    """(n, p) storage rows: normal * 0.05, with special_block(dtype, n) written
    at each element offset of `positions` (clipped at p; a later position
    overwrites an earlier one where they overlap)."""
    rng = np.random.default_rng(seed)
    if dtype == "f64":
        rows = rng.standard_normal((n, p)) * 0.05
    else:
        x = rng.standard_normal((n, p), dtype=np.float32) * np.float32(0.05)
        rows = x if dtype == "f32" else np.stack([orc.f32_to_bf16_bits(r) for r in x]) if dtype == "bf16" \
            else orc.f32_to_f16_bits(x).view(np.uint16).reshape(n, p)
    rows = avoid_fill(rows, dtype).reshape(n, p)
    if not rows.flags.writeable:
        rows = rows.copy()
    block, _ = special_block(dtype, n)
    for pos in positions:
        w = min(block.shape[1], p - pos)
        if w > 0:
            rows[:, pos:pos + w] = block[:, :w]
    return rows


def random_rows(dtype: str, n: int, p: int, seed: int) -> np.ndarray:
    return special_rows(dtype, n, p, (), seed)


WEIGHT_KINDS = ("dirichlet", "zero_in_middle", "negative", "subnormal", "one_hot", "f16_tie")


def special_weights(n: int, kind: str, dtype: str = "f32") -> np.ndarray:
    """The weights of one kind, resolved as the reference resolves a weight
    list (fp32-rounded; exact doubles for f64).
    zero_in_middle: weight 0 on inf_inputs(dtype, n), so those columns are
    0 * Inf = NaN; negative: 1, 1, 1 then negative weights (n <= 3: the last
    one negative), so the overflow column's three values meet unit weights;
    subnormal: 1e-39 in the middle; one_hot: 1 in the middle, 0 elsewhere;
    f16_tie (beyond the five kinds above, for column group G): positive weights
    whose product with that column's fp16 value is a double-rounding tie."""
    w = np.random.default_rng(1000 + n).dirichlet(np.ones(n))
    if kind == "zero_in_middle":
        w[inf_inputs(dtype, n)] = 0.0
    elif kind == "negative":
        w = np.array([1.0, 1.0, 1.0] + [-0.5 / (1 + i % 3) for i in range(max(n - 3, 0))])[:n]
        if n <= 3:
            w[n - 1] = -1.0
    elif kind == "subnormal":
        w[n // 2] = 1e-39
    elif kind == "one_hot":
        w = np.zeros(n)
        w[n // 2] = 1.0
    elif kind == "f16_tie":
        w = np.array(f16_tie_pool(max(129, n))[0][:n])
    elif kind != "dirichlet":
        raise ValueError(kind)
    lst = [float(v) for v in w]
    return orc.reference_weights_f64(n, lst) if dtype == "f64" else orc.reference_weights(n, lst)


def edge_positions(p: int, tile_elems: int, E: int):
    """Element offsets at which a specials block goes for a launch over p
    elements in tiles of tile_elems (deferred launches: R * 2048): the first
    vector of the first full tile, a vector in the middle of a wave's 64-vector
    span (lane 32 of wave 1), the last vector of the last full tile, the middle
    of the partial tile, and the scalar tail (the last p mod E elements)."""
    nvec = p // E
    full = nvec * E // tile_elems
    pos = []
    if full >= 1:
        pos += [0, min(96 * E, tile_elems - E), full * tile_elems - E]
    part = nvec * E - full * tile_elems
    if part > 0:
        pos.append(full * tile_elems + part // 2 // E * E)
    if p % E:
        pos.append(nvec * E)
    return sorted(set(pos))


# ---- one guarded launch of the flat reduce (GPU tests and their child processes) ---------
def expected_reduce(op: str, rows, w, dtype: str) -> np.ndarray:
    """The oracle's result of op "exact" / "fast" (weighted reduce) or "mean"."""
    if op == "mean":
        return orc.mean(list(rows), dtype)
    if op == "exact" and dtype == "f32":
        return orc.wreduce_rows_f32(np.asarray(rows), w)
    return orc.wreduce(list(rows), w, dtype, mode=op)


def reduce_case(op: str, dtype: str, rows, w, device, out_offset: int = 0, in_offsets=None, alias: bool = False,
                expected=None, alias_index: int = 0):
    """_native.wreduce (op "exact" / "fast") or _native.mean (op "mean") of the
    storage rows into a guarded output `out_offset` bytes off alignment
    (inputs: `in_offsets` bytes each; alias: the output is input `alias_index`,
    and `in_offsets` are those of the other inputs, in order). Returns
    the list of problems found, empty when the guards are clean, the view
    equals the oracle bit for bit and no other input changed."""
    from dasklearn_amd import _native
    rows = np.asarray(rows)
    n, p = rows.shape
    assert 0 <= alias_index < n
    h = guarded(p * ESIZE[dtype], dtype, device, offset=out_offset)
    others = [i for i in range(n) if not (alias and i == alias_index)]
    xs = place([rows[i] for i in others], dtype, device, in_offsets)
    kept = list(xs)  # the separately placed inputs, rows[others]: what must not change
    if alias:
        h.view.copy_(to_torch(rows[alias_index], dtype))
        xs.insert(alias_index, h.view)
    if op == "mean":
        _native.mean(xs, h.view)
    else:
        _native.wreduce(xs, w, h.view, _native.DLSIM_EXACT if op == "exact" else _native.DLSIM_FAST)
    torch.cuda.synchronize()
    exp = expected_reduce(op, rows, w, dtype) if expected is None else expected
    problems = []
    bad = check_guards(h)
    if bad:
        problems.append(f"guard bytes written (view, offset, value): {bad[:8]}")
    got = from_torch(h.view, dtype)
    if not same_bits(got, exp, dtype):
        problems.append(f"differs from the oracle ({unwritten(h)} elements unwritten): " + diff_report(got, exp, dtype))
    if not inputs_unchanged(kept, [rows[i] for i in others], dtype):
        problems.append("an input changed")
    return problems


# ---- a hand computation of the exact fold (the reference-only pre-check) -------------------
def _round_to(x32_or_64, dtype: str):
    if dtype in ("f32", "f64"):
        return x32_or_64
    return decode(encode(x32_or_64.astype(np.float64), dtype), dtype).astype(np.float32)


def hand_wreduce(rows, w, dtype: str, fused_product: bool = False) -> np.ndarray:
    """fedavg.py's fold in numpy, one IEEE operation per line: acc = x0 * 0,
    then acc = round(acc + round(w_i * x_i)) in input order; fp32 arithmetic
    rounded to the 16-bit format after every operation for bf16 / f16, double
    arithmetic for f64. Returns storage.
    fused_product (f16 only): the WRONG fold of a kernel that rounds the exact
    product straight to fp16, skipping the fp32 rounding; what column group G
    must tell from the right one."""
    ft = np.float64 if dtype == "f64" else np.float32
    x = [decode(r, dtype).astype(ft) for r in rows]
    with np.errstate(all="ignore"):
        acc = x[0] * ft(0.0)
        for wi, xi in zip(np.asarray(w, dtype=ft), x):
            if fused_product:
                assert dtype == "f16"
                prod = (np.float64(wi) * xi.astype(np.float64)).astype(np.float16).astype(np.float32)
            else:
                prod = _round_to(wi * xi, dtype)
            acc = _round_to(acc + prod, dtype)
    return encode(acc.astype(np.float64), dtype)


def classify(v) -> np.ndarray:
    """Per value: "nan", "+inf", "-inf", "+0", "-0" or "finite"."""
    v = np.asarray(v, dtype=np.float64)
    out = np.where(np.isnan(v), "nan", np.where(np.isinf(v), np.where(v > 0, "+inf", "-inf"),
                                                np.where(v == 0, np.where(np.signbit(v), "-0", "+0"), "finite")))
    return out


def hand_fast_class(rows, w, dtype: str) -> np.ndarray:
    """classify() of the FAST fold (acc = x0 * 0, then acc = fma(w_i, x_i, acc),
    one final rounding) computed in doubles. A double is not an exact fma, so
    only the class is meaningful, and only for columns whose terms are zeros,
    infinities, NaNs or far from cancelling: column groups A to D without the
    -tiny product."""
    x = [decode(r, dtype) for r in rows]
    with np.errstate(all="ignore"):
        acc = x[0] * 0.0
        for wi, xi in zip(np.asarray(w, dtype=np.float64), x):
            acc = wi * xi + acc
    return classify(acc)
