"""The edge-test harness (tests/_edge_util.py) against fake "kernels": numpy
functions that write the oracle result into the guarded view, correctly or
with one of the faults the GPU edge tests exist to catch. Then the
reference-only pre-check: the oracle on every (dtype, fan-in, weight kind) the
GPU edge tests use, against a hand computation of the fold in numpy."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_util as eu
from oracle import oracle as orc

CPU = torch.device("cpu")
ALL_DTYPES = ["f32", "bf16", "f16", "f64"]


def _case(dtype, n=3, p=37):
    rows = eu.special_rows(dtype, n, p, (0,), seed=3)
    w = eu.special_weights(n, "dirichlet", dtype)
    return rows, orc.wreduce(list(rows), w, dtype)


def _write(h, k, exp, dtype, first=0, count=None):
    """The fake kernel's store: elements [first, first + count) of view k."""
    t = eu.to_torch(exp, dtype)
    count = t.numel() - first if count is None else count
    h.views[k][first:first + count].copy_(t[first:first + count])


def _write_raw(h, byte_off, value_elem, dtype):
    """A stray store of one element at an absolute byte offset of the buffer."""
    raw = np.frombuffer(eu.bits_of(np.asarray([value_elem]), dtype).tobytes(), dtype=np.uint8)
    h.buf[byte_off:byte_off + raw.size].copy_(torch.from_numpy(raw.copy()))


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("offset_elems", [0, 1])
def test_clean_writer_passes(dtype, offset_elems):
    rows, exp = _case(dtype)
    h = eu.guarded(exp.size * eu.ESIZE[dtype], dtype, CPU, offset=offset_elems * eu.ESIZE[dtype])
    assert h.buf.numel() % 256 == 0 and h.buf.numel() >= 2 * 4096 + exp.size * eu.ESIZE[dtype]
    assert eu.unwritten(h) == exp.size  # prefilled: nothing written yet
    _write(h, 0, exp, dtype)
    assert eu.check_guards(h) == []
    assert eu.same_bits(eu.from_torch(h.view, dtype), exp, dtype)
    assert eu.unwritten(h) == 0


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_write_one_element_before_the_view_is_reported(dtype):
    rows, exp = _case(dtype)
    esz = eu.ESIZE[dtype]
    h = eu.guarded(exp.size * esz, dtype, CPU)
    _write(h, 0, exp, dtype)
    start = h.regions[0][0]
    _write_raw(h, start - esz, eu.encode([1.0], dtype)[0], dtype)
    bad = eu.check_guards(h)
    assert bad and all(k == 0 for k, _, _ in bad)
    assert {off for _, off, _ in bad} <= set(range(-esz, 0)) and min(off for _, off, _ in bad) >= -esz
    assert eu.same_bits(eu.from_torch(h.view, dtype), exp, dtype)  # the view itself is right


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_write_one_element_after_the_view_is_reported(dtype):
    rows, exp = _case(dtype)
    esz = eu.ESIZE[dtype]
    h = eu.guarded(exp.size * esz, dtype, CPU, offset=16)
    _write(h, 0, exp, dtype)
    start, nb = h.regions[0]
    _write_raw(h, start + nb, eu.encode([1.0], dtype)[0], dtype)
    bad = eu.check_guards(h)
    assert bad and {off for _, off, _ in bad} <= set(range(nb, nb + esz))
    # 1.0 has a zero low byte in every format: the reported bytes are the changed ones only
    raw = eu.bits_of(eu.encode([1.0], dtype), dtype).tobytes()
    assert sorted(bad) == sorted((0, nb + i, b) for i, b in enumerate(raw) if b != eu.FILL)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_write_into_a_gap_of_guarded_many_is_reported(dtype):
    esz = eu.ESIZE[dtype]
    E = eu.VEC_ELEMS[dtype]
    sizes = [1, 3, E, E + 1, 2048, 0, 5]
    h = eu.guarded_many(sizes, dtype, CPU, gap=16)
    for (s, nb), n in zip(h.regions, sizes):
        assert s % 16 == 0 and nb == n * esz
    for (s0, nb0), (s1, _) in zip(h.regions, h.regions[1:]):
        assert 16 <= s1 - (s0 + nb0) < 32  # only a canary between neighbours
    assert h.regions[0][0] == 4096 and h.buf.numel() - sum(h.regions[-1]) >= 4096
    exps = []
    for k, n in enumerate(sizes):
        exps.append(eu.random_rows(dtype, 1, n, 10 + k)[0])
        _write(h, k, exps[-1], dtype)
    assert eu.check_guards(h) == []
    s, nb = h.regions[3]
    _write_raw(h, s + nb + 16 - esz, eu.encode([1.0], dtype)[0], dtype)  # the last element of view 3's gap
    bad = eu.check_guards(h)
    assert bad and all(k == 3 and nb + 16 - esz <= off < nb + 16 for k, off, _ in bad)
    for k, e in enumerate(exps):
        assert eu.same_bits(eu.from_torch(h.views[k], dtype), e, dtype)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_element_left_unwritten_fails_the_view_comparison(dtype):
    rows, exp = _case(dtype)
    for skip in (0, exp.size // 2, exp.size - 1):
        h = eu.guarded(exp.size * eu.ESIZE[dtype], dtype, CPU)
        _write(h, 0, exp, dtype, 0, skip)
        _write(h, 0, exp, dtype, skip + 1)
        assert eu.check_guards(h) == []
        assert not eu.same_bits(eu.from_torch(h.view, dtype), exp, dtype)
        assert eu.unwritten(h) == 1


def test_inputs_unchanged_sees_one_changed_byte():
    rows = eu.random_rows("bf16", 3, 100, 1)
    devs = eu.place(list(rows), "bf16", CPU, offsets=[0, 2, 16])
    assert [d.data_ptr() % 128 for d in devs] == [0, 2, 16]
    assert eu.inputs_unchanged(devs, rows, "bf16")
    devs[1][99] = 1.0
    assert not eu.inputs_unchanged(devs, rows, "bf16")


# ---- reduce_case's bookkeeping, on a fake kernel ------------------------------------------------
def _fake_native(monkeypatch, spoil=None):
    """_native.wreduce replaced by the oracle's fold of the tensors it is given,
    in the order it is given them, stored to `out` once every input is read (as
    the ABI allows out == inputs[i]); spoil: an input position it then
    overwrites with ones. Returns the list the calls are recorded in."""
    from dasklearn_amd import _native
    calls = []

    def wreduce(xs, w, out, mode=_native.DLSIM_EXACT):
        calls.append(([x.data_ptr() for x in xs], out.data_ptr()))
        res = orc.wreduce_rows_f32(np.stack([eu.from_torch(x, "f32") for x in xs]), w)
        out.copy_(eu.to_torch(res, "f32"))
        if spoil is not None:
            xs[spoil].fill_(1.0)

    monkeypatch.setattr(_native, "wreduce", wreduce)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    return calls


def _alias_case(n=5, p=37):
    rows = eu.special_rows("f32", n, p, (0,), seed=9)
    return rows, eu.special_weights(n, "dirichlet", "f32")  # five different weights: the order matters


@pytest.mark.parametrize("alias_index", [0, 1, 4])
def test_reduce_case_puts_the_aliased_output_at_alias_index(monkeypatch, alias_index):
    calls = _fake_native(monkeypatch)
    rows, w = _alias_case()
    assert eu.reduce_case("exact", "f32", rows, w, CPU, alias=True, alias_index=alias_index) == []
    (ins, out), = calls
    assert len(ins) == 5 and ins.index(out) == alias_index and ins.count(out) == 1
    # the other inputs in their order: the same rows folded in any other order differ
    moved = np.roll(rows, 1, axis=0)
    assert not orc.same_bits(orc.wreduce_rows_f32(moved, w), orc.wreduce_rows_f32(rows, w))
    assert eu.reduce_case("exact", "f32", rows, w, CPU, alias=True, alias_index=alias_index,
                          expected=orc.wreduce_rows_f32(moved, w)) != []


def test_reduce_case_alias_defaults_to_input_0_and_no_alias_ignores_the_index(monkeypatch):
    calls = _fake_native(monkeypatch)
    rows, w = _alias_case()
    assert eu.reduce_case("exact", "f32", rows, w, CPU, alias=True) == []
    assert eu.reduce_case("exact", "f32", rows, w, CPU) == []
    assert eu.reduce_case("exact", "f32", rows, w, CPU, alias_index=3) == []
    (a_ins, a_out), (b_ins, b_out), (c_ins, c_out) = calls
    assert a_ins[0] == a_out and b_out not in b_ins and c_out not in c_ins


@pytest.mark.parametrize("alias_index", [0, 2, 4])
def test_reduce_case_reports_a_changed_input_but_not_the_aliased_one(monkeypatch, alias_index):
    rows, w = _alias_case()
    for spoil in range(5):
        _fake_native(monkeypatch, spoil=spoil)
        found = eu.reduce_case("exact", "f32", rows, w, CPU, alias=True, alias_index=alias_index)
        if spoil == alias_index:  # the output itself: the view no longer equals the oracle
            assert found and all("input changed" not in f for f in found)
        else:
            assert found == ["an input changed"]


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_generators_never_produce_the_fill_pattern(dtype):
    fill = eu.fill_pattern(dtype)
    a = np.full(8, fill, dtype=eu.bits_of(eu.encode([0.0], dtype), dtype).dtype)
    assert not (eu.bits_of(eu.avoid_fill(a.view(eu._STORE[dtype]), dtype), dtype) == fill).any()
    rows = eu.special_rows(dtype, 5, 5000, (0, 100), 2)
    assert not (eu.bits_of(rows, dtype) == fill).any()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("p,tile", [(2 * 2048 + 4 * 37 + 3, 2048), (2 * 4 * 2048 + 2048 + 4 * 37 + 3, 4 * 2048),
                                    (2 * 5 * 2048 + 2, 5 * 2048), (2 * 4 * 2048, 4 * 2048), (7, 2048)])
def test_special_blocks_land_at_the_edge_positions(dtype, p, tile):
    E = eu.VEC_ELEMS[dtype]
    n = 9
    pos = eu.edge_positions(p, tile, E)
    nvec = p // E
    full = nvec * E // tile
    if full:
        assert pos[0] == 0 and (96 * E in pos or tile - E in pos)  # the first vector; lane 32 of wave 1
        assert full * tile - E in pos  # the last vector of the last full tile
    if nvec * E > full * tile:
        assert any(full * tile <= q < nvec * E for q in pos)  # inside the partial tile
    if p % E:
        assert pos[-1] == nvec * E  # the scalar tail
    assert all(0 <= q < p and q % E == 0 for q in pos)
    rows = eu.special_rows(dtype, n, p, pos, seed=5)
    block, names = eu.special_block(dtype, n)
    assert rows.shape == (n, p) and block.shape == (n, len(names)) and len(names) < 70
    for i, q in enumerate(pos):
        w = min(block.shape[1], p - q)
        if i + 1 < len(pos):
            w = min(w, pos[i + 1] - q)  # a later block overwrites where they overlap
        assert w >= 1
        assert np.array_equal(eu.bits_of(rows[:, q:q + w], dtype), eu.bits_of(block[:, :w], dtype)), (q, w)


def test_default_small_shape_is_two_tiles_a_partial_tile_and_a_tail():
    p = 2 * 2048 + 4 * 37 + 3
    assert p // 4 == 2 * 512 + 37 and p % 4 == 3  # fp32: 37 vectors and a 3-element tail
    assert p // 8 == 2 * 256 + 18 and p % 8 == 7  # 2-byte: 18 vectors and a 7-element tail
    assert eu.edge_positions(p, 2048, 4) == [0, 384, 4092, 4096 + 72, 4244]


# ---- the reference-only pre-check -------------------------------------------------------------
# every fan-in the GPU edge tests use (tests/test_gpu_edges_*.py)
EDGE_FAN_INS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 128, 129)


def _col(names, prefix):
    return [i for i, s in enumerate(names) if s.startswith(prefix)]


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("n", EDGE_FAN_INS)
@pytest.mark.parametrize("kind", eu.WEIGHT_KINDS)
def test_oracle_on_the_special_block_matches_a_hand_computation(dtype, n, kind):
    """If the oracle disagrees with IEEE arithmetic done by hand here, the
    oracle is wrong (a finding), not the kernels."""
    block, names = eu.special_block(dtype, n)
    w = eu.special_weights(n, kind, dtype)
    got = orc.wreduce(list(block), w, dtype)
    val = eu.decode(eu.bits_of(got, dtype).view(eu._STORE[dtype]), dtype)
    # the whole block, one IEEE operation at a time
    hand = eu.hand_wreduce(list(block), w, dtype)
    assert eu.same_bits(got, hand, dtype), eu.diff_report(got, hand, dtype) + f" {names}"
    # A: +-Inf in input 0 only: the seed x0 * 0 is NaN; D: a NaN in the middle
    for i in _col(names, "A_") + _col(names, "D_"):
        assert np.isnan(val[i]), names[i]
    if kind == "zero_in_middle":  # 0 * Inf = NaN must survive
        for i in _col(names, "B_"):
            assert np.isnan(val[i]), names[i]
    wv = np.asarray(w, dtype=np.float64)
    for i in _col(names, "B_match"):  # +Inf in input j1, -Inf in j2: NaN unless the weights' signs differ
        j1, j2 = (int(s) for s in names[i].split("_")[2:])
        with np.errstate(all="ignore"):
            p1, p2 = wv[j1] * np.inf, wv[j2] * -np.inf
        seed_nan = 0 in (j1, j2)  # an Inf in input 0: the seed x0 * 0 is NaN already
        assert np.isnan(val[i]) == bool(seed_nan or np.isnan(p1) or np.isnan(p2) or p1 != p2), names[i]
    # C: signed zeros by the sign rules. The seed x0 * (+0) has x0's sign, a
    # product w * x of zeros has the sign sign(w) xor sign(x) (a zero weight is
    # +0), and a sum of zeros is -0 only when every term is -0.
    for i in _col(names, "C_all_neg_zero") + _col(names, "C_neg_zero_last_pos"):
        xneg = np.signbit(eu.decode(block[:, i], dtype))
        all_neg = bool(xneg[0]) and bool((np.signbit(wv) != xneg).all())
        assert val[i] == 0 and bool(np.signbit(val[i])) == all_neg, (names[i], val[i])
    i = _col(names, "C_all_neg_zero")[0]
    if kind != "negative":  # no negative weight: -0 survives
        assert np.signbit(val[i])
    i = _col(names, "C_neg_tiny_product")[0]
    if (np.abs(wv) <= 0.5).all() and not (wv < 0).any():  # every product underflows to -0
        assert val[i] == 0 and np.signbit(val[i]), (names[i], val[i])


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", EDGE_FAN_INS)
def test_oracle_mean_on_the_special_block(dtype, n):
    """The mean sums from +0 (torch.stack(...).mean(0)): all -0 gives +0, an
    Inf in one input gives that Inf, a NaN or +Inf with -Inf gives NaN.
    (dlsim_mean takes no fp64, so no GPU edge test runs it.)"""
    block, names = eu.special_block(dtype, n)
    val = eu.decode(eu.bits_of(orc.mean(list(block), dtype), dtype).view(eu._STORE[dtype]), dtype)
    i = _col(names, "C_all_neg_zero")[0]
    assert val[i] == 0 and not np.signbit(val[i])
    for i in _col(names, "D_") + (_col(names, "B_match") if n > 1 else []):
        assert np.isnan(val[i]), names[i]
    assert val[_col(names, "A_pos")[0]] == np.inf and val[_col(names, "A_neg")[0]] == -np.inf


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("n", EDGE_FAN_INS)
@pytest.mark.parametrize("kind", eu.WEIGHT_KINDS)
def test_oracle_fast_on_the_special_block(dtype, n, kind):
    """FAST (an fma chain seeded x0 * 0, one final rounding), fp64 included as
    the GPU edge tests run it: NaN wherever input 0 is not finite or a zero
    weight meets an Inf; all -0 stays -0 under weights that are never negative;
    and on the zero / Inf / NaN columns (groups A to D without the -tiny
    product) the oracle's result has the class (NaN, +-Inf, +-0, finite) of
    the same chain computed by hand in doubles."""
    block, names = eu.special_block(dtype, n)
    w = eu.special_weights(n, kind, dtype)
    fast = orc.wreduce(list(block), w, dtype, mode="fast")
    fv = eu.decode(eu.bits_of(fast, dtype).view(eu._STORE[dtype]), dtype)
    for i in _col(names, "A_") + _col(names, "D_"):
        assert np.isnan(fv[i]), names[i]
    if kind == "zero_in_middle":
        for i in _col(names, "B_"):
            assert np.isnan(fv[i]), names[i]
    i = _col(names, "C_all_neg_zero")[0]
    wv = np.asarray(w, dtype=np.float64)
    # fma(w, -0, -0): the product is -0 for w >= 0 (a zero weight is +0), +0 for w < 0
    assert fv[i] == 0 and bool(np.signbit(fv[i])) == (not (wv < 0).any()), (names[i], fv[i])
    if kind != "negative":
        assert np.signbit(fv[i])
    cols = [c for c in _col(names, "A_") + _col(names, "B_") + _col(names, "C_") + _col(names, "D_")
            if names[c] != "C_neg_tiny_product"]
    hand = eu.hand_fast_class(list(block[:, cols]), w, dtype)
    assert list(eu.classify(fv[cols])) == list(hand), [names[c] for c in cols]


@pytest.mark.parametrize("n", EDGE_FAN_INS)
def test_f16_tie_columns_tell_two_roundings_from_one(n):
    """Column group G (fp16) under the "f16_tie" weights: the reference's fold
    (product rounded to fp32, then to fp16) and a fold whose product is rounded
    once, straight to fp16, give different bits in every G column, and the
    oracle gives the reference's. The columns sit at the first input, either
    side of the first boundary between load groups, the middle and the last."""
    block, names = eu.special_block("f16", n)
    cols = _col(names, "G_f16_tie_")
    at = [int(names[c].rsplit("_", 1)[1]) for c in cols]
    assert at == sorted({0, 3, 4, n // 2, n - 1} & set(range(n))) and at
    w = eu.special_weights(n, "f16_tie", "f16")
    assert w.dtype == np.float32 and w.size == n and (w > 0).all()
    sub = block[:, cols]
    twice = eu.hand_wreduce(list(sub), w, "f16")
    once = eu.hand_wreduce(list(sub), w, "f16", fused_product=True)
    assert (eu.bits_of(twice, "f16") != eu.bits_of(once, "f16")).all(), [names[c] for c in cols]
    assert np.isfinite(eu.decode(twice, "f16")).all() and np.isfinite(eu.decode(once, "f16")).all()
    assert eu.same_bits(orc.wreduce(list(sub), w, "f16"), twice, "f16")
    for c, i in zip(cols, at):  # one non-zero input per column: the product is the result
        x = eu.decode(block[:, c], "f16")
        assert np.count_nonzero(x) == 1 and x[i] != 0
        # the definition, spelled out on the one product
        exact = float(w[i]) * x[i]
        assert np.float16(np.float32(w[i]) * np.float32(x[i])) != np.float16(exact)


def test_zero_in_middle_weights_are_zero_exactly_where_the_infs_are():
    for dtype in ALL_DTYPES:
        g = eu.group_size(dtype)
        for n in EDGE_FAN_INS:
            idx = eu.inf_inputs(dtype, n)
            assert idx == (sorted({g - 1, g, n - 1}) if n > g else sorted({n // 2, n - 1}))
            w = eu.special_weights(n, "zero_in_middle", dtype)
            assert all(w[i] == 0 for i in idx) and (np.count_nonzero(w) == n - len(idx))
            assert eu.special_weights(n, "subnormal", dtype)[n // 2] == (
                1e-39 if dtype == "f64" else np.float32(1e-39))
            assert (eu.special_weights(n, "negative", dtype) < 0).any()
            oh = eu.special_weights(n, "one_hot", dtype)
            assert oh[n // 2] == 1 and np.count_nonzero(oh) == 1
