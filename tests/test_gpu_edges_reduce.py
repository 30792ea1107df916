"""Guard bands and special values on every tiled launch path of the flat
reduce (GPU): _native.wreduce (EXACT and FAST) and _native.mean.

Every case runs three checks (tests/_edge_util.py reduce_case): the 0xA5
guard bytes around the output are untouched, the output (prefilled with 0xA5,
so an unwritten element shows) equals the oracle bit for bit, and the inputs
are unchanged.

The inputs are normal * 0.05 rows with the specials block of
_edge_util.special_block written at _edge_util.edge_positions: the first
vector, a vector in the middle of a wave's span, the last vector of the last
full tile, the partial tile and the scalar tail. The block's column groups:
  A  +-Inf in input 0 only (the seed x0 * 0 is NaN)
  B  Inf in input G-1, G and n-1 (G = the kernels' group of 8 / 4 inputs), and
     +Inf with -Inf in two groups; the zero_in_middle weights put 0 on them
  C  all -0; all -0 but +0 last; a -tiny product that underflows to -0
  D  a NaN in a middle input only
  E  the dtype's subnormals as inputs and as a product
  F  values whose sum overflows the dtype in the middle of the fold
  G  fp16: in one input, the value whose product with that input's weight of
     the f16_tie kind is the double-rounding tie (to fp32, then to fp16, against
     once straight to fp16); 0 in the others, so the product is the result
The default shape is p = 2 * 2048 + 4 * 37 + 3: two full tiles, a partial tile
of 37 vectors and a 3-element tail in fp32; 18 vectors and a 7-element tail
for the 2-byte types.
"""
from __future__ import annotations

import pytest
import torch

import _edge_util as eu
from dasklearn_amd import _native

pytestmark = pytest.mark.gpu

P_SMALL = 2 * 2048 + 4 * 37 + 3
ALL_DTYPES = ["f32", "bf16", "f16", "f64"]
FIXED = [1, 2, 3, 8, 9, 14]  # the fixed fan-in tiled kernel (2-byte types: up to 9, above that the grouped form)
GROUPED = [15, 17, 128]  # the grouped kernel-argument form
DEVSLOTS = [129]  # pointers and weights in a device table


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def ops_of(dtype):
    return ("exact", "fast") if dtype == "f64" else ("exact", "fast", "mean")  # dlsim_mean takes no fp64


def small_tile(dtype, n):
    """Elements of a tile of the launch a small output takes (dispatch.hpp
    fixed_shape / grouped_shape, size class 0)."""
    fixed_max = 14 if eu.ESIZE[dtype] >= 4 else 9
    vpt = 1 if (n > fixed_max or eu.ESIZE[dtype] == 2) else 2
    return 256 * vpt * eu.VEC_ELEMS[dtype]


def assert_tiled(n, p, dtype, op):
    if dtype != "f64":  # dlsim_kernel_name takes the fp32 / bf16 / fp16 policies
        mode = None if op == "mean" else _native.DLSIM_EXACT if op == "exact" else _native.DLSIM_FAST
        assert _native.kernel_name(n, p, eu.DTYPES[dtype], mode) == "dlsim::k_wreduce_tiles"


def run_all_kinds(dtype, n, p, tile, seed, **kw):
    rows = eu.special_rows(dtype, n, p, eu.edge_positions(p, tile, eu.VEC_ELEMS[dtype]), seed)
    for op in ops_of(dtype):
        assert_tiled(n, p, dtype, op)
        for kind in (("dirichlet",) if op == "mean" else eu.WEIGHT_KINDS):
            w = eu.special_weights(n, kind, dtype)
            problems = eu.reduce_case(op, dtype, rows, w, dev(), **kw)
            assert not problems, (op, kind, problems)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("n", FIXED + GROUPED + DEVSLOTS)
def test_tiled_launch_guards_and_specials(n, dtype):
    """Fixed fan-in tiled (n <= 14; 2-byte: <= 9), the grouped kernel-argument
    form (15, 17, 128) and DevSlots (129), at the default small shape and at
    one with no partial tile and no tail, every weight kind."""
    run_all_kinds(dtype, n, P_SMALL, small_tile(dtype, n), seed=n)
    if n in (3, 17, 129):
        run_all_kinds(dtype, n, 2 * 2048, small_tile(dtype, n), seed=n + 1)  # whole tiles: the guard starts at nvec
        run_all_kinds(dtype, n, 2 * 2048 + 16, small_tile(dtype, n), seed=n + 2, out_offset=16)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("n", [3, 17, 129])
def test_scalar_kernel_guards_and_specials(n, dtype):
    """The scalar kernel: the output one element off alignment, then one input
    one element off alignment (the last one, then input 0)."""
    esz = eu.ESIZE[dtype]
    p = 2 * 256 + 37
    rows = eu.special_rows(dtype, n, p, (0, 255, 256, p - 3), seed=100 + n)
    for kw in (dict(out_offset=esz), dict(in_offsets=[0] * (n - 1) + [esz]), dict(in_offsets=[esz] + [0] * (n - 1))):
        for op in ops_of(dtype):
            for kind in (("dirichlet",) if op == "mean" else eu.WEIGHT_KINDS):
                problems = eu.reduce_case(op, dtype, rows, eu.special_weights(n, kind, dtype), dev(), **kw)
                assert not problems, (kw, op, kind, problems)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("n", [3, 17])
def test_output_aliasing_input_0_inside_a_guarded_buffer(n, dtype):
    run_all_kinds(dtype, n, P_SMALL, small_tile(dtype, n), seed=200 + n, alias=True)


# f32 size classes of the fixed fan-in tiled kernel (dispatch.hpp size_class): VPT 4 block map
# from 8 MB per stream, VPT 4 wave map from 20 MB, and VPT 4 below 8 MB for fan-in >= 6
# when the tiles spread evenly over the CUs (v4_tiles_even: 256 tiles on 256 CUs)
@pytest.mark.parametrize("n,p", [(2, 2_000_003), (2, 5_000_003), (8, 1_048_579)])
def test_f32_size_classes_guards_and_specials(n, p):
    tile = 256 * 4 * 4
    rows = eu.special_rows("f32", n, p, eu.edge_positions(p, tile, 4), seed=p % 1000)
    for op, kind in (("exact", "dirichlet"), ("exact", "zero_in_middle"), ("fast", "negative"), ("mean", "dirichlet")):
        assert_tiled(n, p, "f32", op)
        problems = eu.reduce_case(op, "f32", rows, eu.special_weights(n, kind, "f32"), dev())
        assert not problems, (op, kind, problems)


def test_bf16_large_class_global_nt_stores():
    """bf16 n = 2 at 48,000,011 elements (96 MB per stream): VPT 4, block map,
    plain global nt stores with no buffer range behind them. The only large
    case; one weight kind."""
    n, p = 2, 48_000_011
    tile = 256 * 4 * 8
    rows = eu.special_rows("bf16", n, p, eu.edge_positions(p, tile, 8), seed=48)
    assert_tiled(n, p, "bf16", "exact")
    problems = eu.reduce_case("exact", "bf16", rows, eu.special_weights(n, "zero_in_middle", "bf16"), dev())
    assert not problems, problems
    torch.cuda.empty_cache()
