"""Block-quantised sharing without a GPU: the argument checks of dlsim_quantize,
dlsim_dequantize and dlsim_quant_wreduce (decided before any HIP call),
dlsim_quant_geometry at the block and tile boundaries, the buffer sizes, and the
worker tasks' export."""
from __future__ import annotations

import ctypes

import pytest
import torch

from dasklearn_amd import _native, functions

F32, BF16, F16, F64 = 0, 1, 2, 3
X, RES, CODES, SCALES, OUT = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20  # fake device addresses, 1 MiB apart


def quantize(x=X, resid=RES, p=1000, dtype=F32, bits=8, rounding=0, codes=CODES, scales=SCALES):
    lib = _native.load()
    rc = lib.dlsim_quantize(x, resid, p, dtype, bits, rounding, 7, codes, scales, None)
    return rc, lib.dlsim_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(dtype=F16), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(dtype=F64), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(bits=5), -1, "bits must be 4 or 8"),
    (dict(rounding=2), -1, "unknown rounding"),
    (dict(p=1 << 31), -1, "2^31"),
    (dict(x=0), -1, "null model"),
    (dict(codes=0), -1, "null code or scale"),
    (dict(scales=0), -1, "null code or scale"),
    (dict(scales=SCALES + 2), -1, "4-byte aligned"),
    (dict(resid=X + 4), -1, "model overlaps the residual"),
    (dict(codes=X + 3999), -1, "model overlaps the code"),
    (dict(scales=X), -1, "model overlaps the scale"),
    (dict(codes=RES), -1, "residual overlaps the code"),
    (dict(scales=RES + 3996), -1, "residual overlaps the scale"),
    (dict(scales=CODES + 996), -1, "code output overlaps the scale"),
    (dict(scales=CODES + 496, bits=4), -1, "code output overlaps the scale"),  # 500 code bytes at 4 bits
    (dict(p=0, x=0, resid=0, codes=0, scales=0), 0, ""),  # nothing launched, no pointer read
])
def test_quantize_argument_errors_need_no_gpu(kwargs, code, text):
    rc, msg = quantize(**kwargs)
    assert rc == code and text in msg, (rc, msg)


def dequantize(codes=CODES, scales=SCALES, p=1000, dtype=BF16, bits=4, out=OUT):
    lib = _native.load()
    rc = lib.dlsim_dequantize(codes, scales, p, dtype, bits, out, None)
    return rc, lib.dlsim_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(dtype=F16), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(bits=16), -1, "bits must be 4 or 8"),
    (dict(p=1 << 31), -1, "2^31"),
    (dict(codes=0), -1, "null code or scale"),
    (dict(out=0), -1, "null output"),
    (dict(out=CODES + 499), -1, "output overlaps the codes"),
    (dict(out=SCALES - 1998), -1, "output overlaps the scales"),
    (dict(p=0, codes=0, scales=0, out=0), 0, ""),
])
def test_dequantize_argument_errors_need_no_gpu(kwargs, code, text):
    rc, msg = dequantize(**kwargs)
    assert rc == code and text in msg, (rc, msg)


def wreduce(p=1000, m=1, bits=(8,), own=X, out=OUT, codes=CODES, scales=SCALES, dtype=F32):
    lib = _native.load()
    arr = ctypes.c_void_p * max(m, 1)
    rc = lib.dlsim_quant_wreduce(own, m, arr(*[codes] * max(m, 0)), arr(*[scales] * max(m, 0)),
                                 (ctypes.c_int * max(m, 1))(*bits), (ctypes.c_float * (max(m, 0) + 1))(*[1.0] * (max(m, 0) + 1)),
                                 out, p, dtype, None)
    return rc, lib.dlsim_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(dtype=F64), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(m=32, bits=(8,) * 32), -1, "0 <= m <= 31 (got 32)"),
    (dict(m=-1, bits=()), -1, "0 <= m <= 31 (got -1)"),
    (dict(bits=(2,)), -1, "bits must be 4 or 8"),
    (dict(p=1 << 31), -1, "2^31"),
    (dict(own=0), -1, "null dense row"),
    (dict(codes=0), -1, "null code or scale"),
    (dict(scales=SCALES + 1), -1, "4-byte aligned"),
    (dict(out=X + 4), -1, "partially overlaps the dense row"),
    (dict(out=CODES - 3000), -1, "overlaps the codes or scales"),
    (dict(out=SCALES - 3996), -1, "overlaps the codes or scales"),
    (dict(p=0, own=0, out=0, codes=0, scales=0), 0, ""),
])
def test_quant_wreduce_argument_errors_need_no_gpu(kwargs, code, text):
    rc, msg = wreduce(**kwargs)
    assert rc == code and text in msg, (rc, msg)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_geometry_at_the_block_and_tile_boundaries(dt):
    g = _native.quant_geometry(1, dt)
    tile, rtile, cap = g["tile_elems"], g["reduce_tile_elems"], g["max_blocks"]
    assert g["block_elems"] == 256 and rtile == 4096 and (g["max_tasks"], g["max_neighbours"]) == (32, 80)
    assert tile == 2 * 256 * (16 // torch.empty((), dtype=dt).element_size())
    zero = _native.quant_geometry(0, dt)
    assert (zero["blocks"], zero["reduce_blocks"], zero["code_bytes"], zero["n_scales"]) == (0, 0, 0, 0)
    for p, scales in [(1, 1), (255, 1), (256, 1), (257, 2), (4095, 16), (4097, 17)]:
        for bits in (8, 4):
            g = _native.quant_geometry(p, dt, bits)
            assert g["n_scales"] == scales and g["code_bytes"] == (p if bits == 8 else (p + 1) // 2), (p, bits, g)
    for key, t in (("blocks", tile), ("reduce_blocks", rtile)):
        for p, blocks in [(1, 1), (t, 1), (t + 1, 2), (cap * t, cap), (cap * t + 1, (cap + 2) // 2),
                          (2 * cap * t, cap), (2 * cap * t + 1, -(-(2 * cap + 1) // 3))]:
            assert _native.quant_geometry(p, dt)[key] == blocks, (key, p)
    with pytest.raises(TypeError):
        _native.quant_geometry(10, torch.float16)
    with pytest.raises(_native.DlsimError, match="bits must be 4 or 8"):
        _native.quant_geometry(10, dt, 3)


def test_worker_tasks_are_exported_and_unsupported_dtypes_are_named():
    assert "quantize" in functions.__all__ and "aggregate_quantized" in functions.__all__
    from dasklearn_amd.quant import QuantSharer
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 and bfloat16"):
            QuantSharer(torch.nn.Linear(3, 2).to(dt))
    with pytest.raises(ValueError, match="bits"):
        QuantSharer(torch.nn.Linear(3, 2), bits=2)
    with pytest.raises(ValueError, match="rounding"):
        QuantSharer(torch.nn.Linear(3, 2), rounding="up")
