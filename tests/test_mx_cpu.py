"""MX sharing without a GPU: the argument checks of every dlsim_mx_* entry
(decided before any HIP call), zero elements as a no-op, and the byte counts of
dlsim_mx_geometry."""
from __future__ import annotations

import ctypes

import pytest
import torch

from dasklearn_amd import _native, functions

F32, BF16, F16, F64 = 0, 1, 2, 3
X, RES, CODES, SCALES, OUT = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20  # fake device addresses, 1 MiB apart


def quantize(x=X, resid=RES, p=1000, dtype=F32, fmt=0, codes=CODES, scales=SCALES):
    lib = _native.load()
    rc = lib.dlsim_mx_quantize(x, resid, p, dtype, fmt, codes, scales, None)
    return rc, lib.dlsim_last_error().decode()


def dequantize(codes=CODES, scales=SCALES, p=1000, dtype=BF16, fmt=2, out=OUT):
    lib = _native.load()
    rc = lib.dlsim_mx_dequantize(codes, scales, p, dtype, fmt, out, None)
    return rc, lib.dlsim_last_error().decode()


def wreduce(p=1000, m=1, fmts=(0,), own=X, out=OUT, codes=CODES, scales=SCALES, dtype=F32):
    lib = _native.load()
    arr = ctypes.c_void_p * max(m, 1)
    rc = lib.dlsim_mx_wreduce(own, m, arr(*[codes] * max(m, 0)), arr(*[scales] * max(m, 0)),
                              (ctypes.c_int * max(m, 1))(*fmts), (ctypes.c_float * (max(m, 0) + 1))(*[1.0] * (max(m, 0) + 1)),
                              out, p, dtype, None)
    return rc, lib.dlsim_last_error().decode()


@pytest.mark.parametrize("call,kwargs,code,text", [
    (quantize, dict(dtype=F16), -2, "DLSIM_F32 and DLSIM_BF16"),
    (quantize, dict(dtype=F64), -2, "DLSIM_F32 and DLSIM_BF16"),
    (quantize, dict(fmt=3), -1, "unknown format 3"),
    (quantize, dict(p=1 << 31), -1, "2^31"),
    (quantize, dict(x=0), -1, "null model"),
    (quantize, dict(codes=0), -1, "null code or scale"),
    (quantize, dict(scales=0), -1, "null code or scale"),
    (quantize, dict(resid=X + 4), -1, "model overlaps the residual"),
    (quantize, dict(codes=X + 3999), -1, "model overlaps the code output"),
    (quantize, dict(scales=X), -1, "model overlaps the scale output"),
    (quantize, dict(codes=RES), -1, "residual overlaps the code output"),
    (quantize, dict(scales=RES + 3999), -1, "residual overlaps the scale output"),
    (quantize, dict(scales=CODES + 999), -1, "code output overlaps the scale output"),
    (quantize, dict(scales=CODES + 499, fmt=2), -1, "code output overlaps the scale output"),  # 500 code bytes in FP4
    (quantize, dict(p=0, x=0, resid=0, codes=0, scales=0), 0, ""),  # nothing launched, no pointer read
    (dequantize, dict(dtype=F16), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dequantize, dict(fmt=-1), -1, "unknown format -1"),
    (dequantize, dict(p=1 << 31), -1, "2^31"),
    (dequantize, dict(codes=0), -1, "null code or scale"),
    (dequantize, dict(out=0), -1, "null output"),
    (dequantize, dict(out=CODES + 499), -1, "output overlaps the codes"),
    (dequantize, dict(out=SCALES - 1999), -1, "output overlaps the scales"),
    (dequantize, dict(p=0, codes=0, scales=0, out=0), 0, ""),
    (wreduce, dict(dtype=F64), -2, "DLSIM_F32 and DLSIM_BF16"),
    (wreduce, dict(m=32, fmts=(0,) * 32), -1, "0 <= m <= 31 (got 32)"),
    (wreduce, dict(m=-1, fmts=()), -1, "0 <= m <= 31 (got -1)"),
    (wreduce, dict(fmts=(8,)), -1, "unknown format 8"),
    (wreduce, dict(p=1 << 31), -1, "2^31"),
    (wreduce, dict(own=0), -1, "null dense row"),
    (wreduce, dict(codes=0), -1, "null code or scale"),
    (wreduce, dict(out=X + 4), -1, "partially overlaps the dense row"),
    (wreduce, dict(out=CODES - 3000), -1, "overlaps the codes or scales"),
    (wreduce, dict(out=SCALES - 3999), -1, "overlaps the codes or scales"),
    (wreduce, dict(p=0, own=0, out=0, codes=0, scales=0), 0, ""),
])
def test_argument_errors_and_empty_rows_need_no_gpu(call, kwargs, code, text):
    rc, msg = call(**kwargs)
    assert rc == code and text in msg, (rc, msg)


def test_batched_and_host_only_entries_reject_bad_arguments():
    lib = _native.load()
    assert lib.dlsim_mx_wreduce_batched(-1, None, None, None, None, None, None, None, None, F32, None) == -1
    assert lib.dlsim_mx_wreduce_batched(0, None, None, None, None, None, None, None, None, F32, None) == 0
    assert lib.dlsim_mx_wreduce_batched(1, None, None, None, None, None, None, None, None, F32, None) == -1
    assert lib.dlsim_mx_geometry(10, F32, 0, None) == -1 and b"null result" in lib.dlsim_last_error()
    assert lib.dlsim_mx_kernel_name(0, None, 0, 0, F32) == b"" and lib.dlsim_mx_kernel_name(3, None, 0, 5, F32) == b""
    assert lib.dlsim_mx_kernel_name(2, None, 0, 5, F16) == b""
    ptrs = (ctypes.c_void_p * 2)(X, X + 4)
    assert lib.dlsim_mx_kernel_name(1, ptrs, 1, 5, BF16) == b"dlsim::k_mx_dequantize<vec>"
    assert lib.dlsim_mx_kernel_name(1, ptrs, 2, 5, BF16) == b"dlsim::k_mx_dequantize<scalar>"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_geometry_byte_counts_and_grids(dt):
    g = _native.mx_geometry(1, dt)
    tile, cap = g["tile_elems"], g["max_blocks"]
    assert g["block_elems"] == 32 and g["reduce_tile_elems"] == 4096 and (g["max_tasks"], g["max_neighbours"]) == (32, 80)
    assert tile == 2 * 256 * (16 // torch.empty((), dtype=dt).element_size())
    for p, scales in [(0, 0), (1, 1), (32, 1), (33, 2), (4097, 129)]:
        for fmt in ("fp8_e4m3", "fp8_e5m2", "fp4"):
            g = _native.mx_geometry(p, dt, fmt)
            assert (g["code_bytes"], g["scale_bytes"]) == ((p + 1) // 2 if fmt == "fp4" else p, scales) == _native.mx_sizes(p, fmt)
    assert (_native.mx_geometry(0, dt)["blocks"], _native.mx_geometry(0, dt)["reduce_blocks"]) == (0, 0)
    for key, t in (("blocks", tile), ("reduce_blocks", 4096)):
        for p, blocks in [(1, 1), (t, 1), (t + 1, 2), (cap * t, cap), (cap * t + 1, (cap + 2) // 2)]:
            assert _native.mx_geometry(p, dt)[key] == blocks, (key, p)
    with pytest.raises(TypeError):
        _native.mx_geometry(10, torch.float16)
    with pytest.raises(ValueError, match="format"):
        _native.mx_geometry(10, dt, "fp6")


def test_python_layer_names_unsupported_formats_and_dtypes():
    from dasklearn_amd.mx import MXSharer
    assert "quantize" in functions.__all__ and "aggregate_quantized" in functions.__all__
    with pytest.raises(ValueError, match="format"):
        MXSharer(torch.nn.Linear(3, 2), fmt="fp6")
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        MXSharer(torch.nn.Linear(3, 2).half())
