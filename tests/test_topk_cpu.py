"""Top-k sharing without a GPU: the argument checks of dlsim_topk_select and
dlsim_sparse_wreduce (decided before any HIP call), dlsim_topk_geometry at the
tile boundaries, TopKSharer's split of k over dtype groups, and the worker
tasks' export."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from dasklearn_amd import _native, functions
from dasklearn_amd.sparse import split_k

F32, BF16, F16, F64 = 0, 1, 2, 3
X, REF, IDX, VAL = 1 << 20, 2 << 20, 3 << 20, 4 << 20  # fake device addresses, 1 MiB apart


def select(x=X, ref=REF, p=1000, k=10, dtype=F32, idx=IDX, val=VAL):
    lib = _native.load()
    rc = lib.dlsim_topk_select(x, ref, p, k, dtype, idx, val, None, None)
    return rc, lib.dlsim_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(dtype=F16), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(dtype=F64), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(k=-1), -1, "0 <= k <= n_elems"),
    (dict(k=1001), -1, "0 <= k <= n_elems"),
    (dict(p=1 << 31, k=1), -1, "2^31"),
    (dict(x=0), -1, "null"),
    (dict(ref=0), -1, "null"),
    (dict(idx=0), -1, "null"),
    (dict(val=0), -1, "null"),
    (dict(idx=REF + 3996), -1, "last-shared copy overlaps the index"),
    (dict(val=REF), -1, "last-shared copy overlaps the value"),
    (dict(x=REF + 4), -1, "model overlaps the last-shared"),
    (dict(k=0, x=0, ref=0, idx=0, val=0), 0, ""),  # nothing to select: no pointer is read
    (dict(p=0, k=0), 0, ""),
])
def test_topk_select_argument_errors_need_no_gpu(kwargs, code, text):
    rc, msg = select(**kwargs)
    assert rc == code and text in msg, (rc, msg)


def sparse(p=1000, m=1, ks=(10,), own=X, out=REF, idx=IDX, val=VAL, dtype=F32):
    lib = _native.load()
    arr = ctypes.c_void_p * max(m, 1)
    rc = lib.dlsim_sparse_wreduce(own, m, arr(*[idx] * m), arr(*[val] * m), (ctypes.c_longlong * max(m, 1))(*ks),
                                  (ctypes.c_float * (m + 1))(*[1.0] * (m + 1)), out, p, dtype, None)
    return rc, lib.dlsim_last_error().decode()


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(dtype=F16), -2, "DLSIM_F32 and DLSIM_BF16"),
    (dict(m=32, ks=(1,) * 32), -1, "n must be <= 32 (got 33)"),
    (dict(m=-1, ks=()), -1, "m must be >= 0"),
    (dict(ks=(1001,)), -1, "0 <= k <= n_elems"),
    (dict(out=X + 4), -1, "partially overlaps the dense row"),
    (dict(out=IDX), -1, "overlaps an index or value list"),
    (dict(val=0), -1, "null index or value"),
    (dict(own=0), -1, "null dense row"),
    (dict(p=0, ks=(0,), own=0, out=0), 0, ""),
])
def test_sparse_wreduce_argument_errors_need_no_gpu(kwargs, code, text):
    rc, msg = sparse(**kwargs)
    assert rc == code and text in msg, (rc, msg)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_topk_geometry_at_the_tile_boundaries(dt):
    g = _native.topk_geometry(1, dt)
    vec, tile, cap = g["vec_tile"], g["block_tile"], g["max_blocks"]
    assert vec == 256 * (16 // torch.empty((), dtype=dt).element_size()) and tile % vec == 0
    assert _native.topk_geometry(0, dt)["blocks"] == 0 and _native.topk_geometry(0, dt)["workspace_bytes"] == 0
    for p, blocks in [(1, 1), (tile, 1), (tile + 1, 2), (cap * tile, cap), (cap * tile + 1, (cap + 1) // 2 + (cap + 1) % 2),
                      (2 * cap * tile, cap), (2 * cap * tile + 1, -(-(2 * cap + 1) // 3))]:
        g = _native.topk_geometry(p, dt)
        assert g["blocks"] == blocks, (p, g)
        assert g["workspace_bytes"] == 4 * (3 * 2048 + 16 + 2 * blocks)
    with pytest.raises(TypeError):
        _native.topk_geometry(10, torch.float16)


@pytest.mark.parametrize("sizes", [[10], [7, 3], [1, 1, 1], [1000, 1], [5, 0, 5], [62006, 40]])
def test_split_of_k_sums_to_k_and_fits_every_group(sizes):
    total = sum(sizes)
    for k in sorted({0, 1, 2, total // 7, total // 2, total - 1, total}):
        shares = split_k(k, sizes)
        assert sum(shares) == k and all(0 <= s <= n for s, n in zip(shares, sizes)), (k, shares)
        assert all(s >= k * n // total for s, n in zip(shares, sizes))  # the floors first
    with pytest.raises(ValueError):
        split_k(total + 1, sizes)


def test_worker_tasks_are_exported_and_unsupported_dtypes_are_named():
    assert "sparsify" in functions.__all__ and "aggregate_sparse" in functions.__all__
    from dasklearn_amd.sparse import TopKSharer
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 and bfloat16"):
            TopKSharer(torch.nn.Linear(3, 2).to(dt), k=1)
    assert np.array_equal(TopKSharer(torch.nn.Linear(3, 2), ratio=0.5).shares, [4])
