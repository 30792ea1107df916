"""ctypes binding of the HIP C ABI (include/dlsim.h -> lib/libdlsim_hip.so).

This is the only way the package computes: there is no CPU fallback. If the
library is missing or no GPU is visible, calls raise loudly.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional, Sequence

import numpy as np

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
LIB_PATH = os.path.join(LIB_DIR, "libdlsim_hip.so")

DLSIM_F32 = 0
DLSIM_BF16 = 1
DLSIM_F16 = 2
DLSIM_F64 = 3
DLSIM_EXACT = 0
DLSIM_FAST = 1
MAX_FUSED_INPUTS = 128
DLSIM_E_ARG = -1
DLSIM_E_RCCL = -4
DLSIM_E_PEER = -5  # another rank failed (dlsim_wreduce_sharded's agreement step)
DLSIM_E_DISAGREE = -6  # the ranks passed different n_elems / fan-in / dtype / gather
DLSIM_GATHER_NONE = 0
DLSIM_GATHER_BCAST = 1
DLSIM_GATHER_ALLGATHER = 2


def ab_env(name: str, default: Optional[str] = None) -> Optional[str]:
    """A DLSIM_* A/B switch (tuning studies): os.environ[name] only when
    DLSIM_AB=1 is set as well, else `default` -- the library's rule
    (csrc/ab_env.hpp), so a stray variable cannot change what runs."""
    if os.environ.get("DLSIM_AB") != "1":
        return default
    return os.environ.get(name, default)

# Every symbol include/dlsim.h declares (tests/test_abi.py checks the header
# against this list and the library's exports).
EXPORTS = (
    "dlsim_wreduce",
    "dlsim_wreduce_f64",
    "dlsim_wreduce_tensors",
    "dlsim_wreduce_batched",
    "dlsim_batch_table_bytes",
    "dlsim_batch_table_fill",
    "dlsim_batch_table_launch",
    "dlsim_mean",
    "dlsim_mean_batched",
    "dlsim_chunk_mean_batched",
    "dlsim_chunk_mean_ilp_begin",
    "dlsim_chunk_mean_plan",
    "dlsim_rccl_bind",
    "dlsim_wreduce_sharded",
    "dlsim_wreduce_sharded_f64",
    "dlsim_wreduce_mixed",
    "dlsim_sgd_step",
    "dlsim_sgd_step_tensors",
    "dlsim_sgd_momentum_step",
    "dlsim_sgd_momentum_step_tensors",
    "dlsim_robust_reduce",
    "dlsim_robust_reduce_tensors",
    "dlsim_robust_reduce_batched",
    "dlsim_robust_batch_geometry",
    "dlsim_robust_reduce_tensors_batched",
    "dlsim_robust_nearest_reduce",
    "dlsim_robust_nearest_reduce_tensors",
    "dlsim_pairwise_sqdist",
    "dlsim_pairwise_sqdist_tensors",
    "dlsim_pairdist_geometry",
    "dlsim_pairwise_sqdist_batched",
    "dlsim_pairdist_batch_geometry",
    "dlsim_wreduce_dist_batched",
    "dlsim_reducedist_batch_geometry",
    "dlsim_wreduce_dist",
    "dlsim_wreduce_dist_tensors",
    "dlsim_reducedist_geometry",
    "dlsim_device_alloc",
    "dlsim_device_free",
    "dlsim_pool_alloc",
    "dlsim_pool_free",
    "dlsim_pool_stats",
    "dlsim_sharded_plan_create",
    "dlsim_sharded_plan_run",
    "dlsim_sharded_plan_run_f64",
    "dlsim_sharded_plan_destroy",
    "dlsim_host_wreduce",
    "dlsim_host_wreduce_zc",
    "dlsim_host_wreduce_resident",
    "dlsim_host_chunk_mean",
    "dlsim_host_pack",
    "dlsim_shard_range",
    "dlsim_probe_pattern",
    "dlsim_kernel_name",
    "dlsim_last_error",
    "dlsim_version",
)

_lib = None
_lock = threading.Lock()


class ChunkLaunch(ctypes.Structure):
    """dlsim_chunk_launch (include/dlsim.h): one launch of a chunk-mean call."""
    _fields_ = [("form", ctypes.c_int), ("mf", ctypes.c_int), ("rows", ctypes.c_int), ("bpt", ctypes.c_int),
                ("grid", ctypes.c_uint), ("ntasks", ctypes.c_int), ("first_task", ctypes.c_int)]


CHUNK_FORMS = ("tiled_few", "tiled", "table", "defer_rf4", "defer_rf8", "defer_m")  # DLSIM_CHUNK_*


class DlsimError(RuntimeError):
    """A dlsim_* call returned a negative code."""

    def __init__(self, fn: str, rc: int, msg: str):
        super().__init__(f"{fn} failed (rc={rc}): {msg}")
        self.rc = rc


def load() -> ctypes.CDLL:
    """Load libdlsim_hip.so (built by __graft_entry__.build()); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"HIP extension not built: {LIB_PATH} is missing. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` at the repo root.")
        lib = ctypes.CDLL(LIB_PATH)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.dlsim_wreduce.argtypes = [ctypes.POINTER(vp), i, ctypes.POINTER(ctypes.c_float), vp,
                                      sz, i, i, vp]
        lib.dlsim_wreduce.restype = i
        lib.dlsim_wreduce_f64.argtypes = [ctypes.POINTER(vp), i, ctypes.POINTER(ctypes.c_double), vp, sz, i, vp]
        lib.dlsim_wreduce_f64.restype = i
        lib.dlsim_wreduce_tensors.argtypes = [ctypes.POINTER(vp), i, i, ctypes.POINTER(sz),
                                              ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp),
                                              i, i, vp]
        lib.dlsim_wreduce_tensors.restype = i
        lib.dlsim_wreduce_batched.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp),
                                              ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp),
                                              ctypes.POINTER(sz), i, i, vp]
        lib.dlsim_wreduce_batched.restype = i
        lib.dlsim_batch_table_bytes.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(sz), i,
                                                ctypes.POINTER(sz)]
        lib.dlsim_batch_table_bytes.restype = i
        lib.dlsim_batch_table_fill.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp),
                                               ctypes.POINTER(ctypes.c_float), ctypes.POINTER(vp),
                                               ctypes.POINTER(sz), i, vp, sz]
        lib.dlsim_batch_table_fill.restype = i
        lib.dlsim_batch_table_launch.argtypes = [vp, vp, i, i, vp]
        lib.dlsim_batch_table_launch.restype = i
        lib.dlsim_mean.argtypes = [ctypes.POINTER(vp), i, vp, sz, i, vp]
        lib.dlsim_mean.restype = i
        lib.dlsim_mean_batched.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                           ctypes.POINTER(sz), i, vp]
        lib.dlsim_mean_batched.restype = i
        lib.dlsim_chunk_mean_batched.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                 ctypes.POINTER(sz), i, i, vp]
        lib.dlsim_chunk_mean_batched.restype = i
        lib.dlsim_chunk_mean_ilp_begin.argtypes = [i, sz, i]
        lib.dlsim_chunk_mean_ilp_begin.restype = sz
        lib.dlsim_chunk_mean_plan.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                              ctypes.POINTER(sz), i, i, i, ctypes.POINTER(ChunkLaunch), i,
                                              ctypes.POINTER(i)]
        lib.dlsim_chunk_mean_plan.restype = i
        lib.dlsim_rccl_bind.argtypes = [ctypes.c_char_p]
        lib.dlsim_rccl_bind.restype = i
        lib.dlsim_wreduce_sharded.argtypes = [ctypes.POINTER(vp), sz, i, ctypes.POINTER(ctypes.c_float), vp, sz, i,
                                              i, vp, i, vp]
        lib.dlsim_wreduce_sharded.restype = i
        lib.dlsim_wreduce_sharded_f64.argtypes = [ctypes.POINTER(vp), sz, i, ctypes.POINTER(ctypes.c_double), vp,
                                                  sz, i, vp, i, vp]
        lib.dlsim_wreduce_sharded_f64.restype = i
        lib.dlsim_sharded_plan_create.argtypes = [vp, sz, i, i, i, vp, ctypes.POINTER(vp)]
        lib.dlsim_sharded_plan_create.restype = i
        lib.dlsim_sharded_plan_run.argtypes = [vp, ctypes.POINTER(vp), sz, ctypes.POINTER(ctypes.c_float), vp, i, vp]
        lib.dlsim_sharded_plan_run.restype = i
        lib.dlsim_sharded_plan_run_f64.argtypes = [vp, ctypes.POINTER(vp), sz, ctypes.POINTER(ctypes.c_double), vp,
                                                   i, vp]
        lib.dlsim_sharded_plan_run_f64.restype = i
        lib.dlsim_sharded_plan_destroy.argtypes = [vp]
        lib.dlsim_sharded_plan_destroy.restype = i
        lib.dlsim_host_wreduce.argtypes = [i, i, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                           ctypes.POINTER(ctypes.c_float), vp, vp, sz, vp, vp, i, i, sz, i,
                                           vp, vp, vp]
        lib.dlsim_host_wreduce.restype = i
        lib.dlsim_host_wreduce_zc.argtypes = [i, i, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                              ctypes.POINTER(ctypes.c_float), vp, sz, vp, i, i, i, vp]
        lib.dlsim_host_wreduce_zc.restype = i
        lib.dlsim_host_wreduce_resident.argtypes = [i, i, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                                    ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i),
                                                    ctypes.POINTER(vp), vp, sz, vp, vp, i, i, i, vp]
        lib.dlsim_host_wreduce_resident.restype = i
        lib.dlsim_host_chunk_mean.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(sz), vp, vp,
                                              sz, ctypes.POINTER(vp), ctypes.POINTER(vp), i, i, i, vp, vp, vp]
        lib.dlsim_host_chunk_mean.restype = i
        lib.dlsim_host_pack.argtypes = [i, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz), vp, i]
        lib.dlsim_host_pack.restype = i
        lib.dlsim_shard_range.argtypes = [sz, i, i, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        lib.dlsim_shard_range.restype = i
        lib.dlsim_probe_pattern.argtypes = [ctypes.POINTER(vp), i, vp, sz, i, vp]
        lib.dlsim_probe_pattern.restype = i
        lib.dlsim_wreduce_mixed.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i), i, ctypes.POINTER(ctypes.c_double),
                                            vp, i, sz, vp]
        lib.dlsim_wreduce_mixed.restype = i
        lib.dlsim_sgd_step.argtypes = [vp, vp, vp, sz, ctypes.c_double, ctypes.c_double, i, vp]
        lib.dlsim_sgd_step.restype = i
        lib.dlsim_sgd_step_tensors.argtypes = [i, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                               ctypes.POINTER(sz), ctypes.c_double, ctypes.c_double, i, vp]
        lib.dlsim_sgd_step_tensors.restype = i
        dbl = ctypes.c_double
        lib.dlsim_sgd_momentum_step.argtypes = [vp, vp, vp, vp, vp, sz, dbl, dbl, dbl, i, vp]
        lib.dlsim_sgd_momentum_step.restype = i
        lib.dlsim_sgd_momentum_step_tensors.argtypes = [i] + [ctypes.POINTER(vp)] * 5 + [ctypes.POINTER(sz), dbl, dbl,
                                                                                        dbl, i, vp]
        lib.dlsim_sgd_momentum_step_tensors.restype = i
        lib.dlsim_robust_reduce.argtypes = [ctypes.POINTER(vp), i, i, i, vp, sz, i, vp]
        lib.dlsim_robust_reduce.restype = i
        lib.dlsim_robust_reduce_tensors.argtypes = [ctypes.POINTER(vp), i, i, ctypes.POINTER(sz), ctypes.POINTER(sz),
                                                    i, i, vp, i, vp]
        lib.dlsim_robust_reduce_tensors.restype = i
        lib.dlsim_robust_reduce_batched.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(i),
                                                    ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(sz), i, vp]
        lib.dlsim_robust_reduce_batched.restype = i
        lib.dlsim_robust_batch_geometry.argtypes = [i, i, ctypes.POINTER(sz), ctypes.POINTER(i), ctypes.POINTER(i)]
        lib.dlsim_robust_batch_geometry.restype = i
        lib.dlsim_robust_reduce_tensors_batched.argtypes = lib.dlsim_robust_reduce_tensors.argtypes
        lib.dlsim_robust_reduce_tensors_batched.restype = i
        lib.dlsim_robust_nearest_reduce.argtypes = [ctypes.POINTER(vp), i, i, vp, sz, i, vp]
        lib.dlsim_robust_nearest_reduce.restype = i
        lib.dlsim_robust_nearest_reduce_tensors.argtypes = [ctypes.POINTER(vp), i, i, ctypes.POINTER(sz),
                                                            ctypes.POINTER(sz), i, vp, i, vp]
        lib.dlsim_robust_nearest_reduce_tensors.restype = i
        lib.dlsim_pairwise_sqdist.argtypes = [ctypes.POINTER(vp), i, sz, i, vp, i, vp]
        lib.dlsim_pairwise_sqdist.restype = i
        lib.dlsim_pairwise_sqdist_tensors.argtypes = [ctypes.POINTER(vp), i, i, ctypes.POINTER(sz), i, vp, i, vp]
        lib.dlsim_pairwise_sqdist_tensors.restype = i
        lib.dlsim_pairdist_geometry.argtypes = [i, i, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint)]
        lib.dlsim_pairdist_geometry.restype = i
        lib.dlsim_pairwise_sqdist_batched.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(vp),
                                                      ctypes.POINTER(sz), i, ctypes.POINTER(vp), i, vp]
        lib.dlsim_pairwise_sqdist_batched.restype = i
        lib.dlsim_pairdist_batch_geometry.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
        lib.dlsim_pairdist_batch_geometry.restype = i
        dp = ctypes.POINTER(ctypes.c_double)
        lib.dlsim_wreduce_dist.argtypes = [ctypes.POINTER(vp), i, dp, vp, sz, i, vp, i, vp]
        lib.dlsim_wreduce_dist.restype = i
        lib.dlsim_wreduce_dist_tensors.argtypes = [ctypes.POINTER(vp), i, i, ctypes.POINTER(sz), ctypes.POINTER(sz),
                                                   dp, vp, i, vp, i, vp]
        lib.dlsim_wreduce_dist_tensors.restype = i
        lib.dlsim_reducedist_geometry.argtypes = [i, i, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint)]
        lib.dlsim_reducedist_geometry.restype = i
        lib.dlsim_wreduce_dist_batched.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(vp),
                                                   ctypes.POINTER(sz), ctypes.POINTER(sz), dp, ctypes.POINTER(vp), i,
                                                   ctypes.POINTER(vp), i, vp]
        lib.dlsim_wreduce_dist_batched.restype = i
        lib.dlsim_reducedist_batch_geometry.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
        lib.dlsim_reducedist_batch_geometry.restype = i
        lib.dlsim_device_alloc.argtypes = [sz, i, ctypes.POINTER(vp), ctypes.POINTER(i)]
        lib.dlsim_device_alloc.restype = i
        lib.dlsim_device_free.argtypes = [vp]
        lib.dlsim_device_free.restype = i
        u64p = ctypes.POINTER(ctypes.c_ulonglong)
        lib.dlsim_pool_stats.argtypes = [u64p, u64p, u64p]
        lib.dlsim_pool_stats.restype = None
        lib.dlsim_kernel_name.argtypes = [i, sz, i, i]
        lib.dlsim_kernel_name.restype = ctypes.c_char_p
        lib.dlsim_last_error.argtypes = []
        lib.dlsim_last_error.restype = ctypes.c_char_p
        lib.dlsim_version.argtypes = []
        lib.dlsim_version.restype = i
        _lib = lib
        return lib


def kernel_name(n: int, numel: int, torch_dtype, mode: Optional[int] = DLSIM_EXACT) -> str:
    """Name of the kernel dlsim_wreduce (mode DLSIM_EXACT / DLSIM_FAST) or
    dlsim_mean (mode None) launches for n aligned inputs of numel elements
    (dlsim_kernel_name), e.g. "dlsim::k_wreduce_defer"."""
    return load().dlsim_kernel_name(n, numel, dtype_code(torch_dtype), -1 if mode is None else mode).decode()


def _check(fn: str, rc: int) -> None:
    if rc != 0:
        msg = load().dlsim_last_error().decode(errors="replace")
        raise DlsimError(fn, rc, msg)


def version() -> int:
    return load().dlsim_version()


def shard_range(n_elems: int, world: int, rank: int, align_elems: int = 64):
    lib = load()
    b, e = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check("dlsim_shard_range",
           lib.dlsim_shard_range(n_elems, world, rank, align_elems, ctypes.byref(b), ctypes.byref(e)))
    return b.value, e.value


def fp32_weights(weights: Sequence[float]) -> np.ndarray:
    """Python floats -> fp32 with round-to-nearest-even, as the reference's
    `w * p1` converts a Python-float scalar (fedavg.py:25)."""
    return np.asarray([float(w) for w in weights], dtype=np.float64).astype(np.float32)


def f64_weights(weights: Sequence[float]) -> np.ndarray:
    """Python floats as doubles: for a double tensor the reference's `w * p1`
    keeps the weight exact (fedavg.py:25)."""
    return np.asarray([float(w) for w in weights], dtype=np.float64)


def weights_for_dtype(weights: Sequence[float], torch_dtype) -> np.ndarray:
    """The weights as the reference's op sees them for this parameter dtype:
    fp32-rounded for fp32/bf16/fp16 tensors, exact doubles for fp64."""
    import torch
    return f64_weights(weights) if torch_dtype == torch.float64 else fp32_weights(weights)


def dtype_code(torch_dtype, single_task: bool = False) -> int:
    """ABI dtype of a parameter dtype. fp64 (single_task=True) has the
    single-task reduce (dlsim_wreduce_f64) and the chunk means; the batched,
    tensor-list, mean and host-reduce entries take fp32/bf16/fp16 only."""
    import torch
    if torch_dtype == torch.float32:
        return DLSIM_F32
    if torch_dtype == torch.bfloat16:
        return DLSIM_BF16
    if torch_dtype == torch.float16:
        return DLSIM_F16
    if torch_dtype == torch.float64:
        if single_task:
            return DLSIM_F64
        raise TypeError("float64 parameters are reduced one task at a time (dlsim_wreduce_f64); "
                        "this entry point takes float32, bfloat16 and float16")
    raise TypeError(f"aggregation supports float32, bfloat16, float16 and float64 parameters, got {torch_dtype}")


def _stream_handle(device, stream) -> Optional[int]:
    """The hipStream_t of `stream`, or of `device`'s current stream (read raw:
    no torch.cuda.Stream object is built, this runs once per launch)."""
    import torch
    if stream is not None:
        return stream.cuda_stream
    if device is None:
        return torch.cuda.current_stream().cuda_stream
    idx = device.index if isinstance(device, torch.device) else int(device)
    if idx is None:
        idx = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


class ReducePlan:
    """One prepared `dlsim_wreduce` call: pointer and weight arrays built once,
    `launch()` is a single ctypes call (used by hot loops and bench.py)."""

    def __init__(self, inputs, weights_f32: np.ndarray, out, mode: int = DLSIM_EXACT, probe: bool = False):
        import torch
        n = len(inputs)
        if n < 1:
            raise IndexError("list index out of range")
        if len(weights_f32) != n:
            raise AssertionError("weights/models length mismatch")
        dt = dtype_code(out.dtype, single_task=not probe)
        numel = out.numel()
        for t in list(inputs) + [out]:
            if not t.is_cuda:
                raise ValueError("ReducePlan needs device tensors (no CPU path)")
            if t.dtype != out.dtype or t.numel() != numel or not t.is_contiguous():
                raise ValueError("inputs and output must be contiguous, same dtype and size")
            if t.device != out.device:
                raise ValueError("inputs and output must live on one device")
        self.device = out.device
        self.n, self.numel, self.dtype, self.mode = n, numel, dt, mode
        self._keep = (list(inputs), out)  # keep storages alive while planned
        self._ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs])
        if dt == DLSIM_F64:
            # exact double weights (weights_for_dtype); fp32 arrays widen exactly
            self._w = np.ascontiguousarray(weights_f32, dtype=np.float64)
            self._wp = self._w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        else:
            self._w = np.ascontiguousarray(weights_f32, dtype=np.float32)
            self._wp = self._w.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        self._out = ctypes.c_void_p(out.data_ptr())
        self._lib = load()
        self.probe = probe
        torch.cuda.current_device()  # a GPU must be present

    def launch(self, stream=None) -> None:
        if self.probe:
            _check("dlsim_probe_pattern",
                   self._lib.dlsim_probe_pattern(self._ptrs, self.n, self._out, self.numel, self.dtype,
                                                 _stream_handle(self.device, stream)))
            return
        if self.dtype == DLSIM_F64:
            _check("dlsim_wreduce_f64",
                   self._lib.dlsim_wreduce_f64(self._ptrs, self.n, self._wp, self._out, self.numel, self.mode,
                                               _stream_handle(self.device, stream)))
            return
        rc = self._lib.dlsim_wreduce(self._ptrs, self.n, self._wp, self._out, self.numel,
                                     self.dtype, self.mode, _stream_handle(self.device, stream))
        _check("dlsim_wreduce", rc)


def wreduce_mixed(inputs, weights, out, stream=None):
    """dlsim_wreduce_mixed: out = the reference's fold of inputs of different
    dtypes (flat device tensors; inputs[0] has out's dtype), with the
    Python-float weights as doubles. Exact only."""
    n = len(inputs)
    if n < 1:
        raise IndexError("list index out of range")
    if len(weights) != n:
        raise AssertionError("weights/models length mismatch")
    numel = out.numel()
    for t in list(inputs) + [out]:
        if not t.is_cuda or t.device != out.device:
            raise ValueError("wreduce_mixed needs device tensors on one device (no CPU path)")
        if t.numel() != numel or not t.is_contiguous():
            raise ValueError("inputs and output must be contiguous and of one size")
    codes = (ctypes.c_int * n)(*[dtype_code(t.dtype, single_task=True) for t in inputs])
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs])
    w = (ctypes.c_double * n)(*[float(x) for x in weights])
    _check("dlsim_wreduce_mixed",
           load().dlsim_wreduce_mixed(ptrs, codes, n, w, out.data_ptr(), dtype_code(out.dtype, single_task=True),
                                      numel, _stream_handle(out.device, stream)))
    return out


def sgd_kernel_dtype(torch_dtype) -> bool:
    """Whether dlsim_sgd_step has a kernel for this dtype (fp32, bf16, fp64;
    fp16 runs torch's own CPU ops, dasklearn_amd/sgd.py)."""
    import torch
    return torch_dtype in (torch.float32, torch.bfloat16, torch.float64)


def _check_sgd_triple(p, g, out) -> None:
    for t in (p, g, out):
        if not t.is_cuda or t.device != out.device:
            raise ValueError("the SGD step needs device tensors on one device (no CPU path)")
        if t.dtype != out.dtype or t.numel() != out.numel() or not t.is_contiguous():
            raise ValueError("parameter, gradient and output must be contiguous, same dtype and size")


def sgd_step(param, grad, out, lr: float, weight_decay: float, stream=None):
    """dlsim_sgd_step: out = the first step of a fresh torch.optim.SGD(lr,
    weight_decay) on `param` with gradient `grad` (flat device tensors; `out`
    may be `param` or `grad`), stream-ordered."""
    _check_sgd_triple(param, grad, out)
    _check("dlsim_sgd_step",
           load().dlsim_sgd_step(param.data_ptr(), grad.data_ptr(), out.data_ptr(), out.numel(), float(lr),
                                 float(weight_decay), dtype_code(out.dtype, single_task=True),
                                 _stream_handle(out.device, stream)))
    return out


def sgd_step_tensors_raw(param_ptrs: Sequence[int], grad_ptrs: Sequence[int], out_ptrs: Sequence[int],
                         numels: Sequence[int], lr: float, weight_decay: float, dtype: int, stream_handle) -> None:
    """dlsim_sgd_step_tensors on raw device pointers (the caller checked them)."""
    t = len(numels)
    arr = ctypes.c_void_p * max(t, 1)
    _check("dlsim_sgd_step_tensors",
           load().dlsim_sgd_step_tensors(t, arr(*param_ptrs), arr(*grad_ptrs), arr(*out_ptrs),
                                         (ctypes.c_size_t * max(t, 1))(*numels), float(lr), float(weight_decay),
                                         dtype, stream_handle))


def sgd_step_tensors(params, grads, outs, lr: float, weight_decay: float, stream=None):
    """dlsim_sgd_step_tensors: the same step over separate (param, grad, out)
    device tensors of one dtype, in a few launches."""
    if not (len(params) == len(grads) == len(outs)):
        raise ValueError("params, grads and outs must have one length")
    if not outs:
        return outs
    for p, g, o in zip(params, grads, outs):
        _check_sgd_triple(p, g, o)
        if o.dtype != outs[0].dtype or o.device != outs[0].device:
            raise ValueError("one call takes tensors of one dtype on one device")
    sgd_step_tensors_raw([p.data_ptr() for p in params], [g.data_ptr() for g in grads],
                         [o.data_ptr() for o in outs], [o.numel() for o in outs], lr, weight_decay,
                         dtype_code(outs[0].dtype, single_task=True), _stream_handle(outs[0].device, stream))
    return outs


def sgd_momentum_step(param, grad, buf, param_out, buf_out, lr: float, momentum: float, weight_decay: float,
                      stream=None):
    """dlsim_sgd_momentum_step: one step of torch.optim.SGD(lr, momentum > 0,
    weight_decay) on flat device tensors. `buf` None: the first step
    (buf_out = the gradient after weight decay). `param_out` may be `param`
    and `buf_out` may be `buf`; `grad` is only read. Stream-ordered."""
    for t in (param, grad, param_out, buf_out) + (() if buf is None else (buf,)):
        if not t.is_cuda or t.device != param_out.device:
            raise ValueError("the SGD step needs device tensors on one device (no CPU path)")
        if t.dtype != param_out.dtype or t.numel() != param_out.numel() or not t.is_contiguous():
            raise ValueError("parameter, gradient, buffer and outputs must be contiguous, same dtype and size")
    _check("dlsim_sgd_momentum_step",
           load().dlsim_sgd_momentum_step(param.data_ptr(), grad.data_ptr(), None if buf is None else buf.data_ptr(),
                                          param_out.data_ptr(), buf_out.data_ptr(), param_out.numel(), float(lr),
                                          float(momentum), float(weight_decay),
                                          dtype_code(param_out.dtype, single_task=True),
                                          _stream_handle(param_out.device, stream)))
    return param_out, buf_out


def sgd_momentum_step_tensors_raw(param_ptrs: Sequence[int], grad_ptrs: Sequence[int],
                                  buf_ptrs: Sequence[Optional[int]], param_out_ptrs: Sequence[int],
                                  buf_out_ptrs: Sequence[int], numels: Sequence[int], lr: float, momentum: float,
                                  weight_decay: float, dtype: int, stream_handle) -> None:
    """dlsim_sgd_momentum_step_tensors on raw device pointers (the caller
    checked them); a None (or 0) in buf_ptrs is that tensor's first step."""
    t = len(numels)
    arr = ctypes.c_void_p * max(t, 1)
    _check("dlsim_sgd_momentum_step_tensors",
           load().dlsim_sgd_momentum_step_tensors(t, arr(*param_ptrs), arr(*grad_ptrs), arr(*buf_ptrs),
                                                  arr(*param_out_ptrs), arr(*buf_out_ptrs),
                                                  (ctypes.c_size_t * max(t, 1))(*numels), float(lr), float(momentum),
                                                  float(weight_decay), dtype, stream_handle))


SGD_MOMENTUM_TENSORS_PER_LAUNCH = 64  # csrc/sgdm_kernels.hpp kSgdmMaxTensors


# ---- the entries over n <= 32 inputs: order statistics, pairwise distances, reduce-and-measure ----
MAX_ROBUST_INPUTS = 32  # include/dlsim.h DLSIM_MAX_ROBUST_INPUTS
MAX_PAIRDIST_INPUTS = 32  # include/dlsim.h DLSIM_MAX_PAIRDIST_INPUTS
MAX_REDUCEDIST_INPUTS = 32  # include/dlsim.h DLSIM_MAX_REDUCEDIST_INPUTS


def _check_fan_in(n: int, limit: int, message: str) -> None:
    """ValueError(message with its {limit} and {n} filled in) past the limit."""
    if n > limit:
        raise ValueError(message.format(limit=limit, n=n))


def check_robust_fan_in(n: int) -> None:
    _check_fan_in(n, MAX_ROBUST_INPUTS, "the median and trimmed-mean kernels take at most {limit} models (got {n}): "
                                        "the sorting network is held in registers")


def check_pairdist_fan_in(n: int) -> None:
    _check_fan_in(n, MAX_PAIRDIST_INPUTS, "the pairwise-distance kernels take at most {limit} models (got {n})")


def check_reducedist_fan_in(n: int) -> None:
    _check_fan_in(n, MAX_REDUCEDIST_INPUTS, "the reduce-and-measure kernels take at most {limit} models (got {n})")


def _check_flat_inputs(inputs, out, device, what: str):
    """(dtype, numel) of the n >= 1 contiguous device tensors of one dtype and
    size on `device`, `out` (unless None) being one more of them."""
    dt, numel = inputs[0].dtype, inputs[0].numel()
    for t in list(inputs) + ([] if out is None else [out]):
        if not t.is_cuda or t.device != device:
            raise ValueError(f"the {what} needs device tensors on one device (no CPU path)")
        if t.dtype != dt or t.numel() != numel or not t.is_contiguous():
            raise ValueError("inputs and output must be contiguous, same dtype and size")
    return dt, numel


def _check_distances(d2, count: int, what: str) -> None:
    import torch
    if not d2.is_cuda or d2.dtype != torch.float64 or d2.numel() != count or not d2.is_contiguous():
        raise ValueError(f"the distance {what} must be a contiguous float64 device tensor of {count} elements")


def _ptr_array(ptrs):
    """A ctypes array of the pointers (None: null), never of length 0."""
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _size_array(sizes):
    return (ctypes.c_size_t * max(len(sizes), 1))(*sizes)


def _double_array(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def _geometry(symbol: str, n: int, torch_dtype, numel: int):
    tile, blocks = ctypes.c_size_t(0), ctypes.c_uint(0)
    _check(symbol, getattr(load(), symbol)(n, dtype_code(torch_dtype, single_task=True), numel, ctypes.byref(tile),
                                           ctypes.byref(blocks)))
    return tile.value, blocks.value


def robust_reduce(inputs, lo: int, hi: int, out, stream=None):
    """dlsim_robust_reduce: per element, the n inputs' values sorted ascending
    (-0.0 < +0.0, NaN last), out = (s[lo] + ... + s[hi-1]) / (hi - lo). Flat
    device tensors of one dtype (fp32, fp64, bf16, fp16) and size; `out` may
    not share memory with an input. Stream-ordered."""
    n = len(inputs)
    if n < 1:
        raise IndexError("list index out of range")
    check_robust_fan_in(n)
    dt, numel = _check_flat_inputs(inputs, out, out.device, "robust reduce")
    _check("dlsim_robust_reduce",
           load().dlsim_robust_reduce(_ptr_array([t.data_ptr() for t in inputs]), n, int(lo), int(hi), out.data_ptr(),
                                      numel, dtype_code(dt, single_task=True), _stream_handle(out.device, stream)))
    return out


def robust_reduce_tensors_raw(in_ptrs: Sequence[int], n: int, numels: Sequence[int], out_offsets: Sequence[int],
                              lo: int, hi: int, out_base: int, dtype: int, stream_handle) -> None:
    """dlsim_robust_reduce_tensors on pointers the caller has already validated
    (the arena path: every tensor checked against models[0]'s layout, on the
    output's device, contiguous). in_ptrs model-major (tensor k of model i at
    i * t + k); output tensor k at out_base + out_offsets[k] bytes."""
    check_robust_fan_in(n)
    _check("dlsim_robust_reduce_tensors",
           load().dlsim_robust_reduce_tensors(_ptr_array(in_ptrs), n, len(numels), _size_array(numels),
                                              _size_array(out_offsets), int(lo), int(hi), out_base, dtype,
                                              stream_handle))


def robust_reduce_tensors_batched_raw(in_ptrs: Sequence[int], n: int, numels: Sequence[int],
                                      out_offsets: Sequence[int], lo: int, hi: int, out_base: int, dtype: int,
                                      stream_handle) -> None:
    """dlsim_robust_reduce_tensors_batched, as robust_reduce_tensors_raw: every
    non-empty tensor a task of one batched dispatch."""
    check_robust_fan_in(n)
    _check("dlsim_robust_reduce_tensors_batched",
           load().dlsim_robust_reduce_tensors_batched(_ptr_array(in_ptrs), n, len(numels), _size_array(numels),
                                                      _size_array(out_offsets), int(lo), int(hi), out_base, dtype,
                                                      stream_handle))


def robust_nearest_reduce(inputs, keep: int, out, stream=None):
    """dlsim_robust_nearest_reduce: per element, the mean of the `keep` sorted
    values closest to the lower median of the n inputs' values (ties to the
    smaller side; include/dlsim.h has the rule), summed in ascending order.
    Tensors, exceptions and stream order as robust_reduce."""
    n = len(inputs)
    if n < 1:
        raise IndexError("list index out of range")
    check_robust_fan_in(n)
    dt, numel = _check_flat_inputs(inputs, out, out.device, "robust nearest reduce")
    _check("dlsim_robust_nearest_reduce",
           load().dlsim_robust_nearest_reduce(_ptr_array([t.data_ptr() for t in inputs]), n, int(keep),
                                              out.data_ptr(), numel, dtype_code(dt, single_task=True),
                                              _stream_handle(out.device, stream)))
    return out


def robust_nearest_reduce_tensors_raw(in_ptrs: Sequence[int], n: int, numels: Sequence[int],
                                      out_offsets: Sequence[int], keep: int, out_base: int, dtype: int,
                                      stream_handle) -> None:
    """dlsim_robust_nearest_reduce_tensors, as robust_reduce_tensors_raw."""
    check_robust_fan_in(n)
    _check("dlsim_robust_nearest_reduce_tensors",
           load().dlsim_robust_nearest_reduce_tensors(_ptr_array(in_ptrs), n, len(numels), _size_array(numels),
                                                      _size_array(out_offsets), int(keep), out_base, dtype,
                                                      stream_handle))


def _int_array(values):
    return (ctypes.c_int * max(len(values), 1))(*[int(v) for v in values])


def robust_reduce_batched_raw(fan_in: Sequence[int], in_ptrs: Sequence[int], los: Sequence[int],
                              his: Sequence[int], out_ptrs: Sequence[int], numels: Sequence[int], dtype: int,
                              stream_handle) -> None:
    """dlsim_robust_reduce_batched on pointers the caller has already validated
    (task-major: task t's fan_in[t] pointers follow task t-1's)."""
    _check("dlsim_robust_reduce_batched",
           load().dlsim_robust_reduce_batched(len(fan_in), _int_array(fan_in), _ptr_array(in_ptrs), _int_array(los),
                                              _int_array(his), _ptr_array(out_ptrs), _size_array(numels), dtype,
                                              stream_handle))


def robust_reduce_batched(tasks, stream=None):
    """dlsim_robust_reduce_batched: tasks = [(inputs, lo, hi, out)], each as
    robust_reduce takes them (its exceptions too), all of one dtype on one
    device; every task in a few shared launches, bit-identical to one
    robust_reduce call each. No output may share memory with any input or
    output of any task. Stream-ordered. Returns the outputs."""
    if not tasks:
        return []
    dev, dt0 = tasks[0][3].device, tasks[0][3].dtype
    fan, ptrs, los, his, outs, numels = [], [], [], [], [], []
    for inputs, lo, hi, out in tasks:
        n = len(inputs)
        if n < 1:
            raise IndexError("list index out of range")
        check_robust_fan_in(n)
        dt, numel = _check_flat_inputs(inputs, out, dev, "robust reduce")
        if dt != dt0:
            raise ValueError("one batched call takes tasks of one dtype")
        fan.append(n)
        ptrs += [t.data_ptr() for t in inputs]
        los.append(lo)
        his.append(hi)
        outs.append(out.data_ptr())
        numels.append(numel)
    robust_reduce_batched_raw(fan, ptrs, los, his, outs, numels, dtype_code(dt0, single_task=True),
                              _stream_handle(dev, stream))
    return [t[3] for t in tasks]


def robust_batch_geometry(n: int, torch_dtype):
    """(tile_elems, max_tasks, max_ptrs) of dlsim_robust_batch_geometry: the
    elements of one full tile of an aligned task of fan-in n in the batched
    kernel, and the limits of one launch."""
    tile, mt, mp = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
    _check("dlsim_robust_batch_geometry",
           load().dlsim_robust_batch_geometry(int(n), dtype_code(torch_dtype, single_task=True), ctypes.byref(tile),
                                              ctypes.byref(mt), ctypes.byref(mp)))
    return tile.value, mt.value, mp.value


def pairwise_sqdist(inputs, out, accumulate: bool = False, stream=None):
    """dlsim_pairwise_sqdist: out[i][j] = sum_e (double(x_i[e]) - double(x_j[e]))^2
    over n flat device tensors of one dtype (fp32, fp64, bf16, fp16) and size;
    `out` is a contiguous float64 device tensor of n*n elements that shares no
    memory with an input (the inputs may alias each other). accumulate: add to
    what `out` holds (bitwise symmetric, diagonal +0.0, as a call without it
    leaves it). Deterministic (no atomics). Stream-ordered."""
    n = len(inputs)
    if n < 1:
        raise IndexError("list index out of range")
    check_pairdist_fan_in(n)
    _check_distances(out, n * n, "matrix")
    dt, numel = _check_flat_inputs(inputs, None, out.device, "pairwise distance")
    _check("dlsim_pairwise_sqdist",
           load().dlsim_pairwise_sqdist(_ptr_array([t.data_ptr() for t in inputs]), n, numel,
                                        dtype_code(dt, single_task=True), out.data_ptr(), int(bool(accumulate)),
                                        _stream_handle(out.device, stream)))
    return out


def pairwise_sqdist_tensors_raw(in_ptrs: Sequence[int], n: int, numels: Sequence[int], dtype: int, out_ptr: int,
                                accumulate: bool, stream_handle) -> None:
    """dlsim_pairwise_sqdist_tensors, as robust_reduce_tensors_raw; the n*n doubles at out_ptr."""
    check_pairdist_fan_in(n)
    _check("dlsim_pairwise_sqdist_tensors",
           load().dlsim_pairwise_sqdist_tensors(_ptr_array(in_ptrs), n, len(numels), _size_array(numels), dtype,
                                                out_ptr, int(bool(accumulate)), stream_handle))


def pairdist_geometry(n: int, torch_dtype, numel: int):
    """(tile elements, blocks) of dlsim_pairwise_sqdist for n 16-byte-aligned
    inputs of numel elements (dlsim_pairdist_geometry; no GPU needed)."""
    return _geometry("dlsim_pairdist_geometry", n, torch_dtype, numel)


def pairwise_sqdist_batched_raw(fan_in: Sequence[int], n_tensors: Sequence[int], in_ptrs: Sequence[int],
                                numels: Sequence[int], dtype: int, out_ptrs: Sequence[int], accumulate: bool,
                                stream_handle) -> None:
    """dlsim_pairwise_sqdist_batched on pointers the caller has already
    validated: task k's fan_in[k] * n_tensors[k] pointers (model-major) and
    n_tensors[k] lengths follow task k-1's; fan_in[k]^2 doubles at out_ptrs[k]."""
    _check("dlsim_pairwise_sqdist_batched",
           load().dlsim_pairwise_sqdist_batched(len(fan_in), _int_array(fan_in), _int_array(n_tensors),
                                                _ptr_array(in_ptrs), _size_array(numels), dtype,
                                                _ptr_array(out_ptrs), int(bool(accumulate)), stream_handle))


def pairwise_sqdist_batched(tasks, accumulate: bool = False, stream=None):
    """dlsim_pairwise_sqdist_batched: tasks = [(inputs, out)], each as
    pairwise_sqdist takes them (its exceptions too), all of one dtype on one
    device; every matrix in a few shared launches, bit-identical to one
    pairwise_sqdist call each. No matrix may share memory with an input of any
    task or with another matrix; inputs may be shared. Stream-ordered. Returns
    the matrices."""
    if not tasks:
        return []
    dev, dt0 = tasks[0][1].device, None
    fan, ptrs, numels, outs = [], [], [], []
    for inputs, out in tasks:
        n = len(inputs)
        if n < 1:
            raise IndexError("list index out of range")
        check_pairdist_fan_in(n)
        _check_distances(out, n * n, "matrix")
        dt, numel = _check_flat_inputs(inputs, None, dev, "pairwise distance")
        if out.device != dev:
            raise ValueError("the pairwise distance needs device tensors on one device (no CPU path)")
        if dt0 is not None and dt != dt0:
            raise ValueError("one batched call takes tasks of one dtype")
        dt0 = dt
        fan.append(n)
        ptrs += [t.data_ptr() for t in inputs]
        numels.append(numel)
        outs.append(out.data_ptr())
    pairwise_sqdist_batched_raw(fan, [1] * len(fan), ptrs, numels, dtype_code(dt0, single_task=True), outs,
                                accumulate, _stream_handle(dev, stream))
    return [t[1] for t in tasks]


def pairdist_batch_geometry(n: int, torch_dtype):
    """(max_segments, max_ptrs) of dlsim_pairdist_batch_geometry: the limits
    of one launch of the batched distance kernel (no GPU needed)."""
    ms, mp = ctypes.c_int(0), ctypes.c_int(0)
    _check("dlsim_pairdist_batch_geometry",
           load().dlsim_pairdist_batch_geometry(int(n), dtype_code(torch_dtype, single_task=True), ctypes.byref(ms),
                                                ctypes.byref(mp)))
    return ms.value, mp.value


def wreduce_dist(inputs, weights: Sequence[float], out, d2, accumulate: bool = False, stream=None):
    """dlsim_wreduce_dist: `out` = the exact weighted reduce of n flat device
    tensors of one dtype (fp32, fp64, bf16, fp16) and size, bit for bit what
    wreduce gives, and d2[i] = sum_e (double(x_i[e]) - double(out[e]))^2 from
    the same pass. `weights`: n Python floats (fp32-representable unless the
    tensors are fp64). `out` may be None (distances only); it and `d2` (a
    contiguous float64 device tensor of n elements) share no memory with an
    input or each other. accumulate: add to what `d2` holds. Deterministic (no
    atomics). Stream-ordered."""
    n = len(inputs)
    if n < 1:
        raise IndexError("list index out of range")
    check_reducedist_fan_in(n)
    assert len(weights) == n
    _check_distances(d2, n, "vector")
    dt, numel = _check_flat_inputs(inputs, out, d2.device, "reduce-and-measure")
    _check("dlsim_wreduce_dist",
           load().dlsim_wreduce_dist(_ptr_array([t.data_ptr() for t in inputs]), n, _double_array(weights),
                                     None if out is None else out.data_ptr(), numel,
                                     dtype_code(dt, single_task=True), d2.data_ptr(), int(bool(accumulate)),
                                     _stream_handle(d2.device, stream)))
    return out, d2


def wreduce_dist_tensors_raw(in_ptrs: Sequence[int], n: int, numels: Sequence[int], out_offsets: Sequence[int],
                             weights: Sequence[float], out_base: Optional[int], dtype: int, d2_ptr: int,
                             accumulate: bool, stream_handle) -> None:
    """dlsim_wreduce_dist_tensors, as robust_reduce_tensors_raw; the n doubles at d2_ptr."""
    check_reducedist_fan_in(n)
    _check("dlsim_wreduce_dist_tensors",
           load().dlsim_wreduce_dist_tensors(_ptr_array(in_ptrs), n, len(numels), _size_array(numels),
                                             _size_array(out_offsets), _double_array(weights), out_base, dtype,
                                             d2_ptr, int(bool(accumulate)), stream_handle))


def reducedist_geometry(n: int, torch_dtype, numel: int):
    """(tile elements, blocks) of dlsim_wreduce_dist for n 16-byte-aligned
    inputs of numel elements (dlsim_reducedist_geometry; no GPU needed)."""
    return _geometry("dlsim_reducedist_geometry", n, torch_dtype, numel)


def wreduce_dist_batched_raw(fan_in: Sequence[int], n_tensors: Sequence[int], in_ptrs: Sequence[int],
                             numels: Sequence[int], out_offsets: Sequence[int], weights: Sequence[float],
                             out_bases: Sequence[Optional[int]], dtype: int, d2_ptrs: Sequence[int],
                             accumulate: bool, stream_handle) -> None:
    """dlsim_wreduce_dist_batched on pointers the caller has already
    validated: task k's fan_in[k] * n_tensors[k] pointers (model-major),
    n_tensors[k] lengths and output offsets and fan_in[k] weights follow task
    k-1's; out_bases[k] may be None (distances only); fan_in[k] doubles at
    d2_ptrs[k]."""
    _check("dlsim_wreduce_dist_batched",
           load().dlsim_wreduce_dist_batched(len(fan_in), _int_array(fan_in), _int_array(n_tensors),
                                             _ptr_array(in_ptrs), _size_array(numels), _size_array(out_offsets),
                                             _double_array(weights), _ptr_array(out_bases), dtype,
                                             _ptr_array(d2_ptrs), int(bool(accumulate)), stream_handle))


def wreduce_dist_batched(tasks, accumulate: bool = False, stream=None):
    """dlsim_wreduce_dist_batched: tasks = [(inputs, weights, out, d2)], each
    as wreduce_dist takes them (its exceptions too), all of one dtype on one
    device; every output and vector in a few shared launches, bit-identical
    to one wreduce_dist call each. `out` may be None. No output or vector may
    share memory with an input of any task or with another output or vector;
    inputs may be shared. Stream-ordered. Returns [(out, d2)]."""
    if not tasks:
        return []
    dev, dt0 = tasks[0][3].device, None
    fan, ptrs, numels, ws, outs, d2s = [], [], [], [], [], []
    for inputs, weights, out, d2 in tasks:
        n = len(inputs)
        if n < 1:
            raise IndexError("list index out of range")
        check_reducedist_fan_in(n)
        assert len(weights) == n
        _check_distances(d2, n, "vector")
        dt, numel = _check_flat_inputs(inputs, out, dev, "reduce-and-measure")
        if d2.device != dev:
            raise ValueError("reduce-and-measure needs device tensors on one device (no CPU path)")
        if dt0 is not None and dt != dt0:
            raise ValueError("one batched call takes tasks of one dtype")
        dt0 = dt
        fan.append(n)
        ptrs += [t.data_ptr() for t in inputs]
        numels.append(numel)
        ws += [float(w) for w in weights]
        outs.append(None if out is None else out.data_ptr())
        d2s.append(d2.data_ptr())
    wreduce_dist_batched_raw(fan, [1] * len(fan), ptrs, numels, [0] * len(fan), ws, outs,
                             dtype_code(dt0, single_task=True), d2s, accumulate, _stream_handle(dev, stream))
    return [(t[2], t[3]) for t in tasks]


def reducedist_batch_geometry(n: int, torch_dtype):
    """(max_segments, max_ptrs) of dlsim_reducedist_batch_geometry: the limits
    of one launch of the batched reduce-and-measure kernel (no GPU needed)."""
    ms, mp = ctypes.c_int(0), ctypes.c_int(0)
    _check("dlsim_reducedist_batch_geometry",
           load().dlsim_reducedist_batch_geometry(int(n), dtype_code(torch_dtype, single_task=True), ctypes.byref(ms),
                                                  ctypes.byref(mp)))
    return ms.value, mp.value


DLSIM_ALLOC_CONTIGUOUS = 1


def pool_stats() -> dict:
    """dlsim_pool_stats: segments torch's allocator made through
    dlsim_pool_alloc (contiguous / hipMalloc fallback) and the bytes they hold."""
    lib = load()
    c, f, b = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    lib.dlsim_pool_stats(ctypes.byref(c), ctypes.byref(f), ctypes.byref(b))
    return {"contiguous": c.value, "fallback": f.value, "live_bytes": b.value}


class DeviceBlock:
    """One dlsim_device_alloc block on `device`, seen by torch through
    `__cuda_array_interface__` (torch.as_tensor wraps it without a copy and
    keeps this object alive while any view of it exists; the last view's
    release frees the block with dlsim_device_free, which synchronises the
    device — so only long-lived buffers come from here).
    contiguous: the driver gave physically contiguous memory."""

    def __init__(self, nbytes: int, device, contiguous: bool = True):
        import torch
        dev = torch.device(device)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        lib = load()
        p, got = ctypes.c_void_p(), ctypes.c_int(0)
        with torch.cuda.device(idx):
            _check("dlsim_device_alloc",
                   lib.dlsim_device_alloc(int(nbytes), DLSIM_ALLOC_CONTIGUOUS if contiguous else 0,
                                          ctypes.byref(p), ctypes.byref(got)))
        self.ptr, self.nbytes, self.device_index = p.value, int(nbytes), idx
        self.contiguous = bool(got.value)
        self.pid = os.getpid()  # a forked child never frees its parent's block
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False),
                                         "version": 2, "strides": None}

    def tensor(self):
        """A uint8 torch tensor over the whole block (no copy)."""
        import torch
        with torch.cuda.device(self.device_index):
            t = torch.as_tensor(self, device=torch.device("cuda", self.device_index))
        if t.data_ptr() != self.ptr:
            raise RuntimeError("torch copied the device block instead of wrapping it")
        return t

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr and _lib is not None and self.pid == os.getpid():
            try:
                import torch
                with torch.cuda.device(self.device_index):
                    _lib.dlsim_device_free(ptr)
            except Exception:  # interpreter shutdown: the process exit frees it
                pass


def wreduce(inputs, weights_f32, out, mode: int = DLSIM_EXACT, stream=None):
    """out = sum_i w_i * inputs[i] on the device (flat tensors), stream-ordered.
    fp64 tensors take double weights (weights_for_dtype)."""
    ReducePlan(inputs, weights_f32, out, mode).launch(stream)
    return out


class BatchPlan:
    """A prepared batch (one simulated round's aggregate tasks): the descriptor
    table is built once on the host, uploaded once to a device buffer, and
    every `launch()` is one kernel over all tasks (dlsim_batch_table_*)."""

    def __init__(self, tasks, mode: int = DLSIM_EXACT):
        import torch
        self.b = len(tasks)
        out0 = tasks[0][2]
        self.device, self.mode, self.dtype = out0.device, mode, dtype_code(out0.dtype)
        fan, ptrs, ws, outs, numels = [], [], [], [], []
        for inputs, w32, out in tasks:
            if len(w32) != len(inputs):
                raise AssertionError("weights/models length mismatch")
            for t in list(inputs) + [out]:
                if not t.is_cuda or t.dtype != out0.dtype or t.numel() != out.numel() \
                        or not t.is_contiguous() or t.device != self.device:
                    raise ValueError("each task: contiguous device tensors of one dtype, size and device")
            fan.append(len(inputs))
            ptrs.extend(t.data_ptr() for t in inputs)
            ws.extend(np.asarray(w32, dtype=np.float32).tolist())
            outs.append(out.data_ptr())
            numels.append(out.numel())
        lib = load()
        c_fan = (ctypes.c_int * self.b)(*fan)
        c_num = (ctypes.c_size_t * self.b)(*numels)
        nbytes = ctypes.c_size_t(0)
        _check("dlsim_batch_table_bytes",
               lib.dlsim_batch_table_bytes(self.b, c_fan, c_num, self.dtype, ctypes.byref(nbytes)))
        self._h = torch.empty(nbytes.value, dtype=torch.uint8, pin_memory=True)
        _check("dlsim_batch_table_fill",
               lib.dlsim_batch_table_fill(self.b, c_fan, (ctypes.c_void_p * len(ptrs))(*ptrs),
                                          (ctypes.c_float * len(ws))(*ws),
                                          (ctypes.c_void_p * self.b)(*outs), c_num, self.dtype,
                                          self._h.data_ptr(), nbytes.value))
        self._d = self._h.to(self.device, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()  # table resident before any stream uses it
        self._keep = tasks
        self._lib = lib

    def launch(self, stream=None) -> None:
        _check("dlsim_batch_table_launch",
               self._lib.dlsim_batch_table_launch(self._h.data_ptr(), self._d.data_ptr(), self.dtype,
                                                  self.mode, _stream_handle(self.device, stream)))


def wreduce_batched(tasks, mode: int = DLSIM_EXACT, stream=None):
    """tasks: sequence of (inputs, weights_f32, out) — independent reduces,
    launched together (dlsim_wreduce_batched). Returns the outs."""
    lib = load()
    b = len(tasks)
    if b == 0:
        return []
    dt = dtype_code(tasks[0][2].dtype)
    fan, ptrs, ws, outs, numels = [], [], [], [], []
    for inputs, w32, out in tasks:
        if len(inputs) < 1:
            raise IndexError("list index out of range")
        if len(w32) != len(inputs):
            raise AssertionError("weights/models length mismatch")
        for t in list(inputs) + [out]:
            if not t.is_cuda or t.dtype != out.dtype or t.numel() != out.numel() or not t.is_contiguous() \
                    or t.device != out.device:
                raise ValueError("each task: contiguous device tensors of one dtype, size and device")
        if out.dtype != tasks[0][2].dtype or out.device != tasks[0][2].device:
            raise ValueError("all tasks of a batch share dtype and device")
        fan.append(len(inputs))
        ptrs.extend(t.data_ptr() for t in inputs)
        ws.extend(np.asarray(w32, dtype=np.float32).tolist())
        outs.append(out.data_ptr())
        numels.append(out.numel())
    c_fan = (ctypes.c_int * b)(*fan)
    c_ptrs = (ctypes.c_void_p * len(ptrs))(*ptrs)
    c_w = (ctypes.c_float * len(ws))(*ws)
    c_outs = (ctypes.c_void_p * b)(*outs)
    c_num = (ctypes.c_size_t * b)(*numels)
    _check("dlsim_wreduce_batched",
           lib.dlsim_wreduce_batched(b, c_fan, c_ptrs, c_w, c_outs, c_num, dt, mode,
                                     _stream_handle(tasks[0][2].device, stream)))
    return [t[2] for t in tasks]


def mean(inputs, out, stream=None):
    """out = (sum_i inputs[i]) / n on the device (flat tensors), stream-ordered:
    torch.mean(torch.stack(inputs), 0) semantics (dlsim_mean)."""
    lib = load()
    n = len(inputs)
    if n < 1:
        raise IndexError("list index out of range")
    dt = dtype_code(out.dtype)
    for t in list(inputs) + [out]:
        if not t.is_cuda or t.dtype != out.dtype or t.numel() != out.numel() or not t.is_contiguous() \
                or t.device != out.device:
            raise ValueError("inputs and output must be contiguous tensors of one dtype and size "
                             "on one device")
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in inputs])
    _check("dlsim_mean", lib.dlsim_mean(ptrs, n, out.data_ptr(), out.numel(), dt,
                                        _stream_handle(out.device, stream)))
    return out


def mean_batched(tasks, stream=None):
    """tasks: sequence of (inputs, out) — independent means (e.g. every chunk
    index of a reconstruction), launched together (dlsim_mean_batched).
    Returns the outs."""
    lib = load()
    b = len(tasks)
    if b == 0:
        return []
    out0 = tasks[0][1]
    dt = dtype_code(out0.dtype, single_task=True)  # fp64 chunks too (PyTorch's double order)
    fan, ptrs, outs, numels = [], [], [], []
    for inputs, out in tasks:
        if len(inputs) < 1:
            raise IndexError("list index out of range")
        for t in list(inputs) + [out]:
            if not t.is_cuda or t.dtype != out0.dtype or t.numel() != out.numel() or not t.is_contiguous() \
                    or t.device != out0.device:
                raise ValueError("each task: contiguous device tensors of one dtype and size; one device")
        fan.append(len(inputs))
        ptrs.extend(t.data_ptr() for t in inputs)
        outs.append(out.data_ptr())
        numels.append(out.numel())
    _check("dlsim_mean_batched",
           lib.dlsim_mean_batched(b, (ctypes.c_int * b)(*fan), (ctypes.c_void_p * len(ptrs))(*ptrs),
                                  (ctypes.c_void_p * b)(*outs), (ctypes.c_size_t * b)(*numels), dt,
                                  _stream_handle(out0.device, stream)))
    return [t[1] for t in tasks]


def chunk_mean_batched(tasks, threads=None, stream=None):
    """tasks: sequence of (inputs, out) — for each, out = the reference's CPU
    torch.mean(torch.stack(inputs), 0) bit for bit, at `threads` intra-op
    threads (default torch.get_num_threads(): the worker's
    settings.torch_threads, broker.py:31), all in few launches
    (dlsim_chunk_mean_batched). Returns the outs."""
    lib = load()
    b = len(tasks)
    if b == 0:
        return []
    if threads is None:
        import torch
        threads = torch.get_num_threads()
    out0 = tasks[0][1]
    dt = dtype_code(out0.dtype, single_task=True)  # fp64 chunks too (PyTorch's double order)
    fan, ptrs, outs, numels = [], [], [], []
    for inputs, out in tasks:
        if len(inputs) < 1:
            raise IndexError("list index out of range")
        for t in list(inputs) + [out]:
            if not t.is_cuda or t.dtype != out0.dtype or t.numel() != out.numel() or not t.is_contiguous() \
                    or t.device != out0.device:
                raise ValueError("each task: contiguous device tensors of one dtype and size; one device")
        fan.append(len(inputs))
        ptrs.extend(t.data_ptr() for t in inputs)
        outs.append(out.data_ptr())
        numels.append(out.numel())
    _check("dlsim_chunk_mean_batched",
           lib.dlsim_chunk_mean_batched(b, (ctypes.c_int * b)(*fan), (ctypes.c_void_p * len(ptrs))(*ptrs),
                                        (ctypes.c_void_p * b)(*outs), (ctypes.c_size_t * b)(*numels), dt,
                                        int(threads), _stream_handle(out0.device, stream)))
    return [t[1] for t in tasks]


def chunk_mean_batched_raw(fan, ptrs, out_ptrs, numels, dtype: int, threads: int, stream_handle) -> None:
    """dlsim_chunk_mean_batched on pointers the caller has validated
    (ChunkManager.mean_chunk_indices after _pyhost.chunk_scan: contiguous
    device chunks of one dtype on one device, outputs it allocated)."""
    b = len(fan)
    _check("dlsim_chunk_mean_batched",
           load().dlsim_chunk_mean_batched(b, (ctypes.c_int * b)(*fan), (ctypes.c_void_p * len(ptrs))(*ptrs),
                                           (ctypes.c_void_p * b)(*out_ptrs), (ctypes.c_size_t * b)(*numels), dtype,
                                           int(threads), stream_handle))


def host_chunk_mean_raw(fan, ptrs, numels, staging_ptr: int, d_staging_ptr: int, staging_elems: int, out_ptrs,
                        host_ptrs, dtype: int, cpu_threads: int, threads: int, stream_handle, h2d=None,
                        d2h=None) -> None:
    """dlsim_host_chunk_mean on pointers the caller has validated (as
    chunk_mean_batched_raw, host chunks; staging it sized with
    staged_rows_elems)."""
    b = len(fan)
    _check("dlsim_host_chunk_mean",
           load().dlsim_host_chunk_mean(b, (ctypes.c_int * b)(*fan), (ctypes.c_void_p * len(ptrs))(*ptrs),
                                        (ctypes.c_size_t * b)(*numels), staging_ptr, d_staging_ptr, staging_elems,
                                        (ctypes.c_void_p * b)(*out_ptrs),
                                        None if host_ptrs is None else (ctypes.c_void_p * b)(*host_ptrs), dtype,
                                        int(cpu_threads), int(threads), stream_handle, h2d, d2h))


def staged_rows_elems(numels, fan_in, esz: int) -> int:
    """Staging size dlsim_host_chunk_mean needs: every input row at a 256-B
    aligned offset."""
    al = 256 // esz
    return sum(f * ((k + al - 1) // al * al) for k, f in zip(numels, fan_in))


def host_chunk_mean(tasks, staging, d_staging, host_outs=None, threads=None, cpu_threads=None, stream=None,
                    h2d_stream=None, d2h_stream=None):
    """dlsim_host_chunk_mean. tasks: sequence of (host inputs, device out);
    `staging` (pinned) and `d_staging` (device) hold staged_rows_elems()
    elements; host_outs: None or per task a pinned host tensor (or None).
    Returns after packing; synchronise `stream` before reading host_outs or
    freeing the staging."""
    import torch
    lib = load()
    b = len(tasks)
    if b == 0:
        return []
    out0 = tasks[0][1]
    dt = out0.dtype
    fan, ptrs, outs, numels, keep = [], [], [], [], []
    for inputs, out in tasks:
        if len(inputs) < 1:
            raise IndexError("list index out of range")
        if not out.is_cuda or out.dtype != dt or not out.is_contiguous() or out.device != out0.device:
            raise ValueError("outputs: contiguous device tensors of one dtype, one device")
        for x in inputs:
            if x.get_device() != -1 or x.dtype is not dt or x.numel() != out.numel():
                raise ValueError("inputs: host tensors of the output's dtype and size")
            if not x.is_contiguous():
                x = x.contiguous()
                keep.append(x)
            ptrs.append(x.data_ptr())
        fan.append(len(inputs))
        outs.append(out.data_ptr())
        numels.append(out.numel())
    need = staged_rows_elems(numels, fan, out0.element_size())
    if staging.numel() < need or d_staging.numel() < need or staging.dtype != dt or d_staging.dtype != dt \
            or staging.is_cuda or not d_staging.is_cuda or not staging.is_contiguous() \
            or not d_staging.is_contiguous():
        raise ValueError(f"staging: a pinned host and a device buffer of >= {need} elements of the dtype")
    hptrs = None
    if host_outs is not None:
        hp = []
        for h, (_, out) in zip(host_outs, tasks):
            if h is not None and (h.is_cuda or h.dtype != dt or h.numel() != out.numel() or not h.is_contiguous()):
                raise ValueError("host_outs: host tensors of the outputs' dtype and size")
            hp.append(None if h is None else h.data_ptr())
        hptrs = (ctypes.c_void_p * b)(*hp)
    _check("dlsim_host_chunk_mean",
           lib.dlsim_host_chunk_mean(b, (ctypes.c_int * b)(*fan), (ctypes.c_void_p * len(ptrs))(*ptrs),
                                     (ctypes.c_size_t * b)(*numels), staging.data_ptr(), d_staging.data_ptr(),
                                     min(staging.numel(), d_staging.numel()), (ctypes.c_void_p * b)(*outs), hptrs,
                                     dtype_code(dt, single_task=True),  # fp64 chunks too
                                     int(torch.get_num_threads() if cpu_threads is None else cpu_threads),
                                     int(torch.get_num_threads() if threads is None else threads),
                                     _stream_handle(out0.device, stream),
                                     None if h2d_stream is None else h2d_stream.cuda_stream,
                                     None if d2h_stream is None else d2h_stream.cuda_stream))
    return [t[1] for t in tasks]


_RCCL_BOUND = None


def rccl_bind(path: Optional[str] = None) -> str:
    """Bind the RCCL that owns the caller's communicators (default: the
    librccl.so PyTorch loaded, next to libtorch_hip.so)."""
    global _RCCL_BOUND
    if path is None:
        import torch
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if not os.path.exists(path):
            path = "librccl.so.1"
    if _RCCL_BOUND != path:
        _check("dlsim_rccl_bind", load().dlsim_rccl_bind(path.encode()))
        _RCCL_BOUND = path
    return path


def gather_code(gather) -> int:
    """enum dlsim_gather of a `gather` argument: False/True (no gather / the
    grouped broadcasts), an enum value, or "none" / "bcast" / "allgather"."""
    if isinstance(gather, str):
        codes = {"none": DLSIM_GATHER_NONE, "bcast": DLSIM_GATHER_BCAST, "allgather": DLSIM_GATHER_ALLGATHER}
        if gather not in codes:
            raise ValueError(f"gather must be one of {sorted(codes)}, got {gather!r}")
        return codes[gather]
    g = int(gather)
    if g not in (DLSIM_GATHER_NONE, DLSIM_GATHER_BCAST, DLSIM_GATHER_ALLGATHER):
        raise ValueError(f"gather must be 0, 1 or 2 (enum dlsim_gather), got {gather!r}")
    return g


def _check_slices(slices, out):
    n = len(slices)
    if n < 1:
        raise IndexError("list index out of range")
    for x in slices:
        if not x.is_cuda or x.dtype != out.dtype or not x.is_contiguous() or x.device != out.device \
                or x.numel() != slices[0].numel():
            raise ValueError("slices must be equal-length contiguous device tensors of the output's dtype "
                             "and device")
    if not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous device tensor")
    return (ctypes.c_void_p * n)(*[x.data_ptr() for x in slices])


def _weights_arg(weights, n, f64):
    w = np.ascontiguousarray(weights, dtype=np.float64 if f64 else np.float32)
    if w.size != n:
        raise AssertionError("weights/models length mismatch")
    return w, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double if f64 else ctypes.c_float))


def wreduce_sharded(slices, weights_f32, out, comm_ptr: int, gather=True,
                    mode: int = DLSIM_EXACT, stream=None):
    """dlsim_wreduce_sharded: `slices[i]` is this rank's slice of model i,
    `out` the full-size output; `comm_ptr` an RCCL communicator (e.g.
    ProcessGroupNCCL._comm_ptr()); `gather` as gather_code. fp64 tensors go to
    dlsim_wreduce_sharded_f64 and take exact double weights (pass
    weights_for_dtype(weights, torch.float64))."""
    import torch
    lib = load()
    if _RCCL_BOUND is None:  # the caller may have bound another RCCL (tests bind a stub)
        rccl_bind()
    g = gather_code(gather)
    ptrs = _check_slices(slices, out)
    n = len(slices)
    f64 = out.dtype == torch.float64
    w, wp = _weights_arg(weights_f32, n, f64)
    st = _stream_handle(out.device, stream)
    if f64:
        _check("dlsim_wreduce_sharded_f64",
               lib.dlsim_wreduce_sharded_f64(ptrs, slices[0].numel(), n, wp, out.data_ptr(), out.numel(), mode,
                                             ctypes.c_void_p(comm_ptr), g, st))
        return out
    _check("dlsim_wreduce_sharded",
           lib.dlsim_wreduce_sharded(ptrs, slices[0].numel(), n, wp, out.data_ptr(), out.numel(),
                                     dtype_code(out.dtype), mode, ctypes.c_void_p(comm_ptr), g, st))
    return out


def wreduce_sharded_failed(comm_ptr: int, n_elems: int, gather, device, stream=None) -> None:
    """Join dlsim_wreduce_sharded's agreement step as a rank whose arguments
    already failed the caller's own checks (no slices, no output): the library
    tells every other rank, so none enters the gather, and this call returns
    the library's own argument error (raised as DlsimError)."""
    lib = load()
    if _RCCL_BOUND is None:
        rccl_bind()
    _check("dlsim_wreduce_sharded",
           lib.dlsim_wreduce_sharded(None, ctypes.c_size_t(-1 & 0xFFFFFFFFFFFFFFFF), 0, None, None, n_elems,
                                     DLSIM_F32, DLSIM_EXACT, ctypes.c_void_p(comm_ptr), gather_code(gather),
                                     _stream_handle(device, stream)))


class ShardedPlan:
    """dlsim_sharded_plan: the sharded aggregate of one shape (n_elems, n
    models, dtype, gather) on one RCCL communicator, agreed ONCE by every
    rank at construction (a collective call), then run any number of times
    with no agreement and no host wait (`run`). A rank whose run fails its
    local checks still enters the gather and raises afterwards; its peers get
    no error, but its slice arrives as NaN (include/dlsim.h)."""

    def __init__(self, comm_ptr: int, n_elems: int, n: int, dtype, gather=True, device=None, stream=None):
        import torch
        lib = load()
        if _RCCL_BOUND is None:
            rccl_bind()
        self._lib = lib
        self.n_elems, self.n, self.dtype = int(n_elems), int(n), dtype
        self.gather = gather_code(gather)
        self.f64 = dtype == torch.float64
        code = dtype_code(dtype, single_task=True)
        h = ctypes.c_void_p()
        _check("dlsim_sharded_plan_create",
               lib.dlsim_sharded_plan_create(ctypes.c_void_p(comm_ptr), self.n_elems, self.n, code, self.gather,
                                             _stream_handle(device, stream), ctypes.byref(h)))
        self._h = h

    def run(self, slices, weights, out, mode: int = DLSIM_EXACT, stream=None):
        if self._h is None:
            raise ValueError("plan destroyed")
        try:
            if len(slices) != self.n:
                # the library reads the plan's n pointers and weights: fewer
                # would be read past the arrays, more silently dropped
                raise ValueError(f"the plan was made for {self.n} models, got {len(slices)} slices")
            ptrs = _check_slices(slices, out)
            if out.numel() != self.n_elems or out.dtype != self.dtype:
                raise ValueError(f"out must be a full {self.n_elems}-element {self.dtype} buffer")
            w, wp = _weights_arg(weights, len(slices), self.f64)
        except (AssertionError, ValueError, IndexError, TypeError):
            # still enter the gather, so no peer is left waiting in it
            try:
                self.run_failed(getattr(out, "device", None))
            except DlsimError:
                pass
            raise
        fn = "dlsim_sharded_plan_run_f64" if self.f64 else "dlsim_sharded_plan_run"
        _check(fn, getattr(self._lib, fn)(self._h, ptrs, slices[0].numel(), wp, out.data_ptr(), mode,
                                          _stream_handle(out.device, stream)))
        return out

    def run_failed(self, device, stream=None) -> None:
        """Enter the plan's gather as a rank whose own arguments failed the
        caller's checks (no slices, no output): peers are not left waiting;
        raises the library's argument error."""
        if self._h is None:
            raise ValueError("plan destroyed")
        fn = "dlsim_sharded_plan_run_f64" if self.f64 else "dlsim_sharded_plan_run"
        _check(fn, getattr(self._lib, fn)(self._h, None, 0, None, None, DLSIM_EXACT, _stream_handle(device, stream)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            h, self._h = self._h, None
            _check("dlsim_sharded_plan_destroy", self._lib.dlsim_sharded_plan_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chunk_mean_ilp_begin(m: int, n: int, threads: int) -> int:
    """Host rule of dlsim_chunk_mean_batched (no GPU needed)."""
    return int(load().dlsim_chunk_mean_ilp_begin(m, n, threads))


def chunk_mean_plan(tasks, threads: int, cus: int = 0, dtype=None):
    """The launches chunk_mean_batched(tasks, threads) would make
    (dlsim_chunk_mean_plan: decided by the launching code, nothing launched,
    no pointer read). tasks: (inputs, out) tensors as chunk_mean_batched
    takes them, or (input addresses, output address, numel) integers of
    `dtype` (default torch.float32), which only need the alignment and spacing
    of real buffers. cus > 0 stands for the device's CU count (no GPU
    needed); 0 asks the device. Returns one dict per launch, in launch order:
    form (one of CHUNK_FORMS), mf, R, bpt, grid, ntasks, first_task."""
    import torch
    lib = load()
    fan, ptrs, outs, numels = [], [], [], []
    for task in tasks:
        if len(task) == 3:
            ins, out, n = task
            dt = torch.float32 if dtype is None else dtype
            ptrs.extend(int(q) for q in ins)
            outs.append(int(out))
        else:
            ins, out = task
            n, dt = out.numel(), out.dtype
            if dtype is not None and dt != dtype:
                raise ValueError("a task's tensors are not of `dtype`")
            ptrs.extend(t.data_ptr() for t in ins)
            outs.append(out.data_ptr())
        dtype = dt
        fan.append(len(ins))
        numels.append(int(n))
    b = len(fan)
    if b == 0:
        return []
    cap = b + 1  # every launch holds at least one task
    recs = (ChunkLaunch * cap)()
    count = ctypes.c_int(0)
    _check("dlsim_chunk_mean_plan",
           lib.dlsim_chunk_mean_plan(b, (ctypes.c_int * b)(*fan), (ctypes.c_void_p * len(ptrs))(*ptrs),
                                     (ctypes.c_void_p * b)(*outs), (ctypes.c_size_t * b)(*numels),
                                     dtype_code(dtype, single_task=True), int(threads), int(cus), recs, cap,
                                     ctypes.byref(count)))
    assert count.value <= cap
    return [{"form": CHUNK_FORMS[r.form], "mf": r.mf, "R": r.rows, "bpt": r.bpt, "grid": r.grid,
             "ntasks": r.ntasks, "first_task": r.first_task} for r in recs[:count.value]]


def wreduce_tensors_raw(in_ptrs: Sequence[int], n: int, numels: Sequence[int], weights_f32, out_ptrs: Sequence[int],
                       dtype: int, mode: int, stream_handle) -> None:
    """dlsim_wreduce_tensors on pointers the caller has already validated
    (the arena path: every tensor checked against models[0]'s layout, on the
    output's device, contiguous): no per-tensor Python checks.
    in_ptrs model-major (tensor k of model i at i * t + k)."""
    t = len(numels)
    w = np.ascontiguousarray(weights_f32, dtype=np.float32)
    rc = load().dlsim_wreduce_tensors((ctypes.c_void_p * len(in_ptrs))(*in_ptrs), n, t,
                                      (ctypes.c_size_t * t)(*numels), w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                      (ctypes.c_void_p * t)(*out_ptrs), dtype, mode, stream_handle)
    _check("dlsim_wreduce_tensors", rc)


_ROWS_BOUND = False


def wreduce_rows(rows, idx: Sequence[int], numels: Sequence[int], weights_f32: np.ndarray, out_base: int,
                 out_offsets: Sequence[int], dtype: int, mode: int, stream_handle: int, device: int = 0) -> bool:
    """dlsim_wreduce_tensors over tensor k of every model (k in idx;
    rows[i][k] is a tensor of model i), called from C (csrc/pyhost.cpp) with
    the data pointers read from the tensors there: the caller has checked
    shapes and dtypes (the layout). Output tensor j is at out_base +
    out_offsets[j] bytes. Returns False, having launched nothing, when a
    tensor is not contiguous or not on CUDA device `device` (the caller then
    stages it)."""
    global _ROWS_BOUND
    from . import _pyhost
    if not _ROWS_BOUND:
        _pyhost.bind_wreduce_tensors(ctypes.cast(load().dlsim_wreduce_tensors, ctypes.c_void_p).value)
        _ROWS_BOUND = True
    rc = _pyhost.wreduce_rows(rows, idx, numels, weights_f32, out_base, out_offsets, dtype, mode,
                              stream_handle or 0, device)
    if rc is None:
        return False
    _check("dlsim_wreduce_tensors", rc)
    return True


_BATCHED_BOUND = False


def wreduce_rows_multi(tasks, dtype: int, mode: int, stream_handle: int, device: int = 0) -> bool:
    """Many tasks' wreduce_rows in one dlsim_wreduce_batched call (sub-task =
    one parameter tensor of one task), pointers collected in C
    (csrc/pyhost.cpp). tasks: [(rows, idx, numels, weights_f32, out_base,
    out_offsets)] as wreduce_rows takes them. Returns False, having launched
    nothing, when a tensor is not contiguous or not on CUDA device `device`."""
    global _BATCHED_BOUND
    from . import _pyhost
    if not _BATCHED_BOUND:
        _pyhost.bind_wreduce_batched(ctypes.cast(load().dlsim_wreduce_batched, ctypes.c_void_p).value)
        _BATCHED_BOUND = True
    rc = _pyhost.wreduce_rows_multi(tasks, dtype, mode, stream_handle or 0, device)
    if rc is None:
        return False
    _check("dlsim_wreduce_batched", rc)
    return True


def wreduce_tensors(inputs_by_model, weights_f32, outs, mode: int = DLSIM_EXACT, stream=None):
    """Tensor-list form: inputs_by_model[i][k] is tensor k of model i."""
    lib = load()
    n = len(inputs_by_model)
    if n < 1:
        raise IndexError("list index out of range")
    t = len(outs)
    dt = dtype_code(outs[0].dtype) if t else DLSIM_F32
    # get_device(): the CUDA ordinal as an int (-1 on the host), cheaper than
    # building torch.device objects per tensor
    odev = outs[0].get_device() if t else -1
    spec = [(o.dtype, o.numel()) for o in outs]
    if t and (odev < 0 or any(o.get_device() != odev for o in outs)):
        raise ValueError("outputs must be CUDA tensors on one device")
    flat = []
    for row in inputs_by_model:
        if len(row) != t:
            raise ValueError("every model must have the same number of tensors")
        for k, x in enumerate(row):
            d, ne = spec[k]
            if x.get_device() != odev or x.dtype is not d or x.numel() != ne or not x.is_contiguous():
                raise ValueError(f"tensor {k}: device/contiguity/dtype/size mismatch")
            flat.append(x.data_ptr())
    ptrs = (ctypes.c_void_p * len(flat))(*flat)
    numels = (ctypes.c_size_t * t)(*[o.numel() for o in outs])
    optrs = (ctypes.c_void_p * t)(*[o.data_ptr() for o in outs])
    w = np.ascontiguousarray(weights_f32, dtype=np.float32)
    if w.size != n:
        raise AssertionError("weights/models length mismatch")
    dev = outs[0].device if t else None
    rc = lib.dlsim_wreduce_tensors(ptrs, n, t, numels, w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                   optrs, dt, mode, _stream_handle(dev, stream) if t else None)
    _check("dlsim_wreduce_tensors", rc)
    return outs


def host_wreduce_raw(src_ptrs: Sequence[int], n: int, numels: Sequence[int], weights_f32, staging, rows, out,
                     host_out, dtype: int, mode: int, chunk_elems: int, threads: int, stream_handle,
                     h2d_stream=None, d2h_stream=None) -> None:
    """dlsim_host_wreduce on host pointers the caller has already validated
    (the arena path: contiguous host tensors of models[0]'s layout), with
    staging / rows / out / host_out checked here once."""
    if staging.stride(0) != rows.stride(0) or staging.is_cuda or not rows.is_cuda or not out.is_cuda:
        raise ValueError("staging/rows: a pinned host and a device [n, >= total] buffer with equal strides")
    t = len(numels)
    w = np.ascontiguousarray(weights_f32, dtype=np.float32)
    rc = load().dlsim_host_wreduce(
        n, t, (ctypes.c_void_p * len(src_ptrs))(*src_ptrs), (ctypes.c_size_t * t)(*numels),
        w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), staging.data_ptr(), rows.data_ptr(), staging.stride(0),
        out.data_ptr(), None if host_out is None else host_out.data_ptr(), dtype, mode, chunk_elems, threads,
        stream_handle, None if h2d_stream is None else h2d_stream.cuda_stream,
        None if d2h_stream is None else d2h_stream.cuda_stream)
    _check("dlsim_host_wreduce", rc)


def host_wreduce_zc_raw(src_ptrs: Sequence[int], n: int, numels: Sequence[int], weights_f32, staging, host_out,
                        dtype: int, mode: int, threads: int, stream_handle) -> None:
    """dlsim_host_wreduce_zc on host pointers the caller has validated (the
    arena path): `staging` a page-locked [n, stride] row buffer, `host_out` a
    page-locked result; the reduce reads and writes them over PCIe."""
    if staging.is_cuda or host_out.is_cuda or staging.dim() != 2:
        raise ValueError("staging: a page-locked [n, >= total] host buffer; host_out: a page-locked host tensor")
    t = len(numels)
    w = np.ascontiguousarray(weights_f32, dtype=np.float32)
    rc = load().dlsim_host_wreduce_zc(
        n, t, (ctypes.c_void_p * len(src_ptrs))(*src_ptrs), (ctypes.c_size_t * t)(*numels),
        w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), staging.data_ptr(), staging.stride(0),
        host_out.data_ptr(), dtype, mode, threads, stream_handle)
    _check("dlsim_host_wreduce_zc", rc)


_HOST_ZC_BOUND = [False]


def host_zc(all_params, idx, numels: Sequence[int], weights_f32: np.ndarray, staging, host_out, dtype: int,
            mode: int, threads: int, stream_handle: int) -> bool:
    """dlsim_host_wreduce_zc over the models' parameter tensors
    (all_params[i][k] for k in idx), the pointers read in C (_pyhost.host_zc,
    the library bound by address). False (nothing launched) if a tensor is
    not a contiguous host tensor; raises DlsimError on a library error."""
    from . import _pyhost
    if not _HOST_ZC_BOUND[0]:
        _pyhost.bind_host_zc(ctypes.cast(load().dlsim_host_wreduce_zc, ctypes.c_void_p).value)
        _HOST_ZC_BOUND[0] = True
    rc = _pyhost.host_zc(all_params, idx, numels, weights_f32, staging, host_out, dtype, mode, threads,
                         stream_handle or 0)
    if rc is None:
        return False
    _check("dlsim_host_wreduce_zc", rc)
    return True


def host_wreduce_resident_raw(src_ptrs: Sequence[int], n: int, numels: Sequence[int], weights_f32,
                              resident: Sequence[bool], row_ptrs: Sequence[int], staging, out, host_out, dtype: int,
                              mode: int, threads: int, stream_handle) -> None:
    """dlsim_host_wreduce_resident on pointers the caller has validated (the
    arena path with a device cache): src_ptrs model-major, n * len(numels)
    entries (0 for a resident model's tensors); row_ptrs the n device rows;
    staging a pinned [m, stride] buffer for the m non-resident models."""
    t = len(numels)
    w = np.ascontiguousarray(weights_f32, dtype=np.float32)
    stride = staging.stride(0) if staging is not None and staging.dim() == 2 else 0
    rc = load().dlsim_host_wreduce_resident(
        n, t, (ctypes.c_void_p * max(1, len(src_ptrs)))(*src_ptrs), (ctypes.c_size_t * t)(*numels),
        w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_int * n)(*[1 if r else 0 for r in resident]),
        (ctypes.c_void_p * n)(*row_ptrs), None if staging is None else staging.data_ptr(), stride, out.data_ptr(),
        None if host_out is None else host_out.data_ptr(), dtype, mode, threads, stream_handle)
    _check("dlsim_host_wreduce_resident", rc)


def host_wreduce(inputs_by_model, weights_f32, staging, rows, out, host_out=None, mode: int = DLSIM_EXACT,
                 chunk_elems: int = 0, threads: Optional[int] = None, stream=None, h2d_stream=None,
                 d2h_stream=None):
    """dlsim_host_wreduce: inputs_by_model[i][k] is host tensor k of model i
    (one dtype); `staging` (pinned) and `rows` (device) are [n, >= total]
    row buffers with equal row strides; `out` the device result, `host_out`
    an optional pinned host copy. Returns after packing; the copies and
    reduces are queued (synchronise `stream` before reading host_out)."""
    import torch
    lib = load()
    n = len(inputs_by_model)
    if n < 1:
        raise IndexError("list index out of range")
    t = len(inputs_by_model[0])
    dt = out.dtype
    flat, keep = [], []
    numels = [x.numel() for x in inputs_by_model[0]]
    for row in inputs_by_model:
        if len(row) != t:
            raise ValueError("every model must have the same number of tensors")
        for k, x in enumerate(row):
            if x.dtype is not dt or x.get_device() != -1 or x.numel() != numels[k]:
                raise ValueError(f"tensor {k}: host tensors of the output's dtype and size expected")
            if not x.is_contiguous():
                x = x.contiguous()
                keep.append(x)
            flat.append(x.data_ptr())
    total = sum(numels)
    if out.numel() != total or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous device tensor of the models' size")
    if staging.dim() != 2 or rows.dim() != 2 or staging.shape[0] < n or rows.shape[0] < n \
            or staging.stride(0) != rows.stride(0) or staging.stride(1) != 1 or rows.stride(1) != 1 \
            or staging.is_cuda or not rows.is_cuda \
            or staging.dtype != dt or rows.dtype != dt or rows.device != out.device:
        raise ValueError("staging/rows: [n, >= total] buffers of the output's dtype, equal strides")
    if host_out is not None and (host_out.numel() != total or host_out.dtype != dt or host_out.is_cuda
                                 or not host_out.is_contiguous()):
        raise ValueError("host_out must be a host tensor of the output's size and dtype")
    w = np.ascontiguousarray(weights_f32, dtype=np.float32)
    if w.size != n:
        raise AssertionError("weights/models length mismatch")
    st = _stream_handle(out.device, stream)
    rc = lib.dlsim_host_wreduce(
        n, t, (ctypes.c_void_p * len(flat))(*flat), (ctypes.c_size_t * t)(*numels),
        w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), staging.data_ptr(), rows.data_ptr(),
        staging.stride(0), out.data_ptr(), None if host_out is None else host_out.data_ptr(),
        dtype_code(dt), mode, chunk_elems, torch.get_num_threads() if threads is None else threads, st,
        None if h2d_stream is None else h2d_stream.cuda_stream,
        None if d2h_stream is None else d2h_stream.cuda_stream)
    _check("dlsim_host_wreduce", rc)
    return out


def host_pack(srcs, dst_offsets, dst, threads: Optional[int] = None):
    """dlsim_host_pack: copy host tensors srcs[j] (contiguous) into the host
    tensor `dst` at byte offsets dst_offsets[j], on the library's threads."""
    import torch
    if dst.is_cuda or not dst.is_contiguous():
        raise ValueError("dst must be a contiguous host tensor")
    cap = dst.numel() * dst.element_size()
    ptrs, nb = [], []
    for x, o in zip(srcs, dst_offsets):
        if x.get_device() != -1 or not x.is_contiguous():
            raise ValueError("sources must be contiguous host tensors")
        b = x.numel() * x.element_size()
        if o < 0 or o + b > cap:
            raise ValueError("source does not fit dst at its offset")
        ptrs.append(x.data_ptr())
        nb.append(b)
    t = len(ptrs)
    _check("dlsim_host_pack",
           load().dlsim_host_pack(t, (ctypes.c_void_p * max(t, 1))(*ptrs), (ctypes.c_size_t * max(t, 1))(*nb),
                                  (ctypes.c_size_t * max(t, 1))(*dst_offsets), dst.data_ptr(),
                                  int(torch.get_num_threads() if threads is None else threads)))
    return dst


def probe_pattern(inputs, out, stream=None):
    """dlsim_probe_pattern: the reduce's dispatch for these buffers (kernel,
    launch shape, load/store policies) with the fold replaced by a bitwise
    XOR — the memory-only ceiling of this exact access pattern."""
    return ReducePlan(inputs, np.ones(len(inputs), np.float32), out, probe=True).launch(stream)
