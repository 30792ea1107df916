// sgd_kernels.hpp — gfx950 streaming kernels for the first step of a fresh
// torch.optim.SGD (the `gradient_update` task: reference
// dasklearn/functions.py:85-86 -> ModelTrainer.gradient_update,
// model_trainer.py:133-143).
//
// A fresh optimizer's momentum buffer is a clone of the gradient, so momentum
// takes no part; per parameter tensor torch's CPU path runs
//   g' = grad.add(param, alpha=weight_decay)   (only if weight_decay != 0)
//   param.add_(g', alpha=-lr)
// Two input streams, one output stream, two fused multiply-adds per element:
// HBM-bound like the 2-way reduce, and built like its tiled kernel (16-byte
// loads per lane, every load of a tile issued before the first use, one
// 16-byte non-temporal store per vector, block 0 folding the ragged end).
//
// Rounding contract, per element:
//   fp32: g' = fma(f32(wd), p, g); p' = fma(-f32(lr), g', p)
//   fp64: the same with double fma and the exact double scalars
//   bf16: the scalars rounded to bf16 (through fp32); ATen's vector body
//         computes each add in fp32 and rounds its result to bf16 once (the
//         product of two bf16 values is exact in fp32, so fused and unfused
//         agree); ATen's scalar loop, which takes the last len mod 32 elements
//         of every thread's range, also rounds the product to bf16. Which
//         elements those are is CpuLayout below.
// weight_decay == 0 skips the first add (0 * Inf would make a NaN), so the two
// cases are separate instantiations (WD).
#pragma once

#include <cstring>

#include "wreduce_kernels.hpp"

namespace dlsim {

// ---- element policies -------------------------------------------------------
// (names outside scripts/audit_isa.py's POLICIES: these kernels fuse by contract)
template <bool WD>
struct SgdF32 {
  static constexpr int E = 4;
  static constexpr int kBytes = 4;
  static constexpr int kFmt = kFmtF32;
  static constexpr bool kCpuTails = false;
  __device__ static float upd(float p, float g, float nlr, float wd) {
    if constexpr (WD) g = __builtin_fmaf(wd, p, g);
    return __builtin_fmaf(nlr, g, p);
  }
  __device__ static float finish(float a, float) { return a; }
};

template <bool WD>
struct SgdF64 {
  using T = double;
  using W = double;
  static constexpr int E = 2;
  static constexpr int kBytes = 8;
  static constexpr int kFmt = kFmtF32;
  static constexpr bool kCpuTails = false;
  __device__ static double upd(double p, double g, double nlr, double wd) {
    if constexpr (WD) g = __builtin_fma(wd, p, g);
    return __builtin_fma(nlr, g, p);
  }
  __device__ static double finish(double a, float) { return a; }
};

// One hardware conversion (v_cvt_pk_bf16_f32, nearest-even) on every path, so
// the vector and scalar paths of the kernels give the same bits.
__device__ __forceinline__ float sgd_bf16_round(float a) {
  float b = a;
  bf16_round2(a, b);
  return a;
}

template <bool WD>
struct SgdBF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtBF16;
  static constexpr bool kCpuTails = true;
  // ATen's vector body: each add in fp32, its result rounded to bf16
  __device__ static float upd(float p, float g, float nlr, float wd) {
    if constexpr (WD) g = sgd_bf16_round(__builtin_fmaf(wd, p, g));
    return sgd_bf16_round(__builtin_fmaf(nlr, g, p));
  }
  __device__ static void upd2(float& p0, float& p1, float g0, float g1, float nlr, float wd) {
    if constexpr (WD) {
      g0 = __builtin_fmaf(wd, p0, g0);
      g1 = __builtin_fmaf(wd, p1, g1);
      bf16_round2(g0, g1);
    }
    p0 = __builtin_fmaf(nlr, g0, p0);
    p1 = __builtin_fmaf(nlr, g1, p1);
    bf16_round2(p0, p1);
  }
  // ATen's scalar loop: c10::BFloat16 arithmetic, `a + alpha * b` with the
  // product and the sum each rounded to bf16
  __device__ static float upd_tail(float p, float g, float nlr, float wd) {
    if constexpr (WD) g = sgd_bf16_round(g + sgd_bf16_round(wd * p));
    return sgd_bf16_round(p + sgd_bf16_round(nlr * g));
  }
  __device__ static float finish(float a, float) { return a; }
};

// The same rounding on the host (nearest-even; NaN kept), for the scalars the
// dispatch passes to the bf16 kernels.
inline float sgd_host_round_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return f;
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  std::memcpy(&f, &u, 4);
  return f;
}

// ---- which elements ATen's scalar loop takes ----------------------------------
// TensorIterator runs a contiguous n-element op serially below 32768 elements
// (or at one thread), else at::parallel_for splits [0, n) into
// min(threads, ceil(n / 32768)) ranges of ceil(n / ranges) elements. Inside a
// range the vectorised loop takes one vector of 32 bf16 at a time (an AVX-512
// host) and the scalar loop the remaining len mod 32 elements (established on
// the CPU, scripts/probes/probe_sgd_bf16_rule.py). The host computes `chunk`
// (the range length; the whole tensor when serial).
constexpr size_t kSgdCpuGrain = 32768;
constexpr size_t kSgdCpuVec = 32;
constexpr int kSgdCpuThreads = 4;  // the reference worker's torch threads (broker.py:31)

struct CpuLayout {
  size_t n;      // elements of the whole tensor
  size_t chunk;  // elements per thread range (>= 1 when the policy has tails)
  size_t base;   // index in the tensor of this launch's element 0
};

__host__ __device__ inline size_t sgd_cpu_chunk(size_t n, int threads) {
  if (n < kSgdCpuGrain || threads <= 1) return n ? n : 1;
  const size_t ranges_by_grain = (n + kSgdCpuGrain - 1) / kSgdCpuGrain;
  const size_t ranges = ranges_by_grain < static_cast<size_t>(threads) ? ranges_by_grain : static_cast<size_t>(threads);
  return (n + ranges - 1) / ranges;
}

// element j (of this launch) is in a scalar tail
__device__ __forceinline__ bool cpu_tail(const CpuLayout& L, size_t j) {
  j += L.base;
  const size_t b = j / L.chunk * L.chunk;
  const size_t len = L.n - b < L.chunk ? L.n - b : L.chunk;
  return j - b >= len - len % kSgdCpuVec;
}

// elements [e0, e1) of this launch all lie in one range's vector body
__device__ __forceinline__ bool cpu_body(const CpuLayout& L, size_t e0, size_t e1) {
  e0 += L.base;
  e1 += L.base;
  const size_t b = e0 / L.chunk * L.chunk;
  const size_t len = L.n - b < L.chunk ? L.n - b : L.chunk;
  return e1 <= b + (len - len % kSgdCpuVec);
}

template <class Op>
__device__ __forceinline__ acc_t<Op> sgd_elem(acc_t<Op> p, acc_t<Op> g, wt_t<Op> nlr, wt_t<Op> wd, const CpuLayout& L,
                                              size_t j) {
  if constexpr (Op::kCpuTails) {
    if (cpu_tail(L, j)) return Op::upd_tail(p, g, nlr, wd);
  }
  return Op::upd(p, g, nlr, wd);
}

template <class Op>
__device__ __forceinline__ void sgd_scalar_elem(const void* p, const void* g, void* out, size_t j, wt_t<Op> nlr,
                                                wt_t<Op> wd, const CpuLayout& L) {
  const acc_t<Op> xp = load_elem<Op>(p, j), xg = load_elem<Op>(g, j);
  store_elem<Op>(out, j, sgd_elem<Op>(xp, xg, nlr, wd, L, j), 1.0f);
}

// Scalar kernel: any alignment, one element per thread. `out` may be `p` or
// `g` (each element is read before it is written, by the same lane).
template <class Op>
__global__ __launch_bounds__(kBlock) void k_sgd_scalar(const void* p, const void* g, void* out, size_t nelem,
                                                       wt_t<Op> nlr, wt_t<Op> wd, CpuLayout L) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < nelem) sgd_scalar_elem<Op>(p, g, out, j, nlr, wd, L);
}

// One tile: lane's vectors v0 + k*VS, both streams' loads issued before the
// first use. TAILS: some element of the tile may be in a scalar tail.
template <class Op, int VPT, bool CHECK, int STP, bool TAILS, int VS = kBlock>
__device__ __forceinline__ void sgd_tile(const void* p, const void* g, const OutRef& o, size_t v0, size_t nvec,
                                         wt_t<Op> nlr, wt_t<Op> wd, const CpuLayout& L) {
  u32x4 rp[VPT], rg[VPT];
  load_tile<Op, VPT, 1, CHECK, VS>(p, v0, nvec, rp);
  load_tile<Op, VPT, 1, CHECK, VS>(g, v0, nvec, rg);
#pragma unroll
  for (int v = 0; v < VPT; ++v) {
    const size_t idx = v0 + static_cast<size_t>(v) * VS;
    acc_t<Op> xp[Op::E], xg[Op::E];
    unpack<Op>(rp[v], xp);
    unpack<Op>(rg[v], xg);
    if constexpr (TAILS && Op::kCpuTails) {
#pragma unroll
      for (int e = 0; e < Op::E; ++e) xp[e] = sgd_elem<Op>(xp[e], xg[e], nlr, wd, L, idx * Op::E + e);
    } else if constexpr (Op::kBytes == 2) {
#pragma unroll
      for (int e = 0; e < Op::E; e += 2) Op::upd2(xp[e], xp[e + 1], xg[e], xg[e + 1], nlr, wd);
    } else {
#pragma unroll
      for (int e = 0; e < Op::E; ++e) xp[e] = Op::upd(xp[e], xg[e], nlr, wd);
    }
    if (!CHECK || idx < nvec) store_vec<STP>(o, idx, pack<Op>(xp, 1.0f));
  }
}

// A full tile `t` (no bounds checks), by the block or the wave lane map
// (wreduce_kernels.hpp tiles_body).
template <class Op, int VPT, int STP, bool WAVEMAP>
__device__ __forceinline__ void sgd_full_tile(const void* p, const void* g, const OutRef& o, size_t t, size_t nvec,
                                              wt_t<Op> nlr, wt_t<Op> wd, const CpuLayout& L) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  constexpr int VS = WAVEMAP ? 64 : kBlock;
  const size_t lane_off = WAVEMAP ? (threadIdx.x >> 6) * 64 * VPT + (threadIdx.x & 63) : threadIdx.x;
  if constexpr (Op::kCpuTails) {
    // uniform per block: a tile that touches a scalar tail decides per element
    if (!cpu_body(L, t * kTile * Op::E, (t + 1) * kTile * Op::E)) {
      sgd_tile<Op, VPT, false, STP, true, VS>(p, g, o, t * kTile + lane_off, nvec, nlr, wd, L);
      return;
    }
  }
  sgd_tile<Op, VPT, false, STP, false, VS>(p, g, o, t * kTile + lane_off, nvec, nlr, wd, L);
}

// Block 0 (dispatched first) takes the last partial tile and the < E scalar
// tail; blocks 1.. one full tile each (grid-strided when the grid is smaller).
// No __restrict__: `out` may be `p` or `g`.
template <class Op, int VPT, int STP, bool WAVEMAP>
__global__ __launch_bounds__(kBlock) void k_sgd_tiles(const void* p, const void* g, void* out, size_t nvec,
                                                      size_t nelem, wt_t<Op> nlr, wt_t<Op> wd, CpuLayout L) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  const size_t full = nvec / kTile;
  const OutRef o = make_out<STP>(out, nvec);
  const size_t nb = gridDim.x;
  if (blockIdx.x == 0) {
    if (full * kTile < nvec)
      sgd_tile<Op, VPT, true, STP, true>(p, g, o, full * kTile + threadIdx.x, nvec, nlr, wd, L);
    const size_t j = nvec * Op::E + threadIdx.x;
    if (j < nelem) sgd_scalar_elem<Op>(p, g, out, j, nlr, wd, L);
    if (nb > 1) return;
  }
  const size_t workers = nb > 1 ? nb - 1 : 1;
  const size_t first = nb > 1 ? blockIdx.x - 1 : 0;
  for (size_t t = first; t < full; t += workers) sgd_full_tile<Op, VPT, STP, WAVEMAP>(p, g, o, t, nvec, nlr, wd, L);
}

// ---- many tensors in one grid (dlsim_sgd_step_tensors) -------------------------
// A model's gradients arrive as a list of separate tensors, some of ten
// elements: one grid covers up to kSgdMaxTensors (param, grad, out) triples,
// described in the kernel arguments (scalar loads at a wave-uniform index).
// Tensor t owns blocks [block_start[t], block_start[t + 1]): with all three
// bases 16-byte aligned, its first block takes the ragged end and block k >= 1
// full tile k - 1, as k_sgd_tiles; otherwise every block takes a tile's worth
// of elements one at a time. The host lays the blocks out by the same rule
// (sgd_tensor_blocks). Element for element the arithmetic is k_sgd_tiles' and
// k_sgd_scalar's, so a batch equals its tensors' single calls bit for bit.
constexpr int kSgdMaxTensors = 64;

struct SgdSlots {
  const void* p[kSgdMaxTensors];
  const void* g[kSgdMaxTensors];
  void* out[kSgdMaxTensors];
  size_t nelem[kSgdMaxTensors];
  size_t chunk[kSgdMaxTensors];  // CpuLayout::chunk per tensor
  uint32_t block_start[kSgdMaxTensors + 1];
  int ntensors;
};
static_assert(sizeof(SgdSlots) <= 4096, "kernel arguments");

__host__ __device__ inline bool sgd_aligned16(const void* p, const void* g, const void* out) {
  return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
}

// blocks of one tensor in a VPT batch
template <class Op>
__host__ __device__ inline size_t sgd_tensor_blocks(const void* p, const void* g, const void* out, size_t nelem,
                                                    int vpt) {
  const size_t tile = static_cast<size_t>(kBlock) * static_cast<size_t>(vpt);
  if (sgd_aligned16(p, g, out)) return nelem / Op::E / tile + 1;
  return (nelem + tile * Op::E - 1) / (tile * Op::E);
}

template <class Op, int VPT>
__global__ __launch_bounds__(kBlock) void k_sgd_batch(const SgdSlots s, wt_t<Op> nlr, wt_t<Op> wd) {
  const uint32_t bid = blockIdx.x;
  int t = 0;
#pragma unroll
  for (int j = 1; j < kSgdMaxTensors; ++j) t += (j < s.ntensors && bid >= s.block_start[j]) ? 1 : 0;
  const size_t local = bid - s.block_start[t];
  const void* p = s.p[t];
  const void* g = s.g[t];
  void* out = s.out[t];
  const size_t nelem = s.nelem[t];
  const CpuLayout L{nelem, s.chunk[t], 0};
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  if (!sgd_aligned16(p, g, out)) {
    const size_t j0 = local * kTile * Op::E + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < VPT * Op::E; ++k) {
      const size_t j = j0 + static_cast<size_t>(k) * kBlock;
      if (j < nelem) sgd_scalar_elem<Op>(p, g, out, j, nlr, wd, L);
    }
    return;
  }
  const size_t nvec = nelem / Op::E;
  const size_t full = nvec / kTile;
  const OutRef o = make_out<kStNT>(out, nvec);
  if (local == 0) {
    if (full * kTile < nvec)
      sgd_tile<Op, VPT, true, kStNT, true>(p, g, o, full * kTile + threadIdx.x, nvec, nlr, wd, L);
    const size_t j = nvec * Op::E + threadIdx.x;
    if (j < nelem) sgd_scalar_elem<Op>(p, g, out, j, nlr, wd, L);
    return;
  }
  sgd_full_tile<Op, VPT, kStNT, false>(p, g, o, local - 1, nvec, nlr, wd, L);
}

}  // namespace dlsim
