// sgdm_kernels.hpp — gfx950 streaming kernels for every step of the SGD the
// reference configures (SGDOptimizer, dasklearn/optimizer/sgd.py, stepped by
// ModelTrainer.train, model_trainer.py:89-92,126): momentum > 0, dampening 0,
// no Nesterov. Per parameter tensor torch's CPU path
// (torch.optim.sgd._single_tensor_sgd) runs
//   g'  = grad.add(param, alpha=weight_decay)   (only if weight_decay != 0)
//   buf = clone(g')                             (this parameter's first step)
//   buf = buf.mul_(momentum).add_(g', alpha=1)  (every later step)
//   param.add_(buf, alpha=-lr)
// Three input streams (two on a first step), two output streams: HBM-bound,
// built like the fresh-SGD step's kernels (sgd_kernels.hpp): 16-byte
// non-temporal loads per lane, every load of a tile issued before the first
// use, 16-byte stores of both results, block 0 folding the ragged end.
//
// Rounding contract, per element:
//   fp32: g' = fma(f32(wd), p, g); buf' = f32(f32(m) * buf) + g' (a rounded
//         product, then a plain add: NOT fused); p' = fma(-f32(lr), buf', p)
//   fp64: the same in double with the exact double scalars
//   bf16: the two alpha adds as sgd_kernels.hpp (scalars rounded to bf16; one
//         rounding in ATen's vector body, the product rounded too in its
//         scalar tail, CpuLayout); the momentum scalar stays fp32: the product
//         in fp32 rounded to bf16, the sum in fp32 rounded to bf16, wherever
//         the element lies.
// The library is built with -ffp-contract=off; the product and the sum of the
// buffer update are two statements under the pragma below all the same.
#pragma once

#include "sgd_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

template <class W>
struct SgdmArgs {
  W nlr, mom, wd;
};

// ---- element policies -------------------------------------------------------
// (names outside scripts/audit_isa.py's POLICIES: these kernels fuse by
// contract in the two alpha adds). FIRST: no buffer yet, buf' = g'.
// upd(p, b, g, a): p and b (the buffer read; unused when FIRST) become p', buf'.
template <bool WD, bool FIRST>
struct SgdmF32 {
  static constexpr int E = 4;
  static constexpr int kBytes = 4;
  static constexpr int kFmt = kFmtF32;
  static constexpr bool kCpuTails = false;
  static constexpr bool kFirst = FIRST;
  __device__ static void upd(float& p, float& b, float g, const SgdmArgs<float>& a) {
    if constexpr (WD) g = __builtin_fmaf(a.wd, p, g);
    if constexpr (!FIRST) {
      const float mb = a.mom * b;
      g = mb + g;
    }
    b = g;
    p = __builtin_fmaf(a.nlr, g, p);
  }
  __device__ static float finish(float a, float) { return a; }
};

template <bool WD, bool FIRST>
struct SgdmF64 {
  using T = double;
  using W = double;
  static constexpr int E = 2;
  static constexpr int kBytes = 8;
  static constexpr int kFmt = kFmtF32;
  static constexpr bool kCpuTails = false;
  static constexpr bool kFirst = FIRST;
  __device__ static void upd(double& p, double& b, double g, const SgdmArgs<double>& a) {
    if constexpr (WD) g = __builtin_fma(a.wd, p, g);
    if constexpr (!FIRST) {
      const double mb = a.mom * b;
      g = mb + g;
    }
    b = g;
    p = __builtin_fma(a.nlr, g, p);
  }
  __device__ static double finish(double a, float) { return a; }
};

template <bool WD, bool FIRST>
struct SgdmBF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtBF16;
  static constexpr bool kCpuTails = true;
  static constexpr bool kFirst = FIRST;
  // mul_(momentum) keeps the scalar in fp32; product and sum each computed in
  // fp32 and rounded to bf16 (the same in ATen's vector body and scalar loop)
  __device__ static float buf_upd(float b, float g, float mom) {
    const float mb = sgd_bf16_round(mom * b);
    return sgd_bf16_round(mb + g);
  }
  // ATen's vector body: each alpha add in fp32, its result rounded to bf16
  __device__ static void upd(float& p, float& b, float g, const SgdmArgs<float>& a) {
    if constexpr (WD) g = sgd_bf16_round(__builtin_fmaf(a.wd, p, g));
    if constexpr (!FIRST) g = buf_upd(b, g, a.mom);
    b = g;
    p = sgd_bf16_round(__builtin_fmaf(a.nlr, g, p));
  }
  // two elements at a time (one v_cvt_pk_bf16_f32 per rounding)
  __device__ static void upd2(float& p0, float& p1, float& b0, float& b1, float g0, float g1,
                              const SgdmArgs<float>& a) {
    if constexpr (WD) {
      g0 = __builtin_fmaf(a.wd, p0, g0);
      g1 = __builtin_fmaf(a.wd, p1, g1);
      bf16_round2(g0, g1);
    }
    if constexpr (!FIRST) {
      float m0 = a.mom * b0, m1 = a.mom * b1;
      bf16_round2(m0, m1);
      g0 = m0 + g0;
      g1 = m1 + g1;
      bf16_round2(g0, g1);
    }
    b0 = g0;
    b1 = g1;
    p0 = __builtin_fmaf(a.nlr, g0, p0);
    p1 = __builtin_fmaf(a.nlr, g1, p1);
    bf16_round2(p0, p1);
  }
  // ATen's scalar loop: c10::BFloat16 arithmetic, `x + alpha * y` with the
  // product and the sum each rounded to bf16
  __device__ static void upd_tail(float& p, float& b, float g, const SgdmArgs<float>& a) {
    if constexpr (WD) g = sgd_bf16_round(g + sgd_bf16_round(a.wd * p));
    if constexpr (!FIRST) g = buf_upd(b, g, a.mom);
    b = g;
    p = sgd_bf16_round(p + sgd_bf16_round(a.nlr * g));
  }
  __device__ static float finish(float a, float) { return a; }
};

template <class Op>
__device__ __forceinline__ void sgdm_elem(acc_t<Op>& p, acc_t<Op>& b, acc_t<Op> g, const SgdmArgs<wt_t<Op>>& a,
                                          const CpuLayout& L, size_t j) {
  if constexpr (Op::kCpuTails) {
    if (cpu_tail(L, j)) {
      Op::upd_tail(p, b, g, a);
      return;
    }
  }
  Op::upd(p, b, g, a);
}

// One element, any alignment. pout may be p and bout may be b (the lane reads
// the element of every stream before it writes).
template <class Op>
__device__ __forceinline__ void sgdm_scalar_elem(const void* p, const void* g, const void* b, void* pout, void* bout,
                                                 size_t j, const SgdmArgs<wt_t<Op>>& a, const CpuLayout& L) {
  acc_t<Op> xp = load_elem<Op>(p, j);
  const acc_t<Op> xg = load_elem<Op>(g, j);
  acc_t<Op> xb = 0;
  if constexpr (!Op::kFirst) xb = load_elem<Op>(b, j);
  sgdm_elem<Op>(xp, xb, xg, a, L, j);
  store_elem<Op>(pout, j, xp, 1.0f);
  store_elem<Op>(bout, j, xb, 1.0f);
}

template <class Op>
__global__ __launch_bounds__(kBlock) void k_sgdm_scalar(const void* p, const void* g, const void* b, void* pout,
                                                        void* bout, size_t nelem, SgdmArgs<wt_t<Op>> a, CpuLayout L) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < nelem) sgdm_scalar_elem<Op>(p, g, b, pout, bout, j, a, L);
}

// One tile: lane's vectors v0 + k*VS, all streams' loads issued before the
// first use (VPT 4: 48 VGPRs of loads in flight per lane, 32 on a first step).
// TAILS: some element of the tile may be in a scalar tail.
template <class Op, int VPT, bool CHECK, int STP, bool TAILS, int VS = kBlock>
__device__ __forceinline__ void sgdm_tile(const void* p, const void* g, const void* b, const OutRef& op,
                                          const OutRef& ob, size_t v0, size_t nvec, const SgdmArgs<wt_t<Op>>& a,
                                          const CpuLayout& L) {
  u32x4 rp[VPT], rg[VPT], rb[VPT];
  load_tile<Op, VPT, 1, CHECK, VS>(p, v0, nvec, rp);
  load_tile<Op, VPT, 1, CHECK, VS>(g, v0, nvec, rg);
  if constexpr (!Op::kFirst) load_tile<Op, VPT, 1, CHECK, VS>(b, v0, nvec, rb);
#pragma unroll
  for (int v = 0; v < VPT; ++v) {
    const size_t idx = v0 + static_cast<size_t>(v) * VS;
    acc_t<Op> xp[Op::E], xg[Op::E], xb[Op::E];
    unpack<Op>(rp[v], xp);
    unpack<Op>(rg[v], xg);
    if constexpr (!Op::kFirst) {
      unpack<Op>(rb[v], xb);
    } else {
#pragma unroll
      for (int e = 0; e < Op::E; ++e) xb[e] = 0;
    }
    if constexpr (TAILS && Op::kCpuTails) {
#pragma unroll
      for (int e = 0; e < Op::E; ++e) sgdm_elem<Op>(xp[e], xb[e], xg[e], a, L, idx * Op::E + e);
    } else if constexpr (Op::kBytes == 2) {
#pragma unroll
      for (int e = 0; e < Op::E; e += 2) Op::upd2(xp[e], xp[e + 1], xb[e], xb[e + 1], xg[e], xg[e + 1], a);
    } else {
#pragma unroll
      for (int e = 0; e < Op::E; ++e) Op::upd(xp[e], xb[e], xg[e], a);
    }
    if (!CHECK || idx < nvec) {
      store_vec<STP>(op, idx, pack<Op>(xp, 1.0f));
      store_vec<STP>(ob, idx, pack<Op>(xb, 1.0f));
    }
  }
}

template <class Op, int VPT, int STP, bool WAVEMAP>
__device__ __forceinline__ void sgdm_full_tile(const void* p, const void* g, const void* b, const OutRef& op,
                                               const OutRef& ob, size_t t, size_t nvec, const SgdmArgs<wt_t<Op>>& a,
                                               const CpuLayout& L) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  constexpr int VS = WAVEMAP ? 64 : kBlock;
  const size_t lane_off = WAVEMAP ? (threadIdx.x >> 6) * 64 * VPT + (threadIdx.x & 63) : threadIdx.x;
  if constexpr (Op::kCpuTails) {
    // uniform per block: a tile that touches a scalar tail decides per element
    if (!cpu_body(L, t * kTile * Op::E, (t + 1) * kTile * Op::E)) {
      sgdm_tile<Op, VPT, false, STP, true, VS>(p, g, b, op, ob, t * kTile + lane_off, nvec, a, L);
      return;
    }
  }
  sgdm_tile<Op, VPT, false, STP, false, VS>(p, g, b, op, ob, t * kTile + lane_off, nvec, a, L);
}

// The ragged end of a buffer: the last partial tile and the < E scalar tail.
template <class Op, int VPT, int STP>
__device__ __forceinline__ void sgdm_ragged(const void* p, const void* g, const void* b, void* pout, void* bout,
                                            const OutRef& op, const OutRef& ob, size_t nvec, size_t nelem,
                                            const SgdmArgs<wt_t<Op>>& a, const CpuLayout& L) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  const size_t full = nvec / kTile;
  if (full * kTile < nvec)
    sgdm_tile<Op, VPT, true, STP, true>(p, g, b, op, ob, full * kTile + threadIdx.x, nvec, a, L);
  const size_t j = nvec * Op::E + threadIdx.x;
  if (j < nelem) sgdm_scalar_elem<Op>(p, g, b, pout, bout, j, a, L);
}

// Block 0 (dispatched first) takes the ragged end; blocks 1.. one full tile
// each (grid-strided when the grid is smaller). No __restrict__: pout may be
// p and bout may be b.
template <class Op, int VPT, int STP, bool WAVEMAP>
__global__ __launch_bounds__(kBlock) void k_sgdm_tiles(const void* p, const void* g, const void* b, void* pout,
                                                       void* bout, size_t nvec, size_t nelem, SgdmArgs<wt_t<Op>> a,
                                                       CpuLayout L) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  const size_t full = nvec / kTile;
  const OutRef op = make_out<STP>(pout, nvec);
  const OutRef ob = make_out<STP>(bout, nvec);
  const size_t nb = gridDim.x;
  if (blockIdx.x == 0) {
    sgdm_ragged<Op, VPT, STP>(p, g, b, pout, bout, op, ob, nvec, nelem, a, L);
    if (nb > 1) return;
  }
  const size_t workers = nb > 1 ? nb - 1 : 1;
  const size_t first = nb > 1 ? blockIdx.x - 1 : 0;
  for (size_t t = first; t < full; t += workers)
    sgdm_full_tile<Op, VPT, STP, WAVEMAP>(p, g, b, op, ob, t, nvec, a, L);
}

// ---- many tensors in one grid (dlsim_sgd_momentum_step_tensors) ----------------
// As k_sgd_batch: one grid covers up to kSgdmMaxTensors (param, grad, buf,
// param_out, buf_out) tuples described in the kernel arguments. Five pointers,
// the length and the first block per tensor are 52 bytes, so 64 tensors take
// 3.3 KiB of the 4 KiB argument space (the bf16 range length is recomputed on
// the device, sgd_cpu_chunk). buf[t] == nullptr is that tensor's first step: a
// parameter that had no gradient on earlier steps gets its buffer later than
// its neighbours. Element for element the arithmetic is k_sgdm_tiles' and
// k_sgdm_scalar's, so a batch equals its tensors' single calls bit for bit.
constexpr int kSgdmMaxTensors = 64;

struct SgdmSlots {
  const void* p[kSgdmMaxTensors];
  const void* g[kSgdmMaxTensors];
  const void* b[kSgdmMaxTensors];
  void* pout[kSgdmMaxTensors];
  void* bout[kSgdmMaxTensors];
  size_t nelem[kSgdmMaxTensors];
  uint32_t block_start[kSgdmMaxTensors + 1];
  int ntensors;
};
static_assert(sizeof(SgdmSlots) + 3 * sizeof(double) + 256 <= 4096, "kernel arguments (with the hidden ones)");

__host__ __device__ inline bool sgdm_aligned16(const void* p, const void* g, const void* b, const void* pout,
                                               const void* bout) {
  return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(b) |
           reinterpret_cast<uintptr_t>(pout) | reinterpret_cast<uintptr_t>(bout)) & 15u) == 0;
}

// blocks of one tensor in a VPT batch (b == nullptr counts as aligned)
template <class Op>
__host__ __device__ inline size_t sgdm_tensor_blocks(const void* p, const void* g, const void* b, const void* pout,
                                                     const void* bout, size_t nelem, int vpt) {
  const size_t tile = static_cast<size_t>(kBlock) * static_cast<size_t>(vpt);
  if (sgdm_aligned16(p, g, b, pout, bout)) return nelem / Op::E / tile + 1;
  return (nelem + tile * Op::E - 1) / (tile * Op::E);
}

template <class Op, int VPT>
__device__ __forceinline__ void sgdm_batch_block(const void* p, const void* g, const void* b, void* pout, void* bout,
                                                 size_t nelem, size_t local, const SgdmArgs<wt_t<Op>>& a) {
  const CpuLayout L{nelem, Op::kCpuTails ? sgd_cpu_chunk(nelem, kSgdCpuThreads) : 1, 0};
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  if (!sgdm_aligned16(p, g, b, pout, bout)) {
    const size_t j0 = local * kTile * Op::E + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < VPT * Op::E; ++k) {
      const size_t j = j0 + static_cast<size_t>(k) * kBlock;
      if (j < nelem) sgdm_scalar_elem<Op>(p, g, b, pout, bout, j, a, L);
    }
    return;
  }
  const size_t nvec = nelem / Op::E;
  const OutRef op = make_out<kStNT>(pout, nvec);
  const OutRef ob = make_out<kStNT>(bout, nvec);
  if (local == 0) {
    sgdm_ragged<Op, VPT, kStNT>(p, g, b, pout, bout, op, ob, nvec, nelem, a, L);
    return;
  }
  sgdm_full_tile<Op, VPT, kStNT, false>(p, g, b, op, ob, local - 1, nvec, a, L);
}

// OpFirst / OpLater: the two forms of one (dtype, weight decay) policy
template <class OpFirst, class OpLater, int VPT>
__global__ __launch_bounds__(kBlock) void k_sgdm_batch(const SgdmSlots s, SgdmArgs<wt_t<OpLater>> a) {
  const uint32_t bid = blockIdx.x;
  int t = 0;
#pragma unroll
  for (int j = 1; j < kSgdmMaxTensors; ++j) t += (j < s.ntensors && bid >= s.block_start[j]) ? 1 : 0;
  const size_t local = bid - s.block_start[t];
  const void* b = s.b[t];
  if (b == nullptr)
    sgdm_batch_block<OpFirst, VPT>(s.p[t], s.g[t], nullptr, s.pout[t], s.bout[t], s.nelem[t], local, a);
  else
    sgdm_batch_block<OpLater, VPT>(s.p[t], s.g[t], b, s.pout[t], s.bout[t], s.nelem[t], local, a);
}

}  // namespace dlsim
