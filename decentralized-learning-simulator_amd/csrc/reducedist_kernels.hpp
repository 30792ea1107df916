// reducedist_kernels.hpp — gfx950 kernels for "reduce and measure": the exact
// weighted reduce of n flat buffers and, in the same pass over them, every
// input's squared L2 distance to the reduce's own output. The
// primitive under the geometric median (smoothed Weiszfeld) and centered
// clipping (gradient_aggregation/geomed.py), and the consensus distance to the
// weighted mean. The reference has no such code: its one aggregator is FedAvg
// (dasklearn/gradient_aggregation/fedavg.py).
//
// Contract, per element e and input i:
//   out[e] = the DLSIM_EXACT fold of wreduce_kernels.hpp: acc = x_0[e] * 0, then
//            acc = fl(acc + fl(w_i * x_i[e])) in input order, through the same
//            element policies (F32Exact, F64Exact, BF16Exact, F16Exact), so
//            the arithmetic is shared by construction;
//   d2[i]  = sum_e (double(x_i[e]) - double(out[e]))^2 with out[e] the stored,
//            rounded value, the subtraction in double and each term entering
//            its accumulator with one explicit fma(d, d, acc). The unit is
//            built with -ffp-contract=off; the fma is written out, hence the
//            policy names outside scripts/audit_isa.py's POLICIES.
//
// While a lane folds an element it holds all n values of that element in
// registers, so the n differences cost no further memory traffic: one pass
// over HBM where a reduce followed by a distance kernel takes two.
//
// Register plan. A lane takes W bytes of every row per tile and keeps
// n * W <= 128 bytes of rows beside n double accumulators:
//   n <= 4, n <= 8   W = 16  (the tiled reduce's shape; CAP 4 or 8)
//   n <= 16          W = 8   (CAP 16)
//   n <= 32          W = 4   (CAP 32; fp64: 8, one element)
// so every fan-in reads each row exactly once and the rows in flight per lane
// stay at <= 32 VGPRs (64 for fp64 at n > 16) beside <= 64 of accumulators.
// CAP is compile-time (accumulators and rows indexed by constants stay in
// registers); rows i >= n of a CAP load nothing and are never read. All loads
// of a tile issue before the first use.
//
// The summation order of d2 is pairdist's (pairdist_kernels.hpp), whose block
// end and finish sum this file calls: per lane over the tiles its block
// strides over, the 64 lanes of a wave (xor butterfly), the four waves in wave
// order, then in k_reducedist_finish the blocks (lane l adds blocks l, l + 64,
// ... in order, then the butterfly). No atomics; the grid is a function of
// (n, dtype, n_elems, alignment class) alone.
#pragma once

#include "pairdist_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kRdMaxInputs = 32;
static_assert(kRdMaxInputs <= kPdSlots, "one partial sum per input and block");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---- policies -------------------------------------------------------------------
// Fold: the exact element policy whose init / step / step2 / finish make out[e].
struct RdF32 {
  using Fold = F32Exact;
};
struct RdF64 {
  using Fold = F64Exact;
};
struct RdBF16 {
  using Fold = BF16Exact;
};
struct RdF16 {
  using Fold = F16Exact;
};

// Pointers and weights travel in the kernarg segment (scalar loads). rd_tile
// reads them through ptr(i) / wt(i), so that a segment of a batched launch
// (RdTaskArgs, reducedist_batch_kernels.hpp) can stand in for the flat call's.
template <class W>
struct RdSlots {
  const void* p[kRdMaxInputs];
  W w[kRdMaxInputs];
  __device__ const void* ptr(int i) const { return p[i]; }
  __device__ W wt(int i) const { return w[i]; }
};

// bytes a lane takes of one row per tile on the vector path
constexpr int rd_width_bytes(int elem_bytes, int cap) {
  const int w = cap <= 8 ? 16 : cap <= 16 ? 8 : 4;
  return w < elem_bytes ? elem_bytes : w;
}
template <class Op, int CAP>
constexpr int rd_width() {
  return rd_width_bytes(Op::Fold::kBytes, CAP);
}

// WB bytes at item idx, in the low dwords of a 16-byte vector (the rest zero,
// never used: unpack's work on them folds away)
template <int WB>
__device__ __forceinline__ u32x4 rd_ld(const void* p, size_t idx) {
  if constexpr (WB == 16) {
    return ld16<1>(p, idx);
  } else if constexpr (WB == 8) {
    const u32x2 v = __builtin_nontemporal_load(static_cast<const u32x2*>(p) + idx);
    return u32x4{v[0], v[1], 0u, 0u};
  } else {
    const uint32_t v = __builtin_nontemporal_load(static_cast<const uint32_t*>(p) + idx);
    return u32x4{v, 0u, 0u, 0u};
  }
}

template <int WB>
__device__ __forceinline__ void rd_st(void* p, size_t idx, const u32x4& r) {
  // The 16-byte store is plain, the 8- and 4-byte ones are non-temporal. Three runs
  // with three policies did not separate them: the runs differ by as much as the
  // policies.
  if constexpr (WB == 16) {
    st16<false>(p, idx, r);
  } else if constexpr (WB == 8) {
    __builtin_nontemporal_store(u32x2{r[0], r[1]}, static_cast<u32x2*>(p) + idx);
  } else {
    __builtin_nontemporal_store(r[0], static_cast<uint32_t*>(p) + idx);
  }
}

// One item (W bytes, or one element when !VEC) per lane and row: all loads,
// the fold in input order, the store, then per row and element one
// subtraction and one fma. CHECK: lanes at idx >= count load, store and add
// nothing.
template <class Op, int CAP, bool VEC, bool CHECK, class S>
__device__ __forceinline__ void rd_tile(const S& s, int n, void* __restrict__ out, size_t idx, size_t count,
                                        double (&acc)[CAP]) {
  using F = typename Op::Fold;
  using T = acc_t<F>;
  constexpr int WB = rd_width<Op, CAP>();
  constexpr int EV = VEC ? WB / F::kBytes : 1;
  const bool live = !CHECK || idx < count;
  T x[CAP][EV];
  if constexpr (VEC) {
    u32x4 r[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
      r[i] = u32x4{0u, 0u, 0u, 0u};
      if (i < n && live) r[i] = rd_ld<WB>(s.ptr(i), idx);
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
      T full[F::E];
      unpack<F>(r[i], full);
#pragma unroll
      for (int e = 0; e < EV; ++e) x[i][e] = full[e];
    }
  } else {
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
      x[i][0] = 0;
      if (i < n && live) x[i][0] = load_elem<F>(s.ptr(i), idx);
    }
  }
  T a[EV];
#pragma unroll
  for (int e = 0; e < EV; ++e) a[e] = F::init(x[0][e]);
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < n) {
      if constexpr (EV == 1) {
        a[0] = F::step(a[0], s.wt(i), x[i][0]);
      } else {
#pragma unroll
        for (int e = 0; e < EV; e += 2) F::step2(a[e], a[e + 1], s.wt(i), x[i][e], x[i][e + 1]);
      }
    }
  if (live) {
    if (out) {
      if constexpr (VEC) {
        T full[F::E];
#pragma unroll
        for (int e = 0; e < F::E; ++e) full[e] = a[e < EV ? e : 0];  // the first W bytes are stored
        rd_st<WB>(out, idx, pack<F>(full, 1.0f));
      } else {
        store_elem<F>(out, idx, a[0], 1.0f);
      }
    }
    double o[EV];
#pragma unroll
    for (int e = 0; e < EV; ++e) o[e] = static_cast<double>(F::finish(a[e], 1.0f));  // the stored value
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < n) {
#pragma unroll
        for (int e = 0; e < EV; ++e) {
          const double d = static_cast<double>(x[i][e]) - o[e];
          acc[i] = __builtin_fma(d, d, acc[i]);
        }
      }
  }
}

// Block b of nblk: it takes the full tiles b, b + nblk, ..., the partial tile
// goes to block (full tiles) mod nblk and the elements past the last whole
// item to the last block; every block stores its CAP partial sums to
// ws[i * nblk + b] (zeros where it had no tile, or for rows i >= n).
// out == nullptr: distances only. red: kBlock / 64 rows of kPdSlots.
template <class Op, int CAP, bool VEC, class S>
__device__ __forceinline__ void rd_block(const S& s, int n, void* __restrict__ out, size_t nelem,
                                         double* __restrict__ ws, size_t nblk, size_t b, double (*red)[kPdSlots]) {
  using F = typename Op::Fold;
  constexpr int EV = VEC ? rd_width<Op, CAP>() / F::kBytes : 1;
  double acc[CAP];
#pragma unroll
  for (int k = 0; k < CAP; ++k) acc[k] = 0.0;
  const size_t items = nelem / EV;  // whole vectors, or elements
  const size_t full = items / kBlock;
  for (size_t t = b; t < full; t += nblk)
    rd_tile<Op, CAP, VEC, false>(s, n, out, t * kBlock + threadIdx.x, items, acc);
  if (full * kBlock < items && full % nblk == b)
    rd_tile<Op, CAP, VEC, true>(s, n, out, full * kBlock + threadIdx.x, items, acc);
  if constexpr (VEC) {
    if (items * EV < nelem && b == nblk - 1)
      rd_tile<Op, CAP, false, true>(s, n, out, items * EV + threadIdx.x, nelem, acc);
  }
  pd_block_sum<CAP>(acc, ws, red, nblk, b);
}

// grid (blocks): rd_block over the launch's own grid.
template <class Op, int CAP, bool VEC>
__global__ __launch_bounds__(kBlock) void k_reducedist(const RdSlots<wt_t<typename Op::Fold>> s, int n,
                                                       void* __restrict__ out, size_t nelem,
                                                       double* __restrict__ ws) {
  static_assert(kBlock == 256, "four waves: the block-end sum names them");
  __shared__ double red[kBlock / 64][kPdSlots];
  rd_block<Op, CAP, VEC>(s, n, out, nelem, ws, gridDim.x, blockIdx.x, red);
}

// One wave per input: its partials of all blocks in pairdist's finish order.
// accumulate: the sum is added to what d2[i] holds, with pd_add_held (the sum
// first, the held value second: the operands `d2[i] + v` compiled to here
// before the batched kernels came, profiles/geomed_batch/finish_add_operands.md),
// so that this kernel and k_reducedist_batch_finish agree on NaN payloads too.
// (A template so that the header, included by two units, defines it once:
// launched as k_reducedist_finish<>.)
template <class = void>
__global__ __launch_bounds__(kBlock) void k_reducedist_finish(const double* __restrict__ ws, unsigned blocks, int n,
                                                              double* __restrict__ d2, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (i >= n) return;
  const double v = pd_finish_sum(ws + static_cast<size_t>(i) * blocks, blocks, lane);
  if (lane == 0) d2[i] = accumulate ? pd_add_held(v, d2[i]) : v;
}

}  // namespace dlsim
