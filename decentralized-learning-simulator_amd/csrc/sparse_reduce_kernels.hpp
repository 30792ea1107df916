// sparse_reduce_kernels.hpp — gfx950 kernel for mixing one dense model with
// top-k sparsified neighbours (dlsim_sparse_wreduce and its batched form;
// DESIGN.md §8r). The reference has no such code: it shares dense models only.
//
// Contract: out[e] holds the bits of the exact weighted reduce
// (wreduce_kernels.hpp, DLSIM_EXACT) over n = m + 1 rows, row 0 the dense row
// `self` and row j the neighbour j densified: val_j at the position of e in
// idx_j, self[e] where e is absent. The arithmetic is the element policy's
// (F32Exact, BF16Exact: init, step, step2, pack), not restated here.
//
// A block owns a run of consecutive tiles of kBlock * E * kSparseVpt
// coordinates. Per tile:
//   1. the tile of self is staged once, into two LDS tiles: `base`, which
//      stays, and `ovl`, which neighbours overlay;
//   2. lane j < m finds the tile's range [lo, hi) of neighbour j's list by a
//      lower-bound search (all neighbours at once; hi is searched only among
//      the next tile-length entries, the indices being strictly ascending, and
//      is the next tile's lo, so a block runs one full search per neighbour);
//   3. the accumulators (registers, one 16-byte vector per lane and row) take
//      x0 * 0 and self's term from `base`;
//   4. per neighbour, in input order: its values of the tile are written over
//      `ovl`, the tile is folded into the accumulators, the written slots are
//      restored from `base`. A neighbour without an entry in the tile folds
//      `ovl` as it stands, between no barriers.
// Dense traffic is self once and out once, sparse traffic each list once.
// An index is only ever used after `index - tile start < tile length` held as
// an unsigned comparison, so a value outside [0, P) is never dereferenced and
// nothing outside out is written, whatever the lists hold. out may be self: a
// tile is read completely before it is written, and tiles are disjoint.
//
// The vector form moves self and out as 16-byte vectors; the scalar form (a
// base off 16-byte alignment) moves them element by element, the results
// passing through `ovl`. Both fold the same LDS tiles the same way.
#pragma once

#include "wreduce_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kSparseVpt = 2;                // rows of kBlock vectors per tile
constexpr unsigned kSparseMaxBlocks = 1024;  // of one task's virtual grid
constexpr int kSparseMaxTasks = 32;          // tasks of one launch
constexpr int kSparseMaxSlots = 80;          // neighbours of one launch, over all its tasks
constexpr int kSparseMaxNeighbours = 31;     // of one task: 32 rows with self

struct SparseTask {
  const void* self;
  void* out;
  uint32_t nelem;
  uint32_t block_start;  // first block of the task in the launch
  uint32_t tpb;          // tiles per block of its virtual grid
  uint32_t slot_off;     // its first neighbour slot
  uint32_t m;            // neighbours
  float w0;              // self's weight
};

struct SparseBatch {
  int ntasks;
  SparseTask t[kSparseMaxTasks];
  const int32_t* idx[kSparseMaxSlots];
  const void* val[kSparseMaxSlots];
  uint32_t k[kSparseMaxSlots];
  float w[kSparseMaxSlots];
};

template <class Op> struct SparseElem { using type = uint32_t; };
template <> struct SparseElem<BF16Exact> { using type = uint16_t; };

template <class Op>
__device__ __forceinline__ float sparse_widen(typename SparseElem<Op>::type b) {
  if constexpr (Op::kBytes == 4) return __uint_as_float(b);
  else return __uint_as_float(static_cast<uint32_t>(b) << 16);
}

// first p in [a, b) with idx[p] >= target, else b
__device__ __forceinline__ uint32_t sparse_lower_bound(const int32_t* idx, uint32_t a, uint32_t b, int64_t target) {
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (idx[mid] < target) a = mid + 1;
    else b = mid;
  }
  return a;
}

template <class Op, bool VEC>
__global__ __launch_bounds__(kBlock) void k_sparse_wreduce(const SparseBatch B) {
  using Elem = typename SparseElem<Op>::type;
  constexpr int E = Op::E;
  constexpr uint32_t kTile = static_cast<uint32_t>(kBlock) * E * kSparseVpt;
  __shared__ __attribute__((aligned(16))) Elem s_base[kTile];
  __shared__ __attribute__((aligned(16))) Elem s_ovl[kTile];
  __shared__ uint32_t s_lo[kSparseMaxNeighbours + 1], s_hi[kSparseMaxNeighbours + 1];
  const int tid = threadIdx.x;
  int ti = 0;
  for (int i = 1; i < B.ntasks; ++i)
    if (B.t[i].block_start <= blockIdx.x) ti = i;
  const SparseTask& T = B.t[ti];
  const uint32_t P = T.nelem, s0 = T.slot_off;
  const int m = static_cast<int>(T.m);
  const Elem* const self = static_cast<const Elem*>(T.self);
  Elem* const out = static_cast<Elem*>(T.out);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x - T.block_start) * T.tpb;
  if (tid < m) s_hi[tid] = sparse_lower_bound(B.idx[s0 + tid], 0, B.k[s0 + tid], static_cast<int64_t>(tile0 * kTile));
  for (uint32_t tt = 0; tt < T.tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kTile;
    if (c64 >= P) break;  // block-uniform
    const uint32_t c0 = static_cast<uint32_t>(c64);
    const uint32_t len = P - c0 < kTile ? P - c0 : kTile;
    const uint32_t nfull = len / E, rem = len - nfull * E;
    // 1. stage self
    if constexpr (VEC) {
#pragma unroll
      for (int r = 0; r < kSparseVpt; ++r) {
        const uint32_t lv = r * kBlock + tid;
        if (lv < nfull) {
          const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(self + c0) + lv);
          reinterpret_cast<u32x4*>(s_base)[lv] = v;
          reinterpret_cast<u32x4*>(s_ovl)[lv] = v;
        }
      }
      if (static_cast<uint32_t>(tid) < rem) s_base[nfull * E + tid] = s_ovl[nfull * E + tid] = self[c0 + nfull * E + tid];
    } else {
      for (uint32_t i = tid; i < len; i += kBlock) s_base[i] = s_ovl[i] = self[c0 + i];
    }
    // 2. the tile's range of every neighbour's list
    if (tid < m) {
      const uint32_t lo = s_hi[tid], kk = B.k[s0 + tid];
      s_lo[tid] = lo;
      s_hi[tid] = sparse_lower_bound(B.idx[s0 + tid], lo, kk - lo < len ? kk : lo + len, static_cast<int64_t>(c0) + len);
    }
    __syncthreads();
    // 3. x0 * 0, then self's term
    float acc[kSparseVpt][E], acc_tail = 0.0f;
    const auto fold = [&](const Elem* src, float w, bool first) {
#pragma unroll
      for (int r = 0; r < kSparseVpt; ++r) {
        const uint32_t lv = r * kBlock + tid;
        if (lv < nfull) {
          float x[E];
          unpack<Op>(reinterpret_cast<const u32x4*>(src)[lv], x);
          if (first) {
#pragma unroll
            for (int e = 0; e < E; ++e) acc[r][e] = Op::init(x[e]);
          }
#pragma unroll
          for (int e = 0; e < E; e += 2) Op::step2(acc[r][e], acc[r][e + 1], w, x[e], x[e + 1]);
        }
      }
      if (static_cast<uint32_t>(tid) < rem) {
        const float x = sparse_widen<Op>(src[nfull * E + tid]);
        if (first) acc_tail = Op::init(x);
        acc_tail = Op::step(acc_tail, w, x);
      }
    };
    fold(s_base, T.w0, true);
    // 4. the neighbours, in input order
    for (int j = 0; j < m; ++j) {
      const uint32_t lo = s_lo[j], hi = s_hi[j];
      const int32_t* const ip = B.idx[s0 + j];
      const Elem* const vp = static_cast<const Elem*>(B.val[s0 + j]);
      if (hi > lo) {
        __syncthreads();  // every lane has folded the tile as it stood
        for (uint32_t p = lo + tid; p < hi; p += kBlock) {
          const uint32_t off = static_cast<uint32_t>(ip[p]) - c0;
          if (off < len) s_ovl[off] = vp[p];
        }
        __syncthreads();
      }
      fold(s_ovl, B.w[s0 + j], false);
      if (hi > lo) {
        __syncthreads();
        for (uint32_t p = lo + tid; p < hi; p += kBlock) {
          const uint32_t off = static_cast<uint32_t>(ip[p]) - c0;
          if (off < len) s_ovl[off] = s_base[off];
        }
        __syncthreads();
      }
    }
    // store
    if constexpr (VEC) {
#pragma unroll
      for (int r = 0; r < kSparseVpt; ++r) {
        const uint32_t lv = r * kBlock + tid;
        if (lv < nfull) __builtin_nontemporal_store(pack<Op>(acc[r], 1.0f), reinterpret_cast<u32x4*>(out + c0) + lv);
      }
      if (static_cast<uint32_t>(tid) < rem) store_elem<Op>(out + c0, nfull * E + tid, acc_tail, 1.0f);
      __syncthreads();  // the next tile restages base and ovl, and rewrites the ranges
    } else {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kSparseVpt; ++r) {
        const uint32_t lv = r * kBlock + tid;
        if (lv < nfull) reinterpret_cast<u32x4*>(s_ovl)[lv] = pack<Op>(acc[r], 1.0f);
      }
      if (static_cast<uint32_t>(tid) < rem) store_elem<Op>(s_ovl, nfull * E + tid, acc_tail, 1.0f);
      __syncthreads();
      for (uint32_t i = tid; i < len; i += kBlock) out[c0 + i] = s_ovl[i];
      __syncthreads();
    }
  }
}

}  // namespace dlsim
