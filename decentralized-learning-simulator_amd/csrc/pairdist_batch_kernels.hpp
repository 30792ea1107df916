// pairdist_batch_kernels.hpp — the pairwise squared-distance kernels
// (pairdist_kernels.hpp) over many independent matrices in one grid
// (DESIGN.md §8n): the Krum or Multi-Krum distances of one simulated round's
// peers. The shape of k_robust_batch (robust_batch_kernels.hpp): descriptors
// in the kernel arguments, the block index mapped to its piece of work through
// a prefix array.
//
// The unit of work is a segment: what one dlsim_pairwise_sqdist call is, n_s
// rows of nelem_s elements that add into one matrix. A matrix is one or more
// consecutive segments (a model's tensors). All segments of a launch share the
// flat kernel's class (the 4-row unit, the 8-row unit, or diagonal and cross
// units for n > 8) and its form (16-byte vectors, or element by element);
// each has its own fan-in, length, pointers and workspace offset.
//
// The flat kernel's summation order is a function of its grid alone. Segment s
// therefore owns units_s x blocks_s consecutive entries of the batch's grid,
// with blocks_s what the flat call's first grid dimension would be, and entry
// (u, b) runs pd_block with (blocks_s, b) in place of (gridDim.x, blockIdx.x):
// the same tiles, the same partials at the same workspace slots, bit for bit.
// k_pairdist_batch_finish then adds, per matrix and pair, the segments'
// partials in segment order, each with pd_finish_sum, as consecutive flat
// calls with accumulate = 1 would.
#pragma once

#include "pairdist_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kPdBatchMaxSegs = 32;
constexpr int kPdBatchMaxPtrs = 192;

// 32-bit fields and pointers only: they are read with scalar loads at a
// run-time (wave-uniform) index (RobBatchSlots). A segment fits one launch's
// 32-bit byte range, so its length fits 32 bits. Matrix m is the segments
// mat_seg[m] .. mat_seg[m + 1]; its fan-in is that of its first segment.
struct PdBatchSlots {
  const void* p[kPdBatchMaxPtrs];
  double* d2[kPdBatchMaxSegs];                // per matrix
  uint32_t block_start[kPdBatchMaxSegs + 1];  // first grid entry of each segment
  uint32_t blocks[kPdBatchMaxSegs];           // the segment's virtual first grid dimension
  uint32_t ws_off[kPdBatchMaxSegs];           // doubles from the launch's workspace to the segment's partials
  uint32_t nelem[kPdBatchMaxSegs];
  uint32_t ptr_off[kPdBatchMaxSegs];
  uint32_t fan_in[kPdBatchMaxSegs];
  uint32_t mat_seg[kPdBatchMaxSegs + 1];   // first segment of each matrix
  uint32_t mat_wave[kPdBatchMaxSegs + 1];  // first finish wave (pair) of each matrix
  uint32_t mat_acc[kPdBatchMaxSegs];       // 1: add to what the matrix holds
  int nsegs;
  int nmats;
};
static_assert(sizeof(PdBatchSlots) <= 4096, "kernel arguments");

// The last t < count with start[t] <= f, as a count over a compile-time range
// (batch_find_task's form: no dependent scan).
__device__ __forceinline__ int pd_batch_find(const uint32_t (&start)[kPdBatchMaxSegs + 1], int count, uint32_t f) {
  int t = 0;
#pragma unroll
  for (int j = 1; j < kPdBatchMaxSegs; ++j) t += (j < count && f >= start[j]) ? 1 : 0;
  return t;
}

// One segment's rows (PdSlots' accessor): off is wave-uniform and i comes from
// unrolled loops, so p[off + i] stays a scalar load (RobTaskArgs).
struct PdTaskArgs {
  const PdBatchSlots& b;
  int off;
  __device__ const void* ptr(int i) const { return b.p[off + i]; }
};

// grid: block_start[nsegs] entries. Entry e of segment s is block e % blocks_s
// of unit e / blocks_s (the flat grid's order: blocks fastest).
template <class Op, int CAP, bool CROSS, bool VEC>
__global__ __launch_bounds__(kBlock) void k_pairdist_batch(const PdBatchSlots s, double* __restrict__ ws) {
  static_assert(kBlock == 256, "four waves: the block-end sum names them");
  __shared__ double red[kBlock / 64][kPdSlots];
  const uint32_t bid = blockIdx.x;
  const int g = pd_batch_find(s.block_start, s.nsegs, bid);
  const uint32_t local = bid - s.block_start[g];
  const uint32_t nblk = s.blocks[g];
  const uint32_t u = CROSS ? local / nblk : 0u;
  const uint32_t b = local - u * nblk;
  const PdTaskArgs a{s, static_cast<int>(s.ptr_off[g])};
  pd_block<Op, CAP, CROSS, VEC>(a, static_cast<int>(s.fan_in[g]), static_cast<size_t>(s.nelem[g]), ws + s.ws_off[g],
                                static_cast<int>(u), nblk, b, red);
}

// One wave per (matrix, pair i < j): the matrix's segments of this launch in
// segment order, each segment's blocks summed as k_pairdist_finish sums them
// (pd_finish_sum), the sums added one after the other to d2[i][j] (mat_acc) or
// to the first of them: the double additions of consecutive flat calls with
// accumulate = 1. d2[i][j] and d2[j][i] get the same bits; the wave of a
// matrix's pair 0 writes its +0.0 diagonal unless accumulating. cap: rows of
// the launch's diagonal units (4 or 8).
template <class = void>
__global__ __launch_bounds__(kBlock) void k_pairdist_batch_finish(const PdBatchSlots s,
                                                                  const double* __restrict__ ws, int cap) {
  const int lane = threadIdx.x & 63;
  const uint32_t w =
      __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
  if (w >= s.mat_wave[s.nmats]) return;
  const int m = pd_batch_find(s.mat_wave, s.nmats, w);
  const int pair = static_cast<int>(w - s.mat_wave[m]);
  const uint32_t g0 = s.mat_seg[m], g1 = s.mat_seg[m + 1];
  const int n = static_cast<int>(s.fan_in[g0]);
  const bool acc = s.mat_acc[m] != 0;
  double* const d2 = s.d2[m];
  if (pair == 0 && !acc && lane < n) d2[static_cast<size_t>(lane) * (n + 1)] = 0.0;
  int i, j;
  const int where = pd_pair_slot(pair, n, cap, i, j);
  double* const pij = d2 + static_cast<size_t>(i) * n + j;
  double r = acc ? *pij : 0.0;
  bool first = !acc;
  for (uint32_t g = g0; g < g1; ++g) {
    const uint32_t blocks = s.blocks[g];
    const double v = pd_finish_sum(ws + s.ws_off[g] + static_cast<size_t>(where) * blocks, blocks, lane);
    if (first) r = v;
    else r = pd_add_held(v, r);  // k_pairdist_finish's add, operand for operand (NaN payloads)
    first = false;
  }
  if (lane == 0) {
    *pij = r;
    d2[static_cast<size_t>(j) * n + i] = r;
  }
}

}  // namespace dlsim
