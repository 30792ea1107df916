// reducedist_batch_kernels.hpp — the "reduce and measure" kernels
// (reducedist_kernels.hpp) over many independent calls in one grid: one pass
// of the geometric median or of centered clipping for every peer of a
// simulated round. The shape of k_pairdist_batch
// (pairdist_batch_kernels.hpp): descriptors in the kernel arguments, the block
// index mapped to its piece of work through a prefix array.
//
// The unit of work is a segment: what one dlsim_wreduce_dist call is, n_s rows
// of nelem_s elements with n_s weights, one output (or none: distances only)
// and n_s partial sums per block. A distance vector belongs to one task and is
// the sum of that task's consecutive segments (a model's tensors). All
// segments of a launch share the flat kernel's capacity (CAP 4, 8, 16 or 32),
// its form (16-byte-aligned vectors, or element by element) and the dtype;
// each has its own fan-in, length, pointers, weights, output and workspace
// offset.
//
// The flat kernel's summation order is a function of its grid alone. Segment s
// therefore owns blocks_s consecutive entries of the batch's grid, with
// blocks_s the flat call's grid, and entry b runs rd_block with (blocks_s, b)
// in place of (gridDim.x, blockIdx.x): the same tiles, the same stores, the
// same partials at the same workspace slots, bit for bit.
// k_reducedist_batch_finish then adds, per vector and input, the segments'
// partials in segment order, each with pd_finish_sum, as consecutive flat
// calls with accumulate = 1 would.
#pragma once

#include "pairdist_batch_kernels.hpp"
#include "reducedist_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kRdBatchMaxSegs = 32;
static_assert(kRdBatchMaxSegs == kPdBatchMaxSegs, "pd_batch_find searches both families' prefix arrays");

// Row pointers (and weights, one per pointer) of one launch: what leaves the
// descriptors inside the 4 KiB of kernel arguments.
template <class W>
constexpr int rd_batch_max_ptrs() {
  return sizeof(W) == 8 ? 128 : 192;
}

// 32-bit fields and pointers only: they are read with scalar loads at a
// run-time (wave-uniform) index (PdBatchSlots). A segment fits one launch's
// 32-bit byte range, so its length fits 32 bits. Vector v is the segments
// vec_seg[v] .. vec_seg[v + 1]; its fan-in is that of its first segment.
template <class W>
struct RdBatchSlots {
  static constexpr int kPtrs = rd_batch_max_ptrs<W>();
  const void* p[kPtrs];
  W w[kPtrs];                                 // weight of row p[k]
  void* out[kRdBatchMaxSegs];                 // per segment; null: distances only
  double* d2[kRdBatchMaxSegs];                // per vector
  uint32_t block_start[kRdBatchMaxSegs + 1];  // first grid entry of each segment
  uint32_t blocks[kRdBatchMaxSegs];           // the segment's virtual grid
  uint32_t ws_off[kRdBatchMaxSegs];           // doubles from the launch's workspace to the segment's partials
  uint32_t nelem[kRdBatchMaxSegs];
  uint32_t ptr_off[kRdBatchMaxSegs];
  uint32_t fan_in[kRdBatchMaxSegs];
  uint32_t vec_seg[kRdBatchMaxSegs + 1];   // first segment of each vector
  uint32_t vec_wave[kRdBatchMaxSegs + 1];  // first finish wave (input) of each vector
  uint32_t vec_acc[kRdBatchMaxSegs];       // 1: add to what the vector holds
  int nsegs;
  int nvecs;
};
static_assert(sizeof(RdBatchSlots<float>) <= 4096, "kernel arguments");
static_assert(sizeof(RdBatchSlots<double>) <= 4096, "kernel arguments");

// One segment's rows and weights (RdSlots' accessors): off is wave-uniform and
// i comes from unrolled loops, so p[off + i] and w[off + i] stay scalar loads
// (PdTaskArgs).
template <class W>
struct RdTaskArgs {
  const RdBatchSlots<W>& b;
  int off;
  __device__ const void* ptr(int i) const { return b.p[off + i]; }
  __device__ W wt(int i) const { return b.w[off + i]; }
};

// grid: block_start[nsegs] entries. Entry e of segment s is block
// e - block_start[s] of the segment's blocks_s.
template <class Op, int CAP, bool VEC>
__global__ __launch_bounds__(kBlock) void k_reducedist_batch(const RdBatchSlots<wt_t<typename Op::Fold>> arg,
                                                             double* __restrict__ ws) {
  static_assert(kBlock == 256, "four waves: the block-end sum names them");
  using W = wt_t<typename Op::Fold>;
  __shared__ double red[kBlock / 64][kPdSlots];
  // The rows' loops index the slots at run time; read through the by-value
  // argument, the CAP 32 kernels of the 2-byte dtypes kept a private copy of
  // all of it (4000 bytes of scratch per lane). It is the first kernel
  // argument: read it in place in the kernarg segment (k_wreduce_defer).
  const RdBatchSlots<W>& s = *(const RdBatchSlots<W>*)__builtin_amdgcn_kernarg_segment_ptr();
  (void)arg;
  const uint32_t bid = blockIdx.x;
  const int g = pd_batch_find(s.block_start, s.nsegs, bid);
  const uint32_t b = bid - s.block_start[g];
  const RdTaskArgs<W> a{s, static_cast<int>(s.ptr_off[g])};
  rd_block<Op, CAP, VEC>(a, static_cast<int>(s.fan_in[g]), s.out[g], static_cast<size_t>(s.nelem[g]),
                         ws + s.ws_off[g], s.blocks[g], b, red);
}

// One wave per (vector, input i): the vector's segments of this launch in
// segment order, each segment's blocks summed as k_reducedist_finish sums them
// (pd_finish_sum), the sums added one after the other to d2[i] (vec_acc) or to
// the first of them: the double additions of consecutive flat calls with
// accumulate = 1, operand for operand (pd_add_held: the sum first, the held
// value second, as k_reducedist_finish).
template <class W>
__global__ __launch_bounds__(kBlock) void k_reducedist_batch_finish(const RdBatchSlots<W> s,
                                                                    const double* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const uint32_t w =
      __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
  if (w >= s.vec_wave[s.nvecs]) return;
  const int m = pd_batch_find(s.vec_wave, s.nvecs, w);
  const uint32_t i = w - s.vec_wave[m];
  const uint32_t g0 = s.vec_seg[m], g1 = s.vec_seg[m + 1];
  const bool acc = s.vec_acc[m] != 0;
  double* const pi = s.d2[m] + i;
  double r = acc ? *pi : 0.0;
  bool first = !acc;
  for (uint32_t g = g0; g < g1; ++g) {
    const uint32_t blocks = s.blocks[g];
    const double v = pd_finish_sum(ws + s.ws_off[g] + static_cast<size_t>(i) * blocks, blocks, lane);
    if (first) r = v;
    else r = pd_add_held(v, r);
    first = false;
  }
  if (lane == 0) *pi = r;
}

}  // namespace dlsim
