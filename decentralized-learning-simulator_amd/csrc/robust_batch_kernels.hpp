// robust_batch_kernels.hpp — the order-statistic kernels (robust_kernels.hpp)
// over many independent tasks in one grid: the medians or
// trimmed means of one simulated round's peers, or the tensors of one model
// that lives in separate device tensors. The shape of k_wreduce_batch
// (wreduce_kernels.hpp): descriptors in the kernel arguments, blocks
// 0 .. ntasks-1 the tasks' first blocks (the ragged end: a partial tile, then
// the scalar tail), behind them every task's full tiles.
//
// All tasks of a launch share one capacity class CAP (4, 8, 16 or 32: the
// sorting network and the tile geometry of the flat kernels); each has its own
// fan-in n_t <= CAP, window [lo_t, hi_t), length and output. The tile bodies
// are the flat kernels' (rob_tile, rob_half_tile, rob_scalar_elem) behind
// another accessor, so a task computes bit for bit what dlsim_robust_reduce
// computes. A task with a pointer off a 16-byte boundary rides along element
// by element: its blocks take kBlock elements each through rob_scalar_elem.
#pragma once

#include "robust_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kRobBatchMaxTasks = 32;
constexpr int kRobBatchMaxPtrs = 192;

// 32-bit fields only: they are read with scalar loads at a run-time
// (wave-uniform) index; 16-bit fields compiled to vector loads
// (wreduce_kernels.hpp BatchSlots). A task's vector (or 8-byte unit) count
// follows from nelem.
struct RobBatchSlots {
  const void* p[kRobBatchMaxPtrs];
  void* out[kRobBatchMaxTasks];
  size_t nelem[kRobBatchMaxTasks];
  uint32_t block_start[kRobBatchMaxTasks + 1];  // first full tile of each task
  uint32_t ptr_off[kRobBatchMaxTasks];
  uint32_t fan_in[kRobBatchMaxTasks];
  uint32_t lo[kRobBatchMaxTasks];
  uint32_t hi[kRobBatchMaxTasks];
  uint32_t scalar[kRobBatchMaxTasks];  // 1: a pointer is off alignment, element by element
  int ntasks;
};
static_assert(sizeof(RobBatchSlots) <= 4096, "kernel arguments");

// The task of full-tile entry f: the last t with block_start[t] <= f, as a
// count over a compile-time range (batch_find_task's form: no dependent scan).
__device__ __forceinline__ int rob_batch_find_task(const RobBatchSlots& s, uint32_t f) {
  int t = 0;
#pragma unroll
  for (int j = 1; j < kRobBatchMaxTasks; ++j) t += (j < s.ntasks && f >= s.block_start[j]) ? 1 : 0;
  return t;
}

// One task's view of the batch (RobSlots' accessor): off is wave-uniform and
// i comes from unrolled loops, so p[off + i] stays a scalar load.
struct RobTaskArgs {
  const RobBatchSlots& b;
  int off;
  __device__ const void* ptr(int i) const { return b.p[off + i]; }
};

// elements of one full tile of an aligned task, by class (the flat kernels'
// geometry): kBlock * VPT vectors with VPT 4, 2, 1; kBlock 8-byte units at 32
template <int CAP> constexpr int rob_batch_vpt() { return CAP >= 16 ? 1 : 16 / CAP; }
template <class Op, int CAP>
constexpr size_t rob_batch_tile_elems() {
  return CAP == 32 ? static_cast<size_t>(kBlock) * (Op::E / 2) : static_cast<size_t>(kBlock) * rob_batch_vpt<CAP>() * Op::E;
}

template <class Op, int CAP, int STP>
__global__ __launch_bounds__(kBlock) void k_robust_batch(const RobBatchSlots s) {
  const uint32_t bid = blockIdx.x;
  int t = 0;
  uint32_t local = 0;  // 0: the task's first block; f: its full tile f - 1
  if (bid < static_cast<uint32_t>(s.ntasks)) {
    t = static_cast<int>(bid);
  } else {
    const uint32_t f = bid - static_cast<uint32_t>(s.ntasks);
    t = rob_batch_find_task(s, f);
    local = f - s.block_start[t] + 1;
  }
  const RobTaskArgs a{s, static_cast<int>(s.ptr_off[t])};
  const int n = static_cast<int>(s.fan_in[t]);
  const int lo = static_cast<int>(s.lo[t]), hi = static_cast<int>(s.hi[t]);
  void* const out = s.out[t];
  const size_t nelem = s.nelem[t];
  size_t j;  // the element this lane folds alone, if below nelem
  if (s.scalar[t]) {
    const size_t chunk = local == 0 ? nelem / kBlock : local - 1;  // first block: the ragged end
    j = chunk * kBlock + threadIdx.x;
  } else if constexpr (CAP == 32) {
    const size_t nunit = nelem / (Op::E / 2);
    if (local != 0) {
      rob_half_tile<Op, CAP, false>(a, n, lo, hi, out, static_cast<size_t>(local - 1) * kBlock + threadIdx.x, nunit);
      return;
    }
    const size_t full = nunit / kBlock;
    if (full * kBlock < nunit) rob_half_tile<Op, CAP, true>(a, n, lo, hi, out, full * kBlock + threadIdx.x, nunit);
    j = nunit * (Op::E / 2) + threadIdx.x;
  } else {
    constexpr int VPT = rob_batch_vpt<CAP>();
    constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
    const size_t nvec = nelem / Op::E;
    const OutRef o = make_out<STP>(out, nvec);
    if (local != 0) {
      rob_tile<Op, CAP, VPT, false, STP>(a, n, lo, hi, o, static_cast<size_t>(local - 1) * kTile + threadIdx.x, nvec);
      return;
    }
    const size_t full = nvec / kTile;
    if (full * kTile < nvec) rob_tile<Op, CAP, VPT, true, STP>(a, n, lo, hi, o, full * kTile + threadIdx.x, nvec);
    j = nvec * Op::E + threadIdx.x;
  }
  if (j < nelem) rob_scalar_elem<Op, CAP>(a, n, lo, hi, out, j);
}

}  // namespace dlsim
