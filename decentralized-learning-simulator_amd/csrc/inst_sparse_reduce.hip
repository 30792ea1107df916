// inst_sparse_reduce.hip — instantiation unit: the sparse mixing kernel
// (sparse_reduce_kernels.hpp) and its host dispatch, behind
// dlsim_sparse_wreduce, dlsim_sparse_wreduce_batched, dlsim_sparse_geometry
// and dlsim_sparse_kernel_name (dlsim_abi.hip checks the arguments).
#include "sparse_reduce_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

SparseGeom sparse_geometry(size_t nelem, int dtype) {
  const size_t E = dtype == DLSIM_F32 ? dlsim::F32Exact::E : dlsim::BF16Exact::E;
  SparseGeom g;
  g.tile = static_cast<size_t>(dlsim::kBlock) * E * dlsim::kSparseVpt;
  g.max_blocks = dlsim::kSparseMaxBlocks;
  const size_t tiles = (nelem + g.tile - 1) / g.tile;
  g.tpb = static_cast<unsigned>((tiles + g.max_blocks - 1) / g.max_blocks);
  g.blocks = tiles ? static_cast<unsigned>((tiles + g.tpb - 1) / g.tpb) : 0;
  return g;
}

const char* sparse_kernel_name(bool vec) {
  return vec ? "dlsim::k_sparse_wreduce<vec>" : "dlsim::k_sparse_wreduce<scalar>";
}

void sparse_batch_limits(int* max_tasks, int* max_slots) {
  *max_tasks = dlsim::kSparseMaxTasks;
  *max_slots = dlsim::kSparseMaxSlots;
}

namespace {

template <class Op>
hipError_t sparse_launch(const dlsim::SparseBatch& s, unsigned blocks, bool vec, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((dlsim::k_sparse_wreduce<Op, true>), dim3(blocks), dim3(dlsim::kBlock), 0, st, s);
  else hipLaunchKernelGGL((dlsim::k_sparse_wreduce<Op, false>), dim3(blocks), dim3(dlsim::kBlock), 0, st, s);
  return hipGetLastError();
}

}  // namespace

// Task t: the dense row self[t] (nelem[t] < 2^31 elements), m[t] <= 31 neighbours whose lists and
// weights follow task t-1's in idx / val / k / w (w holds self's weight first, then the neighbours').
// Everything is checked by the caller. Tasks without an element launch nothing; the others ride in
// launches of at most kSparseMaxTasks tasks and kSparseMaxSlots neighbours, 16-byte aligned tasks
// (self and out) and the others in launches of their own, each on the virtual grid of its flat call.
hipError_t sparse_run(int b, const void* const* self, const int* m, const int32_t* const* idx, const void* const* val,
                      const long long* k, const float* w, void* const* out, const size_t* nelem, int dtype,
                      hipStream_t st) {
  std::vector<size_t> slot(static_cast<size_t>(b) + 1, 0);
  for (int t = 0; t < b; ++t) slot[t + 1] = slot[t] + static_cast<size_t>(m[t]);
  for (int form = 0; form < 2; ++form) {  // 0: vector, 1: scalar
    dlsim::SparseBatch s;
    std::memset(&s, 0, sizeof(s));
    unsigned blocks = 0;
    int slots = 0;
    const auto flush = [&]() -> hipError_t {
      if (s.ntasks == 0) return hipSuccess;
      const hipError_t e = dtype == DLSIM_F32 ? sparse_launch<dlsim::F32Exact>(s, blocks, form == 0, st)
                                              : sparse_launch<dlsim::BF16Exact>(s, blocks, form == 0, st);
      std::memset(&s, 0, sizeof(s));
      blocks = 0;
      slots = 0;
      return e;
    };
    for (int t = 0; t < b; ++t) {
      if (nelem[t] == 0) continue;
      const bool vec = aligned16(self[t]) && aligned16(out[t]);
      if (vec != (form == 0)) continue;
      const SparseGeom g = sparse_geometry(nelem[t], dtype);
      if (s.ntasks == dlsim::kSparseMaxTasks || slots + m[t] > dlsim::kSparseMaxSlots ||
          static_cast<uint64_t>(blocks) + g.blocks > 0x7fffffffull) {
        const hipError_t e = flush();
        if (e != hipSuccess) return e;
      }
      dlsim::SparseTask& d = s.t[s.ntasks++];
      d.self = self[t];
      d.out = out[t];
      d.nelem = static_cast<uint32_t>(nelem[t]);
      d.block_start = blocks;
      d.tpb = g.tpb;
      d.slot_off = static_cast<uint32_t>(slots);
      d.m = static_cast<uint32_t>(m[t]);
      d.w0 = w[slot[t] + static_cast<size_t>(t)];
      for (int j = 0; j < m[t]; ++j) {
        s.idx[slots + j] = idx[slot[t] + j];
        s.val[slots + j] = val[slot[t] + j];
        s.k[slots + j] = static_cast<uint32_t>(k[slot[t] + j]);
        s.w[slots + j] = w[slot[t] + static_cast<size_t>(t) + 1 + j];
      }
      slots += m[t];
      blocks += g.blocks;
    }
    const hipError_t e = flush();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace dlsim_host
