// inst_topk.hip — instantiation unit: the top-k selection kernels
// (topk_kernels.hpp) and their host dispatch, behind dlsim_topk_select,
// dlsim_topk_geometry and dlsim_topk_kernel_name (dlsim_abi.hip checks the
// arguments).
#include "topk_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

TopkGeom topk_geometry(size_t nelem, int dtype) {
  const size_t E = dtype == DLSIM_F32 ? dlsim::TopkF32::E : dlsim::TopkBF16::E;
  TopkGeom g;
  g.vec_tile = static_cast<size_t>(dlsim::kBlock) * E;
  g.block_tile = g.vec_tile * dlsim::kTopkVpt;
  g.max_blocks = dlsim::kTopkMaxBlocks;
  const size_t tiles = (nelem + g.block_tile - 1) / g.block_tile;
  g.tpb = static_cast<unsigned>((tiles + g.max_blocks - 1) / g.max_blocks);
  g.blocks = tiles ? static_cast<unsigned>((tiles + g.tpb - 1) / g.tpb) : 0;
  g.ws_bytes = tiles ? sizeof(uint32_t) * (static_cast<size_t>(dlsim::kTopkWsCountsOff) + 2 * g.blocks) : 0;
  return g;
}

const char* topk_kernel_name(bool vec) { return vec ? "dlsim::k_topk_write<vec>" : "dlsim::k_topk_write<scalar>"; }

namespace {

template <class Op, bool VEC>
hipError_t topk_launch(const void* x, void* ref, size_t nelem, uint32_t k, const TopkGeom& g, int32_t* idx, void* val,
                       uint32_t* threshold, hipStream_t st) {
  // the call's own workspace, allocated and freed in stream order: histograms, state words, block counts
  return with_partials((g.ws_bytes + sizeof(double) - 1) / sizeof(double), st, [&](double* mem) {
    uint32_t* const ws = reinterpret_cast<uint32_t*>(mem);
    const dim3 grid(g.blocks), block(dlsim::kBlock);
    hipLaunchKernelGGL(dlsim::k_topk_clear, dim3((dlsim::kTopkWsCountsOff + dlsim::kBlock - 1) / dlsim::kBlock), block, 0,
                       st, ws, k);
    hipLaunchKernelGGL((dlsim::k_topk_hist<Op, 0, VEC>), grid, block, 0, st, x, ref, nelem, g.tpb, ws);
    hipLaunchKernelGGL((dlsim::k_topk_hist<Op, 1, VEC>), grid, block, 0, st, x, ref, nelem, g.tpb, ws);
    hipLaunchKernelGGL((dlsim::k_topk_hist<Op, 2, VEC>), grid, block, 0, st, x, ref, nelem, g.tpb, ws);
    hipLaunchKernelGGL((dlsim::k_topk_count<Op, VEC>), grid, block, 0, st, x, ref, nelem, g.tpb, ws, threshold);
    hipLaunchKernelGGL((dlsim::k_topk_write<Op, VEC>), grid, block, 0, st, x, ref, nelem, g.tpb, ws, k, idx, val);
    return hipGetLastError();
  });
}

}  // namespace

// 1 <= k <= nelem < 2^31, dtype fp32 or bf16, no null pointer, no overlap: checked by the caller
hipError_t topk_select(const void* x, void* ref, size_t nelem, uint32_t k, int dtype, int32_t* idx, void* val,
                       uint32_t* threshold, hipStream_t st) {
  const TopkGeom g = topk_geometry(nelem, dtype);
  const bool vec = aligned16(x) && aligned16(ref);
  if (dtype == DLSIM_F32)
    return vec ? topk_launch<dlsim::TopkF32, true>(x, ref, nelem, k, g, idx, val, threshold, st)
               : topk_launch<dlsim::TopkF32, false>(x, ref, nelem, k, g, idx, val, threshold, st);
  return vec ? topk_launch<dlsim::TopkBF16, true>(x, ref, nelem, k, g, idx, val, threshold, st)
             : topk_launch<dlsim::TopkBF16, false>(x, ref, nelem, k, g, idx, val, threshold, st);
}

}  // namespace dlsim_host
