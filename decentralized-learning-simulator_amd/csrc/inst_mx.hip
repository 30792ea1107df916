// inst_mx.hip — instantiation unit: the MX sharing kernels (mx_kernels.hpp)
// and their host dispatch, behind dlsim_mx_quantize, dlsim_mx_dequantize,
// dlsim_mx_wreduce, dlsim_mx_wreduce_batched, dlsim_mx_geometry and
// dlsim_mx_kernel_name (dlsim_abi.hip checks the arguments).
#include "mx_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

MxGeom mx_geometry(size_t nelem, int dtype, int fmt) {
  const size_t E = dtype == DLSIM_F32 ? dlsim::F32Exact::E : dlsim::BF16Exact::E;
  const auto grid = [](size_t nelem, size_t tile, unsigned* tpb) {
    const size_t tiles = (nelem + tile - 1) / tile;
    *tpb = static_cast<unsigned>((tiles + dlsim::kQuantMaxBlocks - 1) / dlsim::kQuantMaxBlocks);
    return tiles ? static_cast<unsigned>((tiles + *tpb - 1) / *tpb) : 0u;
  };
  MxGeom g;
  g.block = dlsim::kMxBlock;
  g.max_blocks = dlsim::kQuantMaxBlocks;
  g.tile = static_cast<size_t>(dlsim::kBlock) * E * dlsim::kMxVpt;
  g.blocks = grid(nelem, g.tile, &g.tpb);
  g.reduce_tile = dlsim::kMxTile;
  g.reduce_blocks = grid(nelem, g.reduce_tile, &g.reduce_tpb);
  g.code_bytes = fmt == DLSIM_MX_FP4_E2M1 ? (nelem + 1) / 2 : nelem;
  g.scale_bytes = (nelem + g.block - 1) / g.block;
  return g;
}

const char* mx_kernel_name(int op, bool vec) {
  static const char* const names[3][2] = {{"dlsim::k_mx_quantize<scalar>", "dlsim::k_mx_quantize<vec>"},
                                          {"dlsim::k_mx_dequantize<scalar>", "dlsim::k_mx_dequantize<vec>"},
                                          {"dlsim::k_mx_wreduce<scalar>", "dlsim::k_mx_wreduce<vec>"}};
  return names[op][vec ? 1 : 0];
}

void mx_batch_limits(int* max_tasks, int* max_slots) {
  *max_tasks = dlsim::kQuantMaxTasks;
  *max_slots = dlsim::kQuantMaxSlots;
}

namespace {

template <class Op, int FMT>
hipError_t mx_quantize_launch(const void* x, void* e, uint32_t nelem, const MxGeom& g, uint8_t* codes, uint8_t* scales,
                              bool vec, hipStream_t st) {
  const dim3 grid(g.blocks), block(dlsim::kBlock);
  if (e) {
    if (vec) hipLaunchKernelGGL((dlsim::k_mx_quantize<Op, FMT, true, true>), grid, block, 0, st, x, e, nelem, g.tpb, codes, scales);
    else hipLaunchKernelGGL((dlsim::k_mx_quantize<Op, FMT, true, false>), grid, block, 0, st, x, e, nelem, g.tpb, codes, scales);
  } else {
    if (vec) hipLaunchKernelGGL((dlsim::k_mx_quantize<Op, FMT, false, true>), grid, block, 0, st, x, e, nelem, g.tpb, codes, scales);
    else hipLaunchKernelGGL((dlsim::k_mx_quantize<Op, FMT, false, false>), grid, block, 0, st, x, e, nelem, g.tpb, codes, scales);
  }
  return hipGetLastError();
}

template <class Op, int FMT>
hipError_t mx_dequantize_launch(const uint8_t* codes, const uint8_t* scales, uint32_t nelem, const MxGeom& g, void* out,
                                bool vec, hipStream_t st) {
  const dim3 grid(g.blocks), block(dlsim::kBlock);
  if (vec) hipLaunchKernelGGL((dlsim::k_mx_dequantize<Op, FMT, true>), grid, block, 0, st, codes, scales, nelem, g.tpb, out);
  else hipLaunchKernelGGL((dlsim::k_mx_dequantize<Op, FMT, false>), grid, block, 0, st, codes, scales, nelem, g.tpb, out);
  return hipGetLastError();
}

template <class Op>
hipError_t mx_reduce_launch(const dlsim::MxBatch& s, unsigned blocks, bool vec, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((dlsim::k_mx_wreduce<Op, true>), dim3(blocks), dim3(dlsim::kBlock), 0, st, s);
  else hipLaunchKernelGGL((dlsim::k_mx_wreduce<Op, false>), dim3(blocks), dim3(dlsim::kBlock), 0, st, s);
  return hipGetLastError();
}

}  // namespace

// 1 <= nelem < 2^31, dtype fp32 or bf16, a known format, no null pointer but e, no overlap: checked by the caller.
// vec: x, e and codes are 16-byte aligned.
hipError_t mx_quantize_run(const void* x, void* e, size_t nelem, int dtype, int fmt, void* codes, void* scales,
                           hipStream_t st) {
  const MxGeom g = mx_geometry(nelem, dtype, fmt);
  const bool vec = aligned16(x) && aligned16(e) && aligned16(codes);
  const uint32_t n = static_cast<uint32_t>(nelem);
  uint8_t* const c = static_cast<uint8_t*>(codes);
  uint8_t* const s = static_cast<uint8_t*>(scales);
  if (dtype == DLSIM_F32)
    return fmt == DLSIM_MX_FP8_E4M3   ? mx_quantize_launch<dlsim::F32Exact, dlsim::kMxE4M3>(x, e, n, g, c, s, vec, st)
           : fmt == DLSIM_MX_FP8_E5M2 ? mx_quantize_launch<dlsim::F32Exact, dlsim::kMxE5M2>(x, e, n, g, c, s, vec, st)
                                      : mx_quantize_launch<dlsim::F32Exact, dlsim::kMxE2M1>(x, e, n, g, c, s, vec, st);
  return fmt == DLSIM_MX_FP8_E4M3   ? mx_quantize_launch<dlsim::BF16Exact, dlsim::kMxE4M3>(x, e, n, g, c, s, vec, st)
         : fmt == DLSIM_MX_FP8_E5M2 ? mx_quantize_launch<dlsim::BF16Exact, dlsim::kMxE5M2>(x, e, n, g, c, s, vec, st)
                                    : mx_quantize_launch<dlsim::BF16Exact, dlsim::kMxE2M1>(x, e, n, g, c, s, vec, st);
}

// vec: codes and out are 16-byte aligned
hipError_t mx_dequantize_run(const void* codes, const void* scales, size_t nelem, int dtype, int fmt, void* out,
                             hipStream_t st) {
  const MxGeom g = mx_geometry(nelem, dtype, fmt);
  const bool vec = aligned16(codes) && aligned16(out);
  const uint32_t n = static_cast<uint32_t>(nelem);
  const uint8_t* const c = static_cast<const uint8_t*>(codes);
  const uint8_t* const s = static_cast<const uint8_t*>(scales);
  if (dtype == DLSIM_F32)
    return fmt == DLSIM_MX_FP8_E4M3   ? mx_dequantize_launch<dlsim::F32Exact, dlsim::kMxE4M3>(c, s, n, g, out, vec, st)
           : fmt == DLSIM_MX_FP8_E5M2 ? mx_dequantize_launch<dlsim::F32Exact, dlsim::kMxE5M2>(c, s, n, g, out, vec, st)
                                      : mx_dequantize_launch<dlsim::F32Exact, dlsim::kMxE2M1>(c, s, n, g, out, vec, st);
  return fmt == DLSIM_MX_FP8_E4M3   ? mx_dequantize_launch<dlsim::BF16Exact, dlsim::kMxE4M3>(c, s, n, g, out, vec, st)
         : fmt == DLSIM_MX_FP8_E5M2 ? mx_dequantize_launch<dlsim::BF16Exact, dlsim::kMxE5M2>(c, s, n, g, out, vec, st)
                                    : mx_dequantize_launch<dlsim::BF16Exact, dlsim::kMxE2M1>(c, s, n, g, out, vec, st);
}

// Task t: the dense row self[t] (nelem[t] < 2^31 elements), m[t] <= 31 neighbours whose codes, scale bytes, formats
// and weights follow task t-1's (w holds self's weight first, then the neighbours'). Everything is checked by the
// caller. Tasks without an element launch nothing; the others ride in launches of at most kQuantMaxTasks tasks
// and kQuantMaxSlots neighbours, tasks whose self, out and code buffers are all 16-byte aligned in vector-form
// launches and the others in scalar-form launches, each on the virtual grid of its flat call.
hipError_t mx_reduce_run(int b, const void* const* self, const int* m, const void* const* codes, const void* const* scales,
                         const int* fmt, const float* w, void* const* out, const size_t* nelem, int dtype, hipStream_t st) {
  std::vector<size_t> slot(static_cast<size_t>(b) + 1, 0);
  for (int t = 0; t < b; ++t) slot[t + 1] = slot[t] + static_cast<size_t>(m[t]);
  for (int form = 0; form < 2; ++form) {  // 0: vector, 1: scalar
    dlsim::MxBatch s;
    std::memset(&s, 0, sizeof(s));
    unsigned blocks = 0;
    int slots = 0;
    const auto flush = [&]() -> hipError_t {
      if (s.ntasks == 0) return hipSuccess;
      const hipError_t e = dtype == DLSIM_F32 ? mx_reduce_launch<dlsim::F32Exact>(s, blocks, form == 0, st)
                                              : mx_reduce_launch<dlsim::BF16Exact>(s, blocks, form == 0, st);
      std::memset(&s, 0, sizeof(s));
      blocks = 0;
      slots = 0;
      return e;
    };
    for (int t = 0; t < b; ++t) {
      if (nelem[t] == 0) continue;
      bool vec = aligned16(self[t]) && aligned16(out[t]);
      for (int j = 0; j < m[t]; ++j) vec = vec && aligned16(codes[slot[t] + j]);
      if (vec != (form == 0)) continue;
      const MxGeom g = mx_geometry(nelem[t], dtype, DLSIM_MX_FP8_E4M3);
      if (s.ntasks == dlsim::kQuantMaxTasks || slots + m[t] > dlsim::kQuantMaxSlots ||
          static_cast<uint64_t>(blocks) + g.reduce_blocks > 0x7fffffffull) {
        const hipError_t e = flush();
        if (e != hipSuccess) return e;
      }
      dlsim::QuantTask& d = s.t[s.ntasks++];
      d.self = self[t];
      d.out = out[t];
      d.nelem = static_cast<uint32_t>(nelem[t]);
      d.block_start = blocks;
      d.tpb = g.reduce_tpb;
      d.slot_off = static_cast<uint32_t>(slots);
      d.m = static_cast<uint32_t>(m[t]);
      d.w0 = w[slot[t] + static_cast<size_t>(t)];
      for (int j = 0; j < m[t]; ++j) {
        s.codes[slots + j] = static_cast<const uint8_t*>(codes[slot[t] + j]);
        s.scales[slots + j] = static_cast<const uint8_t*>(scales[slot[t] + j]);
        s.fmt[slots + j] = static_cast<uint32_t>(fmt[slot[t] + j]);
        s.w[slots + j] = w[slot[t] + static_cast<size_t>(t) + 1 + j];
      }
      slots += m[t];
      blocks += g.reduce_blocks;
    }
    const hipError_t e = flush();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace dlsim_host
