// inst_quant.hip — instantiation unit: the block-quantisation kernels
// (quant_kernels.hpp) and their host dispatch, behind dlsim_quantize,
// dlsim_dequantize, dlsim_quant_wreduce, dlsim_quant_wreduce_batched,
// dlsim_quant_geometry and dlsim_quant_kernel_name (dlsim_abi.hip checks the
// arguments).
#include "quant_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

QuantGeom quant_geometry(size_t nelem, int dtype, int bits) {
  const size_t E = dtype == DLSIM_F32 ? dlsim::F32Exact::E : dlsim::BF16Exact::E;
  const auto grid = [](size_t nelem, size_t tile, unsigned* tpb) {
    const size_t tiles = (nelem + tile - 1) / tile;
    *tpb = static_cast<unsigned>((tiles + dlsim::kQuantMaxBlocks - 1) / dlsim::kQuantMaxBlocks);
    return tiles ? static_cast<unsigned>((tiles + *tpb - 1) / *tpb) : 0u;
  };
  QuantGeom g;
  g.block = dlsim::kQuantBlockElems;
  g.max_blocks = dlsim::kQuantMaxBlocks;
  g.tile = static_cast<size_t>(dlsim::kBlock) * E * dlsim::kQuantVpt;
  g.blocks = grid(nelem, g.tile, &g.tpb);
  g.reduce_tile = dlsim::kQuantTile;
  g.reduce_blocks = grid(nelem, g.reduce_tile, &g.reduce_tpb);
  g.code_bytes = bits == 8 ? nelem : (nelem + 1) / 2;
  g.n_scales = (nelem + g.block - 1) / g.block;
  return g;
}

const char* quant_kernel_name(int op, bool vec) {
  static const char* const names[3][2] = {{"dlsim::k_quantize<scalar>", "dlsim::k_quantize<vec>"},
                                          {"dlsim::k_dequantize<scalar>", "dlsim::k_dequantize<vec>"},
                                          {"dlsim::k_quant_wreduce<scalar>", "dlsim::k_quant_wreduce<vec>"}};
  return names[op][vec ? 1 : 0];
}

void quant_batch_limits(int* max_tasks, int* max_slots) {
  *max_tasks = dlsim::kQuantMaxTasks;
  *max_slots = dlsim::kQuantMaxSlots;
}

namespace {

template <class Op, int BITS, bool STOCH, bool RESID>
hipError_t quantize_launch(const void* x, void* e, uint32_t nelem, const QuantGeom& g, uint32_t seed, uint8_t* codes,
                           float* scales, bool vec, hipStream_t st) {
  const dim3 grid(g.blocks), block(dlsim::kBlock);
  if (vec) hipLaunchKernelGGL((dlsim::k_quantize<Op, BITS, STOCH, RESID, true>), grid, block, 0, st, x, e, nelem, g.tpb, seed, codes, scales);
  else hipLaunchKernelGGL((dlsim::k_quantize<Op, BITS, STOCH, RESID, false>), grid, block, 0, st, x, e, nelem, g.tpb, seed, codes, scales);
  return hipGetLastError();
}

template <class Op, int BITS>
hipError_t quantize_pick(const void* x, void* e, uint32_t nelem, const QuantGeom& g, bool stoch, uint32_t seed,
                         uint8_t* codes, float* scales, bool vec, hipStream_t st) {
  if (stoch) return e ? quantize_launch<Op, BITS, true, true>(x, e, nelem, g, seed, codes, scales, vec, st)
                      : quantize_launch<Op, BITS, true, false>(x, e, nelem, g, seed, codes, scales, vec, st);
  return e ? quantize_launch<Op, BITS, false, true>(x, e, nelem, g, seed, codes, scales, vec, st)
           : quantize_launch<Op, BITS, false, false>(x, e, nelem, g, seed, codes, scales, vec, st);
}

template <class Op, int BITS>
hipError_t dequantize_launch(const uint8_t* codes, const float* scales, uint32_t nelem, const QuantGeom& g, void* out,
                             bool vec, hipStream_t st) {
  const dim3 grid(g.blocks), block(dlsim::kBlock);
  if (vec) hipLaunchKernelGGL((dlsim::k_dequantize<Op, BITS, true>), grid, block, 0, st, codes, scales, nelem, g.tpb, out);
  else hipLaunchKernelGGL((dlsim::k_dequantize<Op, BITS, false>), grid, block, 0, st, codes, scales, nelem, g.tpb, out);
  return hipGetLastError();
}

template <class Op>
hipError_t quant_reduce_launch(const dlsim::QuantBatch& s, unsigned blocks, bool vec, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((dlsim::k_quant_wreduce<Op, true>), dim3(blocks), dim3(dlsim::kBlock), 0, st, s);
  else hipLaunchKernelGGL((dlsim::k_quant_wreduce<Op, false>), dim3(blocks), dim3(dlsim::kBlock), 0, st, s);
  return hipGetLastError();
}

}  // namespace

// 1 <= nelem < 2^31, dtype fp32 or bf16, bits 4 or 8, no null pointer but e, no overlap: checked by the caller.
// vec: x, e and codes are 16-byte aligned.
hipError_t quantize_run(const void* x, void* e, size_t nelem, int dtype, int bits, bool stoch, uint32_t seed, void* codes,
                        float* scales, hipStream_t st) {
  const QuantGeom g = quant_geometry(nelem, dtype, bits);
  const bool vec = aligned16(x) && aligned16(e) && aligned16(codes);
  const uint32_t n = static_cast<uint32_t>(nelem);
  uint8_t* const c = static_cast<uint8_t*>(codes);
  if (dtype == DLSIM_F32)
    return bits == 8 ? quantize_pick<dlsim::QuantF32, 8>(x, e, n, g, stoch, seed, c, scales, vec, st)
                     : quantize_pick<dlsim::QuantF32, 4>(x, e, n, g, stoch, seed, c, scales, vec, st);
  return bits == 8 ? quantize_pick<dlsim::QuantBF16, 8>(x, e, n, g, stoch, seed, c, scales, vec, st)
                   : quantize_pick<dlsim::QuantBF16, 4>(x, e, n, g, stoch, seed, c, scales, vec, st);
}

// vec: codes and out are 16-byte aligned
hipError_t dequantize_run(const void* codes, const float* scales, size_t nelem, int dtype, int bits, void* out,
                          hipStream_t st) {
  const QuantGeom g = quant_geometry(nelem, dtype, bits);
  const bool vec = aligned16(codes) && aligned16(out);
  const uint32_t n = static_cast<uint32_t>(nelem);
  const uint8_t* const c = static_cast<const uint8_t*>(codes);
  if (dtype == DLSIM_F32)
    return bits == 8 ? dequantize_launch<dlsim::F32Exact, 8>(c, scales, n, g, out, vec, st)
                     : dequantize_launch<dlsim::F32Exact, 4>(c, scales, n, g, out, vec, st);
  return bits == 8 ? dequantize_launch<dlsim::BF16Exact, 8>(c, scales, n, g, out, vec, st)
                   : dequantize_launch<dlsim::BF16Exact, 4>(c, scales, n, g, out, vec, st);
}

// Task t: the dense row self[t] (nelem[t] < 2^31 elements), m[t] <= 31 neighbours whose codes, scales, bits and
// weights follow task t-1's (w holds self's weight first, then the neighbours'). Everything is checked by the
// caller. Tasks without an element launch nothing; the others ride in launches of at most kQuantMaxTasks tasks
// and kQuantMaxSlots neighbours, tasks whose self, out and code buffers are all 16-byte aligned in vector-form
// launches and the others in scalar-form launches, each on the virtual grid of its flat call.
hipError_t quant_reduce_run(int b, const void* const* self, const int* m, const void* const* codes,
                            const float* const* scales, const int* bits, const float* w, void* const* out,
                            const size_t* nelem, int dtype, hipStream_t st) {
  std::vector<size_t> slot(static_cast<size_t>(b) + 1, 0);
  for (int t = 0; t < b; ++t) slot[t + 1] = slot[t] + static_cast<size_t>(m[t]);
  for (int form = 0; form < 2; ++form) {  // 0: vector, 1: scalar
    dlsim::QuantBatch s;
    std::memset(&s, 0, sizeof(s));
    unsigned blocks = 0;
    int slots = 0;
    const auto flush = [&]() -> hipError_t {
      if (s.ntasks == 0) return hipSuccess;
      const hipError_t e = dtype == DLSIM_F32 ? quant_reduce_launch<dlsim::F32Exact>(s, blocks, form == 0, st)
                                              : quant_reduce_launch<dlsim::BF16Exact>(s, blocks, form == 0, st);
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
      const QuantGeom g = quant_geometry(nelem[t], dtype, 8);
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
        s.scales[slots + j] = scales[slot[t] + j];
        s.bits[slots + j] = static_cast<uint32_t>(bits[slot[t] + j]);
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
