// inst_gramwide.hip — instantiation unit: the wide Gram-matrix squared-distance
// kernels (gramwide_kernels.hpp, 33 <= n <= 128) and their host dispatch,
// behind dlsim_gram_sqdist_wide, dlsim_gram_sqdist_wide_tensors and
// dlsim_gramwide_geometry (dlsim_abi.hip checks the arguments). n <= 32 is
// inst_gramdist.hip's.
#include "gramwide_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

hipError_t gramdist_flat(const void* const* in, int n, size_t nelem, int dtype, double* d2, int accumulate,
                         hipStream_t st);
void gramdist_geometry(int dtype, size_t nelem, size_t* tile_elems, unsigned* blocks);

namespace {

// Blocks of one launch: two resident blocks (of up to 72 KiB of LDS) on each
// of the 256 CUs of an MI355X. A constant, so that the summation order is the
// same on every device.
constexpr unsigned kGramwideGridBlocks = 512;
constexpr int kNarrowInputs = 2 * dlsim::kGdRows;  // up to here the narrow kernel serves

struct GwGeom {
  size_t tile;      // elements a block takes per step (both alignment classes)
  unsigned blocks;  // grid
};

GwGeom gw_geometry(size_t nelem) {
  GwGeom g;
  g.tile = dlsim::kGwKElems;
  const size_t tiles = (nelem + g.tile - 1) / g.tile;
  g.blocks = static_cast<unsigned>(std::min<size_t>(kGramwideGridBlocks, std::max<size_t>(tiles, 1)));
  return g;
}

// the compiled row-block class of n rows
int gw_class(int n) { return n <= 64 ? 4 : n <= 96 ? 6 : 8; }

template <class Op, int NRB>
void gw_launch_class(bool vec, unsigned blocks, const dlsim::GwRows& s, int n, size_t nelem, double* ws,
                     uint32_t* masks, hipStream_t st) {
  const dim3 grid(blocks), block(dlsim::kBlock);
  if (vec) hipLaunchKernelGGL((dlsim::k_gramwide<Op, NRB, true>), grid, block, 0, st, s, n, nelem, ws, masks);
  else hipLaunchKernelGGL((dlsim::k_gramwide<Op, NRB, false>), grid, block, 0, st, s, n, nelem, ws, masks);
}

// 32 < n <= 128, nelem > 0
template <class Op>
hipError_t gw_run(const void* const* in, int n, size_t nelem, double* d2, int accumulate, hipStream_t st) {
  bool vec = true;
  for (int i = 0; i < n; ++i) vec = vec && aligned16(in[i]);
  dlsim::GwRows s;
  std::memset(&s, 0, sizeof(s));
  const int nrb = gw_class(n);
  const size_t slots = static_cast<size_t>(dlsim::gw_products(nrb)) * dlsim::kGdBlockSlots;
  // Inputs too long for 32-bit byte offsets go as consecutive ranges; every
  // range after the first accumulates.
  return for_each_range(nelem, Op::kBytes, [&](size_t o, size_t len) {
    for (int i = 0; i < n; ++i) s.p[i] = static_cast<const char*>(in[i]) + o * Op::kBytes;
    const GwGeom g = gw_geometry(len);
    // the blocks' partials, then their row masks (four 32-bit words, two doubles, per block)
    return with_partials(slots * g.blocks + 2 * static_cast<size_t>(g.blocks), st, [&](double* ws) {
      uint32_t* const masks = reinterpret_cast<uint32_t*>(ws + slots * g.blocks);
      if (nrb == 4) gw_launch_class<Op, 4>(vec, g.blocks, s, n, len, ws, masks, st);
      else if (nrb == 6) gw_launch_class<Op, 6>(vec, g.blocks, s, n, len, ws, masks, st);
      else gw_launch_class<Op, 8>(vec, g.blocks, s, n, len, ws, masks, st);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(dlsim::k_gramwide_finish<>, dim3(finish_blocks(n * (n - 1) / 2)), dim3(dlsim::kBlock), 0, st,
                         static_cast<const double*>(ws), static_cast<const uint32_t*>(masks), g.blocks, n, nrb, d2,
                         (accumulate || o > 0) ? 1 : 0);
      return hipGetLastError();
    });
  });
}

}  // namespace

// 1 <= n <= 128, dtype fp32 / bf16 / fp16, d2 apart from the inputs: checked by the caller
hipError_t gramwide_flat(const void* const* in, int n, size_t nelem, int dtype, double* d2, int accumulate,
                         hipStream_t st) {
  if (n <= kNarrowInputs) return gramdist_flat(in, n, nelem, dtype, d2, accumulate, st);
  if (nelem == 0) {  // no term: zeros, or nothing to add (as gramdist_flat)
    if (accumulate) return hipSuccess;
    return hipMemsetAsync(d2, 0, sizeof(double) * static_cast<size_t>(n) * n, st);
  }
  if (dtype == DLSIM_F32) return gw_run<dlsim::GdF32>(in, n, nelem, d2, accumulate, st);
  if (dtype == DLSIM_BF16) return gw_run<dlsim::GdBF16>(in, n, nelem, d2, accumulate, st);
  return gw_run<dlsim::GdF16>(in, n, nelem, d2, accumulate, st);
}

// The tile and grid of the kernel that serves n (no HIP call).
void gramwide_geometry(int n, int dtype, size_t nelem, size_t* tile_elems, unsigned* blocks) {
  if (n <= kNarrowInputs) return gramdist_geometry(dtype, nelem, tile_elems, blocks);
  const GwGeom g = gw_geometry(nelem);
  *tile_elems = g.tile;
  *blocks = g.blocks;
}

}  // namespace dlsim_host
