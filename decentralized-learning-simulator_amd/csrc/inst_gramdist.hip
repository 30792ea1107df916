// inst_gramdist.hip — instantiation unit: the Gram-matrix squared-distance
// kernels (gramdist_kernels.hpp) and their host dispatch, behind
// dlsim_gram_sqdist, dlsim_gram_sqdist_tensors and dlsim_gramdist_geometry
// (dlsim_abi.hip checks the arguments).
#include "gramdist_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

namespace {

// Blocks of one launch: two resident blocks (two waves per SIMD, so that one
// wave's loads run under the other's matrix instructions) on each of the 256
// CUs of an MI355X. A constant, so that the summation order is the same on
// every device.
constexpr unsigned kGramGridBlocks = 512;

struct GdGeom {
  size_t tile;      // elements a block takes per step
  unsigned blocks;  // grid
};

// elems16: elements of a 16-byte vector; vec: every base is 16-byte aligned
GdGeom gd_geometry(int elems16, size_t nelem, bool vec) {
  GdGeom g;
  g.tile = static_cast<size_t>(dlsim::kGdTileItems) * (vec ? elems16 : 1);
  const size_t tiles = (nelem + g.tile - 1) / g.tile;
  g.blocks = static_cast<unsigned>(std::min<size_t>(kGramGridBlocks, std::max<size_t>(tiles, 1)));
  return g;
}

template <class Op, bool VEC>
void gd_launch_main(unsigned blocks, const dlsim::PdSlots& s, int n, size_t nelem, double* ws, uint32_t* masks,
                    hipStream_t st) {
  const dim3 grid(blocks), block(dlsim::kBlock);
  if (n <= dlsim::kGdRows) hipLaunchKernelGGL((dlsim::k_gramdist<Op, 1, VEC>), grid, block, 0, st, s, n, nelem, ws, masks);
  else hipLaunchKernelGGL((dlsim::k_gramdist<Op, 2, VEC>), grid, block, 0, st, s, n, nelem, ws, masks);
}

// 2 <= n <= 32, nelem > 0
template <class Op>
hipError_t gd_run(const void* const* in, int n, size_t nelem, double* d2, int accumulate, hipStream_t st) {
  bool vec = true;
  for (int i = 0; i < n; ++i) vec = vec && aligned16(in[i]);
  dlsim::PdSlots s;
  std::memset(&s, 0, sizeof(s));
  const size_t slots = static_cast<size_t>(n <= dlsim::kGdRows ? 1 : 3) * dlsim::kGdBlockSlots;
  // Inputs too long for 32-bit byte offsets go as consecutive ranges; every
  // range after the first accumulates.
  return for_each_range(nelem, Op::kBytes, [&](size_t o, size_t len) {
    for (int i = 0; i < n; ++i) s.p[i] = static_cast<const char*>(in[i]) + o * Op::kBytes;
    const GdGeom g = gd_geometry(Op::E, len, vec);
    // the blocks' partials, then their row masks (two 32-bit masks to a double)
    return with_partials(slots * g.blocks + (g.blocks + 1) / 2, st, [&](double* ws) {
      uint32_t* const masks = reinterpret_cast<uint32_t*>(ws + slots * g.blocks);
      if (vec) gd_launch_main<Op, true>(g.blocks, s, n, len, ws, masks, st);
      else gd_launch_main<Op, false>(g.blocks, s, n, len, ws, masks, st);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(dlsim::k_gramdist_finish<>, dim3(finish_blocks(n * (n - 1) / 2)), dim3(dlsim::kBlock), 0, st,
                         static_cast<const double*>(ws), static_cast<const uint32_t*>(masks), g.blocks, n, d2,
                         (accumulate || o > 0) ? 1 : 0);
      return hipGetLastError();
    });
  });
}

}  // namespace

// 1 <= n <= 32, dtype fp32 / bf16 / fp16, d2 apart from the inputs: checked by the caller
hipError_t gramdist_flat(const void* const* in, int n, size_t nelem, int dtype, double* d2, int accumulate,
                         hipStream_t st) {
  if (n == 1 || nelem == 0) {  // no term: zeros, or nothing to add (as pairdist_flat)
    if (accumulate) return hipSuccess;
    return hipMemsetAsync(d2, 0, sizeof(double) * static_cast<size_t>(n) * n, st);
  }
  if (dtype == DLSIM_F32) return gd_run<dlsim::GdF32>(in, n, nelem, d2, accumulate, st);
  if (dtype == DLSIM_BF16) return gd_run<dlsim::GdBF16>(in, n, nelem, d2, accumulate, st);
  return gd_run<dlsim::GdF16>(in, n, nelem, d2, accumulate, st);
}

// The 16-byte aligned path's tile and grid (no HIP call).
void gramdist_geometry(int dtype, size_t nelem, size_t* tile_elems, unsigned* blocks) {
  const GdGeom g = gd_geometry(dtype == DLSIM_F32 ? 4 : 8, nelem, true);
  *tile_elems = g.tile;
  *blocks = g.blocks;
}

}  // namespace dlsim_host
