// inst_pairdist.hip — instantiation unit: the pairwise squared-distance
// kernels (pairdist_kernels.hpp) and their host dispatch, behind
// dlsim_pairwise_sqdist, dlsim_pairwise_sqdist_tensors and
// dlsim_pairdist_geometry (dlsim_abi.hip checks the arguments).
#include "pairdist_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

// (PdGeom: partials.hpp)
PdGeom pd_geometry(int n, int elems16, size_t nelem, bool vec) {
  PdGeom g;
  g.cap = n <= 4 ? 4 : dlsim::kPdGroup;
  g.cross = n > dlsim::kPdGroup;
  const unsigned groups = static_cast<unsigned>((n + dlsim::kPdGroup - 1) / dlsim::kPdGroup);
  g.units = g.cross ? groups * groups : 1;  // G diagonal + 2 * G (G - 1) / 2 cross
  g.active = 1;
  if (g.cross) {
    g.active = 0;
    for (unsigned a = 0; a < groups; ++a) {
      if (n - static_cast<int>(a) * dlsim::kPdGroup >= 2) ++g.active;
      for (unsigned b = a + 1; b < groups; ++b)
        for (int half = 0; half < 2; ++half)
          if (n - static_cast<int>(b) * dlsim::kPdGroup - half * dlsim::kPdCross >= 1) ++g.active;
    }
  }
  g.tile = static_cast<size_t>(dlsim::kBlock) * (vec ? elems16 : 1);
  const size_t tiles = (nelem + g.tile - 1) / g.tile;
  const size_t cap = kDistGridBlocks / g.active;
  g.blocks = static_cast<unsigned>(std::min(cap, std::max<size_t>(tiles, 1)));
  return g;
}

namespace {

template <class Op, bool VEC>
void pd_launch_main(const PdGeom& g, const dlsim::PdSlots& s, int n, size_t nelem, double* ws, hipStream_t st) {
  const dim3 grid(g.blocks, g.units), block(dlsim::kBlock);
  if (g.cross) hipLaunchKernelGGL((dlsim::k_pairdist<Op, 8, true, VEC>), grid, block, 0, st, s, n, nelem, ws);
  else if (g.cap == 4) hipLaunchKernelGGL((dlsim::k_pairdist<Op, 4, false, VEC>), grid, block, 0, st, s, n, nelem, ws);
  else hipLaunchKernelGGL((dlsim::k_pairdist<Op, 8, false, VEC>), grid, block, 0, st, s, n, nelem, ws);
}

// 2 <= n <= 32, nelem > 0
template <class Op>
hipError_t pd_run(const void* const* in, int n, size_t nelem, double* d2, int accumulate, hipStream_t st) {
  bool vec = true;
  for (int i = 0; i < n; ++i) vec = vec && aligned16(in[i]);
  dlsim::PdSlots s;
  std::memset(&s, 0, sizeof(s));
  // Inputs too long for 32-bit byte offsets go as consecutive ranges; every
  // range after the first accumulates.
  return for_each_range(nelem, Op::kBytes, [&](size_t o, size_t len) {
    for (int i = 0; i < n; ++i) s.p[i] = static_cast<const char*>(in[i]) + o * Op::kBytes;
    const PdGeom g = pd_geometry(n, Op::E, len, vec);
    return with_partials(static_cast<size_t>(dlsim::kPdSlots) * g.units * g.blocks, st, [&](double* ws) {
      if (vec) pd_launch_main<Op, true>(g, s, n, len, ws, st);
      else pd_launch_main<Op, false>(g, s, n, len, ws, st);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(dlsim::k_pairdist_finish<>, dim3(finish_blocks(n * (n - 1) / 2)), dim3(dlsim::kBlock), 0, st,
                         static_cast<const double*>(ws), g.blocks, n, g.cap, d2, (accumulate || o > 0) ? 1 : 0);
      return hipGetLastError();
    });
  });
}

int pd_elems16(int dtype) { return dtype == DLSIM_F64 ? 2 : dtype == DLSIM_F32 ? 4 : 8; }

}  // namespace

// 1 <= n <= 32, dtype known, d2 apart from the inputs: checked by the caller
hipError_t pairdist_flat(const void* const* in, int n, size_t nelem, int dtype, double* d2, int accumulate,
                         hipStream_t st) {
  if (n == 1 || nelem == 0) {  // no term: zeros, or nothing to add
    if (accumulate) return hipSuccess;
    return hipMemsetAsync(d2, 0, sizeof(double) * static_cast<size_t>(n) * n, st);
  }
  if (dtype == DLSIM_F32) return pd_run<dlsim::PdF32>(in, n, nelem, d2, accumulate, st);
  if (dtype == DLSIM_BF16) return pd_run<dlsim::PdBF16>(in, n, nelem, d2, accumulate, st);
  if (dtype == DLSIM_F16) return pd_run<dlsim::PdF16>(in, n, nelem, d2, accumulate, st);
  return pd_run<dlsim::PdF64>(in, n, nelem, d2, accumulate, st);
}

// The 16-byte aligned path's tile and grid (no HIP call).
void pairdist_geometry(int n, int dtype, size_t nelem, size_t* tile_elems, unsigned* blocks) {
  const PdGeom g = pd_geometry(n, pd_elems16(dtype), nelem, true);
  *tile_elems = g.tile;
  *blocks = g.blocks;
}

}  // namespace dlsim_host
