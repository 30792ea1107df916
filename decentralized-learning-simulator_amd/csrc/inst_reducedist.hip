// inst_reducedist.hip — instantiation unit: the fused "reduce and measure"
// kernels (reducedist_kernels.hpp) and their host dispatch, behind
// dlsim_wreduce_dist, dlsim_wreduce_dist_tensors and dlsim_reducedist_geometry
// (dlsim_abi.hip checks the arguments).
#include "reducedist_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

// vec: every base is 16-byte aligned (partials.hpp: a segment of a batched launch takes it too)
RdGeom rd_geometry(int n, int elem_bytes, size_t nelem, bool vec) {
  RdGeom g;
  g.cap = n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32;
  g.tile = static_cast<size_t>(dlsim::kBlock) * (vec ? dlsim::rd_width_bytes(elem_bytes, g.cap) / elem_bytes : 1);
  const size_t tiles = (nelem + g.tile - 1) / g.tile;
  g.blocks = static_cast<unsigned>(std::min<size_t>(kDistGridBlocks, std::max<size_t>(tiles, 1)));
  return g;
}

namespace {

template <class Op, bool VEC, class S>
void rd_launch_main(const RdGeom& g, const S& s, int n, void* out, size_t nelem, double* ws, hipStream_t st) {
  const dim3 grid(g.blocks), block(dlsim::kBlock);
  if (g.cap == 4) hipLaunchKernelGGL((dlsim::k_reducedist<Op, 4, VEC>), grid, block, 0, st, s, n, out, nelem, ws);
  else if (g.cap == 8) hipLaunchKernelGGL((dlsim::k_reducedist<Op, 8, VEC>), grid, block, 0, st, s, n, out, nelem, ws);
  else if (g.cap == 16) hipLaunchKernelGGL((dlsim::k_reducedist<Op, 16, VEC>), grid, block, 0, st, s, n, out, nelem, ws);
  else hipLaunchKernelGGL((dlsim::k_reducedist<Op, 32, VEC>), grid, block, 0, st, s, n, out, nelem, ws);
}

// 1 <= n <= 32, nelem > 0; out may be null
template <class Op>
hipError_t rd_run(const void* const* in, int n, const double* w, void* out, size_t nelem, double* d2, int accumulate,
                  hipStream_t st) {
  using F = typename Op::Fold;
  using W = dlsim::wt_t<F>;
  bool vec = !out || aligned16(out);
  for (int i = 0; i < n; ++i) vec = vec && aligned16(in[i]);
  dlsim::RdSlots<W> s;
  std::memset(&s, 0, sizeof(s));
  for (int i = 0; i < n; ++i) s.w[i] = static_cast<W>(w[i]);
  // Ranges too long for one launch's 32-bit byte offsets go as consecutive
  // pieces; every piece after the first accumulates.
  return for_each_range(nelem, F::kBytes, [&](size_t o, size_t len) {
    for (int i = 0; i < n; ++i) s.p[i] = static_cast<const char*>(in[i]) + o * F::kBytes;
    void* const outp = out ? static_cast<char*>(out) + o * F::kBytes : nullptr;
    const RdGeom g = rd_geometry(n, F::kBytes, len, vec);
    return with_partials(static_cast<size_t>(g.cap) * g.blocks, st, [&](double* ws) {
      if (vec) rd_launch_main<Op, true>(g, s, n, outp, len, ws, st);
      else rd_launch_main<Op, false>(g, s, n, outp, len, ws, st);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(dlsim::k_reducedist_finish<>, dim3(finish_blocks(n)), dim3(dlsim::kBlock), 0, st,
                         static_cast<const double*>(ws), g.blocks, n, d2, (accumulate || o > 0) ? 1 : 0);
      return hipGetLastError();
    });
  });
}

}  // namespace

// 1 <= n <= 32, dtype known, weights representable, buffers apart: checked by the caller
hipError_t reducedist_flat(const void* const* in, int n, const double* w, void* out, size_t nelem, int dtype,
                           double* d2, int accumulate, hipStream_t st) {
  if (nelem == 0) {  // no term: zeros, or nothing to add
    if (accumulate) return hipSuccess;
    return hipMemsetAsync(d2, 0, sizeof(double) * static_cast<size_t>(n), st);
  }
  if (dtype == DLSIM_F32) return rd_run<dlsim::RdF32>(in, n, w, out, nelem, d2, accumulate, st);
  if (dtype == DLSIM_BF16) return rd_run<dlsim::RdBF16>(in, n, w, out, nelem, d2, accumulate, st);
  if (dtype == DLSIM_F16) return rd_run<dlsim::RdF16>(in, n, w, out, nelem, d2, accumulate, st);
  return rd_run<dlsim::RdF64>(in, n, w, out, nelem, d2, accumulate, st);
}

// The 16-byte aligned path's tile and grid (no HIP call).
void reducedist_geometry(int n, int dtype, size_t nelem, size_t* tile_elems, unsigned* blocks) {
  const RdGeom g = rd_geometry(n, dtype == DLSIM_F64 ? 8 : dtype == DLSIM_F32 ? 4 : 2, nelem, true);
  *tile_elems = g.tile;
  *blocks = g.blocks;
}

}  // namespace dlsim_host
