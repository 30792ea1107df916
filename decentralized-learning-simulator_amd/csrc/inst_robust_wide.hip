// inst_robust_wide.hip — instantiation unit: the wide order-statistic kernels
// (robust_wide_kernels.hpp, 33 <= n <= 128) and their host dispatch, behind
// dlsim_robust_reduce_wide, dlsim_robust_reduce_wide_tensors and
// dlsim_robust_wide_geometry (dlsim_abi.hip checks the arguments). n <= 32 is
// inst_robust.hip's.
#include "robust_wide_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

hipError_t robust_flat(const void* const* in, int n, int lo, int hi, void* out, size_t nelem, int dtype,
                       hipStream_t st);

namespace {

// lanes that share one element's values: the compiled class of n rows
int rw_class(int n) { return n <= dlsim::kRobMaxInputs ? 1 : n <= 2 * dlsim::kRwSlots ? 2 : 4; }

// 32 < n <= 32 G, nelem > 0. No allocation, no synchronisation: two kinds of launch.
template <class Op, int G>
hipError_t rw_launch(const void* const* in, int n, int lo, int hi, void* out, size_t nelem, hipStream_t st) {
  constexpr size_t kGroups = dlsim::rw_groups<G>();
  bool aligned = aligned16(out);
  for (int i = 0; i < n; ++i) aligned = aligned && aligned16(in[i]);
  dlsim::RwRows<G> s;
  std::memset(&s, 0, sizeof(s));
  if (!aligned) {
    for (int i = 0; i < n; ++i) s.p[i] = in[i];
    const size_t blocks = (nelem + kGroups - 1) / kGroups;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dlsim::k_robust_wide_elems<Op, G>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0,
                       st, s, n, lo, hi, out, nelem);
    return hipGetLastError();
  }
  // longer outputs go as consecutive ranges of 32-bit byte offsets, as the
  // n <= 32 kernels' (elements are independent; a multiple of every tile size)
  return for_each_range(nelem, Op::kBytes, [&](size_t o, size_t len) {
    for (int i = 0; i < n; ++i) s.p[i] = static_cast<const char*>(in[i]) + o * Op::kBytes;
    void* const dst = static_cast<char*>(out) + o * Op::kBytes;
    const size_t nunit = len * Op::kBytes / 8;
    const size_t blocks = nunit / kGroups + 1;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dlsim::k_robust_wide<Op, G>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0, st,
                       s, n, lo, hi, dst, nunit, len);
    return hipGetLastError();
  });
}

template <class Op>
hipError_t rw_run(const void* const* in, int n, int lo, int hi, void* out, size_t nelem, hipStream_t st) {
  if (rw_class(n) == 2) return rw_launch<Op, 2>(in, n, lo, hi, out, nelem, st);
  return rw_launch<Op, 4>(in, n, lo, hi, out, nelem, st);
}

}  // namespace

// 1 <= n <= 128, 0 <= lo < hi <= n, nelem > 0, dtype known, no overlap: checked by the caller
hipError_t robust_wide_flat(const void* const* in, int n, int lo, int hi, void* out, size_t nelem, int dtype,
                            hipStream_t st) {
  if (rw_class(n) == 1) return robust_flat(in, n, lo, hi, out, nelem, dtype, st);
  if (dtype == DLSIM_F32) return rw_run<dlsim::RobF32>(in, n, lo, hi, out, nelem, st);
  if (dtype == DLSIM_BF16) return rw_run<dlsim::RobBF16>(in, n, lo, hi, out, nelem, st);
  if (dtype == DLSIM_F16) return rw_run<dlsim::RobF16>(in, n, lo, hi, out, nelem, st);
  return rw_run<dlsim::RobF64>(in, n, lo, hi, out, nelem, st);
}

// The tile of the kernel that serves n and the lanes that share an element
// there (no HIP call). n <= 32: a block of k_robust_halves's units for 17..32,
// of k_robust_tiles's vectors below.
void robust_wide_geometry(int n, int dtype, size_t* tile_elems, int* lanes_per_elem) {
  const size_t esz = dtype == DLSIM_F64 ? 8 : dtype == DLSIM_F32 ? 4 : 2;
  const int g = rw_class(n);
  *lanes_per_elem = g;
  if (g > 1) *tile_elems = static_cast<size_t>(dlsim::kBlock / g) * (8 / esz);
  else if (n > 16) *tile_elems = static_cast<size_t>(dlsim::kBlock) * (8 / esz);
  else *tile_elems = static_cast<size_t>(dlsim::kBlock) * (n <= 4 ? 4 : n <= 8 ? 2 : 1) * (16 / esz);
}

}  // namespace dlsim_host
