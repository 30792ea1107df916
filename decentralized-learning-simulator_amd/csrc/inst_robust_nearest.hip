// inst_robust_nearest.hip — instantiation unit: the mean-around-the-median
// kernels (robust_nearest_kernels.hpp) and their host dispatch, behind
// dlsim_robust_nearest_reduce and dlsim_robust_nearest_reduce_tensors
// (dlsim_abi.hip checks the arguments). The launch shapes are inst_robust.hip's.
#include "robust_nearest_kernels.hpp"

#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

namespace {

// Vectors per lane by capacity, as inst_robust.hip's rob_vpt.
template <int CAP> constexpr int near_vpt() { return CAP >= 16 ? 1 : 16 / CAP; }

template <class Op, int CAP>
hipError_t near_launch_cap(const void* const* in, int n, int keep, void* out, size_t nelem, hipStream_t st) {
  constexpr int kVptCap = near_vpt<CAP>();
  constexpr int kStp = store_policy<Op>();
  constexpr bool kHalves = CAP == 32;
  bool aligned = aligned16(out);
  for (int i = 0; i < n; ++i) aligned = aligned && aligned16(in[i]);
  dlsim::RobSlots<CAP> s;
  std::memset(&s, 0, sizeof(s));
  if (!aligned) {
    for (int i = 0; i < n; ++i) s.p[i] = in[i];
    const size_t blocks = (nelem + dlsim::kBlock - 1) / dlsim::kBlock;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dlsim::k_nearest_scalar<Op, CAP>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0,
                       st, s, n, keep, out, nelem);
    return hipGetLastError();
  }
  // buffer stores take 32-bit byte offsets: longer outputs go as consecutive
  // ranges (elements are independent; a multiple of every tile size)
  return for_each_range(nelem, Op::kBytes, [&](size_t o, size_t len) {
    for (int i = 0; i < n; ++i) s.p[i] = static_cast<const char*>(in[i]) + o * Op::kBytes;
    void* const dst = static_cast<char*>(out) + o * Op::kBytes;
    if constexpr (kHalves) {
      const size_t nunit = len * Op::kBytes / 8;
      const size_t blocks = nunit / dlsim::kBlock + 1;
      if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
      hipLaunchKernelGGL((dlsim::k_nearest_halves<Op, CAP>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock),
                         0, st, s, n, keep, dst, nunit, len);
    } else {
      const size_t nvec = len / Op::E;
      const size_t blocks = nvec / (static_cast<size_t>(dlsim::kBlock) * kVptCap) + 1;
      if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
      hipLaunchKernelGGL((dlsim::k_nearest_tiles<Op, CAP, kVptCap, kStp>), dim3(static_cast<unsigned>(blocks)),
                         dim3(dlsim::kBlock), 0, st, s, n, keep, dst, nvec, len);
    }
    return hipGetLastError();
  });
}

template <class Op>
hipError_t near_launch(const void* const* in, int n, int keep, void* out, size_t nelem, hipStream_t st) {
  if (n <= 4) return near_launch_cap<Op, 4>(in, n, keep, out, nelem, st);
  if (n <= 8) return near_launch_cap<Op, 8>(in, n, keep, out, nelem, st);
  if (n <= 16) return near_launch_cap<Op, 16>(in, n, keep, out, nelem, st);
  return near_launch_cap<Op, 32>(in, n, keep, out, nelem, st);
}

}  // namespace

// 1 <= keep <= n <= 32, nelem > 0, dtype known, no overlap: checked by the caller
hipError_t robust_nearest_flat(const void* const* in, int n, int keep, void* out, size_t nelem, int dtype,
                               hipStream_t st) {
  if (dtype == DLSIM_F32) return near_launch<dlsim::RobF32>(in, n, keep, out, nelem, st);
  if (dtype == DLSIM_BF16) return near_launch<dlsim::RobBF16>(in, n, keep, out, nelem, st);
  if (dtype == DLSIM_F16) return near_launch<dlsim::RobF16>(in, n, keep, out, nelem, st);
  return near_launch<dlsim::RobF64>(in, n, keep, out, nelem, st);
}

}  // namespace dlsim_host
