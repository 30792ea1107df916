// inst_sgd.hip — instantiation unit: the fresh-SGD step kernels
// (sgd_kernels.hpp) and their host dispatch, behind dlsim_sgd_step and
// dlsim_sgd_step_tensors (dlsim_abi.hip checks the arguments).
#include "sgd_kernels.hpp"

#include "dispatch.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

// The scalars as the reference's ops see them for this element type: torch
// converts the Python floats -lr and weight_decay to the tensor's dtype
// (fp32: one rounding; bf16: through fp32, c10::BFloat16's constructor;
// fp64: exact). The rule lives here and nowhere else.
template <class W>
struct SgdScalars {
  W nlr, wd;
};

template <class Op>
SgdScalars<dlsim::wt_t<Op>> sgd_scalars(double lr, double wd) {
  if constexpr (Op::kBytes == 8) {
    return {-lr, wd};
  } else if constexpr (Op::kBytes == 4) {
    return {static_cast<float>(-lr), static_cast<float>(wd)};
  } else {
    return {dlsim::sgd_host_round_bf16(static_cast<float>(-lr)),
            dlsim::sgd_host_round_bf16(static_cast<float>(wd))};
  }
}

// The 2-way reduce's launch shapes by size class (dispatch.hpp fixed_shape):
// the same three streams of the same size.
template <class Op, int C>
hipError_t sgd_launch_class(const void* p, const void* g, void* out, size_t nelem, const SgdScalars<dlsim::wt_t<Op>>& a,
                            const dlsim::CpuLayout& L, hipStream_t st) {
  constexpr Shape k = fixed_shape<Op, C>();
  const size_t nvec = nelem / Op::E;
  const size_t blocks = nvec / (static_cast<size_t>(dlsim::kBlock) * k.vpt) + 1;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL((dlsim::k_sgd_tiles<Op, k.vpt, k.store, k.wave>), dim3(static_cast<unsigned>(blocks)),
                     dim3(dlsim::kBlock), 0, st, p, g, out, nvec, nelem, a.nlr, a.wd, L);
  return hipGetLastError();
}

template <class Op>
hipError_t sgd_flat_op(const void* p, const void* g, void* out, size_t nelem, double lr, double wd, hipStream_t st) {
  const auto a = sgd_scalars<Op>(lr, wd);
  const size_t cpu_chunk = dlsim::sgd_cpu_chunk(nelem, dlsim::kSgdCpuThreads);
  if (!dlsim::sgd_aligned16(p, g, out)) {
    const size_t blocks = (nelem + dlsim::kBlock - 1) / dlsim::kBlock;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dlsim::k_sgd_scalar<Op>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0, st, p, g,
                       out, nelem, a.nlr, a.wd, dlsim::CpuLayout{nelem, cpu_chunk, 0});
    return hipGetLastError();
  }
  // buffer stores take 32-bit byte offsets: longer outputs go as consecutive
  // ranges (elements are independent; a multiple of every tile size)
  const size_t range = kMaxLaunchOutBytes / Op::kBytes;
  const int c = size_class<Op>(nelem, 2);
  for (size_t b = 0; b < nelem; b += range) {
    const size_t len = std::min(range, nelem - b);
    const char* pb = static_cast<const char*>(p) + b * Op::kBytes;
    const char* gb = static_cast<const char*>(g) + b * Op::kBytes;
    char* ob = static_cast<char*>(out) + b * Op::kBytes;
    const dlsim::CpuLayout L{nelem, cpu_chunk, b};
    const hipError_t e = c == 0   ? sgd_launch_class<Op, 0>(pb, gb, ob, len, a, L, st)
                         : c == 1 ? sgd_launch_class<Op, 1>(pb, gb, ob, len, a, L, st)
                                  : sgd_launch_class<Op, 2>(pb, gb, ob, len, a, L, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <class Op>
hipError_t sgd_tensors_op(int t, const void* const* p, const void* const* g, void* const* out, const size_t* nelem,
                          double lr, double wd, hipStream_t st) {
  const auto a = sgd_scalars<Op>(lr, wd);
  // vectors per lane by the largest tensor, as the batched reduce (batch_vpt)
  size_t mx = 0;
  for (int k = 0; k < t; ++k) mx = std::max(mx, nelem[k]);
  const int vpt = mx * Op::kBytes < kBatchSmallBytes ? 1 : 4;
  dlsim::SgdSlots s;
  std::memset(&s, 0, sizeof(s));
  size_t blocks = 0;
  auto flush = [&]() -> hipError_t {
    if (s.ntensors == 0) return hipSuccess;
    s.block_start[s.ntensors] = static_cast<uint32_t>(blocks);
    if (vpt == 1)
      hipLaunchKernelGGL((dlsim::k_sgd_batch<Op, 1>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0, st, s,
                         a.nlr, a.wd);
    else
      hipLaunchKernelGGL((dlsim::k_sgd_batch<Op, 4>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0, st, s,
                         a.nlr, a.wd);
    s.ntensors = 0;
    blocks = 0;
    return hipGetLastError();
  };
  for (int k = 0; k < t; ++k) {
    if (nelem[k] == 0) continue;
    const size_t nb = dlsim::sgd_tensor_blocks<Op>(p[k], g[k], out[k], nelem[k], vpt);
    if (nb > 0x7fffffffu) return hipErrorInvalidValue;
    if (s.ntensors == dlsim::kSgdMaxTensors || blocks + nb > 0x7fffffffu) {
      const hipError_t e = flush();
      if (e != hipSuccess) return e;
    }
    const int i = s.ntensors++;
    s.p[i] = p[k];
    s.g[i] = g[k];
    s.out[i] = out[k];
    s.nelem[i] = nelem[k];
    s.chunk[i] = dlsim::sgd_cpu_chunk(nelem[k], dlsim::kSgdCpuThreads);
    s.block_start[i] = static_cast<uint32_t>(blocks);
    blocks += nb;
  }
  return flush();
}

// f(Op{}) with the policy of (dtype, weight_decay != 0); dtype checked by the caller
template <class F>
hipError_t with_sgd_policy(int dtype, bool wd, F&& f) {
  if (dtype == DLSIM_F32) return wd ? f(dlsim::SgdF32<true>{}) : f(dlsim::SgdF32<false>{});
  if (dtype == DLSIM_BF16) return wd ? f(dlsim::SgdBF16<true>{}) : f(dlsim::SgdBF16<false>{});
  return wd ? f(dlsim::SgdF64<true>{}) : f(dlsim::SgdF64<false>{});
}

hipError_t sgd_flat(const void* p, const void* g, void* out, size_t nelem, double lr, double wd, int dtype,
                    hipStream_t st) {
  return with_sgd_policy(dtype, wd != 0.0,
                         [&](auto op) { return sgd_flat_op<decltype(op)>(p, g, out, nelem, lr, wd, st); });
}

hipError_t sgd_tensors(int t, const void* const* p, const void* const* g, void* const* out, const size_t* nelem,
                       double lr, double wd, int dtype, hipStream_t st) {
  return with_sgd_policy(dtype, wd != 0.0,
                         [&](auto op) { return sgd_tensors_op<decltype(op)>(t, p, g, out, nelem, lr, wd, st); });
}

}  // namespace dlsim_host
