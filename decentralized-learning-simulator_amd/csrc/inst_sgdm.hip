// inst_sgdm.hip — instantiation unit: the momentum-SGD step kernels
// (sgdm_kernels.hpp) and their host dispatch, behind dlsim_sgd_momentum_step
// and dlsim_sgd_momentum_step_tensors (dlsim_abi.hip checks the arguments).
#include "sgdm_kernels.hpp"

#include "dispatch.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

namespace {

// The scalars as the reference's ops see them for this element type: -lr and
// weight_decay are `alpha`s, converted to the tensor's dtype (fp32: one
// rounding; bf16: through fp32 to bf16; fp64: exact); momentum is mul_'s
// scalar, which bf16 keeps in fp32 (ATen's opmath type). The rule lives here
// and nowhere else.
template <class Op>
dlsim::SgdmArgs<dlsim::wt_t<Op>> sgdm_scalars(double lr, double mom, double wd) {
  if constexpr (Op::kBytes == 8) {
    return {-lr, mom, wd};
  } else if constexpr (Op::kBytes == 4) {
    return {static_cast<float>(-lr), static_cast<float>(mom), static_cast<float>(wd)};
  } else {
    return {dlsim::sgd_host_round_bf16(static_cast<float>(-lr)), static_cast<float>(mom),
            dlsim::sgd_host_round_bf16(static_cast<float>(wd))};
  }
}

// The fresh-SGD step's launch shapes by size class (dispatch.hpp fixed_shape,
// fan-in 2): streams of the same size, one more read and one more write.
template <class Op, int C>
hipError_t sgdm_launch_class(const void* p, const void* g, const void* b, void* pout, void* bout, size_t nelem,
                             const dlsim::SgdmArgs<dlsim::wt_t<Op>>& a, const dlsim::CpuLayout& L, hipStream_t st) {
  constexpr Shape k = fixed_shape<Op, C>();
  const size_t nvec = nelem / Op::E;
  const size_t blocks = nvec / (static_cast<size_t>(dlsim::kBlock) * k.vpt) + 1;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL((dlsim::k_sgdm_tiles<Op, k.vpt, k.store, k.wave>), dim3(static_cast<unsigned>(blocks)),
                     dim3(dlsim::kBlock), 0, st, p, g, b, pout, bout, nvec, nelem, a, L);
  return hipGetLastError();
}

template <class Op>
hipError_t sgdm_flat_op(const void* p, const void* g, const void* b, void* pout, void* bout, size_t nelem, double lr,
                        double mom, double wd, hipStream_t st) {
  const auto a = sgdm_scalars<Op>(lr, mom, wd);
  const size_t cpu_chunk = dlsim::sgd_cpu_chunk(nelem, dlsim::kSgdCpuThreads);
  if (!dlsim::sgdm_aligned16(p, g, b, pout, bout)) {
    const size_t blocks = (nelem + dlsim::kBlock - 1) / dlsim::kBlock;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dlsim::k_sgdm_scalar<Op>), dim3(static_cast<unsigned>(blocks)), dim3(dlsim::kBlock), 0, st, p,
                       g, b, pout, bout, nelem, a, dlsim::CpuLayout{nelem, cpu_chunk, 0});
    return hipGetLastError();
  }
  // buffer stores take 32-bit byte offsets: longer outputs go as consecutive
  // ranges (elements are independent; a multiple of every tile size)
  const size_t range = kMaxLaunchOutBytes / Op::kBytes;
  const int c = size_class<Op>(nelem, 2);
  for (size_t o = 0; o < nelem; o += range) {
    const size_t len = std::min(range, nelem - o);
    const size_t ob = o * Op::kBytes;
    const char* pb = static_cast<const char*>(p) + ob;
    const char* gb = static_cast<const char*>(g) + ob;
    const char* bb = b ? static_cast<const char*>(b) + ob : nullptr;
    char* po = static_cast<char*>(pout) + ob;
    char* bo = static_cast<char*>(bout) + ob;
    const dlsim::CpuLayout L{nelem, cpu_chunk, o};
    const hipError_t e = c == 0   ? sgdm_launch_class<Op, 0>(pb, gb, bb, po, bo, len, a, L, st)
                         : c == 1 ? sgdm_launch_class<Op, 1>(pb, gb, bb, po, bo, len, a, L, st)
                                  : sgdm_launch_class<Op, 2>(pb, gb, bb, po, bo, len, a, L, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <class OpFirst, class OpLater>
hipError_t sgdm_tensors_op(int t, const void* const* p, const void* const* g, const void* const* b,
                           void* const* pout, void* const* bout, const size_t* nelem, double lr, double mom, double wd,
                           hipStream_t st) {
  using Op = OpLater;
  const auto a = sgdm_scalars<Op>(lr, mom, wd);
  // vectors per lane by the largest tensor, as the batched reduce (batch_vpt)
  size_t mx = 0;
  for (int k = 0; k < t; ++k) mx = std::max(mx, nelem[k]);
  const int vpt = mx * Op::kBytes < kBatchSmallBytes ? 1 : 4;
  dlsim::SgdmSlots s;
  std::memset(&s, 0, sizeof(s));
  size_t blocks = 0;
  auto flush = [&]() -> hipError_t {
    if (s.ntensors == 0) return hipSuccess;
    s.block_start[s.ntensors] = static_cast<uint32_t>(blocks);
    if (vpt == 1)
      hipLaunchKernelGGL((dlsim::k_sgdm_batch<OpFirst, OpLater, 1>), dim3(static_cast<unsigned>(blocks)),
                         dim3(dlsim::kBlock), 0, st, s, a);
    else
      hipLaunchKernelGGL((dlsim::k_sgdm_batch<OpFirst, OpLater, 4>), dim3(static_cast<unsigned>(blocks)),
                         dim3(dlsim::kBlock), 0, st, s, a);
    s.ntensors = 0;
    blocks = 0;
    return hipGetLastError();
  };
  for (int k = 0; k < t; ++k) {
    if (nelem[k] == 0) continue;
    const size_t nb = dlsim::sgdm_tensor_blocks<Op>(p[k], g[k], b[k], pout[k], bout[k], nelem[k], vpt);
    if (nb > 0x7fffffffu) return hipErrorInvalidValue;
    if (s.ntensors == dlsim::kSgdmMaxTensors || blocks + nb > 0x7fffffffu) {
      const hipError_t e = flush();
      if (e != hipSuccess) return e;
    }
    const int i = s.ntensors++;
    s.p[i] = p[k];
    s.g[i] = g[k];
    s.b[i] = b[k];
    s.pout[i] = pout[k];
    s.bout[i] = bout[k];
    s.nelem[i] = nelem[k];
    s.block_start[i] = static_cast<uint32_t>(blocks);
    blocks += nb;
  }
  return flush();
}

// f(OpFirst{}, OpLater{}) with the policies of (dtype, weight_decay != 0); dtype checked by the caller
template <class F>
hipError_t with_sgdm_policy(int dtype, bool wd, F&& f) {
  if (dtype == DLSIM_F32)
    return wd ? f(dlsim::SgdmF32<true, true>{}, dlsim::SgdmF32<true, false>{})
              : f(dlsim::SgdmF32<false, true>{}, dlsim::SgdmF32<false, false>{});
  if (dtype == DLSIM_BF16)
    return wd ? f(dlsim::SgdmBF16<true, true>{}, dlsim::SgdmBF16<true, false>{})
              : f(dlsim::SgdmBF16<false, true>{}, dlsim::SgdmBF16<false, false>{});
  return wd ? f(dlsim::SgdmF64<true, true>{}, dlsim::SgdmF64<true, false>{})
            : f(dlsim::SgdmF64<false, true>{}, dlsim::SgdmF64<false, false>{});
}

}  // namespace

// b == nullptr: the first step (buf_out = g')
hipError_t sgdm_flat(const void* p, const void* g, const void* b, void* pout, void* bout, size_t nelem, double lr,
                     double mom, double wd, int dtype, hipStream_t st) {
  return with_sgdm_policy(dtype, wd != 0.0, [&](auto first, auto later) {
    if (b == nullptr) return sgdm_flat_op<decltype(first)>(p, g, b, pout, bout, nelem, lr, mom, wd, st);
    return sgdm_flat_op<decltype(later)>(p, g, b, pout, bout, nelem, lr, mom, wd, st);
  });
}

hipError_t sgdm_tensors(int t, const void* const* p, const void* const* g, const void* const* b, void* const* pout,
                        void* const* bout, const size_t* nelem, double lr, double mom, double wd, int dtype,
                        hipStream_t st) {
  return with_sgdm_policy(dtype, wd != 0.0, [&](auto first, auto later) {
    return sgdm_tensors_op<decltype(first), decltype(later)>(t, p, g, b, pout, bout, nelem, lr, mom, wd, st);
  });
}

}  // namespace dlsim_host
