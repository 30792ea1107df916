// inst_robust_batch.hip — instantiation unit: the batched order-statistic
// kernel (robust_batch_kernels.hpp) and its host dispatch, behind
// dlsim_robust_reduce_batched and dlsim_robust_reduce_tensors_batched
// (dlsim_abi.hip checks the arguments).
#include "robust_batch_kernels.hpp"

#include "abi_common.hpp"
#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

hipError_t robust_flat(const void* const* in, int n, int lo, int hi, void* out, size_t nelem, int dtype,
                       hipStream_t st);

namespace {

constexpr int rob_class(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }

struct RobBatchTask {
  const void* const* in;
  int n, lo, hi;
  void* out;
  size_t nelem;
};

// Tasks g[0 .. count) of one class in one launch: count <= 32, their fan-ins
// sum to <= 192, each output below the single-launch byte limit.
template <class Op, int CAP>
hipError_t rob_batch_launch(const RobBatchTask* g, int count, hipStream_t st) {
  dlsim::RobBatchSlots s;
  std::memset(&s, 0, sizeof(s));
  s.ntasks = count;
  uint32_t off = 0;
  size_t blk = 0;
  for (int t = 0; t < count; ++t) {
    const RobBatchTask& k = g[t];
    bool aligned = aligned16(k.out);
    for (int i = 0; i < k.n; ++i) {
      s.p[off + i] = k.in[i];
      aligned = aligned && aligned16(k.in[i]);
    }
    s.out[t] = k.out;
    s.nelem[t] = k.nelem;
    s.ptr_off[t] = off;
    s.fan_in[t] = static_cast<uint32_t>(k.n);
    s.lo[t] = static_cast<uint32_t>(k.lo);
    s.hi[t] = static_cast<uint32_t>(k.hi);
    s.scalar[t] = aligned ? 0u : 1u;
    s.block_start[t] = static_cast<uint32_t>(blk);
    blk += k.nelem / (aligned ? dlsim::rob_batch_tile_elems<Op, CAP>() : static_cast<size_t>(dlsim::kBlock));
    off += static_cast<uint32_t>(k.n);
  }
  s.block_start[count] = static_cast<uint32_t>(blk);
  const size_t blocks = blk + static_cast<size_t>(count);
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL((dlsim::k_robust_batch<Op, CAP, store_policy<Op>()>), dim3(static_cast<unsigned>(blocks)),
                     dim3(dlsim::kBlock), 0, st, s);
  return hipGetLastError();
}

template <class Op, int CAP>
hipError_t rob_batch_class(const std::vector<RobBatchTask>& tasks, hipStream_t st) {
  std::vector<RobBatchTask> g;
  g.reserve(dlsim::kRobBatchMaxTasks);
  int ptrs = 0;
  auto flush = [&]() {
    const hipError_t e = g.empty() ? hipSuccess : rob_batch_launch<Op, CAP>(g.data(), static_cast<int>(g.size()), st);
    g.clear();
    ptrs = 0;
    return e;
  };
  for (const RobBatchTask& k : tasks) {
    if (rob_class(k.n) != CAP) continue;
    if (static_cast<int>(g.size()) == dlsim::kRobBatchMaxTasks || ptrs + k.n > dlsim::kRobBatchMaxPtrs) {
      const hipError_t e = flush();
      if (e != hipSuccess) return e;
    }
    g.push_back(k);
    ptrs += k.n;
  }
  return flush();
}

template <class Op>
hipError_t rob_batch(const std::vector<RobBatchTask>& tasks, hipStream_t st) {
  hipError_t e = rob_batch_class<Op, 4>(tasks, st);
  if (e == hipSuccess) e = rob_batch_class<Op, 8>(tasks, st);
  if (e == hipSuccess) e = rob_batch_class<Op, 16>(tasks, st);
  if (e == hipSuccess) e = rob_batch_class<Op, 32>(tasks, st);
  return e;
}

}  // namespace

// Task t reads in[o_t .. o_t + fan_in[t]) (o_t the running sum of the fan-ins).
// Every task checked by the caller as robust_flat's, and no output shares a
// byte with another task's buffers: the tasks are regrouped by capacity class
// (launches in class order, each split at 32 tasks / 192 pointers), so they
// run in no promised order. Empty tasks are skipped; a task whose output
// exceeds one launch's byte limit goes alone through robust_flat.
hipError_t robust_batched(int b, const int* fan_in, const void* const* in, const int* lo, const int* hi,
                          void* const* outs, const size_t* nelem, int dtype, hipStream_t st) {
  const size_t esz = elem_bytes(dtype);
  std::vector<RobBatchTask> tasks;
  tasks.reserve(static_cast<size_t>(b));
  size_t off = 0;
  for (int t = 0; t < b; ++t) {
    const void* const* row = in + off;
    off += static_cast<size_t>(fan_in[t]);
    if (nelem[t] == 0) continue;
    if (nelem[t] * esz > kMaxLaunchOutBytes) {
      const hipError_t e = robust_flat(row, fan_in[t], lo[t], hi[t], outs[t], nelem[t], dtype, st);
      if (e != hipSuccess) return e;
      continue;
    }
    tasks.push_back({row, fan_in[t], lo[t], hi[t], outs[t], nelem[t]});
  }
  if (tasks.empty()) return hipSuccess;
  if (dtype == DLSIM_F32) return rob_batch<dlsim::RobF32>(tasks, st);
  if (dtype == DLSIM_BF16) return rob_batch<dlsim::RobBF16>(tasks, st);
  if (dtype == DLSIM_F16) return rob_batch<dlsim::RobF16>(tasks, st);
  return rob_batch<dlsim::RobF64>(tasks, st);
}

// elements of one full tile of an aligned task of fan-in n (its capacity class)
size_t robust_batch_tile_elems(int n, int dtype) {
  auto by_class = [&](auto op) -> size_t {
    using Op = decltype(op);
    switch (rob_class(n)) {
      case 4: return dlsim::rob_batch_tile_elems<Op, 4>();
      case 8: return dlsim::rob_batch_tile_elems<Op, 8>();
      case 16: return dlsim::rob_batch_tile_elems<Op, 16>();
      default: return dlsim::rob_batch_tile_elems<Op, 32>();
    }
  };
  if (dtype == DLSIM_F32) return by_class(dlsim::RobF32{});
  if (dtype == DLSIM_BF16) return by_class(dlsim::RobBF16{});
  if (dtype == DLSIM_F16) return by_class(dlsim::RobF16{});
  return by_class(dlsim::RobF64{});
}

}  // namespace dlsim_host
