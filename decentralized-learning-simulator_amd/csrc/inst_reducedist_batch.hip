// inst_reducedist_batch.hip — instantiation unit: the batched "reduce and
// measure" kernels (reducedist_batch_kernels.hpp) and their host dispatch,
// behind dlsim_wreduce_dist_batched and dlsim_reducedist_batch_geometry
// (dlsim_abi.hip checks the arguments).
#include "reducedist_batch_kernels.hpp"

#include "abi_common.hpp"
#include "fanin_checks.hpp"
#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

hipError_t reducedist_flat(const void* const* in, int n, const double* w, void* out, size_t nelem, int dtype,
                           double* d2, int accumulate, hipStream_t st);

namespace {

static_assert(dlsim::kRdBatchMaxSegs == DLSIM_REDUCEDIST_BATCH_MAX_SEGMENTS, "dlsim.h states the launch limit");

// the flat kernel's capacities: CAP 4, 8, 16, 32
constexpr int kRdClasses = 4;
constexpr int rd_class(int n) { return n <= 4 ? 0 : n <= 8 ? 1 : n <= 16 ? 2 : 3; }

struct RdSeg {
  const void* row[dlsim::kRdMaxInputs];
  const double* w;  // the task's n weights
  void* out;        // null: distances only
  int n;
  size_t nelem;
  bool vec;
  int task;
  RdGeom g;
};

// Consecutive segments [first, first + count) of one class and form.
struct RdLaunch {
  size_t first;
  int count;
  size_t ws_off;  // doubles from the call's workspace
};

template <class Op, bool VEC, class S>
void rd_batch_main(int cls, const S& s, unsigned grid, double* ws, hipStream_t st) {
  const dim3 g(grid), block(dlsim::kBlock);
  if (cls == 0) hipLaunchKernelGGL((dlsim::k_reducedist_batch<Op, 4, VEC>), g, block, 0, st, s, ws);
  else if (cls == 1) hipLaunchKernelGGL((dlsim::k_reducedist_batch<Op, 8, VEC>), g, block, 0, st, s, ws);
  else if (cls == 2) hipLaunchKernelGGL((dlsim::k_reducedist_batch<Op, 16, VEC>), g, block, 0, st, s, ws);
  else hipLaunchKernelGGL((dlsim::k_reducedist_batch<Op, 32, VEC>), g, block, 0, st, s, ws);
}

// One launch pair: segs[0 .. count) with their vectors d2s[seg.task]; started[task]: an earlier
// launch of this call has written the vector, so this one continues by accumulation.
template <class Op>
hipError_t rd_batch_launch(int cls, const RdSeg* segs, int count, double* const* d2s, int accumulate,
                           std::vector<char>& started, double* ws, hipStream_t st) {
  using W = dlsim::wt_t<typename Op::Fold>;
  dlsim::RdBatchSlots<W> s;
  std::memset(&s, 0, sizeof(s));
  s.nsegs = count;
  uint32_t off = 0, blk = 0, wso = 0, waves = 0;
  int vecs = 0;
  for (int k = 0; k < count; ++k) {
    const RdSeg& sg = segs[k];
    for (int i = 0; i < sg.n; ++i) {
      s.p[off + i] = sg.row[i];
      s.w[off + i] = static_cast<W>(sg.w[i]);
    }
    s.out[k] = sg.out;
    s.block_start[k] = blk;
    s.blocks[k] = sg.g.blocks;
    s.ws_off[k] = wso;
    s.nelem[k] = static_cast<uint32_t>(sg.nelem);
    s.ptr_off[k] = off;
    s.fan_in[k] = static_cast<uint32_t>(sg.n);
    if (k == 0 || sg.task != segs[k - 1].task) {
      s.vec_seg[vecs] = static_cast<uint32_t>(k);
      s.vec_wave[vecs] = waves;
      s.vec_acc[vecs] = (accumulate || started[sg.task]) ? 1u : 0u;
      s.d2[vecs] = d2s[sg.task];
      started[sg.task] = 1;
      waves += static_cast<uint32_t>(sg.n);
      ++vecs;
    }
    off += static_cast<uint32_t>(sg.n);
    blk += sg.g.blocks;
    wso += static_cast<uint32_t>(sg.g.cap) * sg.g.blocks;
  }
  s.block_start[count] = blk;
  s.vec_seg[vecs] = static_cast<uint32_t>(count);
  s.vec_wave[vecs] = waves;
  s.nvecs = vecs;
  if (segs[0].vec) rd_batch_main<Op, true>(cls, s, blk, ws, st);
  else rd_batch_main<Op, false>(cls, s, blk, ws, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dlsim::k_reducedist_batch_finish<W>, dim3(finish_blocks(static_cast<int>(waves))),
                     dim3(dlsim::kBlock), 0, st, s, static_cast<const double*>(ws));
  return hipGetLastError();
}

template <class Op>
hipError_t rd_batch(std::vector<RdSeg> (&cls)[kRdClasses], int b, double* const* d2s, int accumulate,
                    hipStream_t st) {
  using F = typename Op::Fold;
  constexpr int kMaxPtrs = dlsim::rd_batch_max_ptrs<dlsim::wt_t<F>>();
  // the launches of every class, then one workspace for all their partials
  std::vector<RdLaunch> launches[kRdClasses];
  size_t total = 0;
  for (int c = 0; c < kRdClasses; ++c) {
    std::vector<RdSeg>& segs = cls[c];
    int ptrs = 0;
    for (size_t k = 0; k < segs.size(); ++k) {
      RdSeg& sg = segs[k];
      sg.g = rd_geometry(sg.n, F::kBytes, sg.nelem, sg.vec);
      std::vector<RdLaunch>& ls = launches[c];
      if (ls.empty() || ls.back().count == dlsim::kRdBatchMaxSegs || ptrs + sg.n > kMaxPtrs ||
          segs[ls.back().first].vec != sg.vec) {
        ls.push_back({k, 0, total});
        ptrs = 0;
      }
      ++ls.back().count;
      ptrs += sg.n;
      total += static_cast<size_t>(sg.g.cap) * sg.g.blocks;
    }
  }
  if (total == 0) return hipSuccess;
  std::vector<char> started(static_cast<size_t>(b), 0);
  return with_partials(total, st, [&](double* ws) {
    for (int c = 0; c < kRdClasses; ++c)
      for (const RdLaunch& l : launches[c]) {
        const hipError_t e =
            rd_batch_launch<Op>(c, cls[c].data() + l.first, l.count, d2s, accumulate, started, ws + l.ws_off, st);
        if (e != hipSuccess) return e;
      }
    return hipSuccess;
  });
}

}  // namespace

// Task k reads fan_in[k] * n_tensors[k] pointers, model-major, n_tensors[k] lengths and output
// offsets and fan_in[k] weights at the running offsets; every task checked by the caller as
// dlsim_wreduce_dist_tensors checks one, and no output or vector shares a byte with another task's
// buffers. A task's non-empty tensors are its segments, in order. The segments are regrouped by
// capacity class; inside a class they keep the list's order and a launch takes consecutive ones of
// one form (at most 32 segments and the weight type's pointer limit), so a vector's segments add in
// the order of its tensors, across launches too. Tasks without an element and tasks with a tensor
// past one launch's byte range go through reducedist_flat, as does a call of one task (the
// precedent of pairdist_batched; the bits are the same either way).
hipError_t reducedist_batched(int b, const int* fan_in, const int* n_tensors, const void* const* in,
                              const size_t* nelem, const size_t* out_off, const double* w, void* const* outs,
                              int dtype, double* const* d2s, int accumulate, hipStream_t st) {
  const size_t esz = elem_bytes(dtype);
  std::vector<RdSeg> cls[kRdClasses];
  size_t po = 0, lo = 0, wo = 0;
  for (int k = 0; k < b; ++k) {
    const int n = fan_in[k], t = n_tensors[k];
    const void* const* ptrs = in + po;
    const size_t* lens = nelem + lo;
    const size_t* offs = out_off ? out_off + lo : nullptr;
    const double* wk = w + wo;
    po += static_cast<size_t>(n) * static_cast<size_t>(t);
    lo += static_cast<size_t>(t);
    wo += static_cast<size_t>(n);
    bool any = false, flat = b == 1;
    for (int j = 0; j < t; ++j) {
      any = any || lens[j] != 0;
      flat = flat || lens[j] * esz > kMaxLaunchOutBytes;
    }
    if (!any) {
      const hipError_t e = reducedist_flat(nullptr, n, wk, nullptr, 0, dtype, d2s[k], accumulate, st);
      if (e != hipSuccess) return e;
      continue;
    }
    RdSeg sg;
    sg.n = n;
    sg.task = k;
    sg.w = wk;
    bool first = true;
    for (int j = 0; j < t; ++j) {
      if (lens[j] == 0) continue;
      gather_row(ptrs, n, t, j, sg.row);
      sg.out = outs[k] ? static_cast<char*>(outs[k]) + offs[j] : nullptr;
      if (flat) {
        const hipError_t e =
            reducedist_flat(sg.row, n, wk, sg.out, lens[j], dtype, d2s[k], (accumulate || !first) ? 1 : 0, st);
        if (e != hipSuccess) return e;
        first = false;
        continue;
      }
      sg.nelem = lens[j];
      sg.vec = !sg.out || aligned16(sg.out);
      for (int i = 0; i < n; ++i) sg.vec = sg.vec && aligned16(sg.row[i]);
      cls[rd_class(n)].push_back(sg);
    }
  }
  if (dtype == DLSIM_F32) return rd_batch<dlsim::RdF32>(cls, b, d2s, accumulate, st);
  if (dtype == DLSIM_BF16) return rd_batch<dlsim::RdBF16>(cls, b, d2s, accumulate, st);
  if (dtype == DLSIM_F16) return rd_batch<dlsim::RdF16>(cls, b, d2s, accumulate, st);
  return rd_batch<dlsim::RdF64>(cls, b, d2s, accumulate, st);
}

// The limits of one launch for this dtype's weight type (no HIP call).
void reducedist_batch_geometry(int dtype, int* max_segments, int* max_ptrs) {
  *max_segments = dlsim::kRdBatchMaxSegs;
  *max_ptrs = dtype == DLSIM_F64 ? dlsim::rd_batch_max_ptrs<double>() : dlsim::rd_batch_max_ptrs<float>();
}

}  // namespace dlsim_host
