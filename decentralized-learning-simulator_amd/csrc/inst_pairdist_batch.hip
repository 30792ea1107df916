// inst_pairdist_batch.hip — instantiation unit: the batched pairwise
// squared-distance kernels (pairdist_batch_kernels.hpp) and their host
// dispatch, behind dlsim_pairwise_sqdist_batched (dlsim_abi.hip checks the
// arguments).
#include "pairdist_batch_kernels.hpp"

#include "abi_common.hpp"
#include "fanin_checks.hpp"
#include "partials.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

hipError_t pairdist_flat(const void* const* in, int n, size_t nelem, int dtype, double* d2, int accumulate,
                         hipStream_t st);

namespace {

static_assert(dlsim::kPdBatchMaxSegs == DLSIM_PAIRDIST_BATCH_MAX_SEGMENTS &&
                  dlsim::kPdBatchMaxPtrs == DLSIM_PAIRDIST_BATCH_MAX_PTRS,
              "dlsim.h states the launch limits");

// the flat kernel's classes: 0 the 4-row unit, 1 the 8-row unit, 2 diagonal and cross units
constexpr int kPdClasses = 3;
constexpr int pd_class(int n) { return n <= 4 ? 0 : n <= dlsim::kPdGroup ? 1 : 2; }

struct PdSeg {
  const void* row[dlsim::kPdMaxInputs];
  int n;
  size_t nelem;
  bool vec;
  int task;
  PdGeom g;
};

// Consecutive segments [first, first + count) of one class and form.
struct PdLaunch {
  size_t first;
  int count;
  size_t ws_off;  // doubles from the call's workspace
};

template <class Op, bool VEC>
void pd_batch_main(int cls, const dlsim::PdBatchSlots& s, unsigned grid, double* ws, hipStream_t st) {
  const dim3 g(grid), block(dlsim::kBlock);
  if (cls == 2) hipLaunchKernelGGL((dlsim::k_pairdist_batch<Op, 8, true, VEC>), g, block, 0, st, s, ws);
  else if (cls == 0) hipLaunchKernelGGL((dlsim::k_pairdist_batch<Op, 4, false, VEC>), g, block, 0, st, s, ws);
  else hipLaunchKernelGGL((dlsim::k_pairdist_batch<Op, 8, false, VEC>), g, block, 0, st, s, ws);
}

// One launch pair: segs[0 .. count) with their matrices d2s[seg.task]; started[task]: an earlier
// launch of this call has written the matrix, so this one continues by accumulation.
template <class Op>
hipError_t pd_batch_launch(int cls, const PdSeg* segs, int count, double* const* d2s, int accumulate,
                           std::vector<char>& started, double* ws, hipStream_t st) {
  dlsim::PdBatchSlots s;
  std::memset(&s, 0, sizeof(s));
  s.nsegs = count;
  uint32_t off = 0, blk = 0, wso = 0, waves = 0;
  int mats = 0;
  for (int k = 0; k < count; ++k) {
    const PdSeg& sg = segs[k];
    for (int i = 0; i < sg.n; ++i) s.p[off + i] = sg.row[i];
    s.block_start[k] = blk;
    s.blocks[k] = sg.g.blocks;
    s.ws_off[k] = wso;
    s.nelem[k] = static_cast<uint32_t>(sg.nelem);
    s.ptr_off[k] = off;
    s.fan_in[k] = static_cast<uint32_t>(sg.n);
    if (k == 0 || sg.task != segs[k - 1].task) {
      s.mat_seg[mats] = static_cast<uint32_t>(k);
      s.mat_wave[mats] = waves;
      s.mat_acc[mats] = (accumulate || started[sg.task]) ? 1u : 0u;
      s.d2[mats] = d2s[sg.task];
      started[sg.task] = 1;
      waves += static_cast<uint32_t>(sg.n * (sg.n - 1) / 2);
      ++mats;
    }
    off += static_cast<uint32_t>(sg.n);
    blk += sg.g.units * sg.g.blocks;
    wso += static_cast<uint32_t>(dlsim::kPdSlots) * sg.g.units * sg.g.blocks;
  }
  s.block_start[count] = blk;
  s.mat_seg[mats] = static_cast<uint32_t>(count);
  s.mat_wave[mats] = waves;
  s.nmats = mats;
  if (segs[0].vec) pd_batch_main<Op, true>(cls, s, blk, ws, st);
  else pd_batch_main<Op, false>(cls, s, blk, ws, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dlsim::k_pairdist_batch_finish<>, dim3(finish_blocks(static_cast<int>(waves))),
                     dim3(dlsim::kBlock), 0, st, s, static_cast<const double*>(ws), cls == 0 ? 4 : dlsim::kPdGroup);
  return hipGetLastError();
}

template <class Op>
hipError_t pd_batch(std::vector<PdSeg> (&cls)[kPdClasses], int b, double* const* d2s, int accumulate,
                    hipStream_t st) {
  // the launches of every class, then one workspace for all their partials
  std::vector<PdLaunch> launches[kPdClasses];
  size_t total = 0;
  for (int c = 0; c < kPdClasses; ++c) {
    std::vector<PdSeg>& segs = cls[c];
    int ptrs = 0;
    for (size_t k = 0; k < segs.size(); ++k) {
      PdSeg& sg = segs[k];
      sg.g = pd_geometry(sg.n, Op::E, sg.nelem, sg.vec);
      std::vector<PdLaunch>& ls = launches[c];
      if (ls.empty() || ls.back().count == dlsim::kPdBatchMaxSegs || ptrs + sg.n > dlsim::kPdBatchMaxPtrs ||
          segs[ls.back().first].vec != sg.vec) {
        ls.push_back({k, 0, total});
        ptrs = 0;
      }
      ++ls.back().count;
      ptrs += sg.n;
      total += static_cast<size_t>(dlsim::kPdSlots) * sg.g.units * sg.g.blocks;
    }
  }
  if (total == 0) return hipSuccess;
  std::vector<char> started(static_cast<size_t>(b), 0);
  return with_partials(total, st, [&](double* ws) {
    for (int c = 0; c < kPdClasses; ++c)
      for (const PdLaunch& l : launches[c]) {
        const hipError_t e =
            pd_batch_launch<Op>(c, cls[c].data() + l.first, l.count, d2s, accumulate, started, ws + l.ws_off, st);
        if (e != hipSuccess) return e;
      }
    return hipSuccess;
  });
}

}  // namespace

// Task k reads fan_in[k] * n_tensors[k] pointers, model-major, and n_tensors[k] lengths at the
// running offsets; every task checked by the caller as dlsim_pairwise_sqdist_tensors checks one, and
// no matrix shares a byte with another task's buffers. A task's non-empty tensors are its segments,
// in order. The segments are regrouped by class; inside a class they keep the list's order and a
// launch takes consecutive ones of one form (at most 32 segments and 192 pointers), so a matrix's
// segments add in the order of its tensors, across launches too. Tasks without a term (one model, no
// element) and tasks with a tensor past one launch's byte range go through pairdist_flat. So does a
// call of one task: alone, a large task measured 6 % slower behind the batch's descriptors than
// through k_pairdist (79.4 against 74.7 us at 8 x 11,181,642 fp32, the flat entry's own windows
// within 1.2 us; DESIGN.md §8n, leg (c)), and the bits are the same either way.
hipError_t pairdist_batched(int b, const int* fan_in, const int* n_tensors, const void* const* in,
                            const size_t* nelem, int dtype, double* const* d2s, int accumulate, hipStream_t st) {
  const size_t esz = elem_bytes(dtype);
  std::vector<PdSeg> cls[kPdClasses];
  size_t po = 0, lo = 0;
  for (int k = 0; k < b; ++k) {
    const int n = fan_in[k], t = n_tensors[k];
    const void* const* ptrs = in + po;
    const size_t* lens = nelem + lo;
    po += static_cast<size_t>(n) * static_cast<size_t>(t);
    lo += static_cast<size_t>(t);
    bool any = false, flat = b == 1;
    for (int j = 0; j < t; ++j) {
      any = any || lens[j] != 0;
      flat = flat || lens[j] * esz > kMaxLaunchOutBytes;
    }
    if (n == 1 || !any) {
      const hipError_t e = pairdist_flat(nullptr, n, 0, dtype, d2s[k], accumulate, st);
      if (e != hipSuccess) return e;
      continue;
    }
    PdSeg sg;
    sg.n = n;
    sg.task = k;
    bool first = true;
    for (int j = 0; j < t; ++j) {
      if (lens[j] == 0) continue;
      gather_row(ptrs, n, t, j, sg.row);
      if (flat) {
        const hipError_t e = pairdist_flat(sg.row, n, lens[j], dtype, d2s[k], (accumulate || !first) ? 1 : 0, st);
        if (e != hipSuccess) return e;
        first = false;
        continue;
      }
      sg.nelem = lens[j];
      sg.vec = true;
      for (int i = 0; i < n; ++i) sg.vec = sg.vec && aligned16(sg.row[i]);
      cls[pd_class(n)].push_back(sg);
    }
  }
  if (dtype == DLSIM_F32) return pd_batch<dlsim::PdF32>(cls, b, d2s, accumulate, st);
  if (dtype == DLSIM_BF16) return pd_batch<dlsim::PdBF16>(cls, b, d2s, accumulate, st);
  if (dtype == DLSIM_F16) return pd_batch<dlsim::PdF16>(cls, b, d2s, accumulate, st);
  return pd_batch<dlsim::PdF64>(cls, b, d2s, accumulate, st);
}

}  // namespace dlsim_host
