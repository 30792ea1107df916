// fanin_checks.hpp — the argument checks and the model-major gather that the
// entries over n <= 32 inputs share (dlsim_robust_reduce, dlsim_pairwise_sqdist,
// dlsim_wreduce_dist, their _tensors and _batched forms, dlsim_abi.hip). Host code only.
#pragma once

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "abi_common.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

// dtype first (DLSIM_E_DTYPE), then 1 <= n <= max; `reason`: why max is the limit
inline int check_fan_in(int n, int max, int dtype, const char* reason) {
  if (!known_dtype(dtype) && dtype != DLSIM_F64) return fail(DLSIM_E_DTYPE, "unsupported dtype %d", dtype);
  if (n < 1) return fail(DLSIM_E_ARG, "n must be >= 1 (got %d)", n);
  if (n > max) return fail(DLSIM_E_ARG, "n must be <= %d (got %d): %s", max, n, reason);
  return DLSIM_OK;
}

inline int check_accumulate(int flag) {
  if (flag != 0 && flag != 1) return fail(DLSIM_E_ARG, "accumulate must be 0 or 1 (got %d)", flag);
  return DLSIM_OK;
}

// The n inputs of one tensor (in[i * stride], in_bytes bytes each) against the byte range [lo, hi)
// named `what`: no null input, no byte shared, exact aliasing included. The inputs may alias each
// other. Zero-byte inputs are never read: any pointer will do (torch gives null).
inline int check_inputs_apart(const void* const* in, size_t stride, int n, size_t in_bytes, uintptr_t lo, uintptr_t hi,
                              const char* what) {
  if (in_bytes == 0) return DLSIM_OK;
  for (int i = 0; i < n; ++i) {
    const void* p = in[static_cast<size_t>(i) * stride];
    if (!p) return fail(DLSIM_E_ARG, "null input pointer at index %d", i);
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p);
    if (a0 < hi && lo < a0 + in_bytes) return fail(DLSIM_E_ARG, "%s overlaps input %d", what, i);
  }
  return DLSIM_OK;
}

// The t output ranges [base + offs[k], + n_elems[k] * esz) against each other
// (the tensors run as launches in order on one stream); empty ones share nothing.
inline int check_outputs_apart(int t, const void* base, const size_t* offs, const size_t* n_elems, size_t esz) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(base);
  for (int k = 0; k < t; ++k) {
    if (n_elems[k] == 0) continue;
    const uintptr_t o0 = b + offs[k], o1 = o0 + n_elems[k] * esz;
    for (int j = 0; j < t; ++j) {
      const uintptr_t q0 = b + offs[j];
      if (j != k && n_elems[j] != 0 && q0 < o1 && o0 < q0 + n_elems[j] * esz)
        return fail(DLSIM_E_ARG, "outputs of tensors %d and %d overlap", k, j);
    }
  }
  return DLSIM_OK;
}

// The task list of dlsim_robust_reduce_batched: task t reads in[o_t .. o_t + fan_in[t]), o_t the
// running sum of the fan-ins. Per task, in order: 1 <= fan_in <= max, 0 <= lo < hi <= fan_in, then
// (non-empty tasks) a non-null output that shares no byte with the task's own inputs. The tasks
// against each other are the caller's to check (cross_task_overlap, dispatch.hpp).
inline int check_window_tasks(int b, const int* fan_in, const void* const* in, const int* lo, const int* hi,
                              void* const* outs, const size_t* n_elems, int max, int dtype, const char* reason) {
  if (!known_dtype(dtype) && dtype != DLSIM_F64) return fail(DLSIM_E_DTYPE, "unsupported dtype %d", dtype);
  const size_t esz = elem_bytes(dtype);
  size_t off = 0;
  for (int t = 0; t < b; ++t) {
    const int n = fan_in[t];
    if (n < 1) return fail(DLSIM_E_ARG, "task %d: n must be >= 1 (got %d)", t, n);
    if (n > max) return fail(DLSIM_E_ARG, "task %d: n must be <= %d (got %d): %s", t, max, n, reason);
    if (!(0 <= lo[t] && lo[t] < hi[t] && hi[t] <= n))
      return fail(DLSIM_E_ARG, "task %d: the window must satisfy 0 <= lo < hi <= n (got lo %d, hi %d, n %d)", t,
                  lo[t], hi[t], n);
    if (n_elems[t] != 0) {
      if (!outs[t]) return fail(DLSIM_E_ARG, "task %d: null output pointer", t);
      const uintptr_t o0 = reinterpret_cast<uintptr_t>(outs[t]);
      const int rc = check_inputs_apart(in + off, 1, n, n_elems[t] * esz, o0, o0 + n_elems[t] * esz, "output");
      if (rc != DLSIM_OK) return fail(rc, "task %d: %s", t, std::string(g_err).c_str());
    }
    off += static_cast<size_t>(n);
  }
  return DLSIM_OK;
}

// The task list of dlsim_pairwise_sqdist_batched: task k reads fan_in[k] * n_tensors[k] pointers,
// model-major, and n_tensors[k] lengths at the running offsets, and writes fan_in[k]^2 doubles at
// d2[k]. dtype and accumulate first; then per task, in order: 1 <= fan_in <= max, n_tensors >= 0, a
// non-null matrix; then every non-empty tensor of every task (no null pointer) against every task's
// matrix, and the matrices against each other: no byte shared.
inline int check_pairdist_tasks(int b, const int* fan_in, const int* n_tensors, const void* const* in,
                                const size_t* n_elems, double* const* d2, int max, int dtype, int accumulate,
                                const char* reason) {
  if (!known_dtype(dtype) && dtype != DLSIM_F64) return fail(DLSIM_E_DTYPE, "unsupported dtype %d", dtype);
  int rc = check_accumulate(accumulate);
  if (rc != DLSIM_OK) return rc;
  long long tensors = 0;
  for (int k = 0; k < b; ++k) {
    const int n = fan_in[k];
    if (n < 1) return fail(DLSIM_E_ARG, "task %d: n must be >= 1 (got %d)", k, n);
    if (n > max) return fail(DLSIM_E_ARG, "task %d: n must be <= %d (got %d): %s", k, max, n, reason);
    if (n_tensors[k] < 0) return fail(DLSIM_E_ARG, "task %d: n_tensors must be >= 0 (got %d)", k, n_tensors[k]);
    if (!d2[k]) return fail(DLSIM_E_ARG, "task %d: null distance matrix pointer", k);
    tensors += n_tensors[k];
  }
  if (tensors > 0 && (!in || !n_elems)) return fail(DLSIM_E_ARG, "null array argument");
  struct Mat {
    uintptr_t a, b;
    int task;
  };
  std::vector<Mat> mats(static_cast<size_t>(b));
  for (int k = 0; k < b; ++k) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(d2[k]);
    mats[static_cast<size_t>(k)] = {a, a + sizeof(double) * static_cast<size_t>(fan_in[k]) * fan_in[k], k};
  }
  std::sort(mats.begin(), mats.end(), [](const Mat& x, const Mat& y) { return x.a < y.a; });
  for (size_t k = 1; k < mats.size(); ++k)
    if (mats[k].a < mats[k - 1].b)  // sorted by start and disjoint so far: the ends are sorted too
      return fail(DLSIM_E_ARG, "the distance matrices of tasks %d and %d overlap", mats[k - 1].task, mats[k].task);
  const size_t esz = elem_bytes(dtype);
  size_t po = 0, lo = 0;
  for (int k = 0; k < b; ++k) {
    const int n = fan_in[k], t = n_tensors[k];
    for (int j = 0; j < t; ++j) {
      const size_t bytes = n_elems[lo + j] * esz;
      if (bytes == 0) continue;  // never read: any pointer will do
      for (int i = 0; i < n; ++i) {
        const void* p = in[po + static_cast<size_t>(i) * t + j];
        if (!p) return fail(DLSIM_E_ARG, "task %d, tensor %d: null input pointer at index %d", k, j, i);
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(p), a1 = a0 + bytes;
        auto it = std::upper_bound(mats.begin(), mats.end(), a0, [](uintptr_t v, const Mat& x) { return v < x.b; });
        if (it != mats.end() && it->a < a1)
          return fail(DLSIM_E_ARG, "task %d, tensor %d: the distance matrix of task %d overlaps input %d", k, j,
                      it->task, i);
      }
    }
    po += static_cast<size_t>(n) * static_cast<size_t>(t);
    lo += static_cast<size_t>(t);
  }
  return DLSIM_OK;
}

// The task list of dlsim_wreduce_dist_batched: task k reads fan_in[k] * n_tensors[k] pointers,
// model-major, n_tensors[k] lengths and output offsets and fan_in[k] weights at the running offsets,
// writes fan_in[k] doubles at d2[k] and, unless outs[k] is null, every non-empty tensor's range at
// outs[k] + out_off. dtype and accumulate first; then per task, in order: 1 <= fan_in <= max,
// n_tensors >= 0, a non-null vector, weights that survive fp32 (fp64 buffers take any); then what the
// call writes (vectors and output ranges) against each other, and every non-empty tensor of every
// task (no null pointer) against all of it: no byte shared.
inline int check_reducedist_tasks(int b, const int* fan_in, const int* n_tensors, const void* const* in,
                                  const size_t* n_elems, const size_t* out_off, const double* w, void* const* outs,
                                  double* const* d2, int max, int dtype, int accumulate, const char* reason) {
  if (!known_dtype(dtype) && dtype != DLSIM_F64) return fail(DLSIM_E_DTYPE, "unsupported dtype %d", dtype);
  int rc = check_accumulate(accumulate);
  if (rc != DLSIM_OK) return rc;
  if (!w) return fail(DLSIM_E_ARG, "null weights array");
  long long tensors = 0, out_tensors = 0;
  size_t wo = 0;
  for (int k = 0; k < b; ++k) {
    const int n = fan_in[k];
    if (n < 1) return fail(DLSIM_E_ARG, "task %d: n must be >= 1 (got %d)", k, n);
    if (n > max) return fail(DLSIM_E_ARG, "task %d: n must be <= %d (got %d): %s", k, max, n, reason);
    if (n_tensors[k] < 0) return fail(DLSIM_E_ARG, "task %d: n_tensors must be >= 0 (got %d)", k, n_tensors[k]);
    if (!d2[k]) return fail(DLSIM_E_ARG, "task %d: null distance vector pointer", k);
    if (dtype != DLSIM_F64)
      for (int i = 0; i < n; ++i)
        if (!(static_cast<double>(static_cast<float>(w[wo + i])) == w[wo + i]))
          return fail(DLSIM_E_ARG, "task %d: weight %d (%.17g) is not representable in fp32", k, i, w[wo + i]);
    wo += static_cast<size_t>(n);
    tensors += n_tensors[k];
    if (outs[k]) out_tensors += n_tensors[k];
  }
  if (tensors > 0 && (!in || !n_elems || (out_tensors > 0 && !out_off)))
    return fail(DLSIM_E_ARG, "null array argument");
  const size_t esz = elem_bytes(dtype);
  struct Wr {  // a range the call writes: task's vector (tensor < 0) or one tensor's output
    uintptr_t a, b;
    int task, tensor;
  };
  const auto name = [](const Wr& x) {
    char buf[96];
    if (x.tensor < 0) std::snprintf(buf, sizeof(buf), "the distance vector of task %d", x.task);
    else std::snprintf(buf, sizeof(buf), "the output of task %d, tensor %d", x.task, x.tensor);
    return std::string(buf);
  };
  std::vector<Wr> wr;
  size_t lo = 0;
  for (int k = 0; k < b; ++k) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(d2[k]);
    wr.push_back({a, a + sizeof(double) * static_cast<size_t>(fan_in[k]), k, -1});
    for (int j = 0; j < n_tensors[k]; ++j) {
      const size_t bytes = n_elems[lo + j] * esz;
      if (!outs[k] || bytes == 0) continue;  // nothing stored
      const uintptr_t o = reinterpret_cast<uintptr_t>(outs[k]) + out_off[lo + j];
      wr.push_back({o, o + bytes, k, j});
    }
    lo += static_cast<size_t>(n_tensors[k]);
  }
  std::sort(wr.begin(), wr.end(), [](const Wr& x, const Wr& y) { return x.a < y.a; });
  for (size_t k = 1; k < wr.size(); ++k)
    if (wr[k].a < wr[k - 1].b)  // sorted by start and disjoint so far: the ends are sorted too
      return fail(DLSIM_E_ARG, "%s overlaps %s", name(wr[k - 1]).c_str(), name(wr[k]).c_str());
  size_t po = 0;
  lo = 0;
  for (int k = 0; k < b; ++k) {
    const int n = fan_in[k], t = n_tensors[k];
    for (int j = 0; j < t; ++j) {
      const size_t bytes = n_elems[lo + j] * esz;
      if (bytes == 0) continue;  // never read: any pointer will do
      for (int i = 0; i < n; ++i) {
        const void* p = in[po + static_cast<size_t>(i) * t + j];
        if (!p) return fail(DLSIM_E_ARG, "task %d, tensor %d: null input pointer at index %d", k, j, i);
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(p), a1 = a0 + bytes;
        auto it = std::upper_bound(wr.begin(), wr.end(), a0, [](uintptr_t v, const Wr& x) { return v < x.b; });
        if (it != wr.end() && it->a < a1)
          return fail(DLSIM_E_ARG, "task %d, tensor %d: %s overlaps input %d", k, j, name(*it).c_str(), i);
      }
    }
    po += static_cast<size_t>(n) * static_cast<size_t>(t);
    lo += static_cast<size_t>(t);
  }
  return DLSIM_OK;
}

// row[i] = tensor k of model i, from the model-major in[i * t + k]
inline void gather_row(const void* const* in, int n, int t, int k, const void** row) {
  for (int i = 0; i < n; ++i) row[i] = in[static_cast<size_t>(i) * static_cast<size_t>(t) + k];
}

}  // namespace dlsim_host
