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

// ---- MX sharing (dlsim_mx_*) ----
inline size_t mx_code_bytes(size_t n_elems, int format) { return format == DLSIM_MX_FP4_E2M1 ? (n_elems + 1) / 2 : n_elems; }
inline size_t mx_scale_bytes(size_t n_elems) { return (n_elems + DLSIM_MX_BLOCK - 1) / DLSIM_MX_BLOCK; }

// dtype (DLSIM_E_DTYPE), format and length of every MX entry
inline int check_mx_format(int dtype, int format, size_t n_elems, const char* entry) {
  if (dtype != DLSIM_F32 && dtype != DLSIM_BF16)
    return fail(DLSIM_E_DTYPE, "%s takes DLSIM_F32 and DLSIM_BF16 (got dtype %d): the dtypes of the shipped configurations",
                entry, dtype);
  if (format < DLSIM_MX_FP8_E4M3 || format > DLSIM_MX_FP4_E2M1)
    return fail(DLSIM_E_ARG, "unknown format %d (DLSIM_MX_FP8_E4M3, DLSIM_MX_FP8_E5M2 or DLSIM_MX_FP4_E2M1)", format);
  if (n_elems >> 31) return fail(DLSIM_E_ARG, "n_elems must be < 2^31 (got %zu): the kernels index elements in 32 bits", n_elems);
  return DLSIM_OK;
}

// A buffer of one MX entry: its name in messages, its range. A null pointer with bytes == 0 is an absent buffer.
struct NamedRange {
  const char* name;
  const void* p;
  size_t bytes;
};

// no byte shared between any two of the k buffers, in the order given
inline int check_ranges_apart(const NamedRange* r, int k) {
  for (int i = 0; i < k; ++i)
    for (int j = i + 1; j < k; ++j) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(r[i].p), b = reinterpret_cast<uintptr_t>(r[j].p);
      if (r[i].bytes && r[j].bytes && a < b + r[j].bytes && b < a + r[i].bytes)
        return fail(DLSIM_E_ARG, "the %s overlaps the %s", r[i].name, r[j].name);
    }
  return DLSIM_OK;
}

// The task list of dlsim_mx_wreduce_batched (b >= 1, the arrays laid out as dlsim_quant_wreduce_batched's): per
// task, in order: 0 <= m <= max_m, n_elems < 2^31, non-null dense row and output that coincide or share nothing;
// per neighbour a known format and, in a non-empty task, non-null codes and scales. Then the outputs against
// each other and against everything any other task reads, and against their own task's codes and scales: one
// launch runs its tasks concurrently.
inline int check_mx_reduce_tasks(int b, const void* const* self, const int* m, const void* const* codes,
                                 const void* const* scales, const int* formats, const float* w, void* const* outs,
                                 const size_t* n_elems, size_t esz, int max_m) {
  if (!self || !m || !w || !outs || !n_elems) return fail(DLSIM_E_ARG, "null array argument");
  struct Rg {  // a range some task reads (its dense row: task >= 0; a code or scale buffer: -1 - task) or writes
    uintptr_t a, b;
    int task;
  };
  std::vector<Rg> reads, writes;
  size_t slot = 0;
  for (int t = 0; t < b; ++t) {
    if (m[t] < 0 || m[t] > max_m) return fail(DLSIM_E_ARG, "task %d: m must satisfy 0 <= m <= %d (got %d)", t, max_m, m[t]);
    if (m[t] > 0 && (!codes || !scales || !formats)) return fail(DLSIM_E_ARG, "null array argument");
    const size_t P = n_elems[t];
    if (P >> 31)
      return fail(DLSIM_E_ARG, "task %d: n_elems must be < 2^31 (got %zu): the kernels index elements in 32 bits", t, P);
    if (P && (!self[t] || !outs[t])) return fail(DLSIM_E_ARG, "task %d: null dense row or output pointer", t);
    if (P) {
      const uintptr_t s0 = reinterpret_cast<uintptr_t>(self[t]), o0 = reinterpret_cast<uintptr_t>(outs[t]);
      if (s0 != o0 && s0 < o0 + P * esz && o0 < s0 + P * esz)
        return fail(DLSIM_E_ARG, "task %d: output partially overlaps the dense row", t);
      reads.push_back({s0, s0 + P * esz, t});
      writes.push_back({o0, o0 + P * esz, t});
    }
    for (int j = 0; j < m[t]; ++j, ++slot) {
      if (formats[slot] < DLSIM_MX_FP8_E4M3 || formats[slot] > DLSIM_MX_FP4_E2M1)
        return fail(DLSIM_E_ARG, "task %d, neighbour %d: unknown format %d", t, j, formats[slot]);
      if (P == 0) continue;  // never read: any pointer will do
      if (!codes[slot] || !scales[slot]) return fail(DLSIM_E_ARG, "task %d, neighbour %d: null code or scale pointer", t, j);
      const uintptr_t c0 = reinterpret_cast<uintptr_t>(codes[slot]), z0 = reinterpret_cast<uintptr_t>(scales[slot]);
      reads.push_back({c0, c0 + mx_code_bytes(P, formats[slot]), -1 - t});
      reads.push_back({z0, z0 + mx_scale_bytes(P), -1 - t});
    }
  }
  std::sort(writes.begin(), writes.end(), [](const Rg& x, const Rg& y) { return x.a < y.a; });
  for (size_t i = 1; i < writes.size(); ++i)
    if (writes[i].a < writes[i - 1].b)
      return fail(DLSIM_E_ARG, "the outputs of tasks %d and %d overlap", writes[i - 1].task, writes[i].task);
  for (const Rg& r : reads) {
    auto it = std::upper_bound(writes.begin(), writes.end(), r.a, [](uintptr_t v, const Rg& x) { return v < x.b; });
    for (; it != writes.end() && it->a < r.b; ++it) {
      if (r.task == it->task) continue;  // a task's own dense row (exact or no overlap: checked above)
      if (r.task < 0)
        return fail(DLSIM_E_ARG, "the output of task %d overlaps the codes or scales of task %d", it->task, -1 - r.task);
      return fail(DLSIM_E_ARG, "the output of task %d overlaps the dense row of task %d", it->task, r.task);
    }
  }
  return DLSIM_OK;
}

// row[i] = tensor k of model i, from the model-major in[i * t + k]
inline void gather_row(const void* const* in, int n, int t, int k, const void** row) {
  for (int i = 0; i < n; ++i) row[i] = in[static_cast<size_t>(i) * static_cast<size_t>(t) + k];
}

}  // namespace dlsim_host
