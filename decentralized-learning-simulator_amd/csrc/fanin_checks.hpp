// fanin_checks.hpp — the argument checks and the model-major gather that the
// entries over n <= 32 inputs share (dlsim_robust_reduce, dlsim_pairwise_sqdist,
// dlsim_wreduce_dist and their _tensors forms, dlsim_abi.hip). Host code only.
#pragma once

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

// row[i] = tensor k of model i, from the model-major in[i * t + k]
inline void gather_row(const void* const* in, int n, int t, int k, const void** row) {
  for (int i = 0; i < n; ++i) row[i] = in[static_cast<size_t>(i) * static_cast<size_t>(t) + k];
}

}  // namespace dlsim_host
