// robust_nearest_kernels.hpp — gfx950 streaming kernels for the mean around
// the median (MeaMed / Phocas; the second stage of Bulyan).
// The reference has no such code: its one aggregator is FedAvg
// (dasklearn/gradient_aggregation/fedavg.py). These kernels are
// robust_kernels.hpp's (the same keys, sorting network, element policies,
// RobSlots, loads, stores and launch shapes) with the window chosen per
// element instead of per launch.
//
// Contract, per output element, over its n values and 1 <= keep <= n:
//   s = the values sorted ascending in robust_kernels.hpp's total order
//   m = (n-1)/2, p = s[m]
//   d[j] = +0.0 where s[j] has p's sort key, else fl(|s[j] - p|): one
//          subtraction in the accumulator type; ranked 0 <= ... <= +Inf < NaN
//   the window [lo, lo+keep) starts as [m, m+1) and grows keep - 1 times: by
//   the right neighbour iff it exists and the left one does not exist or is
//   strictly farther (ties go left)
//   acc = s[lo]; for j = lo+1 .. lo+keep-1: acc = acc + s[j]; result = acc / keep
//   rounding and NaN canonicalisation as dlsim_robust_reduce
//
// The walk is not run. Distances never decrease away from m, so
//   lo = m - l,  l = #{ t in 1 .. min(m, keep-1) : m+keep-t > n-1  or  !(d[m+keep-t] < d[m-t]) }
// (tests/test_nearest_cpu.py checks this form against the walk). A distance is
// held as the unsigned integer whose order is its rank: the bits of |x|, all
// ones for a NaN. Pad slots sort to positions >= n and map back to a NaN, so
// their rank is all ones and "past n-1" needs no test of its own. Each
// condition compares two positions exactly `keep` apart and keep is
// wave-uniform: a copy of the ranks is shifted down by keep in log2(CAP)+1
// stages of whole-array moves under scalar predicates, then compared slot by
// slot. l is per lane; the windowed sum runs over the CAP unrolled positions
// under a per-lane predicate, adding nothing where the predicate is false (a
// select, not a multiplication: Inf and NaN outside the window do not leak).
// No register array is indexed by a run-time value, nothing goes to scratch.
#pragma once

#include "robust_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

// rank of a distance |x| as an unsigned integer: 0 <= ... <= +Inf < NaN
__device__ __forceinline__ uint32_t near_rank(float x) {
  return x != x ? ~uint32_t{0} : (__float_as_uint(x) & 0x7fffffffu);
}
__device__ __forceinline__ uint64_t near_rank(double x) {
  return x != x ? ~uint64_t{0} : (__builtin_bit_cast(uint64_t, x) & 0x7fffffffffffffffull);
}

// a[j] = a[j + keep] (all ones past the end), keep in [0, CAP] wave-uniform:
// one stage per bit of keep, the widest shift first (the later, narrower ones
// then move only the slots that are still read)
template <int CAP, int SH, class R>
__device__ __forceinline__ void near_shift(R (&a)[CAP], int keep) {
  if (keep & SH) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) a[j] = j + SH < CAP ? a[j + SH] : static_cast<R>(~R(0));
  }
  if constexpr (SH > 1) near_shift<CAP, SH / 2>(a, keep);
}

// The window mean's numerator for one element. key_at(pos) / value_at(pos):
// the sorted key and its value (accumulator type) at a position; both are
// called with unrolled, hence constant, positions only.
template <int CAP, class T, class KF, class VF>
__device__ __forceinline__ T near_window(int n, int keep, KF&& key_at, VF&& value_at) {
  using R = decltype(near_rank(T{}));
  const int m = (n - 1) >> 1;
  auto pk = key_at(0);
  T p = value_at(0);
#pragma unroll
  for (int pos = 1; pos < CAP / 2; ++pos)
    if (pos == m) {
      pk = key_at(pos);
      p = value_at(pos);
    }
  R d[CAP], far[CAP];
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    d[j] = key_at(j) == pk ? R(0) : near_rank(value_at(j) - p);
    far[j] = d[j];
  }
  near_shift<CAP, CAP>(far, keep);  // far[j] = d[j + keep]
  int l = 0;
#pragma unroll
  for (int j = 0; j < CAP / 2; ++j)
    if (j < m && j > m - keep) l += far[j] < d[j] ? 0 : 1;
  const int lo = m - l;
  T acc = 0;
#pragma unroll
  for (int pos = 0; pos < CAP; ++pos) {
    if (pos > m - keep && pos < m + keep && pos < n) {  // wave-uniform: where any lane's window can lie
      const T x = value_at(pos);
      const int rel = pos - lo;
      acc = rel == 0 ? x : (rel > 0 && rel < keep) ? acc + x : acc;
    }
  }
  return acc;
}

// One element, any alignment (the < E tail and misaligned buffers).
template <class Op, int CAP, class S>
__device__ __forceinline__ void near_scalar_elem(const S& s, int n, int keep, void* out, size_t j) {
  using SK = typename Op::SKey;
  decltype(rob_bits(acc_t<Op>{})) k[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    if (i < n) k[i] = SK::to_key(rob_bits(load_elem<Op>(s.ptr(i), j)));
    else k[i] = SK::kPad;
  }
  rob_sort<CAP>(k);
  const acc_t<Op> a = near_window<CAP, acc_t<Op>>(
      n, keep, [&](int pos) { return k[pos]; }, [&](int pos) { return rob_value(SK::from_key(k[pos])); });
  store_elem<Op>(out, j, a, static_cast<float>(keep));
}

template <class Op, int CAP>
__global__ __launch_bounds__(kBlock) void k_nearest_scalar(const RobSlots<CAP> s, int n, int keep,
                                                           void* __restrict__ out, size_t nelem) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < nelem) near_scalar_elem<Op, CAP>(s, n, keep, out, j);
}

// Sort the CAP keys k (vectors of EV elements each) and write the numerators
// of their EV elements to a[0 .. EV).
template <class Op, int CAP, int EV, class V>
__device__ __forceinline__ void near_sort_window(V (&k)[CAP], int n, int keep, acc_t<Op>* a) {
  using Key = typename Op::Key;
  rob_sort<CAP>(k);
#pragma unroll
  for (int e = 0; e < EV; ++e)
    a[e] = near_window<CAP, acc_t<Op>>(
        n, keep, [&](int pos) { return rob_lane(k[pos], e); },
        [&](int pos) { return Op::from_bits(Key::from_key(rob_lane(k[pos], e))); });
}

// One tile, as rob_tile.
template <class Op, int CAP, int VPT, bool CHECK, int STP, class S>
__device__ __forceinline__ void near_tile(const S& s, int n, int keep, const OutRef& out, size_t v0, size_t nvec) {
  using Key = typename Op::Key;
  using K = typename Op::K;
  using KV = typename Op::KV;
  u32x4 r[CAP][VPT];
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < n) load_tile<Op, VPT, 1, CHECK>(s.ptr(i), v0, nvec, r[i]);
  const float div = static_cast<float>(keep);
#pragma unroll
  for (int v = 0; v < VPT; ++v) {
    KV k[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
      if (i < n) k[i] = Key::to_key(__builtin_bit_cast(KV, r[i][v]));
      else k[i] = rob_splat<KV, K>(Key::kPad);
    }
    acc_t<Op> a[Op::E];
    near_sort_window<Op, CAP, Op::E>(k, n, keep, a);
    const size_t idx = v0 + static_cast<size_t>(v) * kBlock;
    if (!CHECK || idx < nvec) store_vec<STP>(out, idx, pack<Op>(a, div));
  }
}

// Block 0 takes the ragged end, blocks 1.. one full tile each, as k_robust_tiles.
template <class Op, int CAP, int VPT, int STP>
__global__ __launch_bounds__(kBlock) void k_nearest_tiles(const RobSlots<CAP> s, int n, int keep,
                                                          void* __restrict__ out, size_t nvec, size_t nelem) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  const size_t full = nvec / kTile;
  const OutRef o = make_out<STP>(out, nvec);
  const size_t nb = gridDim.x;
  if (blockIdx.x == 0) {
    if (full * kTile < nvec) near_tile<Op, CAP, VPT, true, STP>(s, n, keep, o, full * kTile + threadIdx.x, nvec);
    const size_t j = nvec * Op::E + threadIdx.x;
    if (j < nelem) near_scalar_elem<Op, CAP>(s, n, keep, out, j);
    if (nb > 1) return;
  }
  const size_t workers = nb > 1 ? nb - 1 : 1;
  const size_t first = nb > 1 ? blockIdx.x - 1 : 0;
  for (size_t t = first; t < full; t += workers)
    near_tile<Op, CAP, VPT, false, STP>(s, n, keep, o, t * kTile + threadIdx.x, nvec);
}

// Half a vector per lane (capacity 32), as rob_half_tile.
template <class Op, int CAP, bool CHECK, class S>
__device__ __forceinline__ void near_half_tile(const S& s, int n, int keep, void* out, size_t u0, size_t nunit) {
  using Key = typename Op::Key;
  using K = typename Op::K;
  using HV = decltype(typename Op::KV{}.lo);
  u32x2 r[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < n) {
      r[i] = u32x2{0u, 0u};
      if (!CHECK || u0 < nunit) r[i] = __builtin_nontemporal_load(static_cast<const u32x2*>(s.ptr(i)) + u0);
    }
  HV k[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    if (i < n) k[i] = Key::to_key(__builtin_bit_cast(HV, r[i]));
    else k[i] = rob_splat<HV, K>(Key::kPad);
  }
  // pack() takes a whole vector: the upper half is zeros and its result unused
  acc_t<Op> a[Op::E];
#pragma unroll
  for (int e = 0; e < Op::E; ++e) a[e] = 0;
  near_sort_window<Op, CAP, Op::E / 2>(k, n, keep, a);
  const u32x4 full = pack<Op>(a, static_cast<float>(keep));
  if (!CHECK || u0 < nunit) __builtin_nontemporal_store(u32x2{full[0], full[1]}, static_cast<u32x2*>(out) + u0);
}

template <class Op, int CAP>
__global__ __launch_bounds__(kBlock) void k_nearest_halves(const RobSlots<CAP> s, int n, int keep,
                                                           void* __restrict__ out, size_t nunit, size_t nelem) {
  const size_t full = nunit / kBlock;
  const size_t nb = gridDim.x;
  if (blockIdx.x == 0) {
    if (full * kBlock < nunit) near_half_tile<Op, CAP, true>(s, n, keep, out, full * kBlock + threadIdx.x, nunit);
    const size_t j = nunit * (Op::E / 2) + threadIdx.x;
    if (j < nelem) near_scalar_elem<Op, CAP>(s, n, keep, out, j);
    if (nb > 1) return;
  }
  const size_t workers = nb > 1 ? nb - 1 : 1;
  const size_t first = nb > 1 ? blockIdx.x - 1 : 0;
  for (size_t t = first; t < full; t += workers)
    near_half_tile<Op, CAP, false>(s, n, keep, out, t * kBlock + threadIdx.x, nunit);
}

}  // namespace dlsim
