// robust_wide_kernels.hpp — gfx950 kernels for the coordinate-wise
// order-statistic aggregators over 33 to 128 models. The
// contract is robust_kernels.hpp's, bit for bit; the split of the work is new.
// There one lane holds all CAP keys of its elements; a one-lane network of 128
// is 1,471 exchanges over 128 live key registers. Here a group of G lanes
// shares one 8-byte unit (2 fp32, 1 fp64 or 4 16-bit elements): G = 2 for
// n <= 64, G = 4 for n <= 128, 32 key vectors per lane in both, as
// k_robust_halves keeps.
//
// Lanes. A group is the lanes l, l + 16 (G = 2) and also l + 32, l + 48
// (G = 4) of a wave, l in 0..15: the lanes v_permlane16_swap_b32 and
// v_permlane32_swap_b32 pair up. The lane's rank q in its group is its 16-lane
// row (G = 4) or the row's parity (G = 2, two sets of groups per wave). Rank q
// loads rows 32q .. min(32q + 31, n - 1) of its unit, non-temporally, and pads
// the rest with the pad key; a 16-lane row reads 128 contiguous bytes of each
// of its rows. The row pointers are the kernel's first argument; a lane loads
// its 32 from the kernarg segment at a lane-varying offset (indexing the
// by-value struct with q would make the compiler keep a private copy).
//
// Sort. Keys are stored as y = key ^ m with m zero or all ones per lane:
// complementing reverses the unsigned order, so a lane that sorts y ascending
// with the fixed network holds its keys descending where m is all ones. That
// is how one network and "same slot, lower lane keeps the minimum" serve every
// step (q0 = bit 0 of q, q1 = bit 1):
//   1. y = key ^ (q0 ? ~0 : 0); rob_sort<32> in the lane (191 exchanges).
//   2. y ^= (q0 ^ q1 ? ~0 : 0): both lanes of a pair l, l ^ 16 now share the
//      mask (q1 ? ~0 : 0) and one of them runs ascending, the other
//      descending. Same-slot exchange across lane ^ 16 (32), the 5-stage
//      half-cleaner cascade in the lane (80). G = 2: sorted. G = 4: ranks
//      0, 1 hold a 64-run ascending, ranks 2, 3 (complemented) one that
//      descends over (rank 2's slots, rank 3's slots).
//   3. G = 4: y ^= (q1 ? ~0 : 0), all plain keys again. Same-slot exchange
//      across lane ^ 32 (the ascending run against the descending one: the
//      lower 64 stay in ranks 0, 1), same-slot half-clean across lane ^ 16,
//      the cascade again.
// 303 exchanges per lane for G = 2, 447 for G = 4, and 64 or 96 v_xor. Rank q
// ends with sorted positions 32q .. 32q + 31, ascending.
//
// The cross-lane exchange works on two slots i, j at once and needs no select
// and no copy. v_permlane16_swap_b32 a, b swaps the odd rows of a with the
// even rows of b: after swap(k[i], k[j]) a lane of an even row holds its own
// and its partner's k[i], a lane of an odd row its partner's and its own
// k[j]. One min and one max, and swap(min, max) leaves the minima of slots i
// and j in the even row and the maxima in the odd row. v_permlane32_swap_b32
// does the same for the wave's halves. Per pair of slots and dword: two
// swaps, half a min and half a max per slot. All 64 lanes are active in every
// swap: ragged lanes load nothing, sort zeros and skip the store.
//
// Window. The sum has to stay sequential to keep the bits. Phase r = 0 .. G-1
// is skipped unless [32r, 32r + 32) meets [lo, hi) (kernel arguments, so
// wave-uniform: the median runs one phase). In it every lane continues acc
// over its own 32 slots under the wave-uniform predicate lo <= 32r + i < hi;
// rank r's result is the true one and is broadcast to its group (two swaps)
// if the window goes on. The lane of rank (hi - 1) / 32 divides, rounds,
// canonicalises NaN and stores its 8-byte unit non-temporally.
//
// Ragged end and unaligned buffers: the same group sort over one element per
// group through load_elem / store_elem (keys of the accumulator's width, as
// rob_scalar_elem). Block 0 takes the last partial tile of units and the
// elements past the last whole unit, blocks 1.. one full tile each.
#pragma once

#include "robust_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kRwMaxInputs = 128;
constexpr int kRwSlots = 32;  // key vectors per lane

template <int G>
struct RwRows {
  const void* p[kRwSlots * G];
};

// the units (or elements) of a block: one per group
template <int G> constexpr int rw_groups() { return kBlock / G; }

// Row `row`'s pointer out of the kernarg segment (RwRows is the first argument).
__device__ __forceinline__ const void* rw_row_ptr(int row) {
  typedef const void* Ptr;
  const __attribute__((address_space(4))) Ptr* const args =
      (const __attribute__((address_space(4))) Ptr*)__builtin_amdgcn_kernarg_segment_ptr();
  return args[row];
}

// ---- a key vector as dwords ----------------------------------------------------------
template <class V>
struct RwWords {
  uint32_t w[sizeof(V) / 4];
};

template <int SW>
__device__ __forceinline__ void rw_swap(uint32_t& a, uint32_t& b) {
  static_assert(SW == 16 || SW == 32, "rows of 16 lanes or halves of 32");
  u32x2 r;
  if constexpr (SW == 16) r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  else r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}

template <int SW, class V>
__device__ __forceinline__ void rw_swap_vec(V& a, V& b) {
  RwWords<V> x = __builtin_bit_cast(RwWords<V>, a), y = __builtin_bit_cast(RwWords<V>, b);
#pragma unroll
  for (int d = 0; d < static_cast<int>(sizeof(V) / 4); ++d) rw_swap<SW>(x.w[d], y.w[d]);
  a = __builtin_bit_cast(V, x);
  b = __builtin_bit_cast(V, y);
}

// k[i] ^= mask in every dword (mask zero or all ones: the order reversed or kept)
template <class V>
__device__ __forceinline__ void rw_flip(V (&k)[kRwSlots], uint32_t mask) {
#pragma unroll
  for (int i = 0; i < kRwSlots; ++i) {
    RwWords<V> x = __builtin_bit_cast(RwWords<V>, k[i]);
#pragma unroll
    for (int d = 0; d < static_cast<int>(sizeof(V) / 4); ++d) x.w[d] ^= mask;
    k[i] = __builtin_bit_cast(V, x);
  }
}

// Same-slot compare-exchange with the lane at lane ^ SW, every slot: the lane
// whose bit SW is clear keeps the minima (the header comment).
template <int SW, class V>
__device__ __forceinline__ void rw_cross(V (&k)[kRwSlots]) {
#pragma unroll
  for (int i = 0; i < kRwSlots; i += 2) {
    V a = k[i], b = k[i + 1];
    rw_swap_vec<SW>(a, b);
    V lo = __builtin_elementwise_min(a, b);
    V hi = __builtin_elementwise_max(a, b);
    rw_swap_vec<SW>(lo, hi);
    k[i] = lo;
    k[i + 1] = hi;
  }
}

// A bitonic sequence of 32 to ascending, in the lane: 5 half-cleaners, 80 exchanges.
template <class V>
__device__ __forceinline__ void rw_clean(V (&k)[kRwSlots]) {
#pragma unroll
  for (int d = kRwSlots / 2; d >= 1; d /= 2) {
#pragma unroll
    for (int i = 0; i < kRwSlots; ++i) {
      if ((i & d) == 0) {
        const V lo = __builtin_elementwise_min(k[i], k[i + d]);
        const V hi = __builtin_elementwise_max(k[i], k[i + d]);
        k[i] = lo;
        k[i + d] = hi;
      }
    }
  }
}

// The group's 32 G keys sorted: rank q ends with positions 32q .. 32q + 31.
template <int G, class V>
__device__ __forceinline__ void rw_group_sort(V (&k)[kRwSlots], int q) {
  const uint32_t m1 = (q & 1) ? ~0u : 0u;
  const uint32_t m2 = (G == 4 && (q & 2)) ? ~0u : 0u;
  rw_flip(k, m1);
  rob_sort<kRwSlots>(k);
  rw_flip(k, m1 ^ m2);
  rw_cross<16>(k);
  rw_clean(k);
  if constexpr (G == 4) {
    rw_flip(k, m2);
    rw_cross<32>(k);
    rw_cross<16>(k);
    rw_clean(k);
  }
}

// x of the lanes of rank r, in every lane of their group (r a constant)
template <int G, int R>
__device__ __forceinline__ uint32_t rw_bcast_word(uint32_t x) {
  uint32_t a = x, b = x;
  rw_swap<16>(a, b);  // a: rows 0 0 2 2, b: rows 1 1 3 3
  uint32_t t = (R & 1) ? b : a;
  if constexpr (G == 4) {
    a = t;
    b = t;
    rw_swap<32>(a, b);  // a: the lower half's rows twice, b: the upper half's
    t = (R & 2) ? b : a;
  }
  return t;
}
template <int G, int R>
__device__ __forceinline__ float rw_bcast(float x) {
  return __uint_as_float(rw_bcast_word<G, R>(__float_as_uint(x)));
}
template <int G, int R>
__device__ __forceinline__ double rw_bcast(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint64_t lo = rw_bcast_word<G, R>(static_cast<uint32_t>(u));
  const uint64_t hi = rw_bcast_word<G, R>(static_cast<uint32_t>(u >> 32));
  return __builtin_bit_cast(double, lo | (hi << 32));
}

// Phase R of the window sum over EV accumulators, then the later phases.
// value_at(slot, e): the value of element e of the lane's key at `slot`.
template <int G, int R, int EV, class T, class F>
__device__ __forceinline__ void rw_window(int lo, int hi, T (&acc)[EV], F&& value_at) {
  constexpr int base = kRwSlots * R;
  if (lo < base + kRwSlots && hi > base) {
#pragma unroll
    for (int e = 0; e < EV; ++e) {
      T a = acc[e];
#pragma unroll
      for (int i = 0; i < kRwSlots; ++i) {
        if (base + i >= lo && base + i < hi) {
          const T x = value_at(i, e);
          a = (base + i == lo) ? x : a + x;
        }
      }
      acc[e] = a;
    }
    if constexpr (R + 1 < G) {
      if (hi > base + kRwSlots) {
#pragma unroll
        for (int e = 0; e < EV; ++e) acc[e] = rw_bcast<G, R>(acc[e]);
      }
    }
  }
  if constexpr (R + 1 < G) rw_window<G, R + 1, EV, T>(lo, hi, acc, value_at);
}

// ---- one unit per group ------------------------------------------------------------------
// u: the group's 8-byte unit; ok: it exists (every lane runs the sort).
template <class Op, int G>
__device__ __forceinline__ void rw_unit(int n, int lo, int hi, void* out, size_t u, bool ok, int q) {
  using Key = typename Op::Key;
  using K = typename Op::K;
  using HV = decltype(typename Op::KV{}.lo);
  constexpr int EV = Op::E / 2;
  u32x2 r[kRwSlots];
#pragma unroll
  for (int i = 0; i < kRwSlots; ++i) {
    const int row = kRwSlots * q + i;
    r[i] = u32x2{0u, 0u};
    if (ok && row < n) r[i] = __builtin_nontemporal_load(static_cast<const u32x2*>(rw_row_ptr(row)) + u);
  }
  HV k[kRwSlots];
#pragma unroll
  for (int i = 0; i < kRwSlots; ++i) {
    const HV key = Key::to_key(__builtin_bit_cast(HV, r[i]));
    k[i] = (kRwSlots * q + i < n) ? key : rob_splat<HV, K>(Key::kPad);
  }
  rw_group_sort<G>(k, q);
  acc_t<Op> a[Op::E];
#pragma unroll
  for (int e = 0; e < Op::E; ++e) a[e] = 0;
  acc_t<Op> w[EV];
#pragma unroll
  for (int e = 0; e < EV; ++e) w[e] = 0;
  rw_window<G, 0, EV, acc_t<Op>>(lo, hi, w,
                                 [&](int i, int e) { return Op::from_bits(Key::from_key(rob_lane(k[i], e))); });
#pragma unroll
  for (int e = 0; e < EV; ++e) a[e] = w[e];
  // pack() takes a whole vector: the upper half is zeros and its result unused
  const u32x4 full = pack<Op>(a, static_cast<float>(hi - lo));
  if (ok && q == ((hi - 1) >> 5)) __builtin_nontemporal_store(u32x2{full[0], full[1]}, static_cast<u32x2*>(out) + u);
}

// ---- one element per group (the ragged end, unaligned buffers) ------------------------------
template <class Op, int G>
__device__ __forceinline__ void rw_elem(int n, int lo, int hi, void* out, size_t j, bool ok, int q) {
  using SK = typename Op::SKey;
  using KT = decltype(rob_bits(acc_t<Op>{}));
  KT k[kRwSlots];
#pragma unroll
  for (int i = 0; i < kRwSlots; ++i) {
    const int row = kRwSlots * q + i;
    acc_t<Op> x = 0;
    if (ok && row < n) x = load_elem<Op>(rw_row_ptr(row), j);
    const KT key = SK::to_key(rob_bits(x));
    k[i] = row < n ? key : static_cast<KT>(SK::kPad);
  }
  rw_group_sort<G>(k, q);
  acc_t<Op> w[1] = {0};
  rw_window<G, 0, 1, acc_t<Op>>(lo, hi, w, [&](int i, int) { return rob_value(SK::from_key(k[i])); });
  if (ok && q == ((hi - 1) >> 5)) store_elem<Op>(out, j, w[0], static_cast<float>(hi - lo));
}

// the lane's rank in its group and its group's number in the block
template <int G>
__device__ __forceinline__ void rw_place(int& q, int& g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if constexpr (G == 2) {
    q = (lane >> 4) & 1;
    g = wave * 32 + (lane >> 5) * 16 + (lane & 15);
  } else {
    q = lane >> 4;
    g = wave * 16 + (lane & 15);
  }
}

// nunit: whole 8-byte units of the buffer; block 0 takes the last partial tile
// of units and the elements past them, blocks 1.. one tile of kBlock / G units
// each. Every base is 16-byte aligned and the output overlaps no input (the
// ABI checks).
template <class Op, int G>
__global__ __launch_bounds__(kBlock) void k_robust_wide(const RwRows<G> rows, int n, int lo, int hi,
                                                        void* __restrict__ out, size_t nunit, size_t nelem) {
  constexpr size_t kTile = rw_groups<G>();
  int q, g;
  rw_place<G>(q, g);
  const size_t full = nunit / kTile;
  if (blockIdx.x == 0) {
    if (full * kTile < nunit) {
      const size_t u = full * kTile + g;
      rw_unit<Op, G>(n, lo, hi, out, u, u < nunit, q);
    }
    const size_t j0 = nunit * (Op::E / 2);
    if (j0 < nelem) rw_elem<Op, G>(n, lo, hi, out, j0 + g, j0 + g < nelem, q);
    return;
  }
  const size_t t = blockIdx.x - 1;
  if (t < full) rw_unit<Op, G>(n, lo, hi, out, t * kTile + g, true, q);
}

// any alignment: kBlock / G elements per block
template <class Op, int G>
__global__ __launch_bounds__(kBlock) void k_robust_wide_elems(const RwRows<G> rows, int n, int lo, int hi,
                                                              void* __restrict__ out, size_t nelem) {
  int q, g;
  rw_place<G>(q, g);
  const size_t j = static_cast<size_t>(blockIdx.x) * rw_groups<G>() + g;
  rw_elem<Op, G>(n, lo, hi, out, j, j < nelem, q);
}

}  // namespace dlsim
