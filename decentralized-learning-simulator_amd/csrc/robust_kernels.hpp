// robust_kernels.hpp — gfx950 streaming kernels for the coordinate-wise
// order-statistic aggregators (coordinate median, trimmed mean).
// The reference has no such code: its one aggregator is FedAvg
// (dasklearn/gradient_aggregation/fedavg.py), which the k_wreduce_* kernels
// restate. These kernels have the tiled reduce's shape (wreduce_kernels.hpp):
// 16-byte non-temporal loads, every row's loads of a tile issued before the
// first use, one 16-byte store per vector, block 0 folding the ragged end, a
// scalar kernel for any base that is not 16-byte aligned. The fold is replaced
// by load-all, sort, window-sum.
//
// Contract, per output element, over its n values x_0 .. x_{n-1}:
//   s = the values sorted ascending in the total order
//         -Inf < ... < -0.0 < +0.0 < ... < +Inf < NaN   (all NaNs equal)
//   acc = s[lo]; for j = lo+1 .. hi-1: acc = acc + s[j]; result = acc / (hi-lo)
//   a NaN result is the canonical quiet NaN of the dtype
// fp32 adds and one IEEE fp32 division (fp64: the same in double); bf16 and
// fp16 widen exactly to fp32, add and divide in fp32 and round once to the
// dtype, nearest-even. The library is built with -ffp-contract=off; the
// division is the IEEE sequence (its v_fma are the compiler's, hence policy
// names outside scripts/audit_isa.py's POLICIES).
//
// Sorting: each value maps to an unsigned integer key of its own width whose
// unsigned order is the total order above (sign bit set: all bits flipped;
// clear: sign bit set; any NaN: the one key below the pad key), a fixed
// compare-exchange network (Batcher's odd-even merge sort: 5, 19, 63, 191
// exchanges for capacities 4, 8, 16, 32) runs min/max on the keys, and the
// selected keys map back. The capacity CAP is a compile-time constant with
// n <= CAP at run time; unused slots hold the pad key (all ones), which sorts
// above everything, so pads land at positions >= n and never enter [lo, hi).
// The network is data-independent, and the window is selected by a fully
// unrolled loop over the CAP positions under a wave-uniform predicate: no
// register array is indexed by a run-time value, nothing goes to scratch.
// Capacities 4, 8 and 16 take whole 16-byte vectors per lane (k_robust_tiles),
// capacity 32 half a vector (k_robust_halves, below), to keep its registers.
// A 16-byte vector is four key registers in every dtype: four 32-bit keys,
// two 64-bit keys, or eight 16-bit keys sorted two per register
// (v_pk_min_u16 / v_pk_max_u16). bf16 is the upper half of fp32 and fp16's
// widening is exact, monotone and one to one (zeros and subnormals included),
// so the 16-bit keys order the values exactly as the keys of the widened
// fp32 values would.
#pragma once

#include <utility>

#include "wreduce_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kRobMaxInputs = 32;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

// ---- keys ---------------------------------------------------------------------
template <class V, class K>
__device__ __forceinline__ V rob_splat(K k) {
  if constexpr (std::is_same_v<V, K>) return k;
  else return (V)(k);
}

// all ones where a > b (unsigned), else zero
template <class V, class K>
__device__ __forceinline__ V rob_gt_mask(V a, V b) {
  if constexpr (std::is_same_v<V, K>) return a > b ? static_cast<K>(~K(0)) : K(0);
  else return (V)(a > b);
}

// K: unsigned integer of the element's width; INF: the bits of +Inf. V is K
// or a vector of K.
template <class K, K INF>
struct RobKey {
  static constexpr int kBits = sizeof(K) * 8;
  static constexpr K kSign = static_cast<K>(K(1) << (kBits - 1));
  static constexpr K kAbs = static_cast<K>(kSign - 1);
  static constexpr K kPad = static_cast<K>(~K(0));
  static constexpr K kNaN = static_cast<K>(kPad - 1);

  template <class V>
  __device__ static V to_key(V u) {
    const V neg = u >> rob_splat<V, K>(static_cast<K>(kBits - 1));  // 0 or 1
    const V flip = (rob_splat<V, K>(K(0)) - neg) | rob_splat<V, K>(kSign);
    const V nan = rob_gt_mask<V, K>(u & rob_splat<V, K>(kAbs), rob_splat<V, K>(INF));
    return ((u ^ flip) & ~nan) | (rob_splat<V, K>(kNaN) & nan);
  }
  // the NaN key maps to a NaN (0x7f..fe), the pad key too (never selected)
  __device__ static K from_key(K k) { return (k & kSign) ? static_cast<K>(k ^ kSign) : static_cast<K>(~k); }
};

// ---- the compare-exchange network ----------------------------------------------
struct RobPair {
  unsigned char a, b;
};
struct RobNet {
  RobPair p[192];
  int count;
};
// Batcher's odd-even merge sort over N = 2^k slots, ascending.
template <int N>
constexpr RobNet rob_make_net() {
  RobNet net{};
  for (int p = 1; p < N; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < N; j += 2 * k)
        for (int i = 0; i < k; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            net.p[net.count].a = static_cast<unsigned char>(i + j);
            net.p[net.count].b = static_cast<unsigned char>(i + j + k);
            ++net.count;
          }
  return net;
}
template <int N> inline constexpr RobNet kRobNet = rob_make_net<N>();
static_assert(kRobNet<4>.count == 5 && kRobNet<8>.count == 19 && kRobNet<16>.count == 63 && kRobNet<32>.count == 191,
              "odd-even merge sort sizes");

template <int N, size_t I, class V>
__device__ __forceinline__ void rob_exchange(V (&k)[N]) {
  constexpr int a = kRobNet<N>.p[I].a, b = kRobNet<N>.p[I].b;
  const V lo = __builtin_elementwise_min(k[a], k[b]);
  const V hi = __builtin_elementwise_max(k[a], k[b]);
  k[a] = lo;
  k[b] = hi;
}
template <int N, class V, size_t... I>
__device__ __forceinline__ void rob_sort_seq(V (&k)[N], std::index_sequence<I...>) {
  (rob_exchange<N, I, V>(k), ...);
}
template <int N, class V>
__device__ __forceinline__ void rob_sort(V (&k)[N]) {
  rob_sort_seq<N, V>(k, std::make_index_sequence<kRobNet<N>.count>{});
}

// ---- element policies ------------------------------------------------------------
// K / KV: key type of the vector path and the 16-byte vector of them; SK: key
// type of the scalar path (the accumulator type's width: 16-bit elements sort
// there as widened fp32). from_bits: a vector-path key's value, widened.
// finish(acc, m): the division, the rounding to the dtype, NaN canonicalised.
struct RobF32 {
  static constexpr int E = 4;
  static constexpr int kBytes = 4;
  static constexpr int kFmt = kFmtF32;
  using Key = RobKey<uint32_t, 0x7f800000u>;
  using SKey = Key;
  using K = uint32_t;
  using KV = u32x4;
  __device__ static float from_bits(uint32_t u) { return __uint_as_float(u); }
  __device__ static float finish(float a, float m) {
    const float r = a / m;
    return r != r ? __uint_as_float(0x7fc00000u) : r;
  }
};

struct RobF64 {
  using T = double;
  using W = double;
  static constexpr int E = 2;
  static constexpr int kBytes = 8;
  static constexpr int kFmt = kFmtF32;
  using Key = RobKey<uint64_t, 0x7ff0000000000000ull>;
  using SKey = Key;
  using K = uint64_t;
  using KV = u64x2;
  __device__ static double from_bits(uint64_t u) { return __builtin_bit_cast(double, u); }
  __device__ static double finish(double a, float m) {
    const double r = a / static_cast<double>(m);
    return r != r ? __builtin_bit_cast(double, uint64_t{0x7ff8000000000000ull}) : r;
  }
};

struct RobBF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtBF16;
  using Key = RobKey<uint16_t, 0x7f80u>;
  using SKey = RobKey<uint32_t, 0x7f800000u>;
  using K = uint16_t;
  using KV = u16x8;
  __device__ static float from_bits(uint16_t u) { return __uint_as_float(static_cast<uint32_t>(u) << 16); }
  // bf16_round: nearest-even, a NaN becomes 0x7fc0
  __device__ static float finish(float a, float m) { return bf16_round(a / m); }
};

struct RobF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtF16;
  using Key = RobKey<uint16_t, 0x7c00u>;
  using SKey = RobKey<uint32_t, 0x7f800000u>;
  using K = uint16_t;
  using KV = u16x8;
  __device__ static float from_bits(uint16_t u) { return static_cast<float>(__builtin_bit_cast(_Float16, u)); }
  // the quotient pinned: one fp32 rounding, then the fp16 one (pin_f32);
  // 0x7fc00000 converts to fp16's 0x7e00
  __device__ static float finish(float a, float m) {
    const float r = f16_round(pin_f32(a / m));
    return r != r ? __uint_as_float(0x7fc00000u) : r;
  }
};

// bits of an accumulator-typed value (the scalar path's keys)
__device__ __forceinline__ uint32_t rob_bits(float x) { return __float_as_uint(x); }
__device__ __forceinline__ uint64_t rob_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
__device__ __forceinline__ float rob_value(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ double rob_value(uint64_t u) { return __builtin_bit_cast(double, u); }

// ---- kernel arguments --------------------------------------------------------------
// The n <= CAP input pointers travel in the kernarg segment (scalar loads).
// ptr(i): the accessor every tile body reads its inputs through, so that a
// batch's task view (robust_batch_kernels.hpp RobTaskArgs) runs the same code.
template <int CAP>
struct RobSlots {
  const void* p[CAP];
  __device__ const void* ptr(int i) const { return p[i]; }
};

// s[lo] + s[lo+1] + ... + s[hi-1], seeded with s[lo], over CAP compile-time
// positions; lo and hi are kernel arguments (wave-uniform). value_at(pos) is
// called with the loop's unrolled, hence constant, positions only.
template <int CAP, class T, class F>
__device__ __forceinline__ T rob_window(int lo, int hi, F&& value_at) {
  T acc = 0;
#pragma unroll
  for (int pos = 0; pos < CAP; ++pos) {
    if (pos >= lo && pos < hi) {
      const T x = value_at(pos);
      acc = (pos == lo) ? x : acc + x;
    }
  }
  return acc;
}

// One element, any alignment (the < E tail and misaligned buffers).
template <class Op, int CAP, class S>
__device__ __forceinline__ void rob_scalar_elem(const S& s, int n, int lo, int hi, void* out, size_t j) {
  using SK = typename Op::SKey;
  decltype(rob_bits(acc_t<Op>{})) k[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    if (i < n) k[i] = SK::to_key(rob_bits(load_elem<Op>(s.ptr(i), j)));
    else k[i] = SK::kPad;
  }
  rob_sort<CAP>(k);
  const acc_t<Op> a =
      rob_window<CAP, acc_t<Op>>(lo, hi, [&](int pos) { return rob_value(SK::from_key(k[pos])); });
  store_elem<Op>(out, j, a, static_cast<float>(hi - lo));
}

template <class Op, int CAP>
__global__ __launch_bounds__(kBlock) void k_robust_scalar(const RobSlots<CAP> s, int n, int lo, int hi,
                                                          void* __restrict__ out, size_t nelem) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < nelem) rob_scalar_elem<Op, CAP>(s, n, lo, hi, out, j);
}

// lane e of a key vector (a one-element "vector" is the scalar itself)
template <class V>
__device__ __forceinline__ auto rob_lane(const V& v, int e) {
  if constexpr (std::is_integral_v<V>) return v;
  else return v[e];
}

// Sort the CAP keys k (vectors of EV elements each) and write the window
// means of their EV elements to a[0 .. EV).
template <class Op, int CAP, int EV, class V>
__device__ __forceinline__ void rob_sort_window(V (&k)[CAP], int lo, int hi, acc_t<Op>* a) {
  using Key = typename Op::Key;
  rob_sort<CAP>(k);
#pragma unroll
  for (int e = 0; e < EV; ++e)
    a[e] = rob_window<CAP, acc_t<Op>>(lo, hi,
                                      [&](int pos) { return Op::from_bits(Key::from_key(rob_lane(k[pos], e))); });
}

// One tile: lane's vectors v0 + k*kBlock; the loads of all n rows issue
// before the first use (CAP * VPT * 4 VGPRs in flight per lane).
template <class Op, int CAP, int VPT, bool CHECK, int STP, class S>
__device__ __forceinline__ void rob_tile(const S& s, int n, int lo, int hi, const OutRef& out, size_t v0,
                                         size_t nvec) {
  using Key = typename Op::Key;
  using K = typename Op::K;
  using KV = typename Op::KV;
  u32x4 r[CAP][VPT];
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < n) load_tile<Op, VPT, 1, CHECK>(s.ptr(i), v0, nvec, r[i]);
  const float m = static_cast<float>(hi - lo);
#pragma unroll
  for (int v = 0; v < VPT; ++v) {
    KV k[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
      if (i < n) k[i] = Key::to_key(__builtin_bit_cast(KV, r[i][v]));
      else k[i] = rob_splat<KV, K>(Key::kPad);
    }
    acc_t<Op> a[Op::E];
    rob_sort_window<Op, CAP, Op::E>(k, lo, hi, a);
    const size_t idx = v0 + static_cast<size_t>(v) * kBlock;
    if (!CHECK || idx < nvec) store_vec<STP>(out, idx, pack<Op>(a, m));
  }
}

// Block 0 (dispatched first) takes the ragged end: the last partial tile and
// the < E scalar tail; blocks 1.. one full tile each (grid-strided when the
// grid is smaller). The output overlaps no input (the ABI checks).
template <class Op, int CAP, int VPT, int STP>
__global__ __launch_bounds__(kBlock) void k_robust_tiles(const RobSlots<CAP> s, int n, int lo, int hi,
                                                         void* __restrict__ out, size_t nvec, size_t nelem) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * VPT;
  const size_t full = nvec / kTile;
  const OutRef o = make_out<STP>(out, nvec);
  const size_t nb = gridDim.x;
  if (blockIdx.x == 0) {
    if (full * kTile < nvec) rob_tile<Op, CAP, VPT, true, STP>(s, n, lo, hi, o, full * kTile + threadIdx.x, nvec);
    const size_t j = nvec * Op::E + threadIdx.x;
    if (j < nelem) rob_scalar_elem<Op, CAP>(s, n, lo, hi, out, j);
    if (nb > 1) return;
  }
  const size_t workers = nb > 1 ? nb - 1 : 1;
  const size_t first = nb > 1 ? blockIdx.x - 1 : 0;
  for (size_t t = first; t < full; t += workers)
    rob_tile<Op, CAP, VPT, false, STP>(s, n, lo, hi, o, t * kTile + threadIdx.x, nvec);
}

// ---- half a vector per lane (capacity 32) -------------------------------------------
// At capacity 32 a whole vector per lane is 128 loaded VGPRs beside the keys:
// 256 VGPRs and 8-20 AGPRs, one wave per SIMD; sorting it in two halves, 213-215
// VGPRs and two waves. Here a lane takes 8 bytes of every row (the lower or
// upper half of a vector: 2 fp32, 1 fp64 or 4 16-bit elements) with 8-byte
// non-temporal loads and one 8-byte non-temporal store: 64 loaded VGPRs, 64 of
// keys, 115-153 VGPRs in all, three or four waves per SIMD (DESIGN.md §8j has the
// measurement). A wave still reads 512 contiguous bytes per row.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <class Op, int CAP, bool CHECK, class S>
__device__ __forceinline__ void rob_half_tile(const S& s, int n, int lo, int hi, void* out, size_t u0,
                                              size_t nunit) {
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
  rob_sort_window<Op, CAP, Op::E / 2>(k, lo, hi, a);
  const u32x4 full = pack<Op>(a, static_cast<float>(hi - lo));
  if (!CHECK || u0 < nunit) __builtin_nontemporal_store(u32x2{full[0], full[1]}, static_cast<u32x2*>(out) + u0);
}

// nunit: whole 8-byte units of the buffer; block 0 takes the last partial tile
// of units and the elements past them, blocks 1.. one tile of kBlock units each.
template <class Op, int CAP>
__global__ __launch_bounds__(kBlock) void k_robust_halves(const RobSlots<CAP> s, int n, int lo, int hi,
                                                          void* __restrict__ out, size_t nunit, size_t nelem) {
  const size_t full = nunit / kBlock;
  const size_t nb = gridDim.x;
  if (blockIdx.x == 0) {
    if (full * kBlock < nunit) rob_half_tile<Op, CAP, true>(s, n, lo, hi, out, full * kBlock + threadIdx.x, nunit);
    const size_t j = nunit * (Op::E / 2) + threadIdx.x;
    if (j < nelem) rob_scalar_elem<Op, CAP>(s, n, lo, hi, out, j);
    if (nb > 1) return;
  }
  const size_t workers = nb > 1 ? nb - 1 : 1;
  const size_t first = nb > 1 ? blockIdx.x - 1 : 0;
  for (size_t t = first; t < full; t += workers)
    rob_half_tile<Op, CAP, false>(s, n, lo, hi, out, t * kBlock + threadIdx.x, nunit);
}

}  // namespace dlsim
