// mx_kernels.hpp — gfx950 kernels for MX (OCP microscaling) model sharing
// (dlsim_mx_quantize, dlsim_mx_dequantize, dlsim_mx_wreduce and its batched
// form). The reference has no such code: it shares dense models
// only.
//
// Wire format of a flat row of P elements (fp32 or bf16): blocks of 32
// consecutive elements, the last one possibly short; one scale byte S (E8M0,
// the power of two 2^(S-127)) per block; one element code per element.
//   format 0, FP8 E4M3: emax 8,  max 448,   one byte per element
//   format 1, FP8 E5M2: emax 15, max 57344, one byte per element
//   format 2, FP4 E2M1: emax 2,  max 6,     two per byte, the even element in
//             the low nibble, the high nibble of a last odd element 0
//
// Encode. t_i is the value to send: x_i widened to fp32, or with error feedback
// fl32(x_i + e_i). A = max over the block of bits(t_i) & 0x7fffffff as unsigned
// integers (k_quantize's key).
//   A >= 0x7f800000 (an Inf or NaN in the block): S = 0xFF, every code 0
//   A <  0x1f800000 (largest magnitude below 2^-64): S = 0, every code 0; so
//                   every scale and every decoded value the quantiser can
//                   produce is normal in fp32 (the smallest: E5M2's subnormal
//                   2^-16 times 2^(48-127))
//   otherwise:      S = (A >> 23) - emax, in [48, 252]; q_i encodes the real
//                   number t_i / 2^(S-127): rounded to nearest, ties to the
//                   even code, the exponent unbounded above, the format's
//                   subnormals included; then the magnitude clamped to max
//                   (never Inf or NaN); the code's sign bit is t_i's, also for
//                   -0 and for values that round to zero
// Decode, defined for every byte value: xhat_i = fl32(v(q_i) * 2^(S-127)) for
// S <= 254, one correctly rounded fp32 multiplication (fp32 subnormals
// included), v the OCP value of the code (E4M3 S.1111.111 NaN; E5M2 S.11111.00
// +-Inf, its other all-ones-exponent codes NaN); S = 0xFF: NaN throughout the
// block. For a bf16 row then rounded to bf16, ties to even: a no-op for normal
// values (an element has at most 3 mantissa bits), so with S in [48, 252] every
// decoded value is exact in both dtypes.
// Error feedback: e'_i = fl32(t_i - xhat_i), rounded to the row's dtype, written
// over e_i: NaN throughout a block with S = 0xFF, t_i in an all-zero block.
//
// The conversions are CDNA4's v_cvt_scalef32_pk_*: two elements per
// instruction, the block scale applied in it (the scale operand is the float
// whose bits are S << 23). Their overflow result depends on a mode bit this
// project does not touch, so the encoder first clamps t to +-max * 2^(S-127)
// (an exact product; clamping before the rounding gives what clamping after it
// does, max being a code and rounding monotone). The decoder hands the
// instruction only the scales the quantiser produces, S in [48, 252]; for any
// other S it converts with scale 1 and multiplies by 2^(S-127) once, and
// S = 0xFF multiplies by NaN: nothing rests on what the hardware does with a
// zero, subnormal or NaN scale operand.
//
// k_mx_quantize: a lane owns one 16-byte vector (E elements) of each of a
// tile's kMxVpt rows, as in k_quantize; a block is 8 lanes (fp32) or 4 (bf16),
// its maximum a 3- or 2-step integer butterfly (__shfl_xor; no LDS, no
// barrier), S computed in every lane from the same A. A lane packs its codes
// into whole dwords in registers (fp32 / FP4: two bytes, the odd lane's fetched
// by the even one); the leader lane of a block stores its scale byte. A lane
// whose vector crosses P, and every lane of the scalar form (some base off
// 16-byte alignment), moves elements and code bytes one by one under bound
// checks; both forms compute the same values.
//
// k_mx_dequantize: the plain decode, the same lane-to-vector map.
//
// k_mx_wreduce: out[e] holds the bits of the exact weighted reduce
// (wreduce_kernels.hpp, DLSIM_EXACT) over n = m + 1 rows, row 0 the dense row
// `self`, row j neighbour j decoded as above; the arithmetic is the element
// policy's (init, step2, pack), a weight is never folded into a scale. No LDS
// and no barrier: a lane holds the vectors lv = r * 256 + tid of a tile of 4096
// coordinates of self and of the accumulators, and for each neighbour loads
// from global memory exactly the code bytes of those vectors (fp32 / FP8 a
// dword, so a wave reads 256 contiguous bytes; bf16 / FP8 8 bytes; bf16 / FP4 a
// dword; fp32 / FP4 2 bytes: the lane map of self is fixed before a neighbour's
// format is known, and formats differ per neighbour, so a lane cannot own two
// adjacent vectors for one of them) and its block's scale byte (8 or 4 lanes
// share the address). The loads of kMxGroup neighbours go out in one burst
// before the first is folded. The format of a slot is a wave-uniform branch.
// Nothing but out is written and no byte outside the code and scale buffers is
// read, whatever they hold; out may be self (a lane reads the elements it
// writes, tiles are disjoint).
#pragma once

#include "quant_kernels.hpp"  // the grid cap and the batch limits, shared with block-quantised sharing

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kMxBlock = 32;         // elements of a block (one scale byte)
constexpr int kMxVpt = 2;            // k_mx_quantize / k_mx_dequantize: rows of kBlock vectors per tile
constexpr uint32_t kMxTile = 4096;   // k_mx_wreduce: coordinates of a tile
constexpr int kMxGroup = 4;          // k_mx_wreduce: neighbours whose loads are in flight at a time
constexpr int kMxE4M3 = 0, kMxE5M2 = 1, kMxE2M1 = 2;

typedef short s16x2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int mx_emax(int fmt) { return fmt == kMxE4M3 ? 8 : fmt == kMxE5M2 ? 15 : 2; }
__host__ __device__ constexpr float mx_max(int fmt) { return fmt == kMxE4M3 ? 448.0f : fmt == kMxE5M2 ? 57344.0f : 6.0f; }
__host__ __device__ constexpr uint32_t mx_code_bytes(uint32_t nelem, int fmt) { return fmt == kMxE2M1 ? (nelem + 1) / 2 : nelem; }

// ---- the conversions: two elements per instruction ------------------------------------
// FP8: a / scale and b / scale as two codes in the low (HI = false) or high half of `old`
template <int FMT, bool HI>
__device__ __forceinline__ uint32_t mx_cvt_fp8(uint32_t old, float a, float b, float scale) {
  const s16x2 o = __builtin_bit_cast(s16x2, old);
  if constexpr (FMT == kMxE4M3) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(o, a, b, scale, HI));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(o, a, b, scale, HI));
}

// the codes of the E clamped values c: FP8 one dword per four, FP4 one byte per two
template <int FMT, int E>
__device__ __forceinline__ void mx_encode(const float (&c)[E], float scale, uint32_t (&pk)[2]) {
  pk[0] = pk[1] = 0u;
  if constexpr (FMT == kMxE2M1) {
    pk[0] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk[0], c[0], c[1], scale, 0);
    pk[0] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk[0], c[2], c[3], scale, 1);
    if constexpr (E == 8) {
      pk[0] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk[0], c[4], c[5], scale, 2);
      pk[0] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(pk[0], c[6], c[7], scale, 3);
    }
  } else {
    pk[0] = mx_cvt_fp8<FMT, false>(pk[0], c[0], c[1], scale);
    pk[0] = mx_cvt_fp8<FMT, true>(pk[0], c[2], c[3], scale);
    if constexpr (E == 8) {
      pk[1] = mx_cvt_fp8<FMT, false>(pk[1], c[4], c[5], scale);
      pk[1] = mx_cvt_fp8<FMT, true>(pk[1], c[6], c[7], scale);
    }
  }
}

// v(q) * scale of the E codes of one vector
template <int FMT, int E>
__device__ __forceinline__ void mx_cvt_f32(const uint32_t (&pk)[2], float scale, float (&v)[E]) {
  f32x2 p[4];
  if constexpr (FMT == kMxE2M1) {
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(pk[0], scale, 0);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(pk[0], scale, 1);
    if constexpr (E == 8) {
      p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(pk[0], scale, 2);
      p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(pk[0], scale, 3);
    }
  } else if constexpr (FMT == kMxE4M3) {
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(pk[0], scale, false);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(pk[0], scale, true);
    if constexpr (E == 8) {
      p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(pk[1], scale, false);
      p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(pk[1], scale, true);
    }
  } else {
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(pk[0], scale, false);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(pk[0], scale, true);
    if constexpr (E == 8) {
      p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(pk[1], scale, false);
      p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(pk[1], scale, true);
    }
  }
#pragma unroll
  for (int k = 0; k < E; k += 2) v[k] = p[k / 2][0], v[k + 1] = p[k / 2][1];
}

// xhat of the E codes of one vector under the scale byte S, any byte values. BF: a bf16 row, whose
// values are rounded to bf16 where they can be inexact in it (fp32 subnormals, so S < 48 only).
template <int FMT, int E, bool BF>
__device__ __forceinline__ void mx_decode(const uint32_t (&pk)[2], uint32_t S, float (&xh)[E]) {
  if (S - 48u <= 204u) {  // what the quantiser produces: the scale in the instruction, every result exact
    mx_cvt_f32<FMT, E>(pk, __uint_as_float(S << 23), xh);
  } else {
    mx_cvt_f32<FMT, E>(pk, 1.0f, xh);
    const float mul = __uint_as_float(S == 0xffu ? 0x7fc00000u : S ? S << 23 : 0x00400000u);  // 2^(S-127), or NaN
#pragma unroll
    for (int k = 0; k < E; ++k) xh[k] = xh[k] * mul;
    if constexpr (BF) {
#pragma unroll
      for (int k = 0; k < E; k += 2) bf16_round2(xh[k], xh[k + 1]);
    }
  }
}

// the packed codes of the vector at e0 (full: inside the row, every base aligned), else byte by byte
template <int NB>
__device__ __forceinline__ void mx_load_codes(const uint8_t* codes, uint32_t cb, uint32_t cbytes, bool full, uint32_t (&pk)[2]) {
  pk[0] = pk[1] = 0u;
  if (full) {
    if constexpr (NB == 2) pk[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(codes + cb));
    else pk[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(codes + cb));
    if constexpr (NB == 8) pk[1] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(codes + cb + 4));
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (cb + b < cbytes) pk[b >> 2] |= static_cast<uint32_t>(codes[cb + b]) << (8 * (b & 3));
  }
}

template <class Op, int FMT, bool RESID, bool VEC>
__global__ __launch_bounds__(kBlock) void k_mx_quantize(const void* x, void* resid, uint32_t P, uint32_t tpb,
                                                        uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
  constexpr int E = Op::E;
  constexpr int LPB = kMxBlock / E;                      // lanes of one block: 8 (fp32), 4 (bf16)
  constexpr int NB = FMT == kMxE2M1 ? E / 2 : E;         // code bytes of one vector
  constexpr uint32_t kTile = static_cast<uint32_t>(kBlock) * E * kMxVpt;
  const int tid = threadIdx.x;
  const uint32_t cbytes = mx_code_bytes(P, FMT);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * tpb;
  for (uint32_t tt = 0; tt < tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kTile;
    if (c64 >= P) break;  // block-uniform: every lane of a wave takes part in the butterflies below
    const uint32_t c0 = static_cast<uint32_t>(c64);
    float t[kMxVpt][E];
#pragma unroll
    for (int r = 0; r < kMxVpt; ++r) {
      const uint32_t e0 = c0 + (r * kBlock + tid) * E;
      if (VEC && e0 + E <= P) {
        unpack<Op>(__builtin_nontemporal_load(static_cast<const u32x4*>(x) + e0 / E), t[r]);
        if constexpr (RESID) {
          float ev[E];
          unpack<Op>(__builtin_nontemporal_load(static_cast<const u32x4*>(resid) + e0 / E), ev);
#pragma unroll
          for (int k = 0; k < E; ++k) t[r][k] = t[r][k] + ev[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) {
          t[r][k] = 0.0f;  // past the row: key 0, code 0
          if (e0 + k < P) {
            t[r][k] = load_elem<Op>(x, e0 + k);
            if constexpr (RESID) t[r][k] = t[r][k] + load_elem<Op>(resid, e0 + k);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kMxVpt; ++r) {
      const uint32_t e0 = c0 + (r * kBlock + tid) * E;
      const bool full = VEC && e0 + E <= P;
      uint32_t A = 0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const uint32_t key = __float_as_uint(t[r][k]) & 0x7fffffffu;
        A = key > A ? key : A;
      }
#pragma unroll
      for (int off = 1; off < LPB; off <<= 1) {
        const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), off));
        A = o > A ? o : A;
      }
      const bool dead = A >= 0x7f800000u || A < 0x1f800000u;  // every code 0
      const uint32_t S = A >= 0x7f800000u ? 0xffu : dead ? 0u : (A >> 23) - mx_emax(FMT);
      const float scale = __uint_as_float(dead ? 0x3f800000u : S << 23);
      const float lim = dead ? 0.0f : mx_max(FMT) * scale;  // exact: below 2^((A >> 23) - 126)
      float c[E];
#pragma unroll
      for (int k = 0; k < E; ++k) c[k] = __builtin_amdgcn_fmed3f(t[r][k], -lim, lim);  // a live block holds no NaN
      uint32_t pk[2];
      mx_encode<FMT, E>(c, scale, pk);
      if (dead) pk[0] = pk[1] = 0u;
      // codes: whole dwords where the vector (NB == 2: the lane pair's two vectors) lies inside the row
      const uint32_t cb = FMT == kMxE2M1 ? e0 / 2 : e0;
      bool stored = false;
      if constexpr (NB == 2) {
        const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(pk[0]), 1));
        const uint32_t pe0 = e0 & ~static_cast<uint32_t>(2 * E - 1);  // the even lane's first element
        if (VEC && pe0 + 2 * E <= P) {
          if ((tid & 1) == 0) *reinterpret_cast<uint32_t*>(codes + cb) = (pk[0] & 0xffffu) | (other << 16);
          stored = true;
        }
      } else if (full) {
        *reinterpret_cast<uint32_t*>(codes + cb) = pk[0];
        if constexpr (NB == 8) *reinterpret_cast<uint32_t*>(codes + cb + 4) = pk[1];
        stored = true;
      }
      if (!stored) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (cb + b < cbytes) codes[cb + b] = static_cast<uint8_t>(pk[b >> 2] >> (8 * (b & 3)));
      }
      if (tid % LPB == 0 && e0 < P) scales[e0 / kMxBlock] = static_cast<uint8_t>(S);
      if constexpr (RESID) {
        float xh[E], en[E];
        mx_decode<FMT, E, false>(pk, S, xh);  // exact in bf16 too: S in [48, 252], or 0 over zero codes, or NaN
#pragma unroll
        for (int k = 0; k < E; ++k) en[k] = t[r][k] - xh[k];
        if constexpr (Op::kBytes == 2) {
#pragma unroll
          for (int k = 0; k < E; k += 2) bf16_round2(en[k], en[k + 1]);
        }
        if (full) {
          *(static_cast<u32x4*>(resid) + e0 / E) = pack<Op>(en, 1.0f);
        } else {
#pragma unroll
          for (int k = 0; k < E; ++k)
            if (e0 + k < P) store_elem<Op>(resid, e0 + k, en[k], 1.0f);
        }
      }
    }
  }
}

template <class Op, int FMT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_mx_dequantize(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                          uint32_t P, uint32_t tpb, void* __restrict__ out) {
  constexpr int E = Op::E;
  constexpr int NB = FMT == kMxE2M1 ? E / 2 : E;
  constexpr uint32_t kTile = static_cast<uint32_t>(kBlock) * E * kMxVpt;
  const int tid = threadIdx.x;
  const uint32_t cbytes = mx_code_bytes(P, FMT);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * tpb;
  for (uint32_t tt = 0; tt < tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kTile;
    if (c64 >= P) break;
    const uint32_t c0 = static_cast<uint32_t>(c64);
#pragma unroll
    for (int r = 0; r < kMxVpt; ++r) {
      const uint32_t e0 = c0 + (r * kBlock + tid) * E;
      if (e0 >= P) continue;
      const bool full = VEC && e0 + E <= P;
      uint32_t pk[2];
      mx_load_codes<NB>(codes, FMT == kMxE2M1 ? e0 / 2 : e0, cbytes, full, pk);
      float xh[E];
      mx_decode<FMT, E, Op::kBytes == 2>(pk, scales[e0 / kMxBlock], xh);
      if constexpr (Op::kBytes == 2) {  // pack() truncates: a NaN keeps a mantissa bit whatever the conversion gave it
#pragma unroll
        for (int k = 0; k < E; k += 2) bf16_round2(xh[k], xh[k + 1]);
      }
      if (full) {
        __builtin_nontemporal_store(pack<Op>(xh, 1.0f), static_cast<u32x4*>(out) + e0 / E);
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k)
          if (e0 + k < P) store_elem<Op>(out, e0 + k, xh[k], 1.0f);
      }
    }
  }
}

struct MxBatch {
  int ntasks;
  QuantTask t[kQuantMaxTasks];  // the task record of the block-quantised reduce: rows, grid, slots, self's weight
  const uint8_t* codes[kQuantMaxSlots];
  const uint8_t* scales[kQuantMaxSlots];
  float w[kQuantMaxSlots];
  uint32_t fmt[kQuantMaxSlots];
};

// One neighbour's codes and scale bytes of the lane's vectors of the tile at c0. INNER: a whole tile of the
// vector form, no bound to check; otherwise every vector is checked against the row's end.
template <class Op, int FMT, bool VEC, bool INNER>
__device__ __forceinline__ void mx_fetch(const uint8_t* codes, const uint8_t* scales, uint32_t c0, uint32_t len, uint32_t P,
                                         int tid, uint32_t (&c)[kMxTile / (kBlock * Op::E)][2],
                                         uint32_t (&s)[kMxTile / (kBlock * Op::E)]) {
  constexpr int E = Op::E;
  constexpr int V = kMxTile / (kBlock * E);
  constexpr int NB = FMT == kMxE2M1 ? E / 2 : E;
  const uint32_t cbytes = mx_code_bytes(P, FMT);
#pragma unroll
  for (int r = 0; r < V; ++r) {
    const uint32_t l0 = (r * kBlock + tid) * E;
    c[r][0] = c[r][1] = 0u;
    s[r] = 127u;  // past the row: zero codes times 1
    if (INNER || l0 < len) {
      mx_load_codes<NB>(codes, FMT == kMxE2M1 ? (c0 + l0) / 2 : c0 + l0, cbytes, INNER || (VEC && l0 + E <= len), c[r]);
      s[r] = __builtin_nontemporal_load(scales + (c0 + l0) / kMxBlock);
    }
  }
}

template <class Op, bool VEC, bool INNER>
__device__ __forceinline__ void mx_fetch_any(uint32_t f, const uint8_t* codes, const uint8_t* scales, uint32_t c0, uint32_t len,
                                             uint32_t P, int tid, uint32_t (&c)[kMxTile / (kBlock * Op::E)][2],
                                             uint32_t (&s)[kMxTile / (kBlock * Op::E)]) {
  if (f == kMxE2M1) mx_fetch<Op, kMxE2M1, VEC, INNER>(codes, scales, c0, len, P, tid, c, s);
  else mx_fetch<Op, kMxE4M3, VEC, INNER>(codes, scales, c0, len, P, tid, c, s);  // E5M2: the same bytes
}

// the fold of one neighbour's vectors into the lane's accumulators
template <class Op, int FMT>
__device__ __forceinline__ void mx_fold(const uint32_t (&c)[kMxTile / (kBlock * Op::E)][2],
                                        const uint32_t (&s)[kMxTile / (kBlock * Op::E)], float w,
                                        float (&acc)[kMxTile / (kBlock * Op::E)][Op::E]) {
  constexpr int E = Op::E;
  constexpr int V = kMxTile / (kBlock * E);
#pragma unroll
  for (int r = 0; r < V; ++r) {
    float xh[E];
    mx_decode<FMT, E, Op::kBytes == 2>(c[r], s[r], xh);
#pragma unroll
    for (int k = 0; k < E; k += 2) Op::step2(acc[r][k], acc[r][k + 1], w, xh[k], xh[k + 1]);
  }
}

template <class Op>
__device__ __forceinline__ void mx_fold_any(uint32_t f, const uint32_t (&c)[kMxTile / (kBlock * Op::E)][2],
                                            const uint32_t (&s)[kMxTile / (kBlock * Op::E)], float w,
                                            float (&acc)[kMxTile / (kBlock * Op::E)][Op::E]) {
  if (f == kMxE4M3) mx_fold<Op, kMxE4M3>(c, s, w, acc);
  else if (f == kMxE5M2) mx_fold<Op, kMxE5M2>(c, s, w, acc);
  else mx_fold<Op, kMxE2M1>(c, s, w, acc);
}

template <class Op, bool VEC>
__global__ __launch_bounds__(kBlock) void k_mx_wreduce(const MxBatch B) {
  constexpr int E = Op::E;
  constexpr int V = kMxTile / (kBlock * E);  // vectors of a tile per lane: 4 (fp32), 2 (bf16)
  const int tid = threadIdx.x;
  int ti = 0;
  for (int i = 1; i < B.ntasks; ++i)
    if (B.t[i].block_start <= blockIdx.x) ti = i;
  const QuantTask& T = B.t[ti];
  const uint32_t P = T.nelem, s0 = T.slot_off;
  const int m = static_cast<int>(T.m);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x - T.block_start) * T.tpb;
  for (uint32_t tt = 0; tt < T.tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kMxTile;
    if (c64 >= P) break;  // block-uniform
    const uint32_t c0 = static_cast<uint32_t>(c64);
    const uint32_t len = P - c0 < kMxTile ? P - c0 : kMxTile;
    // x0 * 0, then self's term
    float acc[V][E];
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const uint32_t l0 = (r * kBlock + tid) * E;
      float xs[E];
      if (VEC && l0 + E <= len) {
        unpack<Op>(__builtin_nontemporal_load(static_cast<const u32x4*>(T.self) + (c0 + l0) / E), xs);
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) xs[k] = l0 + k < len ? load_elem<Op>(T.self, c0 + l0 + k) : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < E; ++k) acc[r][k] = Op::init(xs[k]);
#pragma unroll
      for (int k = 0; k < E; k += 2) Op::step2(acc[r][k], acc[r][k + 1], T.w0, xs[k], xs[k + 1]);
    }
    if (VEC && len == kMxTile) {
      for (int g0 = 0; g0 < m; g0 += kMxGroup) {
        const int gn = m - g0 < kMxGroup ? m - g0 : kMxGroup;
        // the group's codes and scale bytes of the lane's vectors, one burst
        uint32_t c[kMxGroup][V][2], s[kMxGroup][V];
#pragma unroll
        for (int j = 0; j < kMxGroup; ++j) {
          if (j < gn) {
            const uint32_t slot = s0 + g0 + j;
            mx_fetch_any<Op, true, true>(B.fmt[slot], B.codes[slot], B.scales[slot], c0, len, P, tid, c[j], s[j]);
          } else {  // never folded; defined, so that no register of the burst is undefined
#pragma unroll
            for (int r = 0; r < V; ++r) c[j][r][0] = c[j][r][1] = s[j][r] = 0u;
          }
        }
#pragma unroll
        for (int j = 0; j < kMxGroup; ++j)
          if (j < gn) mx_fold_any<Op>(B.fmt[s0 + g0 + j], c[j], s[j], B.w[s0 + g0 + j], acc);
      }
    } else {  // the row's last tile, and every tile of the scalar form: one neighbour at a time, every access checked
      for (int j = 0; j < m; ++j) {
        uint32_t c[V][2], s[V];
        mx_fetch_any<Op, VEC, false>(B.fmt[s0 + j], B.codes[s0 + j], B.scales[s0 + j], c0, len, P, tid, c, s);
        mx_fold_any<Op>(B.fmt[s0 + j], c, s, B.w[s0 + j], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const uint32_t l0 = (r * kBlock + tid) * E;
      if (VEC && l0 + E <= len) {
        __builtin_nontemporal_store(pack<Op>(acc[r], 1.0f), static_cast<u32x4*>(T.out) + (c0 + l0) / E);
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k)
          if (l0 + k < len) store_elem<Op>(T.out, c0 + l0 + k, acc[r][k], 1.0f);
      }
    }
  }
}

}  // namespace dlsim
