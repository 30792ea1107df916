// quant_kernels.hpp — gfx950 kernels for block-quantised model sharing
// (dlsim_quantize, dlsim_dequantize, dlsim_quant_wreduce and its batched form;
// DESIGN.md §8s). The reference has no such code: it shares dense models only.
//
// Wire format of a flat row of P elements (fp32 or bf16): blocks of 256
// consecutive elements, the last one possibly short; one fp32 scale per block;
// one signed code q in [-qmax, qmax] per element. bits = 8: qmax = 127, an int8
// per element. bits = 4: qmax = 7, two's-complement nibbles, the even element
// in the low nibble, the high nibble of a last odd element 0.
//
// Arithmetic (every operation one correctly rounded fp32 operation, no
// contraction). t_i is the value to send: x_i widened to fp32, or with error
// feedback fl(x_i + e_i). A = max over the block of bits(t_i) & 0x7fffffff as
// unsigned integers, a = float(A).
//   A >= 0x7f800000 (an Inf or NaN in the block): scale = NaN, every code 0;
//                   the block decodes to NaN throughout
//   a < 2^-96:      scale = +0, every code 0 (sent as zeros; scale and r below
//                   are therefore always normal and finite)
//   otherwise:      scale = fl(a / qmax), r = fl(qmax / a), y_i = fl(t_i * r),
//                   q_i = clamp(round(y_i), -qmax, qmax)
//     nearest:      round = rint (ties to even)
//     stochastic:   round = floor(fl(y_i + u_i)), u_i = float(h_i >> 8) * 2^-24,
//                   h_i = mix32(i ^ mix32(seed)), i the element's index in the row
// Decode: xhat_i = fl(float(q_i) * scale), for bf16 then rounded to bf16 (ties
// to even). With error feedback e'_i = fl(t_i - xhat_i) (xhat_i the decoded
// value, so after the bf16 rounding), rounded to the row's dtype, written over
// e_i. In a NaN-scale block every e'_i is NaN: an Inf or NaN in a model poisons
// the block's residual, as it poisons the block on the wire.
//
// k_quantize: a lane owns one 16-byte vector (E elements) of each of a tile's
// kQuantVpt rows; a quantisation block is the vectors of one wave (fp32: 64
// lanes x 4) or of one half-wave (bf16: 32 lanes x 8). The block maximum is an
// integer butterfly over those lanes (__shfl_xor; no LDS, no barrier). scale
// and r are computed in every lane from the same A: on a SIMD a division in
// one lane issues the instructions of a division in all, and a broadcast would
// add cross-lane moves to it. Codes are packed in registers: 8 bits give one
// dword (fp32) or two (bf16) per lane, 4 bits one dword per lane (bf16) or per
// lane pair (fp32, the odd lane's half fetched by the even one), so a wave
// stores its codes as consecutive dwords. The leader lane of a block stores
// its scale. A lane whose vector crosses P, and every lane of the scalar form
// (some base off 16-byte alignment), moves elements and code bytes one by one
// under bound checks; both forms compute the same values.
//
// k_dequantize: the plain decode, the same lane-to-vector map.
//
// k_quant_wreduce: out[e] holds the bits of the exact weighted reduce
// (wreduce_kernels.hpp, DLSIM_EXACT) over n = m + 1 rows, row 0 the dense row
// `self`, row j neighbour j decoded as above; the arithmetic is the element
// policy's (init, step2, pack), the weight is never folded into the scale. A
// workgroup's tile is 4096 coordinates = 16 quantisation blocks; a lane holds
// the tile's vectors lv = r * 256 + tid of self and of the accumulators, the
// lane-interleaved access of the dense kernels. The neighbours go in groups of
// kQuantGroup: a lane fetches 16 bytes (8 bits) or 8 bytes (4 bits) of each
// neighbour's codes of the tile, all loads of the group in one burst, and
// writes them to LDS, the first lanes the 16 scales per neighbour; after one
// barrier every lane reads back the dwords that match its own vectors and
// decodes them with a sign-extract and an int-to-float convert. bits may differ
// per neighbour: the branch is uniform. A group and not all 31 neighbours at
// once: 31 tiles of codes are 124 KB of LDS (one resident workgroup per CU) or
// 124 VGPRs in flight; 8 are 32.5 KB and 32 VGPRs, four workgroups per CU.
// Nothing but out is written and no byte outside the code and scale buffers is
// read, whatever the codes hold; out may be self (a lane reads the elements it
// writes, tiles are disjoint).
#pragma once

#include "wreduce_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kQuantBlockElems = 256;       // elements of a quantisation block
constexpr int kQuantVpt = 2;                // k_quantize / k_dequantize: rows of kBlock vectors per tile
constexpr unsigned kQuantMaxBlocks = 1024;  // of one virtual grid: four workgroups on each of 256 CUs
constexpr uint32_t kQuantTile = 4096;       // k_quant_wreduce: coordinates of a tile (16 quantisation blocks)
constexpr int kQuantGroup = 8;              // k_quant_wreduce: neighbours whose codes are in LDS at a time
constexpr int kQuantMaxTasks = 32;          // tasks of one launch
constexpr int kQuantMaxSlots = 80;          // neighbours of one launch, over all its tasks
constexpr int kQuantMaxNeighbours = 31;     // of one task: 32 rows with self

// The quantiser's element formats: F32Exact's and BF16Exact's loads, stores and packing under names of
// their own. k_quantize divides (scale = a / qmax, r = qmax / a), and the correctly rounded division is a
// sequence built on v_fma_f32; the ISA audit (scripts/audit_isa.py) forbids fused instructions in every
// kernel named after an exact policy, where one could only be a contracted acc + w * x. k_quantize has
// no such fold; k_dequantize and k_quant_wreduce, which do not divide, keep the exact policies' names
// and stay under the audit.
struct QuantF32 : F32Exact {};
struct QuantBF16 : BF16Exact {};

__host__ __device__ constexpr int quant_qmax(int bits) { return bits == 8 ? 127 : 7; }

__device__ __forceinline__ uint32_t quant_mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

// code k of the packed codes of one vector, sign-extended
template <int BITS>
__device__ __forceinline__ int quant_code(const uint32_t* pk, int k) {
  if constexpr (BITS == 8) return static_cast<int>(pk[k >> 2] << (24 - 8 * (k & 3))) >> 24;
  else return static_cast<int>(pk[0] << (28 - 4 * k)) >> 28;
}

// xhat of the E codes of one vector: fl(float(q) * scale), for bf16 rounded to bf16
template <class Op, int BITS>
__device__ __forceinline__ void quant_decode(const uint32_t* pk, float scale, float (&xh)[Op::E]) {
#pragma unroll
  for (int k = 0; k < Op::E; ++k) xh[k] = static_cast<float>(quant_code<BITS>(pk, k)) * scale;
  if constexpr (Op::kBytes == 2) {
#pragma unroll
    for (int k = 0; k < Op::E; k += 2) bf16_round2(xh[k], xh[k + 1]);
  }
}

__device__ __forceinline__ uint32_t quant_code_bytes(uint32_t nelem, int bits) {
  return bits == 8 ? nelem : (nelem + 1) / 2;
}

template <class Op, int BITS, bool STOCH, bool RESID, bool VEC>
__global__ __launch_bounds__(kBlock) void k_quantize(const void* x, void* resid, uint32_t P, uint32_t tpb, uint32_t seed,
                                                     uint8_t* __restrict__ codes, float* __restrict__ scales) {
  constexpr int E = Op::E;
  constexpr int QMAX = quant_qmax(BITS);
  constexpr int LPB = kQuantBlockElems / E;  // lanes of one quantisation block
  constexpr int NB = E * BITS / 8;           // code bytes of one vector
  constexpr uint32_t kTile = static_cast<uint32_t>(kBlock) * E * kQuantVpt;
  const int tid = threadIdx.x;
  const uint32_t hseed = quant_mix32(seed);
  const uint32_t cbytes = quant_code_bytes(P, BITS);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * tpb;
  for (uint32_t tt = 0; tt < tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kTile;
    if (c64 >= P) break;  // block-uniform: every lane of a wave takes part in the butterflies below
    const uint32_t c0 = static_cast<uint32_t>(c64);
    float t[kQuantVpt][E];
#pragma unroll
    for (int r = 0; r < kQuantVpt; ++r) {
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
    for (int r = 0; r < kQuantVpt; ++r) {
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
      const float a = __uint_as_float(A);
      const bool nan = A >= 0x7f800000u;
      const bool zero = nan || a < 0x1p-96f;  // every code 0
      const float scale = nan ? __uint_as_float(0x7fc00000u) : zero ? 0.0f : a / static_cast<float>(QMAX);
      const float rr = zero ? 0.0f : static_cast<float>(QMAX) / a;
      int q[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const float y = t[r][k] * rr;
        float z;
        if constexpr (STOCH) {
          const uint32_t h = quant_mix32((e0 + k) ^ hseed);
          const float u = static_cast<float>(h >> 8) * 0x1p-24f;
          z = __builtin_floorf(y + u);
        } else {
          z = __builtin_rintf(y);
        }
        const int qi = static_cast<int>(zero ? 0.0f : z);  // |z| <= qmax + 1 otherwise
        q[k] = qi < -QMAX ? -QMAX : qi > QMAX ? QMAX : qi;
      }
      uint32_t pk[2] = {0u, 0u};
#pragma unroll
      for (int k = 0; k < E; ++k) {
        if constexpr (BITS == 8) pk[k >> 2] |= (static_cast<uint32_t>(q[k]) & 0xffu) << (8 * (k & 3));
        else pk[0] |= (static_cast<uint32_t>(q[k]) & 0xfu) << (4 * k);
      }
      // codes: whole dwords where the vector (NB == 2: the lane pair's two vectors) lies inside the row
      const uint32_t cb = BITS == 8 ? e0 : e0 / 2;
      bool stored = false;
      if constexpr (NB == 2) {
        const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(pk[0]), 1));
        const uint32_t pe0 = e0 & ~static_cast<uint32_t>(2 * E - 1);  // the even lane's first element
        if (VEC && pe0 + 2 * E <= P) {
          if ((tid & 1) == 0) *reinterpret_cast<uint32_t*>(codes + cb) = pk[0] | (other << 16);
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
      if (tid % LPB == 0 && e0 < P) scales[e0 / kQuantBlockElems] = scale;
      if constexpr (RESID) {
        float en[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
          float xh = static_cast<float>(q[k]) * scale;
          if constexpr (Op::kBytes == 2) xh = bf16_round(xh);
          en[k] = t[r][k] - xh;
          if constexpr (Op::kBytes == 2) en[k] = bf16_round(en[k]);
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

// the packed codes of the vector at e0 (full: inside the row, every base aligned), else byte by byte
template <int NB>
__device__ __forceinline__ void quant_load_codes(const uint8_t* codes, uint32_t cb, uint32_t cbytes, bool full,
                                                 uint32_t (&pk)[2]) {
  pk[0] = pk[1] = 0u;
  if (full) {
    if constexpr (NB == 2) pk[0] = *reinterpret_cast<const uint16_t*>(codes + cb);
    else pk[0] = *reinterpret_cast<const uint32_t*>(codes + cb);
    if constexpr (NB == 8) pk[1] = *reinterpret_cast<const uint32_t*>(codes + cb + 4);
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (cb + b < cbytes) pk[b >> 2] |= static_cast<uint32_t>(codes[cb + b]) << (8 * (b & 3));
  }
}

template <class Op, int BITS, bool VEC>
__global__ __launch_bounds__(kBlock) void k_dequantize(const uint8_t* __restrict__ codes, const float* __restrict__ scales,
                                                       uint32_t P, uint32_t tpb, void* __restrict__ out) {
  constexpr int E = Op::E;
  constexpr int NB = E * BITS / 8;
  constexpr uint32_t kTile = static_cast<uint32_t>(kBlock) * E * kQuantVpt;
  const int tid = threadIdx.x;
  const uint32_t cbytes = quant_code_bytes(P, BITS);
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * tpb;
  for (uint32_t tt = 0; tt < tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kTile;
    if (c64 >= P) break;
    const uint32_t c0 = static_cast<uint32_t>(c64);
#pragma unroll
    for (int r = 0; r < kQuantVpt; ++r) {
      const uint32_t e0 = c0 + (r * kBlock + tid) * E;
      if (e0 >= P) continue;
      const bool full = VEC && e0 + E <= P;
      uint32_t pk[2];
      quant_load_codes<NB>(codes, BITS == 8 ? e0 : e0 / 2, cbytes, full, pk);
      float xh[E];
      quant_decode<Op, BITS>(pk, scales[e0 / kQuantBlockElems], xh);
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

struct QuantTask {
  const void* self;
  void* out;
  uint32_t nelem;
  uint32_t block_start;  // first block of the task in the launch
  uint32_t tpb;          // tiles per block of its virtual grid
  uint32_t slot_off;     // its first neighbour slot
  uint32_t m;            // neighbours
  float w0;              // self's weight
};

struct QuantBatch {
  int ntasks;
  QuantTask t[kQuantMaxTasks];
  const uint8_t* codes[kQuantMaxSlots];
  const float* scales[kQuantMaxSlots];
  float w[kQuantMaxSlots];
  uint32_t bits[kQuantMaxSlots];
};

// the fold of one neighbour's tile from LDS into the lane's accumulators
template <class Op, int BITS>
__device__ __forceinline__ void quant_fold(const uint8_t* s_codes, const float* s_scale, int tid, float w,
                                           float (&acc)[kQuantTile / (kBlock * Op::E)][Op::E]) {
  constexpr int E = Op::E;
  constexpr int V = kQuantTile / (kBlock * E);
  constexpr int NB = E * BITS / 8;
#pragma unroll
  for (int r = 0; r < V; ++r) {
    const uint32_t lv = r * kBlock + tid;
    uint32_t pk[2] = {0u, 0u};
    if constexpr (NB == 2) pk[0] = reinterpret_cast<const uint16_t*>(s_codes)[lv];
    else if constexpr (NB == 4) pk[0] = reinterpret_cast<const uint32_t*>(s_codes)[lv];
    else {
      pk[0] = reinterpret_cast<const uint32_t*>(s_codes)[2 * lv];
      pk[1] = reinterpret_cast<const uint32_t*>(s_codes)[2 * lv + 1];
    }
    float xh[E];
    quant_decode<Op, BITS>(pk, s_scale[lv * E / kQuantBlockElems], xh);
#pragma unroll
    for (int k = 0; k < E; k += 2) Op::step2(acc[r][k], acc[r][k + 1], w, xh[k], xh[k + 1]);
  }
}

template <class Op, bool VEC>
__global__ __launch_bounds__(kBlock) void k_quant_wreduce(const QuantBatch B) {
  constexpr int E = Op::E;
  constexpr int V = kQuantTile / (kBlock * E);  // vectors of a tile per lane: 4 (fp32), 2 (bf16)
  constexpr int kScales = kQuantTile / kQuantBlockElems;
  __shared__ __attribute__((aligned(16))) uint8_t s_codes[kQuantGroup][kQuantTile];
  __shared__ float s_scale[kQuantGroup][kScales];
  const int tid = threadIdx.x;
  int ti = 0;
  for (int i = 1; i < B.ntasks; ++i)
    if (B.t[i].block_start <= blockIdx.x) ti = i;
  const QuantTask& T = B.t[ti];
  const uint32_t P = T.nelem, s0 = T.slot_off;
  const int m = static_cast<int>(T.m);
  const uint32_t nqb = (P + kQuantBlockElems - 1) / kQuantBlockElems;
  const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x - T.block_start) * T.tpb;
  for (uint32_t tt = 0; tt < T.tpb; ++tt) {
    const uint64_t c64 = (tile0 + tt) * kQuantTile;
    if (c64 >= P) break;  // block-uniform
    const uint32_t c0 = static_cast<uint32_t>(c64);
    const uint32_t len = P - c0 < kQuantTile ? P - c0 : kQuantTile;
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
    for (int g0 = 0; g0 < m; g0 += kQuantGroup) {
      const int gn = m - g0 < kQuantGroup ? m - g0 : kQuantGroup;
      // the group's codes of the tile, one burst
      uint32_t c[kQuantGroup][4];
#pragma unroll
      for (int j = 0; j < kQuantGroup; ++j) {
        c[j][0] = c[j][1] = c[j][2] = c[j][3] = 0u;
        if (j < gn) {
          const uint32_t slot = s0 + g0 + j;
          const bool b8 = B.bits[slot] == 8;
          const uint32_t nbl = b8 ? 16u : 8u, off = tid * nbl;  // the lane's bytes of the tile's codes
          const uint32_t tb = b8 ? len : (len + 1) / 2;          // the tile's code bytes
          const uint8_t* const src = B.codes[slot] + (b8 ? c0 : c0 / 2);
          if (VEC && off + nbl <= tb) {
            if (b8) {
              const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + off));
              c[j][0] = v[0], c[j][1] = v[1], c[j][2] = v[2], c[j][3] = v[3];
            } else {
              c[j][0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src + off));
              c[j][1] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src + off + 4));
            }
          } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
              if (static_cast<uint32_t>(b) < nbl && off + b < tb) c[j][b >> 2] |= static_cast<uint32_t>(src[off + b]) << (8 * (b & 3));
          }
        }
      }
      __syncthreads();  // every lane has folded the previous group (and tile) out of LDS
#pragma unroll
      for (int j = 0; j < kQuantGroup; ++j) {
        if (j < gn) {
          if (B.bits[s0 + g0 + j] == 8) {
            reinterpret_cast<u32x4*>(s_codes[j])[tid] = u32x4{c[j][0], c[j][1], c[j][2], c[j][3]};
          } else {
            reinterpret_cast<uint32_t*>(s_codes[j])[2 * tid] = c[j][0];
            reinterpret_cast<uint32_t*>(s_codes[j])[2 * tid + 1] = c[j][1];
          }
        }
      }
      if (tid < gn * kScales) {
        const uint32_t qb = c0 / kQuantBlockElems + tid % kScales;
        s_scale[tid / kScales][tid % kScales] = qb < nqb ? B.scales[s0 + g0 + tid / kScales][qb] : 0.0f;
      }
      __syncthreads();
      for (int j = 0; j < gn; ++j) {
        const float w = B.w[s0 + g0 + j];
        if (B.bits[s0 + g0 + j] == 8) quant_fold<Op, 8>(s_codes[j], s_scale[j], tid, w, acc);
        else quant_fold<Op, 4>(s_codes[j], s_scale[j], tid, w, acc);
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
