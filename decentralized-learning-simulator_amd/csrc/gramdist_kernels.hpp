// gramdist_kernels.hpp — gfx950 kernels for the matrix of squared L2 distances
// between n <= 32 flat buffers through their Gram matrix on the fp64 matrix
// unit: the opt-in entry dlsim_gram_sqdist beside the exact
// dlsim_pairwise_sqdist (pairdist_kernels.hpp), which reads a row once per
// unit it belongs to; this one reads every row once at any n. The reference
// has no such code (its one aggregator is FedAvg).
//
// Contract: s(v) = v if v is finite, else 0; c[e] = s(x_0[e]);
// y_i[e] = double(s(x_i[e])) - double(c[e]) (one double subtraction, y_0 = 0);
// G_ij = sum_e y_i[e] y_j[e] in double on v_mfma_f64_16x16x4_f64;
// d2[i][j] = max(+0, G_ii + G_jj - 2 G_ij), NaN when row i or j holds a
// non-finite element. Centring on row 0 brings the cancellation of the Gram
// identity down to the scale of the distances themselves.
//
// Operands. Rows form blocks of 16. Lane l of a wave owns row
// 16 rb + (l & 15) and K-slot l >> 4, so that the A operand A[i = l & 15][k =
// l >> 4] and the B operand B[k][j] of the transpose are the same register: a
// diagonal block needs one operand, the 01 block the two row blocks' operands,
// and nothing is transposed. The sum over e has no order of its own: step u of
// a tile gives lane l item 4 u + (l >> 4) of its wave's slab of 32 items (a
// 16-byte vector each, or one element in the scalar form: 512 contiguous bytes
// of every row per wave and tile), and every element of a vector feeds one
// instruction (n <= 16) or three (00, 01, 11). Rows at or past n load nothing
// and are zero operands. All loads of a tile are issued before the first use.
//
// The centre of a lane is row 0's item at the lane's own K-slot, which lane
// l & 48 holds: one ds_bpermute_b32 per loaded dword brings its raw bits over
// (no second load, no further registers across the loads). Finiteness is
// decided on the raw bits (integer compare, select); every lane keeps a flag
// per row block, folded into a 32-bit row mask at the block's end.
//
// A block strides over full tiles without bounds checks (the dealing rule of
// pairdist_kernels.hpp) and keeps its 8 or 24 accumulator registers to its
// end: the four waves' accumulators are added in wave order through LDS, then
// one store of the block's 256 or 768 doubles to ws[slot * blocks + block] and
// of its row mask. k_gramdist_finish takes one wave per pair (i < j): the
// three Gram entries' partials in pairdist's finish order (lane l adds blocks
// l, l + 64, ..., then the butterfly), the masks ORed, one entry formed and
// stored to both halves. No atomics: the bits are a function of the grid,
// which is a function of (n, dtype, n_elems, alignment class).
#pragma once

#include "pairdist_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGdRows = 16;                                // rows of a row block (the instruction's M and N)
constexpr int kGdUnroll = 8;                               // steps of a tile
constexpr int kGdWaveItems = 4 * kGdUnroll;                // items of a wave's slab per row and tile
constexpr int kGdTileItems = (kBlock / 64) * kGdWaveItems;  // items of a block's tile per row
constexpr int kGdBlockSlots = kGdRows * kGdRows;           // doubles of one 16 x 16 partial

// ---- element policies (names outside scripts/audit_isa.py's POLICIES) ---------
struct GdF32 {
  static constexpr int E = 4;
  static constexpr int kBytes = 4;
  static constexpr int kFmt = kFmtF32;
};
struct GdBF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtBF16;
};
struct GdF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtF16;
};

// What a lane holds of one row between the load and the arithmetic: a 16-byte
// vector (VEC) or one element's bits, zero-extended.
template <class Op, bool VEC>
struct GdRaw {
  static constexpr int W = VEC ? 4 : 1;       // dwords
  static constexpr int EV = VEC ? Op::E : 1;  // elements
  uint32_t w[W];
};

// Item idx of a row; zeros past `count` when CHECK.
template <class Op, bool VEC, bool CHECK>
__device__ __forceinline__ GdRaw<Op, VEC> gd_load(const void* p, size_t idx, size_t count) {
  GdRaw<Op, VEC> r;
#pragma unroll
  for (int k = 0; k < GdRaw<Op, VEC>::W; ++k) r.w[k] = 0u;
  if (!CHECK || idx < count) {
    if constexpr (VEC) {
      const u32x4 v = ld16<1>(p, idx);
#pragma unroll
      for (int k = 0; k < 4; ++k) r.w[k] = v[k];
    } else if constexpr (Op::kBytes == 4) {
      r.w[0] = static_cast<const uint32_t*>(p)[idx];
    } else {
      r.w[0] = static_cast<const uint16_t*>(p)[idx];
    }
  }
  return r;
}

// The bits of element e of a loaded item (a 16-bit element zero-extended).
template <class Op, bool VEC>
__device__ __forceinline__ uint32_t gd_bits(const GdRaw<Op, VEC>& r, int e) {
  if constexpr (!VEC || Op::kBytes == 4) return r.w[e];
  else return (e & 1) ? (r.w[e / 2] >> 16) : (r.w[e / 2] & 0xffffu);
}

// s(v) widened to double (exact); bad |= v is not finite. The test is on the
// exponent field of the raw bits.
template <class Op>
__device__ __forceinline__ double gd_value(uint32_t bits, bool& bad) {
  if constexpr (Op::kBytes == 4) {
    const bool nf = (bits & 0x7f800000u) == 0x7f800000u;
    bad = bad || nf;
    return static_cast<double>(__uint_as_float(nf ? 0u : bits));
  } else if constexpr (Op::kFmt == kFmtBF16) {
    const bool nf = (bits & 0x7f80u) == 0x7f80u;
    bad = bad || nf;
    return static_cast<double>(__uint_as_float(nf ? 0u : (bits << 16)));
  } else {
    const bool nf = (bits & 0x7c00u) == 0x7c00u;
    bad = bad || nf;
    return static_cast<double>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(nf ? 0u : bits)));
  }
}

// A wave's slab of one tile: items base .. base + 32 of the NB row blocks'
// rows (p[rb]: the lane's row of block rb, null for a row at or past n).
// NB == 1: acc[0] += Y Y^T. NB == 2: acc[0], acc[1], acc[2] += the 00, 01 and
// 11 blocks.
template <class Op, int NB, bool VEC, bool CHECK>
__device__ __forceinline__ void gd_tile(const void* (&p)[NB], size_t base, size_t count,
                                        f64x4 (&acc)[NB == 1 ? 1 : 3], bool (&bad)[NB]) {
  using Raw = GdRaw<Op, VEC>;
  const int lane = threadIdx.x & 63;
  const size_t first = base + (lane >> 4);
  Raw raw[NB][kGdUnroll];
#pragma unroll
  for (int rb = 0; rb < NB; ++rb)
#pragma unroll
    for (int u = 0; u < kGdUnroll; ++u) {
      if (p[rb]) raw[rb][u] = gd_load<Op, VEC, CHECK>(p[rb], first + 4 * u, count);
      else raw[rb][u] = Raw{};
    }
  const int centre_lane = (lane & 48) << 2;  // ds_bpermute takes a byte address
#pragma unroll
  for (int u = 0; u < kGdUnroll; ++u) {
    Raw c;
#pragma unroll
    for (int k = 0; k < Raw::W; ++k)
      c.w[k] = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(centre_lane, static_cast<int>(raw[0][u].w[k])));
#pragma unroll
    for (int e = 0; e < Raw::EV; ++e) {
      bool centre_bad = false;  // row 0's own lanes flag it
      const double ce = gd_value<Op>(gd_bits<Op, VEC>(c, e), centre_bad);
      double y[NB];
#pragma unroll
      for (int rb = 0; rb < NB; ++rb) {
        const double x = gd_value<Op>(gd_bits<Op, VEC>(raw[rb][u], e), bad[rb]);
        y[rb] = p[rb] ? x - ce : 0.0;
      }
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[0], y[0], acc[0], 0, 0, 0);
      if constexpr (NB == 2) {
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[0], y[1], acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[1], y[1], acc[2], 0, 0, 0);
      }
    }
  }
}

// Row r's pointer for a lane-varying r: a chain of selects over the kernel
// arguments (a dynamic index into them would go through scratch).
__device__ __forceinline__ const void* gd_row_ptr(const PdSlots& s, int r, int n) {
  const void* p = nullptr;
#pragma unroll
  for (int i = 0; i < kPdMaxInputs; ++i)
    if (i == r && i < n) p = s.p[i];
  return p;
}

// Where element (r, c) of a 16 x 16 product sits among a wave's 256 doubles,
// stored register by register: v_mfma_f64_16x16x4_f64 leaves D[r][c] in
// register r >> 2 of lane 16 (r & 3) + c (rows interleave over the four
// 16-lane groups, unlike the fp32 16x16x4 form; read off the device with a
// one-instruction probe, and what tests/test_gpu_gram.py proves).
__device__ __forceinline__ int gd_slot(int r, int c) { return (r >> 2) * 64 + 16 * (r & 3) + c; }

// Block blockIdx.x of gridDim.x over n rows of nelem elements: NB row blocks
// (n <= 16 NB), partials to ws[slot * blocks + block], row mask to masks[block].
template <class Op, int NB, bool VEC>
__global__ __launch_bounds__(kBlock) void k_gramdist(const PdSlots s, int n, size_t nelem, double* __restrict__ ws,
                                                     uint32_t* __restrict__ masks) {
  static_assert(kBlock == 256, "four waves: the block-end sum names them");
  constexpr int NP = NB == 1 ? 1 : 3;
  constexpr int EV = GdRaw<Op, VEC>::EV;
  __shared__ double red[kBlock / 64][NP * kGdBlockSlots];
  __shared__ uint32_t mred[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t nblk = gridDim.x, b = blockIdx.x;
  const void* p[NB];
#pragma unroll
  for (int rb = 0; rb < NB; ++rb) p[rb] = gd_row_ptr(s, kGdRows * rb + (lane & 15), n);
  f64x4 acc[NP];
  bool bad[NB];
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int rb = 0; rb < NB; ++rb) bad[rb] = false;

  const size_t items = nelem / EV;  // whole vectors, or elements
  const size_t full = items / kGdTileItems;
  const size_t slab = static_cast<size_t>(wave) * kGdWaveItems;
  for (size_t t = b; t < full; t += nblk) gd_tile<Op, NB, VEC, false>(p, t * kGdTileItems + slab, items, acc, bad);
  // the partial tile goes to the block next in the deal, the < E elements
  // past the last whole vector to the last block
  if (full * kGdTileItems < items && full % nblk == b)
    gd_tile<Op, NB, VEC, true>(p, full * kGdTileItems + slab, items, acc, bad);
  if constexpr (VEC) {
    if (items * EV < nelem && b == nblk - 1) gd_tile<Op, NB, false, true>(p, items * EV + slab, nelem, acc, bad);
  }

  // the lanes' row flags -> the wave's row mask (lane l: row 16 rb + (l & 15))
  uint32_t m = 0;
#pragma unroll
  for (int rb = 0; rb < NB; ++rb) {
    const uint64_t any = __ballot(bad[rb]);
    m |= static_cast<uint32_t>((any | (any >> 16) | (any >> 32) | (any >> 48)) & 0xffffu) << (kGdRows * rb);
  }
  if (lane == 0) mred[wave] = m;
#pragma unroll
  for (int k = 0; k < NP; ++k)
#pragma unroll
    for (int v = 0; v < 4; ++v) red[wave][k * kGdBlockSlots + v * 64 + lane] = acc[k][v];
  __syncthreads();
  for (int k = threadIdx.x; k < NP * kGdBlockSlots; k += kBlock)
    ws[static_cast<size_t>(k) * nblk + b] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  if (threadIdx.x == 0) masks[b] = (mred[0] | mred[1]) | (mred[2] | mred[3]);
}

// One wave per pair i < j (numbered row by row): G_ii, G_jj and G_ij summed
// over the blocks (pd_finish_sum's order), the blocks' row masks ORed;
// d2[i][j] and d2[j][i] get the same bits. accumulate: the entry is added to
// d2[i][j] first (pd_add_held). The diagonal is written (+0.0) unless
// accumulating.
template <class = void>
__global__ __launch_bounds__(kBlock) void k_gramdist_finish(const double* __restrict__ ws,
                                                            const uint32_t* __restrict__ masks, unsigned blocks,
                                                            int n, double* __restrict__ d2, int accumulate) {
  if (blockIdx.x == 0 && threadIdx.x < static_cast<unsigned>(n) && !accumulate)
    d2[static_cast<size_t>(threadIdx.x) * (n + 1)] = 0.0;
  const int lane = threadIdx.x & 63;
  int pair = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (pair >= n * (n - 1) / 2) return;
  int i = 0;
  while (pair >= n - 1 - i) {
    pair -= n - 1 - i;
    ++i;
  }
  const int j = i + 1 + pair;
  // partial blocks: 0 = rows 0..15 squared, 1 = rows 0..15 against 16..31, 2 = rows 16..31 squared
  const int bi = i / kGdRows, bj = j / kGdRows, li = i % kGdRows, lj = j % kGdRows;
  const int kii = 2 * bi * kGdBlockSlots + gd_slot(li, li);
  const int kjj = 2 * bj * kGdBlockSlots + gd_slot(lj, lj);
  const int kij = (bi + bj) * kGdBlockSlots + gd_slot(li, lj);
  const double gii = pd_finish_sum(ws + static_cast<size_t>(kii) * blocks, blocks, lane);
  const double gjj = pd_finish_sum(ws + static_cast<size_t>(kjj) * blocks, blocks, lane);
  const double gij = pd_finish_sum(ws + static_cast<size_t>(kij) * blocks, blocks, lane);
  uint32_t m = 0;
  for (unsigned b = lane; b < blocks; b += 64) m |= masks[b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m |= __shfl_xor(m, off);
  if (lane == 0) {
    const double d = (gii + gjj) - 2.0 * gij;
    double v = d > 0.0 ? d : 0.0;
    if (m & ((1u << i) | (1u << j))) v = __builtin_nan("");
    double* const pij = d2 + static_cast<size_t>(i) * n + j;
    const double r = accumulate ? pd_add_held(v, *pij) : v;
    *pij = r;
    d2[static_cast<size_t>(j) * n + i] = r;
  }
}

}  // namespace dlsim
