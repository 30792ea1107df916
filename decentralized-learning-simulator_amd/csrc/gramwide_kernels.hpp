// gramwide_kernels.hpp — gfx950 kernels for the matrix of squared L2 distances
// between 33 <= n <= 128 flat buffers through their Gram matrix on the fp64
// matrix unit: dlsim_gram_sqdist_wide, the wide form of
// dlsim_gram_sqdist (gramdist_kernels.hpp, n <= 32), whose contract, element
// policies, loads and value rules it shares. The reference has no such code.
//
// Contract (gramdist_kernels.hpp's): s(v) = v if finite, else 0; c = s(x_0);
// y_i = double(s(x_i)) - double(c); G_ij = sum_e y_i y_j on
// v_mfma_f64_16x16x4_f64; d2[i][j] = max(+0, G_ii + G_jj - 2 G_ij), NaN when
// row i or j holds a non-finite element.
//
// What differs: the narrow kernel's waves each convert and centre every
// operand they multiply and hold every row block's accumulators. Here a block
// of four waves computes each centred double once, leaves it in LDS, and the
// waves multiply disjoint block products out of LDS.
//
// Rows form NRB = 4, 6 or 8 row blocks of 16 (n <= 64, 96, 128; rows at or
// past n load nothing and are zero operands, and a product whose later row
// block is empty is skipped, which leaves the same +0 accumulators). A tile is
// a K-slab of kGwKElems = 64 elements of all 16 NRB rows.
//
// Prelude, once per block and slab. An item is a 16-byte vector (EV = 4 or 8
// elements) or, in the scalar form (misaligned bases, the last < EV elements),
// one element; a slab is KI = 64 / EV items per row, in G = KI / 4 groups of
// four. A wave-wide load takes one group of one row block: lane l has row
// 16 rb + (l & 15) and item 4 g + (l >> 4) of the slab (gramdist's operand
// shape). The G NRB (group, row block) units are dealt round robin to the
// four waves: with G >= 4 (fp32 vectors, the scalar form) wave w takes the
// groups g = w mod 4 of every row block, with G = 2 (16-bit vectors) group w & 1
// of the row blocks of parity w >> 1. The centre of a lane is an extra load of
// row 0's item at the lane's own index (the 16 lanes of a K-slot share the
// address; one load per group a wave takes, not per row block): no wave needs
// another's registers, whichever row blocks it has. Each lane sanitises (on
// the raw bits), subtracts the centre and writes its doubles to LDS; a
// finiteness flag per row block it loads is folded by ballot at the block's
// end into a 128-bit row mask.
//
// LDS slab: slab[k * KS + row], row fastest, KS = 16 NRB + 16 doubles: the K
// stride is an odd multiple of 128 bytes, so the four 16-lane groups of an
// operand read (one ds_read_b64: rows rb*16 .. +16 at k = 4 step + (l >> 4))
// fall on four different 128-byte bank groups of 512 bytes: no conflict. A
// prelude write puts element e of item it at k = e * KI + it, so that its four
// lane groups are one K stride apart as well. (Any bijection serves: the sum
// over k has no order of its own.) 16 NRB + 16 rows of 64 doubles: 40, 56,
// 72 KiB, single-buffered: two blocks per CU fit the 160 KiB, and the other
// block's products run under this block's prelude and barriers. The next
// slab's global loads are issued before the current slab's products and held
// in registers (36 dwords) across them.
//
// Products. The NP = NRB (NRB + 1) / 2 block products (bi <= bj, numbered row
// by row) go round robin to the waves: product q to wave q mod 4, accumulator
// q / 4 (at most 9 products, 72 accumulator registers, at NRB = 8; round robin
// also spreads the products of a last, possibly empty row block evenly). Per
// step a wave reads one operand per row block its products touch and issues
// its products. Waves own disjoint products: no block-end reduction, each wave
// stores its accumulators to ws[slot * blocks + block], slot = 256 q +
// register * 64 + lane (gd_slot within a product). The row mask's four words
// are ORed across the waves through LDS. k_gramwide_finish: one wave per pair
// i < j as k_gramdist_finish. No atomics: the bits are a function of
// (n, dtype, n_elems, alignment class).
//
// Row pointers: 128 pointers are the kernel's first argument (1 KiB at offset
// 0 of the kernarg segment); a lane loads its row's pointer from there at a
// lane-varying offset, once at kernel start (no select chain, no scratch).
#pragma once

#include <utility>

#include "gramdist_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kGwMaxInputs = 128;
constexpr int kGwKElems = 64;  // elements of a slab per row (the tile)
constexpr int kGwSteps = kGwKElems / 4;
constexpr int kGwPad = 16;     // doubles added to the K stride
constexpr int kGwMaskWords = kGwMaxInputs / 32;

struct GwRows {
  const void* p[kGwMaxInputs];
};

constexpr int gw_kstride(int nrb) { return kGdRows * nrb + kGwPad; }
constexpr int gw_products(int nrb) { return nrb * (nrb + 1) / 2; }
constexpr int gw_wave_products(int nrb) { return (gw_products(nrb) + 3) / 4; }
// product (bi <= bj) -> its number, and back
constexpr int gw_pidx(int bi, int bj, int nrb) { return bi * nrb - bi * (bi - 1) / 2 + (bj - bi); }
constexpr int gw_prod_bi(int q, int nrb) {
  int bi = 0;
  while (q >= nrb - bi) {
    q -= nrb - bi;
    ++bi;
  }
  return bi;
}
constexpr int gw_prod_bj(int q, int nrb) {
  int bi = 0;
  while (q >= nrb - bi) {
    q -= nrb - bi;
    ++bi;
  }
  return bi + q;
}
// products of wave w, and whether one of them touches row block rb
constexpr int gw_count(int nrb, int w) { return (gw_products(nrb) - w + 3) / 4; }
constexpr bool gw_needs(int nrb, int w, int rb) {
  for (int q = w; q < gw_products(nrb); q += 4)
    if (gw_prod_bi(q, nrb) == rb || gw_prod_bj(q, nrb) == rb) return true;
  return false;
}
// the same as constants of their types: an index into registers must be one
template <int NRB, int Q>
struct GwProd {
  static constexpr int bi = gw_prod_bi(Q, NRB), bj = gw_prod_bj(Q, NRB);
};
template <int NRB, int W, int RB>
struct GwNeeds {
  static constexpr bool value = gw_needs(NRB, W, RB);
};

// How a slab's items are dealt to the waves (the header comment).
template <class Op, int NRB, bool VEC>
struct GwDeal {
  static constexpr int EV = GdRaw<Op, VEC>::EV;
  static constexpr int KI = kGwKElems / EV;          // items of a slab per row
  static constexpr int G = KI / 4;                   // groups of four items
  static constexpr int GW = G >= 4 ? G / 4 : 1;      // groups a wave takes of a row block
  static constexpr int NR = G >= 4 ? NRB : NRB / 2;  // row blocks a wave takes
  static_assert(G == 2 || G % 4 == 0, "the deal covers every (group, row block) once");
  static_assert(NRB % 2 == 0 && NRB <= kGwMaxInputs / kGdRows, "row-block classes are even");
  __device__ static int rb(int j, int wave) { return G >= 4 ? j : 2 * j + (wave >> 1); }
  __device__ static int group(int gi, int wave) { return G >= 4 ? wave + 4 * gi : (wave & 1); }
};

// Row `row`'s pointer out of the kernarg segment (GwRows is the first
// argument), null at or past n.
__device__ __forceinline__ const void* gw_row_ptr(int row, int n) {
  typedef const void* Ptr;
  const __attribute__((address_space(4))) Ptr* const args =
      (const __attribute__((address_space(4))) Ptr*)__builtin_amdgcn_kernarg_segment_ptr();
  return row < n ? args[row] : nullptr;
}

template <class D>
__device__ __forceinline__ void gw_resolve(int n, const void* (&p)[D::NR]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < D::NR; ++j) p[j] = gw_row_ptr(kGdRows * D::rb(j, wave) + (lane & 15), n);
}

// The wave's items of the slab at item `base`, and row 0's items beside them.
template <class Op, int NRB, bool VEC, bool CHECK>
__device__ __forceinline__ void gw_load(const void* (&p)[GwDeal<Op, NRB, VEC>::NR], const void* p0, size_t base,
                                        size_t count,
                                        GdRaw<Op, VEC> (&raw)[GwDeal<Op, NRB, VEC>::NR][GwDeal<Op, NRB, VEC>::GW],
                                        GdRaw<Op, VEC> (&cen)[GwDeal<Op, NRB, VEC>::GW]) {
  using D = GwDeal<Op, NRB, VEC>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int gi = 0; gi < D::GW; ++gi) {
    const size_t idx = base + 4 * D::group(gi, wave) + (lane >> 4);
    cen[gi] = gd_load<Op, VEC, CHECK>(p0, idx, count);
#pragma unroll
    for (int j = 0; j < D::NR; ++j) {
      if (p[j]) raw[j][gi] = gd_load<Op, VEC, CHECK>(p[j], idx, count);
      else raw[j][gi] = GdRaw<Op, VEC>{};
    }
  }
}

// Sanitise, centre, and write the wave's doubles into the slab.
template <class Op, int NRB, bool VEC>
__device__ __forceinline__ void gw_store(const void* (&p)[GwDeal<Op, NRB, VEC>::NR],
                                         const GdRaw<Op, VEC> (&raw)[GwDeal<Op, NRB, VEC>::NR][GwDeal<Op, NRB, VEC>::GW],
                                         const GdRaw<Op, VEC> (&cen)[GwDeal<Op, NRB, VEC>::GW],
                                         bool (&bad)[GwDeal<Op, NRB, VEC>::NR], double* __restrict__ slab) {
  using D = GwDeal<Op, NRB, VEC>;
  constexpr int KS = gw_kstride(NRB);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int gi = 0; gi < D::GW; ++gi) {
    const int item = 4 * D::group(gi, wave) + (lane >> 4);
#pragma unroll
    for (int e = 0; e < D::EV; ++e) {
      bool centre_bad = false;  // row 0's own lanes flag it
      const double ce = gd_value<Op>(gd_bits<Op, VEC>(cen[gi], e), centre_bad);
      double* const dst = slab + (e * D::KI + item) * KS + (lane & 15);
#pragma unroll
      for (int j = 0; j < D::NR; ++j) {
        const double x = gd_value<Op>(gd_bits<Op, VEC>(raw[j][gi], e), bad[j]);
        dst[kGdRows * D::rb(j, wave)] = p[j] ? x - ce : 0.0;
      }
    }
  }
}

// The 128-bit row mask as two words (no array: nothing to index at run time).
struct GwMask {
  uint64_t lo, hi;
};

// The lanes' row flags -> the wave's share of the row mask.
template <class D>
__device__ __forceinline__ void gw_fold_mask(const bool (&bad)[D::NR], GwMask& m) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < D::NR; ++j) {
    const uint64_t any = __ballot(bad[j]);
    const uint64_t bits = (any | (any >> 16) | (any >> 32) | (any >> 48)) & 0xffffu;
    const int pos = kGdRows * D::rb(j, wave);  // the row block's first row
    m.lo |= pos < 64 ? bits << (pos & 63) : 0u;
    m.hi |= pos < 64 ? 0u : bits << (pos & 63);
  }
}

// One step of wave W's products: an operand per row block they touch, then
// the products whose later row block holds a row (only the last row block of
// a class can be empty: `last` says that it is not).
template <int NRB, int W, int... RB, int... K>
__device__ __forceinline__ void gw_step(const double* __restrict__ src, bool last, f64x4 (&acc)[gw_wave_products(NRB)],
                                        std::integer_sequence<int, RB...>, std::integer_sequence<int, K...>) {
  double op[NRB];
  ((op[RB] = GwNeeds<NRB, W, RB>::value ? src[kGdRows * RB] : 0.0), ...);
  ((GwProd<NRB, W + 4 * K>::bj < NRB - 1 || last
        ? (void)(acc[K] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[GwProd<NRB, W + 4 * K>::bi],
                                                               op[GwProd<NRB, W + 4 * K>::bj], acc[K], 0, 0, 0))
        : (void)0),
   ...);
}

// Wave W's products over the slab.
template <int NRB, int W>
__device__ __forceinline__ void gw_mma(const double* __restrict__ slab, int n, f64x4 (&acc)[gw_wave_products(NRB)]) {
  constexpr int KS = gw_kstride(NRB);
  const int lane = threadIdx.x & 63;
  const double* const src = slab + (lane >> 4) * KS + (lane & 15);
  const bool last = kGdRows * (NRB - 1) < n;
  for (int s = 0; s < kGwSteps; ++s)
    gw_step<NRB, W>(src + 4 * s * KS, last, acc, std::make_integer_sequence<int, NRB>{},
                    std::make_integer_sequence<int, gw_count(NRB, W)>{});
}

template <int NRB>
__device__ __forceinline__ void gw_mma_wave(const double* __restrict__ slab, int n,
                                            f64x4 (&acc)[gw_wave_products(NRB)]) {
  switch (threadIdx.x >> 6) {  // wave-uniform
    case 0: gw_mma<NRB, 0>(slab, n, acc); break;
    case 1: gw_mma<NRB, 1>(slab, n, acc); break;
    case 2: gw_mma<NRB, 2>(slab, n, acc); break;
    default: gw_mma<NRB, 3>(slab, n, acc); break;
  }
}

// Wave W's accumulators to ws[slot * nblk + b].
template <int NRB, int W, int... K>
__device__ __forceinline__ void gw_flush(const f64x4 (&acc)[gw_wave_products(NRB)], double* __restrict__ ws,
                                         size_t nblk, size_t b, std::integer_sequence<int, K...>) {
  const int lane = threadIdx.x & 63;
  (([&] {
#pragma unroll
     for (int v = 0; v < 4; ++v)
       ws[static_cast<size_t>((W + 4 * K) * kGdBlockSlots + v * 64 + lane) * nblk + b] = acc[K][v];
   }()),
   ...);
}

// A slab outside the pipelined loop (the partial tile, the tail): load, write,
// multiply.
template <class Op, int NRB, bool VEC>
__device__ __forceinline__ void gw_single(const void* (&p)[GwDeal<Op, NRB, VEC>::NR], const void* p0, size_t base,
                                          size_t count, bool (&bad)[GwDeal<Op, NRB, VEC>::NR], double* __restrict__ slab,
                                          int n, f64x4 (&acc)[gw_wave_products(NRB)]) {
  using D = GwDeal<Op, NRB, VEC>;
  GdRaw<Op, VEC> raw[D::NR][D::GW], cen[D::GW];
  gw_load<Op, NRB, VEC, true>(p, p0, base, count, raw, cen);
  gw_store<Op, NRB, VEC>(p, raw, cen, bad, slab);
  __syncthreads();
  gw_mma_wave<NRB>(slab, n, acc);
  __syncthreads();
}

// Block blockIdx.x of gridDim.x over n rows (16 (NRB - 2) < n <= 16 NRB) of
// nelem elements: partials to ws[slot * blocks + block], the row mask's words
// to masks[4 block ..]. `rows` must stay the first argument (gw_row_ptr).
template <class Op, int NRB, bool VEC>
__global__ __launch_bounds__(kBlock) void k_gramwide(const GwRows rows, int n, size_t nelem, double* __restrict__ ws,
                                                     uint32_t* __restrict__ masks) {
  static_assert(kBlock == 256, "four waves: the deal and the product table name them");
  using D = GwDeal<Op, NRB, VEC>;
  constexpr int MAXP = gw_wave_products(NRB);
  __shared__ double slab[kGwKElems * gw_kstride(NRB)];
  __shared__ uint32_t mred[kBlock / 64][kGwMaskWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t nblk = gridDim.x, b = blockIdx.x;
  const void* p[D::NR];
  gw_resolve<D>(n, p);
  const void* const p0 = rows.p[0];
  f64x4 acc[MAXP];
  bool bad[D::NR];
  GwMask m{0u, 0u};
#pragma unroll
  for (int k = 0; k < MAXP; ++k) acc[k] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < D::NR; ++j) bad[j] = false;

  const size_t items = nelem / D::EV;  // whole vectors, or elements
  const size_t full = items / D::KI;
  {
    GdRaw<Op, VEC> raw[D::NR][D::GW], cen[D::GW];
    if (b < full) gw_load<Op, NRB, VEC, false>(p, p0, b * D::KI, items, raw, cen);
    for (size_t t = b; t < full; t += nblk) {
      gw_store<Op, NRB, VEC>(p, raw, cen, bad, slab);
      __syncthreads();
      // the next slab's loads fly under this slab's products
      if (t + nblk < full) gw_load<Op, NRB, VEC, false>(p, p0, (t + nblk) * D::KI, items, raw, cen);
      gw_mma_wave<NRB>(slab, n, acc);
      __syncthreads();
    }
  }
  // the partial tile goes to the block next in the deal, the < EV elements
  // past the last whole vector to the last block
  if (full * D::KI < items && full % nblk == b) gw_single<Op, NRB, VEC>(p, p0, full * D::KI, items, bad, slab, n, acc);
  gw_fold_mask<D>(bad, m);
  if constexpr (VEC) {
    if (items * D::EV < nelem && b == nblk - 1) {
      using DS = GwDeal<Op, NRB, false>;
      const void* ps[DS::NR];
      bool bads[DS::NR];
      gw_resolve<DS>(n, ps);
#pragma unroll
      for (int j = 0; j < DS::NR; ++j) bads[j] = false;
      gw_single<Op, NRB, false>(ps, p0, items * D::EV, nelem, bads, slab, n, acc);
      gw_fold_mask<DS>(bads, m);
    }
  }

  if (lane == 0) {
    mred[wave][0] = static_cast<uint32_t>(m.lo);
    mred[wave][1] = static_cast<uint32_t>(m.lo >> 32);
    mred[wave][2] = static_cast<uint32_t>(m.hi);
    mred[wave][3] = static_cast<uint32_t>(m.hi >> 32);
  }
  switch (wave) {
    case 0: gw_flush<NRB, 0>(acc, ws, nblk, b, std::make_integer_sequence<int, gw_count(NRB, 0)>{}); break;
    case 1: gw_flush<NRB, 1>(acc, ws, nblk, b, std::make_integer_sequence<int, gw_count(NRB, 1)>{}); break;
    case 2: gw_flush<NRB, 2>(acc, ws, nblk, b, std::make_integer_sequence<int, gw_count(NRB, 2)>{}); break;
    default: gw_flush<NRB, 3>(acc, ws, nblk, b, std::make_integer_sequence<int, gw_count(NRB, 3)>{}); break;
  }
  __syncthreads();
  if (threadIdx.x < kGwMaskWords)
    masks[b * kGwMaskWords + threadIdx.x] =
        (mred[0][threadIdx.x] | mred[1][threadIdx.x]) | (mred[2][threadIdx.x] | mred[3][threadIdx.x]);
}

// One wave per pair i < j (numbered row by row), as k_gramdist_finish over
// nrb row blocks and the four-word mask: G_ii, G_jj and G_ij summed over the
// blocks (pd_finish_sum's order), the blocks' row masks ORed; d2[i][j] and
// d2[j][i] get the same bits. accumulate: the entry is added to d2[i][j] first
// (pd_add_held). The diagonal is written (+0.0) unless accumulating.
template <class = void>
__global__ __launch_bounds__(kBlock) void k_gramwide_finish(const double* __restrict__ ws,
                                                            const uint32_t* __restrict__ masks, unsigned blocks,
                                                            int n, int nrb, double* __restrict__ d2, int accumulate) {
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
  const int bi = i / kGdRows, bj = j / kGdRows, li = i % kGdRows, lj = j % kGdRows;
  const int kii = gw_pidx(bi, bi, nrb) * kGdBlockSlots + gd_slot(li, li);
  const int kjj = gw_pidx(bj, bj, nrb) * kGdBlockSlots + gd_slot(lj, lj);
  const int kij = gw_pidx(bi, bj, nrb) * kGdBlockSlots + gd_slot(li, lj);
  const double gii = pd_finish_sum(ws + static_cast<size_t>(kii) * blocks, blocks, lane);
  const double gjj = pd_finish_sum(ws + static_cast<size_t>(kjj) * blocks, blocks, lane);
  const double gij = pd_finish_sum(ws + static_cast<size_t>(kij) * blocks, blocks, lane);
  uint32_t m = 0;  // row i's word and row j's, their bits moved to 0 and 1
  for (unsigned b = lane; b < blocks; b += 64)
    m |= ((masks[b * kGwMaskWords + (i >> 5)] >> (i & 31)) & 1u) | (((masks[b * kGwMaskWords + (j >> 5)] >> (j & 31)) & 1u) << 1);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m |= __shfl_xor(m, off);
  if (lane == 0) {
    const double d = (gii + gjj) - 2.0 * gij;
    double v = d > 0.0 ? d : 0.0;
    if (m) v = __builtin_nan("");
    double* const pij = d2 + static_cast<size_t>(i) * n + j;
    const double r = accumulate ? pd_add_held(v, *pij) : v;
    *pij = r;
    d2[static_cast<size_t>(j) * n + i] = r;
  }
}

}  // namespace dlsim
