// pairdist_kernels.hpp — gfx950 kernels for the matrix of squared L2 distances
// between n flat buffers: the primitive under Krum and
// Multi-Krum (gradient_aggregation/krum.py) and the consensus distance of the
// gossip literature. The reference has no such code: its one aggregator is
// FedAvg (dasklearn/gradient_aggregation/fedavg.py).
//
// Contract, for i != j:  d2[i][j] = sum_e (double(x_i[e]) - double(x_j[e]))^2.
// Every value is widened to double (exact for fp32, fp64, bf16, fp16), the
// subtraction is a double subtraction and each term enters its accumulator
// with one fma(d, d, acc), written out because the library is built with
// -ffp-contract=off (hence policy names outside scripts/audit_isa.py's
// POLICIES). The summation order is this file's: per lane over the tiles its
// block strides over, then the 64 lanes of a wave (xor butterfly), the four
// waves of a block in wave order, and in k_pairdist_finish the blocks (lane l
// of a wave adds blocks l, l + 64, ... in order, then the same butterfly).
// There is no float atomic: the order is a function of the grid alone, and
// the grid is a function of (n, dtype, n_elems, alignment class) alone.
//
// Unlike every other kernel of the library this one reduces along the
// parameter axis. Its input side is the tiled reduce's (wreduce_kernels.hpp):
// 256-lane blocks, one 16-byte load per lane and row, every row's load of a
// tile issued before the first use. Rows go in groups of 8 (kPdGroup):
//   * a diagonal unit holds the pairs inside one group: 28 double accumulators
//     per lane beside 8 loaded vectors;
//   * a cross unit holds 8 rows of one group against 4 rows (kPdCross) of a
//     later group: 32 accumulators beside 12 loaded vectors. (8 x 8 would be
//     128 VGPRs of accumulators.)
// n <= 8 is one diagonal unit and reads every row once (n <= 4: a 4-row unit
// of 6 accumulators). Larger n is one launch whose second grid dimension is
// the unit: G = ceil(n / 8) diagonal units, then two cross units per group
// pair; a row is read once per unit it belongs to (about 2x at n = 16, 4x at
// n = 32). Absent rows of a unit (n no multiple of the group) load nothing
// and count as zeros; their slots are never read.
//
// A block strides over full tiles without bounds checks and keeps its
// accumulators in registers until its end: per accumulator a 64-lane shuffle
// reduce, the waves' sums through LDS, one store of the block's partials to
// ws[(unit * kPdSlots + slot) * blocks + block]. k_pairdist_finish then takes
// one wave per pair (i < j), adds the blocks' partials and stores the result
// to d2[i][j] and d2[j][i] (or adds it to d2[i][j] and stores that to both).
// The scalar form (VEC = false: one element per lane and row, any alignment)
// shares all of this.
#pragma once

#include "wreduce_kernels.hpp"

#pragma clang fp contract(off)

namespace dlsim {

constexpr int kPdMaxInputs = 32;
constexpr int kPdGroup = 8;   // rows of a group (and of a diagonal unit)
constexpr int kPdCross = 4;   // rows on the short side of a cross unit
constexpr int kPdSlots = 32;  // partial sums a unit owns per block (28 or 6 used by a diagonal unit)

// ---- element policies ---------------------------------------------------------
// What unpack-style code needs to know of an element; the arithmetic is in
// double for all of them.
struct PdF32 {
  static constexpr int E = 4;
  static constexpr int kBytes = 4;
  static constexpr int kFmt = kFmtF32;
};
struct PdF64 {
  using T = double;
  using W = double;
  static constexpr int E = 2;
  static constexpr int kBytes = 8;
  static constexpr int kFmt = kFmtF32;
};
struct PdBF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtBF16;
};
struct PdF16 {
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  static constexpr int kFmt = kFmtF16;
};

// The n <= 32 input pointers travel in the kernarg segment (scalar loads; a
// unit indexes them with its wave-uniform first row).
struct PdSlots {
  const void* p[kPdMaxInputs];
  __device__ const void* ptr(int i) const { return p[i]; }
};

// What a lane holds of one row between the load and the arithmetic: a 16-byte
// vector (VEC) or one element in its accumulator type.
template <class Op, bool VEC>
struct PdRaw {
  using type = u32x4;
  static constexpr int EV = Op::E;
  __device__ static type zero() { return u32x4{0u, 0u, 0u, 0u}; }
};
template <class Op>
struct PdRaw<Op, false> {
  using type = acc_t<Op>;
  static constexpr int EV = 1;
  __device__ static type zero() { return 0; }
};

// Item idx of a row (vector or element); zeros past `count` when CHECK.
template <class Op, bool VEC, bool CHECK, int LDP>
__device__ __forceinline__ typename PdRaw<Op, VEC>::type pd_load(const void* p, size_t idx, size_t count) {
  typename PdRaw<Op, VEC>::type r = PdRaw<Op, VEC>::zero();
  if (!CHECK || idx < count) {
    if constexpr (VEC) r = ld16<LDP>(p, idx);
    else r = load_elem<Op>(p, idx);
  }
  return r;
}

// Element e of a loaded item, widened to double (exact).
template <class Op, bool VEC>
__device__ __forceinline__ double pd_elem(const typename PdRaw<Op, VEC>::type& r, int e) {
  if constexpr (!VEC) {
    return static_cast<double>(r);
  } else if constexpr (Op::kBytes == 8) {
    return __builtin_bit_cast(double, static_cast<uint64_t>(r[2 * e]) | (static_cast<uint64_t>(r[2 * e + 1]) << 32));
  } else if constexpr (Op::kBytes == 4) {
    return static_cast<double>(__uint_as_float(r[e]));
  } else if constexpr (Op::kFmt == kFmtF16) {
    const uint32_t u = r[e / 2];
    const uint16_t h = static_cast<uint16_t>((e & 1) ? (u >> 16) : (u & 0xffffu));
    return static_cast<double>(__builtin_bit_cast(_Float16, h));
  } else {
    const uint32_t u = r[e / 2];
    return static_cast<double>(__uint_as_float((e & 1) ? (u & 0xffff0000u) : (u << 16)));
  }
}

// accumulators of a unit: RB == 0 is a diagonal unit over RA rows
template <int RA, int RB> constexpr int pd_pairs() { return RB ? RA * RB : RA * (RA - 1) / 2; }
// slot of the pair (i < j) inside a diagonal unit of RA rows (the finish kernel restates it)
constexpr int pd_diag_slot(int ra, int i, int j) { return i * ra - i * (i + 1) / 2 + (j - i - 1); }

// One item per lane and row: all loads first, then element by element the
// rows' values widened and one subtraction and one fma per pair.
// (S: where the row pointers are, PdSlots or a task of a batch, PdTaskArgs.)
template <class Op, int RA, int RB, bool VEC, bool CHECK, int LDP, class S>
__device__ __forceinline__ void pd_tile(const S& s, int a0, int na, int b0, int nb, size_t idx, size_t count,
                                        double (&acc)[pd_pairs<RA, RB>()]) {
  using Raw = PdRaw<Op, VEC>;
  constexpr int kRB = RB ? RB : 1;
  typename Raw::type ra[RA], rb[kRB];
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    ra[i] = Raw::zero();
    if (i < na) ra[i] = pd_load<Op, VEC, CHECK, LDP>(s.ptr(a0 + i), idx, count);
  }
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    rb[j] = Raw::zero();
    if (j < nb) rb[j] = pd_load<Op, VEC, CHECK, LDP>(s.ptr(b0 + j), idx, count);
  }
#pragma unroll
  for (int e = 0; e < Raw::EV; ++e) {
    double xa[RA], xb[kRB];
#pragma unroll
    for (int i = 0; i < RA; ++i) xa[i] = pd_elem<Op, VEC>(ra[i], e);
    if constexpr (RB == 0) {
#pragma unroll
      for (int i = 0; i < RA; ++i)
#pragma unroll
        for (int j = i + 1; j < RA; ++j) {
          const double d = xa[i] - xa[j];
          acc[pd_diag_slot(RA, i, j)] = __builtin_fma(d, d, acc[pd_diag_slot(RA, i, j)]);
        }
    } else {
#pragma unroll
      for (int j = 0; j < RB; ++j) xb[j] = pd_elem<Op, VEC>(rb[j], e);
#pragma unroll
      for (int i = 0; i < RA; ++i)
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const double d = xa[i] - xb[j];
          acc[i * RB + j] = __builtin_fma(d, d, acc[i * RB + j]);
        }
    }
  }
}

// A block's end: per accumulator the 64 lanes of a wave (xor butterfly), the
// four waves through LDS in wave order, one store of the block's partial to
// ws[k * nblk + b]: block b of nblk (gridDim.x / blockIdx.x of a flat launch,
// a segment's own virtual grid in a batch). (Shared with reducedist_kernels.hpp.)
template <int NP>
__device__ __forceinline__ void pd_block_sum(const double (&acc)[NP], double* __restrict__ ws,
                                             double (*red)[kPdSlots], size_t nblk, size_t b) {
  static_assert(NP <= kPdSlots, "a block's partials fit its slots");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    const int k = threadIdx.x;
    ws[static_cast<size_t>(k) * nblk + b] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// One wave's sum of the `blocks` partials at src: lane l adds blocks l,
// l + 64, ... in order, then the butterfly; every lane returns the sum.
__device__ __forceinline__ double pd_finish_sum(const double* __restrict__ src, unsigned blocks, int lane) {
  double v = 0.0;
  for (unsigned b = lane; b < blocks; b += 64) v = v + src[b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

// One unit of one block: rows a0 .. a0 + na (and b0 .. b0 + nb of a cross
// unit) over this block's share of the items, then the block's partial sums
// to ws[slot * nblk + b] (block b of the unit's nblk, as pd_block_sum). Every
// block of a unit stores all its slots, zeros where it had no tile. red:
// kBlock / 64 rows of kPdSlots.
template <class Op, int RA, int RB, bool VEC, int LDP, class S>
__device__ __forceinline__ void pd_unit(const S& s, int a0, int na, int b0, int nb, size_t nelem,
                                        double* __restrict__ ws, double (*red)[kPdSlots], size_t nblk, size_t b) {
  constexpr int NP = pd_pairs<RA, RB>();
  constexpr int EV = PdRaw<Op, VEC>::EV;
  static_assert(NP <= kPdSlots, "a unit's partials fit its slots");
  double acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = 0.0;
  const size_t items = nelem / EV;  // whole vectors, or elements
  const size_t full = items / kBlock;
  for (size_t t = b; t < full; t += nblk)
    pd_tile<Op, RA, RB, VEC, false, LDP>(s, a0, na, b0, nb, t * kBlock + threadIdx.x, items, acc);
  // the partial tile goes to the block next in the deal, the < E elements
  // past the last whole vector to the last block (the one with the fewest tiles)
  if (full * kBlock < items && full % nblk == b)
    pd_tile<Op, RA, RB, VEC, true, LDP>(s, a0, na, b0, nb, full * kBlock + threadIdx.x, items, acc);
  if constexpr (VEC) {
    if (items * EV < nelem && b == nblk - 1)
      pd_tile<Op, RA, RB, false, true, 0>(s, a0, na, b0, nb, items * EV + threadIdx.x, nelem, acc);
  }
  pd_block_sum<NP>(acc, ws, red, nblk, b);
}

// Block b of the nblk blocks of unit u over n rows of nelem elements, ws the
// call's partials. CROSS = false: the one diagonal unit of n <= CAP rows
// (CAP 4 or 8). CROSS = true (CAP 8, n > 8): units 0 .. G-1 are the groups'
// diagonal units, unit G + 2 * pair + half the 8 rows of group ga against
// rows 8 gb + 4 half .. + 4 of group gb, the pairs ga < gb numbered row by
// row. Units without a pair of rows return at once.
template <class Op, int CAP, bool CROSS, bool VEC, class S>
__device__ __forceinline__ void pd_block(const S& s, int n, size_t nelem, double* __restrict__ ws, int u, size_t nblk,
                                         size_t b, double (*red)[kPdSlots]) {
  // rows read by several units stay cacheable; a single unit streams
  constexpr int LDP = CROSS ? 0 : 1;
  double* const wsu = ws + static_cast<size_t>(u) * kPdSlots * nblk;
  if constexpr (!CROSS) {
    pd_unit<Op, CAP, 0, VEC, LDP>(s, 0, n, 0, 0, nelem, wsu, red, nblk, b);
  } else {
    const int groups = (n + kPdGroup - 1) / kPdGroup;
    if (u < groups) {
      const int a0 = u * kPdGroup;
      const int na = min(kPdGroup, n - a0);
      if (na < 2) return;
      pd_unit<Op, kPdGroup, 0, VEC, LDP>(s, a0, na, 0, 0, nelem, wsu, red, nblk, b);
    } else {
      int pair = (u - groups) >> 1, ga = 0;
      const int half = (u - groups) & 1;
      while (pair >= groups - 1 - ga) {
        pair -= groups - 1 - ga;
        ++ga;
      }
      const int gb = ga + 1 + pair;
      const int b0 = gb * kPdGroup + half * kPdCross;
      const int nb = min(kPdCross, n - b0);
      if (nb < 1) return;
      pd_unit<Op, kPdGroup, kPdCross, VEC, LDP>(s, ga * kPdGroup, kPdGroup, b0, nb, nelem, wsu, red, nblk, b);
    }
  }
}

// grid (blocks, units): block blockIdx.x of unit blockIdx.y (pd_block)
template <class Op, int CAP, bool CROSS, bool VEC>
__global__ __launch_bounds__(kBlock) void k_pairdist(const PdSlots s, int n, size_t nelem, double* __restrict__ ws) {
  static_assert(kBlock == 256, "four waves: the block-end sum names them");
  __shared__ double red[kBlock / 64][kPdSlots];
  pd_block<Op, CAP, CROSS, VEC>(s, n, nelem, ws, static_cast<int>(blockIdx.y), gridDim.x, blockIdx.x, red);
}

// sum + held: how a finish kernel adds its sum to what the matrix holds, as one
// instruction with the operands in this order. For numbers the order is
// immaterial; a NaN plus a NaN of another sign or payload (a NaN input in one
// tensor, Inf - Inf in the next) keeps the first operand's bits, and the
// compiler may commute a plain `+` differently in two kernels. Written out so
// that k_pairdist_finish and k_pairdist_batch_finish agree bit for bit. The
// order is the one `*pij + v` compiled to in k_pairdist_finish before the
// batched kernels came (the sum in src0, the loaded value in src1: the device
// assembly lines are in profiles/krum_batch/finish_add_operands.md, DESIGN.md
// §8n), so the flat entry's bits did not move for NaN payloads either.
__device__ __forceinline__ double pd_add_held(double sum, double held) {
  double r;
  asm("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(sum), "v"(held));
  return r;
}

// Pair number `pair` of n rows (i < j, numbered row by row) -> i, j and
// unit * kPdSlots + slot: where the main kernel's units left the pair's
// partials. cap: rows of the diagonal units (4 or 8).
__device__ __forceinline__ int pd_pair_slot(int pair, int n, int cap, int& i, int& j) {
  i = 0;
  while (pair >= n - 1 - i) {
    pair -= n - 1 - i;
    ++i;
  }
  j = i + 1 + pair;
  const int groups = (n + kPdGroup - 1) / kPdGroup;
  const int gi = i / kPdGroup, gj = j / kPdGroup, li = i % kPdGroup, lj = j % kPdGroup;
  int unit, slot;
  if (gi == gj) {
    unit = groups > 1 ? gi : 0;
    slot = pd_diag_slot(cap, li, lj);
  } else {
    unit = groups + 2 * (gi * groups - gi * (gi + 1) / 2 + (gj - gi - 1)) + lj / kPdCross;
    slot = li * kPdCross + lj % kPdCross;
  }
  return unit * kPdSlots + slot;
}

// One wave per pair i < j (numbered row by row): the pair's partials of all
// blocks, lane l adding blocks l, l + 64, ... in order, then the butterfly;
// d2[i][j] and d2[j][i] get the same bits. accumulate: the sum is added to
// d2[i][j] first. The diagonal is written (+0.0) unless accumulating.
// cap: rows of the diagonal units (4 or 8). (A template so that the header,
// included by two units, defines it once: launched as k_pairdist_finish<>.)
template <class = void>
__global__ __launch_bounds__(kBlock) void k_pairdist_finish(const double* __restrict__ ws, unsigned blocks, int n,
                                                            int cap, double* __restrict__ d2, int accumulate) {
  if (blockIdx.x == 0 && threadIdx.x < static_cast<unsigned>(n) && !accumulate)
    d2[static_cast<size_t>(threadIdx.x) * (n + 1)] = 0.0;
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (pair >= n * (n - 1) / 2) return;
  int i, j;
  const int where = pd_pair_slot(pair, n, cap, i, j);
  const double* const src = ws + static_cast<size_t>(where) * blocks;
  const double v = pd_finish_sum(src, blocks, lane);
  if (lane == 0) {
    double* const pij = d2 + static_cast<size_t>(i) * n + j;
    const double r = accumulate ? pd_add_held(v, *pij) : v;
    *pij = r;
    d2[static_cast<size_t>(j) * n + i] = r;
  }
}

}  // namespace dlsim
