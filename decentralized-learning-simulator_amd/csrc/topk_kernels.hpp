// topk_kernels.hpp — gfx950 kernels for top-k sparsified model sharing
// (dlsim_topk_select). The reference has no such code: it shares
// dense models only.
//
// Contract, over the model x and the last-shared copy ref (P elements each):
//   d[e]   = float(x[e]) - float(ref[e])     one fp32 subtraction (bf16 widens exactly)
//   key[e] = the bits of d[e] with the sign bit cleared, as an unsigned integer
// so keys order as |d| < +Inf < NaN: a NaN delta ranks highest and is always
// shared (torch.topk does the same); +0 and -0 both give key 0. Selected are
// the k largest keys; among equal keys at the threshold the lowest indices
// win. idx comes out strictly ascending, val[i] = x[idx[i]] bit for bit, and
// ref[idx[i]] = x[idx[i]]; no other byte of ref changes.
//
// Method: radix select on the 31-bit key in three digit passes (11 + 10 + 10
// bits), then a counting pass and a writing pass. Everything that crosses
// lanes is an integer: LDS and global histogram adds commute, block counts are
// scanned in block order by one block, so the result does not depend on
// scheduling. No float atomics.
//   k_topk_clear        zeroes the histograms and tickets, sets remaining = k
//   k_topk_hist<PASS>   every block builds the digit histogram of the keys whose
//                       higher digits equal the prefix chosen so far (LDS integer
//                       atomics), adds it to the global one, and takes a ticket;
//                       the last block walks the 2048 / 1024 bins from the top
//                       and fixes the digit that holds the k-th largest key
//   k_topk_count        per block: keys > T and keys == T; the last block (a
//                       ticket again) turns both arrays into exclusive prefixes
//   k_topk_write        compacts with wave ballots and population counts from
//                       the block's prefixes: element order is index order, so
//                       idx ascends and the first `need` ties win by construction
// A block owns a run of consecutive tiles (the same run in every pass), a lane
// one 16-byte vector of each of a tile's kTopkVpt rows. The vector form loads
// 16 bytes per lane from x and ref; the scalar form (a base off 16-byte
// alignment) and the last, partial vector load element by element under a
// bound check. The workspace (3 histograms, 16 state words, 2 words per block)
// belongs to the call.
#pragma once

#include "wreduce_kernels.hpp"

namespace dlsim {

constexpr int kTopkVpt = 2;                // rows of kBlock vectors per tile
constexpr unsigned kTopkMaxBlocks = 1024;  // four blocks on each of 256 CUs
constexpr int kTopkBins = 2048;            // the widest digit (11 bits)
// word offsets into the workspace, behind the three histograms: the 16 state words ([0] prefix / T,
// [1] remaining / need, [2..4] hist tickets, [5] count ticket), then the per-block counts gt[blocks], eq[blocks]
constexpr int kTopkWsStateOff = 3 * kTopkBins;
constexpr int kTopkWsCountsOff = kTopkWsStateOff + 16;

__host__ __device__ constexpr int topk_bits(int pass) { return pass == 0 ? 11 : 10; }
__host__ __device__ constexpr int topk_shift(int pass) { return pass == 0 ? 20 : pass == 1 ? 10 : 0; }

struct TopkF32 {
  using Elem = uint32_t;
  static constexpr int E = 4;
  static constexpr int kBytes = 4;
  __device__ static float widen(Elem b) { return __uint_as_float(b); }
  __device__ static Elem lane(const u32x4& r, int e) { return r[e]; }
};

struct TopkBF16 {
  using Elem = uint16_t;
  static constexpr int E = 8;
  static constexpr int kBytes = 2;
  __device__ static float widen(Elem b) { return __uint_as_float(static_cast<uint32_t>(b) << 16); }
  __device__ static Elem lane(const u32x4& r, int e) { return static_cast<Elem>(r[e >> 1] >> (16 * (e & 1))); }
};

template <class Op>
__device__ __forceinline__ uint32_t topk_key(typename Op::Elem x, typename Op::Elem r) {
  return __float_as_uint(Op::widen(x) - Op::widen(r)) & 0x7fffffffu;
}

// The E elements from e0 on: xb = the bits of x, key = their keys, and the
// return value a mask of the elements below P (0 when e0 >= P).
template <class Op, bool VEC>
__device__ __forceinline__ uint32_t topk_load(const void* x, const void* ref, size_t e0, size_t P,
                                              typename Op::Elem (&xb)[Op::E], uint32_t (&key)[Op::E]) {
  using Elem = typename Op::Elem;
  constexpr int E = Op::E;
  if (VEC && e0 + E <= P) {
    const u32x4 vx = static_cast<const u32x4*>(x)[e0 / E];
    const u32x4 vr = static_cast<const u32x4*>(ref)[e0 / E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xb[e] = Op::lane(vx, e);
      key[e] = topk_key<Op>(xb[e], Op::lane(vr, e));
    }
    return (1u << E) - 1u;
  }
  uint32_t valid = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    xb[e] = 0;
    key[e] = 0;
    if (e0 + e < P) {
      xb[e] = static_cast<const Elem*>(x)[e0 + e];
      key[e] = topk_key<Op>(xb[e], static_cast<const Elem*>(ref)[e0 + e]);
      valid |= 1u << e;
    }
  }
  return valid;
}

__device__ __forceinline__ uint32_t topk_peek(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// true in every lane of the block that takes the last ticket; the other
// blocks' global adds are then visible to it
__device__ __forceinline__ bool topk_last_block(uint32_t* ticket, uint32_t* s_flag) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) *s_flag = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  const bool last = *s_flag != 0;
  if (last) __threadfence();
  return last;
}

__global__ __launch_bounds__(kBlock) void k_topk_clear(uint32_t* ws, uint32_t k) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < kTopkWsCountsOff) ws[i] = i == kTopkWsStateOff + 1 ? k : 0u;
}

template <class Op, int PASS, bool VEC>
__global__ __launch_bounds__(kBlock) void k_topk_hist(const void* __restrict__ x, const void* __restrict__ ref, size_t P,
                                                      unsigned tpb, uint32_t* ws) {
  constexpr int BITS = topk_bits(PASS), SHIFT = topk_shift(PASS), NB = 1 << BITS, HI = SHIFT + BITS;
  constexpr size_t kTile = static_cast<size_t>(kBlock) * Op::E * kTopkVpt;
  __shared__ uint32_t h[NB];
  __shared__ uint32_t part[kBlock];
  __shared__ uint32_t s_flag;
  uint32_t* const st = ws + kTopkWsStateOff;
  uint32_t* const gh = ws + PASS * kTopkBins;
  const int tid = threadIdx.x;
  for (int i = tid; i < NB; i += kBlock) h[i] = 0;
  const uint32_t prefix = st[0];
  __syncthreads();
  for (unsigned t = 0; t < tpb; ++t) {
    const size_t base = (static_cast<size_t>(blockIdx.x) * tpb + t) * kTile;
    if (base >= P) break;
    typename Op::Elem xb[kTopkVpt][Op::E];
    uint32_t key[kTopkVpt][Op::E], valid[kTopkVpt];
#pragma unroll
    for (int r = 0; r < kTopkVpt; ++r)
      valid[r] = topk_load<Op, VEC>(x, ref, base + (static_cast<size_t>(r) * kBlock + tid) * Op::E, P, xb[r], key[r]);
#pragma unroll
    for (int r = 0; r < kTopkVpt; ++r)
#pragma unroll
      for (int e = 0; e < Op::E; ++e)
        if (((valid[r] >> e) & 1u) && (key[r][e] >> HI) == (prefix >> HI))
          atomicAdd(&h[(key[r][e] >> SHIFT) & (NB - 1)], 1u);
  }
  __syncthreads();
  for (int i = tid; i < NB; i += kBlock)
    if (h[i]) atomicAdd(&gh[i], h[i]);
  if (!topk_last_block(&st[2 + PASS], &s_flag)) return;
  // the digit of the `remaining`-th largest key: lane t owns the C bins below NB - t*C, walked downwards
  constexpr int C = NB / kBlock;
  const uint32_t remaining = st[1];
  for (int i = tid; i < NB; i += kBlock) h[i] = topk_peek(&gh[i]);
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) sum += h[NB - 1 - (tid * C + c)];
  part[tid] = sum;
  __syncthreads();
  uint32_t above = 0;
  for (int u = 0; u < tid; ++u) above += part[u];
  if (above < remaining && remaining <= above + sum) {
    for (int c = 0; c < C; ++c) {
      const int bin = NB - 1 - (tid * C + c);
      const uint32_t cnt = h[bin];
      if (remaining <= above + cnt) {
        st[0] = prefix | (static_cast<uint32_t>(bin) << SHIFT);
        st[1] = remaining - above;
        break;
      }
      above += cnt;
    }
  }
}

template <class Op, bool VEC>
__global__ __launch_bounds__(kBlock) void k_topk_count(const void* __restrict__ x, const void* __restrict__ ref, size_t P,
                                                       unsigned tpb, uint32_t* ws, uint32_t* threshold) {
  constexpr size_t kTile = static_cast<size_t>(kBlock) * Op::E * kTopkVpt;
  __shared__ uint32_t s_cnt[2];
  __shared__ uint32_t part[2][kBlock];
  __shared__ uint32_t s_flag;
  uint32_t* const st = ws + kTopkWsStateOff;
  uint32_t* const gt = ws + kTopkWsCountsOff;
  uint32_t* const eq = gt + gridDim.x;
  const int tid = threadIdx.x;
  const uint32_t T = st[0];
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  uint32_t cg = 0, ce = 0;
  for (unsigned t = 0; t < tpb; ++t) {
    const size_t base = (static_cast<size_t>(blockIdx.x) * tpb + t) * kTile;
    if (base >= P) break;
    typename Op::Elem xb[kTopkVpt][Op::E];
    uint32_t key[kTopkVpt][Op::E], valid[kTopkVpt];
#pragma unroll
    for (int r = 0; r < kTopkVpt; ++r)
      valid[r] = topk_load<Op, VEC>(x, ref, base + (static_cast<size_t>(r) * kBlock + tid) * Op::E, P, xb[r], key[r]);
#pragma unroll
    for (int r = 0; r < kTopkVpt; ++r)
#pragma unroll
      for (int e = 0; e < Op::E; ++e)
        if ((valid[r] >> e) & 1u) {
          cg += key[r][e] > T ? 1u : 0u;
          ce += key[r][e] == T ? 1u : 0u;
        }
  }
  if (cg) atomicAdd(&s_cnt[0], cg);
  if (ce) atomicAdd(&s_cnt[1], ce);
  __syncthreads();
  if (tid == 0) {
    gt[blockIdx.x] = s_cnt[0];
    eq[blockIdx.x] = s_cnt[1];
  }
  if (!topk_last_block(&st[5], &s_flag)) return;
  // exclusive prefixes over the blocks, in block order: lane t owns C consecutive blocks
  const unsigned nb = gridDim.x, C = (nb + kBlock - 1) / kBlock;
  if (tid == 0 && threshold) *threshold = T;
  uint32_t* const arr[2] = {gt, eq};
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    uint32_t sum = 0;
    for (unsigned c = 0; c < C; ++c) {
      const unsigned b = tid * C + c;
      if (b < nb) sum += topk_peek(&arr[a][b]);
    }
    part[a][tid] = sum;
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    uint32_t run = 0;
    for (int u = 0; u < tid; ++u) run += part[a][u];
    for (unsigned c = 0; c < C; ++c) {
      const unsigned b = tid * C + c;
      if (b < nb) {
        const uint32_t v = topk_peek(&arr[a][b]);
        arr[a][b] = run;
        run += v;
      }
    }
  }
}

template <class Op, bool VEC>
__global__ __launch_bounds__(kBlock) void k_topk_write(const void* __restrict__ x, void* ref, size_t P, unsigned tpb,
                                                       const uint32_t* ws, uint32_t k, int32_t* __restrict__ idx,
                                                       void* __restrict__ val) {
  using Elem = typename Op::Elem;
  constexpr size_t kTile = static_cast<size_t>(kBlock) * Op::E * kTopkVpt;
  constexpr int kWaves = kBlock / 64;
  __shared__ uint32_t s_w[2][kWaves];
  const uint32_t* const st = ws + kTopkWsStateOff;
  const uint32_t T = st[0], need = st[1];
  const int tid = threadIdx.x, wave = tid >> 6;
  const uint64_t below = (uint64_t{1} << (tid & 63)) - 1;  // the lanes of this wave before this one
  uint32_t gt_run = ws[kTopkWsCountsOff + blockIdx.x], eq_run = ws[kTopkWsCountsOff + gridDim.x + blockIdx.x];
  for (unsigned t = 0; t < tpb; ++t) {
    const size_t base = (static_cast<size_t>(blockIdx.x) * tpb + t) * kTile;
    if (base >= P) break;  // block-uniform: every lane reaches the ballots and barriers below
    for (int r = 0; r < kTopkVpt; ++r) {
      const size_t e0 = base + (static_cast<size_t>(r) * kBlock + tid) * Op::E;
      Elem xb[Op::E];
      uint32_t key[Op::E];
      const uint32_t valid = topk_load<Op, VEC>(x, ref, e0, P, xb, key);
      uint32_t mg = 0, me = 0, lt_g = 0, lt_e = 0, tot_g = 0, tot_e = 0;
#pragma unroll
      for (int e = 0; e < Op::E; ++e) {
        const bool v = (valid >> e) & 1u;
        const bool g = v && key[e] > T, q = v && key[e] == T;
        mg |= g ? 1u << e : 0u;
        me |= q ? 1u << e : 0u;
        const uint64_t bg = __ballot(g), be = __ballot(q);
        lt_g += __popcll(bg & below);
        lt_e += __popcll(be & below);
        tot_g += __popcll(bg);
        tot_e += __popcll(be);
      }
      if ((tid & 63) == 0) {
        s_w[0][wave] = tot_g;
        s_w[1][wave] = tot_e;
      }
      __syncthreads();
      uint32_t g_rank = gt_run + lt_g, e_rank = eq_run + lt_e;
#pragma unroll
      for (int u = 0; u < kWaves; ++u) {
        if (u < wave) {
          g_rank += s_w[0][u];
          e_rank += s_w[1][u];
        }
        gt_run += s_w[0][u];
        eq_run += s_w[1][u];
      }
      // element order is index order: a key above T goes behind every earlier one and the ties taken so far
#pragma unroll
      for (int e = 0; e < Op::E; ++e) {
        const bool g = (mg >> e) & 1u, q = (me >> e) & 1u;
        if (g || (q && e_rank < need)) {
          const uint32_t pos = g_rank + (e_rank < need ? e_rank : need);
          if (pos < k) {
            idx[pos] = static_cast<int32_t>(e0 + e);
            static_cast<Elem*>(val)[pos] = xb[e];
            static_cast<Elem*>(ref)[e0 + e] = xb[e];
          }
        }
        g_rank += g ? 1u : 0u;
        e_rank += q ? 1u : 0u;
      }
      __syncthreads();  // s_w is rewritten by the next row
    }
  }
}

}  // namespace dlsim
