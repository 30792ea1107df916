// partials.hpp — what the host dispatches of the n <= 32 input families share (inst_robust.hip,
// inst_pairdist.hip, inst_pairdist_batch.hip, inst_reducedist.hip, inst_reducedist_batch.hip): the split of a long input into
// launches of 32-bit byte offsets, the distance families' grid cap, partial-sum workspace and finish
// grid, and the grid of one pairwise-distance call (PdGeom) and of one reduce-and-measure call
// (RdGeom), which the flat entry and every segment of a batched launch take from the same pd_geometry
// and rd_geometry. Host code only.
#pragma once

#include "dispatch.hpp"

namespace dlsim_host __attribute__((visibility("hidden"))) {

// Blocks of one distance launch, over all its units: four resident blocks (one wave per SIMD each) on
// each of the 256 CUs of an MI355X. A constant, so that the summation order is the same on every device.
constexpr unsigned kDistGridBlocks = 1024;

// f(first element, elements) -> hipError_t for consecutive ranges of at most kMaxLaunchOutBytes (the
// launch limit of the library's other paths; a multiple of every tile size). Stops at the first error.
template <class F>
hipError_t for_each_range(size_t nelem, size_t elem_bytes, F f) {
  const size_t range = kMaxLaunchOutBytes / elem_bytes;
  for (size_t o = 0; o < nelem; o += range) {
    const hipError_t e = f(o, std::min(range, nelem - o));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// body(ws) -> hipError_t with `doubles` doubles of device memory allocated and freed in stream order
// (as the fan-in table of the reduce): the main launch writes the blocks' partials there, the finish
// launch sums them. The body's error comes before the free's.
template <class Body>
hipError_t with_partials(size_t doubles, hipStream_t st, Body body) {
  void* ws = nullptr;
  hipError_t e = hipMallocAsync(&ws, sizeof(double) * doubles, st);
  if (e != hipSuccess) return e;
  e = body(static_cast<double*>(ws));
  const hipError_t e2 = hipFreeAsync(ws, st);
  return e == hipSuccess ? e2 : e;
}

// The grid of one pairwise-distance call (inst_pairdist.hip defines pd_geometry; a segment of a
// batched launch takes the same one, inst_pairdist_batch.hip).
struct PdGeom {
  int cap;          // rows of a diagonal unit: 4 or 8
  bool cross;       // n > 8: diagonal and cross units in one launch
  unsigned units;   // second grid dimension
  unsigned active;  // units that hold at least one pair
  size_t tile;      // elements a block takes per step
  unsigned blocks;  // first grid dimension
};
// elems16: elements of a 16-byte vector; vec: every base is 16-byte aligned
PdGeom pd_geometry(int n, int elems16, size_t nelem, bool vec);

// The grid of one reduce-and-measure call (inst_reducedist.hip defines rd_geometry; a segment of a
// batched launch takes the same one, inst_reducedist_batch.hip).
struct RdGeom {
  int cap;          // compile-time row capacity: 4, 8, 16 or 32
  size_t tile;      // elements a block takes per step
  unsigned blocks;  // grid
};
// vec: every base is 16-byte aligned
RdGeom rd_geometry(int n, int elem_bytes, size_t nelem, bool vec);

inline unsigned finish_blocks(int items) {  // grid of a finish kernel: one wave per item (a pair, an input)
  return static_cast<unsigned>((items + dlsim::kBlock / 64 - 1) / (dlsim::kBlock / 64));
}

}  // namespace dlsim_host
