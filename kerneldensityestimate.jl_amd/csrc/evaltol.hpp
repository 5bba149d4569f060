// evaltol.hpp -- the three passes of a tolerance-bounded evaluation (include/kdehip.h section 5m; kernels in evaltol.hip), as
// the entries in evaluate.hip enqueue them in place of the direct sweep: chunk boxes, the plan (one flag per (query block,
// chunk) tile) and the sweep over the flagged chunks.  What follows them is the evaluation's own finish kernel.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace kdehip {

// One item: the density's leaves, the queries in the order they are processed, the direct call's group split.
struct TolPass {
  const double *src, *w, *qry, *bw;  // (device) [N][D] leaf means, [N] weights, [Nq][D] queries, [D] variances
  int64_t N, Nq, chunks_per_group;
  int32_t ngroups, D, loo;
  uint32_t circ;                     // bit k: dimension k is circular
  double norm0, rel_tol, abs_tol;
  double *partial;                   // (device) [ngroups][Nq], written
  unsigned char *scratch;            // (device) tol_scratch_bytes(N, Nq, D) bytes, 8-byte aligned
  int64_t *stats;                    // (device) int64[2] = tiles visited, tiles in all; or null
};

size_t tol_scratch_bytes(int64_t N, int64_t Nq, int D);
// enqueue only: no atomics, no read-back, the sweep's grid is the direct call's.  `marks`: null, or four events that are
// recorded before the first pass and after each of the three (kdehip_profile_phase_read 3..5).
int enqueue_tol_passes(const TolPass &p, hipStream_t st, hipEvent_t *marks = nullptr);

}  // namespace kdehip
