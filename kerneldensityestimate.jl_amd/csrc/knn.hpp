// knn.hpp -- the three passes of a k-nearest-neighbour search on the ball tree's leaf order (include/kdehip.h section 5n;
// kernels and entries in knn.hip): chunk boxes, the plan (one flag per (query block, chunk) tile) and the sweep over the
// flagged chunks that keeps every query's k best candidates in registers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "../../include/kdehip.h"

namespace kdehip {

// One search: the density's leaves in leaf order, the queries in the order they are processed.
struct KnnPass {
  const double *src;         // (device) [N][D] leaf centres, leaf order
  const int64_t *src_index;  // (device) [N] the 1-based original index of each leaf
  const double *qry;         // (device) [Nq][D] queries (leave-one-out: src itself)
  const int64_t *qry_index;  // (device) [Nq] the 1-based output column of each query, or null: query q writes column q
  int64_t N, Nq;
  int32_t D, k, loo;         // loo: query q IS leaf q of the density and is left out by that index
  uint32_t circ;             // bit j: dimension j is circular
  double scale[KDEHIP_MAX_DIMS];  // s_j > 0 (1 = Euclidean)
  double *d2_out;            // (device) [Nq][k], written
  int64_t *idx_out;          // (device) [Nq][k], written
  unsigned char *scratch;    // (device) knn_scratch_bytes(N, Nq, D, k) bytes, 8-byte aligned
  int64_t *stats;            // (device) int64[2] = tiles visited, tiles in all; or null
};

size_t knn_scratch_bytes(int64_t N, int64_t Nq, int D, int k);
// enqueue only: no atomics, no read-back.  `marks`: null, or four events that are recorded before the first pass and after
// each of the three (kdehip_profile_phase_read 6..8).
int enqueue_knn_passes(const KnnPass &p, hipStream_t st, hipEvent_t *marks = nullptr);

}  // namespace kdehip
