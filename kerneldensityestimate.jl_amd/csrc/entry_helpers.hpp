// entry_helpers.hpp -- the small things every file of entry points (evaluate, loocv, summary, sample, treebuild,
// pack_device, product) used to define for itself.  Not in kdehip_internal.hpp: that header is part of every sampler
// translation unit and holds declarations only (hip_runtime_api.h); this one has macros and device code.  The blocks of
// a call (device block, pinned image, their release) are call_block.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <type_traits>

#include "kdehip_internal.hpp"

// a HIP call that fails ends the entry point with KDEHIP_ERR_HIP and the call's text
#define KDEHIP_CHECK(expr)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return set_error(KDEHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
// a step that has already set its own message
#define KDEHIP_CHECK_RC(expr)          \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != KDEHIP_OK) return rc_;  \
  } while (0)

namespace kdehip {

// the item that owns global block b: the last i with first[i] <= b (first[] ascending, first[n] = the number of blocks)
__device__ __forceinline__ int item_of_block(const int32_t *__restrict__ first, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// f(std::integral_constant<int, D>) for a run-time D in 1..KDEHIP_MAX_DIMS: the way into a `template <int D>` launcher
template <typename F>
int dispatch_dims(int D, F &&f) {
  static_assert(KDEHIP_MAX_DIMS == 8, "one case per dimension count");
  switch (D) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  }
  return KDEHIP_OK;
}

// Bare device scratch of one call from the library's allocation cache (devmem.cpp).  It goes back when the call returns, so
// the work that uses it must be over by then (a call that may return early with work in flight holds a CallBlock).
struct DevBuf {
  void *p = nullptr;
  size_t n = 0;
  ~DevBuf() { if (p) cached_free(p, n); }
  hipError_t alloc(size_t bytes) { n = bytes ? bytes : 1; return cached_malloc(&p, n); }
  template <typename T> T *as() { return static_cast<T *>(p); }
};

// At most this many partial sums per query in the all-pairs sums of the evaluation and of the bandwidth search
// (scratch = 64 * Nq doubles).
constexpr int kEvalMaxGroups = 64;

// The mapping of the all-pairs sum of evaluate.hip and ksum.hip (the sum itself, written once, is pair_sweep.hpp): a block
// owns kEvalThreads queries and one group of consecutive kEvalChunk-point source chunks.
constexpr int kEvalThreads = 256;  // queries per block
constexpr int kEvalChunk = 128;    // source points per staged chunk

// Source chunks are dealt to groups of consecutive chunks: as many groups as it takes to give every CU a few
// blocks (small problems: one chunk per group, the most parallel split), never more than kEvalMaxGroups.
struct GroupSplit { int64_t chunks_per_group; int ngroups; };
inline GroupSplit split_chunks(int64_t N, int64_t Nq, int nprob) {
  const int64_t nchunks = (N + kEvalChunk - 1) / kEvalChunk;
  const int64_t qblocks = ((Nq + kEvalThreads - 1) / kEvalThreads) * (nprob > 0 ? nprob : 1);
  int64_t want = (int64_t(8) * device_cu_count() + qblocks - 1) / qblocks;  // groups for ~8 blocks per CU
  if (want < 1) want = 1;
  if (want > kEvalMaxGroups) want = kEvalMaxGroups;
  if (want > nchunks) want = nchunks;
  GroupSplit g;
  g.chunks_per_group = (nchunks + want - 1) / want;
  g.ngroups = static_cast<int>((nchunks + g.chunks_per_group - 1) / g.chunks_per_group);
  return g;
}

}  // namespace kdehip
