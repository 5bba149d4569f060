// density_args.hpp -- what the entry points on top of PairRun (pair_sweep.hpp) do with a density argument, written ONCE:
// the checks of a host density, of a resident one and of a resident pair, the small checks of a batch's list and items, the
// leaf rows of a resident density, the image [means | weights | bandwidth] of a host density in a call's block, and the
// ending of an enqueue-only call.  Host code only; included by evaluate, varbw, ksum, modes, conditional and mass.
// None of the checks touches a device: an entry makes them all before DeviceGuard::enter.
#pragma once
#include <cmath>
#include <cstring>
#include <string>

#include "device_density.hpp"
#include "pair_sweep.hpp"

namespace kdehip {

// what an entry that reads ONE bandwidth vector says to a density with per-point bandwidths
constexpr char kOneBandwidth[] = "per-point bandwidths are not supported (the reference's kde! never builds them)";

// ---- checks ---------------------------------------------------------------------------------------------------------------

// a host density: there, 1..KDEHIP_MAX_DIMS dimensions, its arrays in place
inline int check_host_density(const kdehip_density *bd) {
  if (!bd) return set_error(KDEHIP_ERR_ARG, "null argument");
  if (bd->ndim < 1 || bd->ndim > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (bd->npts < 1 || !bd->means || !bd->bandwidth || !bd->weights || !bd->permutation)
    return set_error(KDEHIP_ERR_ARG, "malformed density");
  return KDEHIP_OK;
}

// Every leaf of a host density has its first leaf's bandwidth -- the sums read ONE vector (bandwidthMin[1..D],
// BallTreeDensity01.jl:98); otherwise KDEHIP_ERR_UNSUPPORTED in the caller's words.
inline int check_one_bandwidth(const kdehip_density *p, const char *words) {
  const int64_t N = p->npts, D = p->ndim;
  const double *bw = p->bandwidth + N * D;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t k = 0; k < D; ++k)
      if (p->bandwidth[(N + i) * D + k] != bw[k]) return set_error(KDEHIP_ERR_UNSUPPORTED, words);
  return KDEHIP_OK;
}

// a resident density; one_bandwidth: its leaves share ONE bandwidth vector (an entry with checks of another code between
// the two asks for false and tests leaves_share_bandwidth where it always has)
inline int check_resident_density(const kdehip_device_density *bd, bool one_bandwidth) {
  if (!bd) return set_error(KDEHIP_ERR_ARG, "null density");
  if (bd->D < 1 || bd->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (one_bandwidth && !leaves_share_bandwidth(bd)) return set_error(KDEHIP_ERR_UNSUPPORTED, kOneBandwidth);
  return KDEHIP_OK;
}

// bd evaluated at at's points, both resident; `at` may be bd
inline int check_pair(const kdehip_device_density *bd, const kdehip_device_density *at, int loo, bool one_bandwidth) {
  if (!bd || !at) return set_error(KDEHIP_ERR_ARG, "null density");
  if (loo && at != bd) return set_error(KDEHIP_ERR_ARG, "leave_one_out needs at == bd");
  if (bd->D < 1 || bd->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (at->D != bd->D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "evaluate -- dimensions of two BallTreeDensities must match");
  if (at->device != bd->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  if (one_bandwidth && !leaves_share_bandwidth(bd)) return set_error(KDEHIP_ERR_UNSUPPORTED, kOneBandwidth);
  return KDEHIP_OK;
}

// Nq >= 0 queries at p, in the caller's words
inline int check_query_count(const void *p, int64_t Nq, const char *words) {
  if (Nq < 0 || (Nq > 0 && !p)) return set_error(KDEHIP_ERR_ARG, words);
  return KDEHIP_OK;
}

inline int check_circular_mask(uint32_t circ, int D, const char *prefix) {
  if (circ >> D) return set_error(KDEHIP_ERR_ARG, std::string(prefix) + "circular_mask names a dimension the density does not have");
  return KDEHIP_OK;
}

// the list of a batch, and that item's density lives where the first item's does
inline int check_batch_list(int n, const void *items, const char *prefix) {
  if (n < 0 || (n > 0 && !items)) return set_error(KDEHIP_ERR_ARG, std::string(prefix) + "bad item list");
  return KDEHIP_OK;
}
inline int check_same_device(const kdehip_device_density *bd, const kdehip_device_density *first, const char *prefix) {
  if (bd->device != first->device) return set_error(KDEHIP_ERR_ARG, std::string(prefix) + "densities on different devices");
  return KDEHIP_OK;
}

// ---- a resident density's leaves ----------------------------------------------------------------------------------------------

// (2 pi)^(D/2) as the host's libm rounds it: the first factor of gauss_norm
inline double gauss_norm0(int D) { return std::pow(2.0 * M_PI, D / 2.0); }

// The leaf rows of a density's arrays (leaf centres == the points, tree order): N points, N weights, N x D variances of which
// an entry that reads ONE vector takes the first D, the leaf row of the permutation; ref: the mean of node 1, the root.
struct LeafRows {
  const double *src, *w, *bw, *ref;
  const int64_t *perm;
};
inline LeafRows leaf_rows(const kdehip_device_density *bd) {
  const int64_t N = bd->N;
  const int D = bd->D;
  return {bd->means + N * D, bd->weights + N, bd->bandwidth + N * D, bd->means, bd->perm + N};
}

// ---- a host density in a call's image ---------------------------------------------------------------------------------------

// A host density's leaf means and, right behind them, its leaf weights copied to offset `at` of the call's pinned image: the
// device pointers to both.
struct LeafArrays { const double *means, *weights; };
template <typename Run>
LeafArrays pack_leaves(const Run &run, size_t at, const kdehip_density *p) {
  const int64_t N = p->npts, D = p->ndim;
  const size_t o_w = at + sizeof(double) * N * D;
  std::memcpy(run.host() + at, p->means + N * D, sizeof(double) * N * D);
  std::memcpy(run.host() + o_w, p->weights + N, sizeof(double) * N);
  return {reinterpret_cast<const double *>(run.dev() + at), reinterpret_cast<const double *>(run.dev() + o_w)};
}

// A host density at offset 0 of the call's image, [means | weights | bw]: bw the first leaf's D variances, or with per_point
// every leaf's (N x D).  What an entry adds -- queries, the leaf row of the permutation -- starts at host_density_bytes.
inline size_t host_density_bytes(const kdehip_density *bd, bool per_point = false) {
  const int64_t N = bd->npts, D = bd->ndim;
  return sizeof(double) * (N * (D + 1) + (per_point ? N * D : D));
}
// head.src and head.w point at the copies; returns the device pointer to bw
template <typename Run>
const double *pack_host_density(const Run &run, PairHead &head, const kdehip_density *bd, bool per_point = false) {
  const int64_t N = bd->npts, D = bd->ndim;
  const LeafArrays src = pack_leaves(run, 0, bd);
  const size_t o_bw = sizeof(double) * N * (D + 1);
  std::memcpy(run.host() + o_bw, bd->bandwidth + N * D, sizeof(double) * (per_point ? N * D : D));
  head.src = src.means;
  head.w = src.weights;
  return reinterpret_cast<const double *>(run.dev() + o_bw);
}

// ---- the ending of an enqueue-only call ---------------------------------------------------------------------------------------

// The call's blocks go back once the work on the stream is done -- or, when the entry has opened a CaptureScope and the
// stream is being captured, stay until kdehip_clear_cache.  scope == nullptr: an entry that is not capture-aware.
template <typename Run>
int finish_enqueue(Run &run, const CaptureScope *scope, int device) {
  return scope && scope->capturing() ? run.keep(device) : run.defer(device);
}

}  // namespace kdehip
