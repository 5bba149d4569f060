// ksum.hip -- exact overlap measures of two Gaussian-kernel densities by ONE primitive (include/kdehip.h section 5g; no
// reference counterpart: intersIntgAppxIS, src/DualTree01.jl:581-618, approximates the first of them on a grid in 1-D and 2-D):
//   S(A, B; v) = sum_{j<M} b_j sum_{i<N} a_i exp(-1/2 sum_k diff_k(y_jk, x_ik)^2 / v_k)
// with A = (x_i, a_i), B = (y_j, b_j) the leaf points and leaf weights of two densities, v a variance vector (explicit, or
// the sum of the two densities' leaf variances) and diff_k the plain difference, or circ_wrap of it in a circular dimension.
// With normalize, S / ((2 pi)^(D/2) prod_k sqrt(v_k)):
//   integral p q     = S(p, q; v_p + v_q) normalised           (intersIntg)
//   integral (p-q)^2 = the three such integrals                (ise)
//   MMD^2(p, q; h)   = S(p,p;h^2) - 2 S(p,q;h^2) + S(q,q;h^2)  (mmd)
// Host densities (uploaded for the call, blocking) and resident ones (single and blocking, or batched and enqueue-only) run
// ONE path, any number of items described in device memory by KsumItem:
//   ksum_partial_kernel<D>  one launch per distinct D (one more for its items with a circular dimension): the all-pairs sum
//                           of pair_sweep.hpp, the one evaluate.hip runs -- one lane per point of B, A the sources --, then
//                           b_j times the lane's sum reduced over the block in a fixed LDS tree: ONE double per block, no
//                           per-query scratch, no atomics;
//   ksum_reduce_kernel      one thread per item: the block shares in block order, times the scale.
// The full square is summed: no leave-one-out, no triangular shortcut for A == B.  The group split (split_chunks(N, M, 1))
// depends on the pair's sizes alone, so the host entry, a single device call and any batch give the same bits, and S(p, p)
// is S(p, an equal copy of p).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "density_args.hpp"
#include "device_density.hpp"
#include "entry_helpers.hpp"
#include "manifold_arg.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"
#include "pair_sweep.hpp"

using namespace kdehip;

namespace {

// (this unit's own words: not density_args.hpp's kOneBandwidth)
const char kNeedVariances[] = "per-point bandwidths need explicit variances (the sum of the leaf variances is one vector)";

// One sum: the N leaves of A (the head's sources) against the M = Nq leaves of B (its queries).
struct KsumItem : PairHead {
  const double *qw;    // [M] B's leaf weights
  const double *va;    // [D] the variances v, or A's first leaf's when vb is set
  const double *vb;    // null, or [D] B's first leaf's variances: v_k = va[k] + vb[k]
  double *bpart;       // [ngroups * qblocks] the blocks' shares
  double *out;         // the result
  double norm0;        // (2 pi)^(D/2) as the host's libm rounds it
  int32_t ngroups, D, normalize, pad_;
};

__device__ __forceinline__ double ksum_var(const KsumItem &it, int k) { return it.vb ? it.va[k] + it.vb[k] : it.va[k]; }

// bpart[grp * qblocks + qb] = sum over the lanes j of query block qb, in a fixed tree, of
//   b_j * (sum over the source chunks c of group grp, in chunk order, of sum_{i in chunk c} a_i exp(-1/2 sum_k d_k^2 / v_k))
// for the items [0, n) of one D, by the sweep of pair_sweep.hpp with the plain sum as its step.  Every lane walks to the
// block reduction, whatever its group holds; a lane at or beyond M contributes exactly 0.
// CIRC: bit k of masks[i] makes dimension k of item i circular; data in which no difference wraps gives the bits of the
// Euclidean instantiation.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void ksum_partial_kernel(const KsumItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n,
                                                                    const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  __shared__ double red[kEvalThreads];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);  // ib.k < ngroups * qblocks: the item's blocks are exactly its shares
  const KsumItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  double nhib[D];  // -1/(2 v_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / ksum_var(pb, k);
  const double bq = (at.q < pb.Nq) ? pb.qw[at.q] : 0.0;
  double total = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double sum = 0.0;
    each([&](int64_t, double w, double a) { sum += w * exp_nonpos(a, sExpTab); });
    total += sum;
  });
  red[threadIdx.x] = (at.q < pb.Nq) ? total * bq : 0.0;
  __syncthreads();
  const double share = block_tree_sum<kEvalThreads>(red);
  if (threadIdx.x == 0) pb.bpart[ib.k] = share;
}

// one thread per item: the block shares in block order, times the scale -- 1, or with normalize
// 1 / ((2 pi)^(D/2) prod_k sqrt(v_k)) (gauss_norm, as the evaluation forms its norm).  Formed HERE for every route.
__global__ void ksum_reduce_kernel(const KsumItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const KsumItem it = items[i];
  const int64_t nb = ((it.Nq + kEvalThreads - 1) / kEvalThreads) * it.ngroups;
  double s = 0.0;
  int64_t b = 0;
  for (; b + 16 <= nb; b += 16) {  // sixteen loads in flight, added in block order: the bits of the plain loop
    double t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = it.bpart[b + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += t[u];
  }
  for (; b < nb; ++b) s += it.bpart[b];
  double scale = 1.0;
  if (it.normalize) scale = 1.0 / gauss_norm(it.norm0, it.D, [&](int k) { return ksum_var(it, k); });
  *it.out = s * scale;
}

// The run of one call (pair_sweep.hpp PairRun) with the sum's own pieces: the explicit variances in front of the results,
// per item its block shares behind them.  Protocol: fill `items` (sizes, D, normalize), `circ` and `var` -> alloc(prefix
// bytes of caller data) -> point the items at their data (and at result(k), or at the caller's output) -> enqueue(stream) ->
// wait() or defer(device).
class KsumRun : public PairRun<KsumItem> {
 public:
  std::vector<const double *> var;   // per item: the caller's D explicit variances (host), or null: the leaf variances
  int alloc(size_t prefix) {
    const size_t n = items.size();
    int64_t blocks = 0;
    for (KsumItem &it : items) blocks += split(it);
    if (blocks > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "kernel sum too large for one launch");
    Carve c;
    const size_t o_var = carve_head(c, prefix, 1, sizeof(double) * KDEHIP_MAX_DIMS * n, n);
    std::vector<size_t> shares(n);
    for (size_t k = 0; k < n; ++k) shares[k] = c.take(sizeof(double) * sweep_blocks(items[k]));
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) {
      KsumItem &it = items[k];
      it.bpart = reinterpret_cast<double *>(dev() + shares[k]);
      if (!var[k]) continue;
      std::memcpy(host() + o_var + sizeof(double) * KDEHIP_MAX_DIMS * k, var[k], sizeof(double) * it.D);
      it.va = reinterpret_cast<const double *>(dev() + o_var) + KDEHIP_MAX_DIMS * k;
      it.vb = nullptr;
    }
    return KDEHIP_OK;
  }
  // descriptors sorted (by D; Euclidean items before circular ones), one upload, one launch per run of equal (D, circular),
  // one reduce
  int enqueue(hipStream_t st) {
    prepare([&](size_t k) { return 2 * items[k].D + (circ[k] ? 1 : 0); });
    KDEHIP_CHECK(send(st));
    KDEHIP_CHECK_RC(for_each_run([&](const KsumItem &it, const KsumItem *d_it, const int32_t *d_f, int cnt, int blocks,
                                     const uint32_t *d_masks) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<KsumItem>(ksum_partial_kernel<kD, false>, ksum_partial_kernel<kD, true>, blocks, st, d_it, d_f, cnt, d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    hipLaunchKernelGGL(ksum_reduce_kernel, dim3(static_cast<unsigned>((items.size() + 63) / 64)), dim3(64), 0, st, d_items(),
                       static_cast<int>(items.size()));
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
};

// explicit variances: D of them, each finite and > 0
int check_var(const double *var, int64_t D) {
  for (int64_t k = 0; var && k < D; ++k)
    if (!(std::isfinite(var[k]) && var[k] > 0.0)) return set_error(KDEHIP_ERR_ARG, "kernel sum: every variance must be finite and > 0");
  return KDEHIP_OK;
}

// the checks every resident entry makes on one item; none touches a device
int check_resident(const kdehip_device_density *a, const kdehip_device_density *b, const double *var, uint32_t mask) {
  if (!a || !b) return set_error(KDEHIP_ERR_ARG, "null density");
  if (a->D > KDEHIP_MAX_DIMS || b->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (a->D < 1 || b->D < 1) return set_error(KDEHIP_ERR_ARG, "density with no dimensions");
  if (a->D != b->D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "kernel sum -- dimensions of two BallTreeDensities must match");
  if (a->device != b->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  if (!var && !(leaves_share_bandwidth(a) && leaves_share_bandwidth(b)))
    return set_error(KDEHIP_ERR_UNSUPPORTED, kNeedVariances);
  KDEHIP_CHECK_RC(check_var(var, a->D));
  if (mask >> a->D) return set_error(KDEHIP_ERR_ARG, "kernel sum: circular_mask names a dimension the densities do not have");
  return KDEHIP_OK;
}

KsumItem resident_item(const kdehip_device_density *a, const kdehip_device_density *b, int normalize) {
  const LeafRows la = leaf_rows(a), lb = leaf_rows(b);
  KsumItem it{};
  it.src = la.src; it.w = la.w; it.va = la.bw;
  it.qry = lb.src; it.qw = lb.w; it.vb = lb.bw;
  it.norm0 = gauss_norm0(a->D);
  it.N = a->N; it.Nq = b->N; it.D = a->D; it.normalize = normalize ? 1 : 0;
  return it;
}

// a host density as the sum reads it: leaves, weights and (without explicit variances) ONE bandwidth vector
int check_host(const kdehip_density *p, bool need_bw) {
  if (p->npts < 1 || !p->means || !p->weights || (need_bw && !p->bandwidth)) return set_error(KDEHIP_ERR_ARG, "malformed density");
  return need_bw ? check_one_bandwidth(p, kNeedVariances) : KDEHIP_OK;
}

}  // namespace

extern "C" int kdehip_kernel_sum_device_batch(int n, const kdehip_ksum_item *items, double *d_out, void *stream) {
  if (n < 0 || (n > 0 && (!items || !d_out))) return set_error(KDEHIP_ERR_ARG, "kernel sum batch: bad item list");
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    KDEHIP_CHECK_RC(check_resident(items[i].a, items[i].b, items[i].var, items[i].circular_mask));
    if (items[i].a->device != items[0].a->device) return set_error(KDEHIP_ERR_ARG, "kernel sum batch: densities on different devices");
  }
  const int device = items[0].a->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  KsumRun run;
  for (int i = 0; i < n; ++i) {
    run.items.push_back(resident_item(items[i].a, items[i].b, items[i].normalize));
    run.items.back().out = d_out + i;
    run.circ.push_back(items[i].circular_mask);
    run.var.push_back(items[i].var);
  }
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return finish_enqueue(run, nullptr, device);
}

extern "C" int kdehip_kernel_sum_device(const kdehip_device_density *a, const kdehip_device_density *b, const double *var,
                                        int normalize, double *out, const uint8_t *manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident(a, b, var, 0u));
  uint32_t circ = 0;
  if (manifold_arg(manifold, a->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(a->device));
  KsumRun run;
  run.items.push_back(resident_item(a, b, normalize));
  run.circ.push_back(circ);
  run.var.push_back(var);
  KDEHIP_CHECK_RC(run.alloc(0));
  run.items[0].out = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}

extern "C" int kdehip_kernel_sum(const kdehip_density *a, const kdehip_density *b, const double *var, int normalize,
                                 double *out, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!a || !b || !out) return set_error(KDEHIP_ERR_ARG, "null argument");
  const int64_t D = a->ndim, N = a->npts, M = b->npts;
  if (D > KDEHIP_MAX_DIMS || b->ndim > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (D < 1 || b->ndim < 1) return set_error(KDEHIP_ERR_ARG, "density with no dimensions");
  if (b->ndim != D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "kernel sum -- dimensions of two BallTreeDensities must match");
  KDEHIP_CHECK_RC(check_host(a, !var));
  if (b != a) KDEHIP_CHECK_RC(check_host(b, !var));
  KDEHIP_CHECK_RC(check_var(var, D));
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const bool self = a == b;
  // caller data: [a leaf means | a leaf weights | b leaf means | b leaf weights (a == b: neither) | a's, b's first-leaf
  // variances (explicit variances: neither)]
  const size_t o_q = sizeof(double) * N * (D + 1), o_va = o_q + (self ? 0 : sizeof(double) * M * (D + 1));
  const size_t o_vb = o_va + (var ? 0 : sizeof(double) * D), prefix = o_vb + (var ? 0 : sizeof(double) * D);
  KsumRun run;
  KsumItem it{};
  it.norm0 = gauss_norm0(static_cast<int>(D));
  it.N = N; it.Nq = M; it.D = static_cast<int32_t>(D); it.normalize = normalize ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  run.var.push_back(var);
  KDEHIP_CHECK_RC(run.alloc(prefix));
  unsigned char *h = run.host(), *d = run.dev();
  const LeafArrays src = pack_leaves(run, 0, a), qry = self ? src : pack_leaves(run, o_q, b);
  KsumItem &ri = run.items[0];
  ri.src = src.means;
  ri.w = src.weights;
  ri.qry = qry.means;
  ri.qw = qry.weights;
  if (!var) {
    std::memcpy(h + o_va, a->bandwidth + N * D, sizeof(double) * D);
    std::memcpy(h + o_vb, b->bandwidth + M * D, sizeof(double) * D);
    ri.va = reinterpret_cast<const double *>(d + o_va);
    ri.vb = reinterpret_cast<const double *>(d + o_vb);
  }
  ri.out = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}
