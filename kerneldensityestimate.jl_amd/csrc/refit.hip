// refit.hip -- changeWeights! / movePoints! of a RESIDENT density (reference src/BallTreeDensity01.jl:278-309; include/kdehip.h
// section 5r): every leaf takes a new weight and / or moves, the statistics of the internal nodes are recomputed from their
// children, the tree is not re-formed.  Nothing but a few hundred bytes per item leaves HBM (plus, for a density the library
// built, the arrays kdehip_density_download hands out).
//
// The passes of one call, each ONE launch for all items of a batch, all on the calling thread's stream:
//   copy     the source's block (means, variances, weights, permutation, frontier ids) into the result's
//   max      KDEHIP_REFIT_LOGL: per 128-leaf chunk, the largest log-likelihood among the leaves of positive weight
//   sum      ...: per chunk, sum w_i exp(l_i - m), a fixed pairwise tree; fold: the chunks in chunk order -> S
//   leaf     the new leaf values (weights as given, or w_i exp(l_i - m) / S; mean + delta, wrapped where circular), their
//            checks, and per chunk sum w'^2; fold: -> 1 / ess, the checks' flags
//   node     the formula of balltree.cpp summarize / treebuild.hip, one node per lane: one launch per height while some item's
//            height is wider than a workgroup, then the top of every tree in one workgroup per item, a barrier per height
//   facts    what the sampler's packers know about the VALUES (Frontiers.uniform, uratio, bad, lo, hi): partial results per
//            (level, 4096 frontier nodes), folded on the host -- minima, maxima and flags, so the split cannot change them
// No atomics; no fused multiply-add in the node formula (-ffp-contract=off, and none is spelled).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/kdehip.h"
#include "call_block.hpp"
#include "circ_wrap.hpp"
#include "device_density.hpp"
#include "entry_helpers.hpp"
#include "kdehip_internal.hpp"
#include "manifold_arg.hpp"
#include "phase_timer.hpp"

namespace kdehip {

RefitTable::~RefitTable() {
  if (!d_tab) return;
  DeviceGuard guard;
  if (guard.enter(device) == KDEHIP_OK) cached_free(d_tab, bytes);
}

namespace {

constexpr int kChunk = 128;         // leaves per chunk of the Bayes sums (and per block of the leaf pass)
constexpr int kNodeThreads = 256;   // nodes per block of a height; a height at most this wide belongs to the top kernel
constexpr int kCopyWords = 4096;    // 32-bit words per block of the copy
constexpr int kFactNodes = 4096;    // frontier nodes per block of the examination
constexpr int kFactDoubles = 2 + 4 * KDEHIP_MAX_DIMS;  // [uniform, bad, lo[8], hi[8], amax[8], bw0[8]]
constexpr int kScal = 8;            // per item: [m, S, sum w'^2, flags, -, -, -, -]
constexpr int kPart = 4;            // per chunk: [max, sum, sum w'^2, flags]
// the checks' flags (kept as small integers in doubles)
constexpr int kBadLogl = 1, kHasPositive = 2, kBadWeight = 4, kBadDelta = 8, kBadPerm = 16;

struct RefitJob {
  const double *src_means, *src_bw, *src_w;
  const int64_t *src_perm;
  const int32_t *src_front;
  double *means, *bw, *w, *centers, *ranges;  // the result's (centers / ranges: null unless it keeps the twelve arrays)
  const double *values, *delta;
  const int32_t *nodes, *lc, *rc;             // the source's RefitTable
  const int32_t *hoff;                        // H + 1 entries
  double *scal, *part;
  int64_t N;
  int32_t D, kind, leaf_order, nchunks, H, h_top;
  uint32_t circ;
  int32_t pad_;
};
struct CopySeg { uint32_t *dst; const uint32_t *src; int64_t words; };
struct FactJob { int32_t item, level_begin, begin, count; };

__global__ __launch_bounds__(256) void copy_kernel(const CopySeg *__restrict__ segs, const int32_t *__restrict__ first, int nseg) {
  const int s = item_of_block(first, nseg, blockIdx.x);
  const CopySeg g = segs[s];
  const int64_t base = static_cast<int64_t>(blockIdx.x - first[s]) * kCopyWords;
  for (int64_t t = base + threadIdx.x; t < base + kCopyWords && t < g.words; t += 256) g.dst[t] = g.src[t];
}

// original index of leaf position i, or -1 (an uploaded density's permutation is the caller's)
__device__ __forceinline__ int64_t value_index(const RefitJob &J, int64_t i) {
  if (J.leaf_order) return i;
  const int64_t o = J.src_perm[J.N + i] - 1;
  return (o >= 0 && o < J.N) ? o : -1;
}

__global__ __launch_bounds__(kChunk) void bayes_max_kernel(const RefitJob *__restrict__ jobs, const int32_t *__restrict__ first, int n) {
  __shared__ double s_max[kChunk];
  __shared__ int s_flag[kChunk];
  const int it = item_of_block(first, n, blockIdx.x);
  const RefitJob &J = jobs[it];
  const int c = blockIdx.x - first[it], t = threadIdx.x;
  const int64_t i = static_cast<int64_t>(c) * kChunk + t;
  double mx = -INFINITY;
  int fl = 0;
  if (i < J.N) {
    const int64_t o = value_index(J, i);
    if (o < 0) fl |= kBadPerm;
    else {
      const double l = J.values[o], w = J.src_w[J.N + i];
      if (!(l < INFINITY)) fl |= kBadLogl;  // NaN or +Inf
      if (w > 0.0) { fl |= kHasPositive; mx = l; }
    }
  }
  s_max[t] = mx;
  s_flag[t] = fl;
  __syncthreads();
  for (int s = kChunk / 2; s >= 1; s >>= 1) {
    if (t < s) {
      const double a = s_max[t], b = s_max[t + s];
      s_max[t] = (b > a) ? b : a;
      s_flag[t] |= s_flag[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    J.part[static_cast<int64_t>(c) * kPart + 0] = s_max[0];
    J.part[static_cast<int64_t>(c) * kPart + 3] = static_cast<double>(s_flag[0]);
  }
}

// max over the chunk maxima (any order: a maximum), by the whole block
__device__ __forceinline__ double chunk_max(const RefitJob &J, double *s_red) {
  const int t = threadIdx.x, nt = blockDim.x;
  double mx = -INFINITY;
  for (int c = t; c < J.nchunks; c += nt) {
    const double v = J.part[static_cast<int64_t>(c) * kPart + 0];
    mx = (v > mx) ? v : mx;
  }
  s_red[t] = mx;
  __syncthreads();
  for (int s = nt / 2; s >= 1; s >>= 1) {
    if (t < s) { const double a = s_red[t], b = s_red[t + s]; s_red[t] = (b > a) ? b : a; }
    __syncthreads();
  }
  const double m = s_red[0];
  __syncthreads();
  return m;
}

// the term of leaf i in S: w_i exp(l_i - m), exactly 0 for a leaf without weight
__device__ __forceinline__ double bayes_term(double w, double l, double m) { return (w > 0.0) ? w * exp(l - m) : 0.0; }

// the 128 terms of a chunk in the fixed pairwise tree (strides 64, 32, .., 1)
__device__ __forceinline__ double chunk_tree_sum(double v, double *s_red) {
  const int t = threadIdx.x;
  s_red[t] = v;
  __syncthreads();
  for (int s = kChunk / 2; s >= 1; s >>= 1) {
    if (t < s) s_red[t] = s_red[t] + s_red[t + s];
    __syncthreads();
  }
  const double r = s_red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kChunk) void bayes_sum_kernel(const RefitJob *__restrict__ jobs, const int32_t *__restrict__ first, int n) {
  __shared__ double s_red[kChunk];
  const int it = item_of_block(first, n, blockIdx.x);
  const RefitJob &J = jobs[it];
  const int c = blockIdx.x - first[it], t = threadIdx.x;
  const double m = chunk_max(J, s_red);
  const int64_t i = static_cast<int64_t>(c) * kChunk + t;
  double term = 0.0;
  if (i < J.N) {
    const int64_t o = value_index(J, i);
    if (o >= 0) term = bayes_term(J.src_w[J.N + i], J.values[o], m);
  }
  const double sum = chunk_tree_sum(term, s_red);
  if (t == 0) J.part[static_cast<int64_t>(c) * kPart + 1] = sum;
}

// One block per item: column `col` of the chunks' partial results summed in CHUNK ORDER (staged through LDS, added by one
// lane) into scal[dst], the chunks' flags or-ed into scal[3]; with_max: the maximum into scal[0] first.
__global__ __launch_bounds__(256) void fold_kernel(const RefitJob *__restrict__ jobs, const int32_t *__restrict__ which, int col,
                                                   int dst, int with_max) {
  __shared__ double s_red[256];
  __shared__ double s_tile[1024];
  __shared__ int s_flag[256];
  const RefitJob &J = jobs[which[blockIdx.x]];
  const int t = threadIdx.x;
  if (with_max) {
    const double m = chunk_max(J, s_red);
    if (t == 0) J.scal[0] = m;
  }
  double acc = 0.0;
  int fl = 0;
  for (int c0 = 0; c0 < J.nchunks; c0 += 1024) {
    const int cnt = (J.nchunks - c0 < 1024) ? J.nchunks - c0 : 1024;
    for (int c = t; c < cnt; c += 256) {
      s_tile[c] = J.part[static_cast<int64_t>(c0 + c) * kPart + col];
      fl |= static_cast<int>(J.part[static_cast<int64_t>(c0 + c) * kPart + 3]);
    }
    __syncthreads();
    if (t == 0)
      for (int c = 0; c < cnt; ++c) acc = acc + s_tile[c];
    __syncthreads();
  }
  s_flag[t] = fl;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) s_flag[t] |= s_flag[t + s];
    __syncthreads();
  }
  if (t == 0) {
    J.scal[dst] = acc;
    J.scal[3] = static_cast<double>(static_cast<int>(J.scal[3]) | s_flag[0]);
  }
}

__global__ __launch_bounds__(kChunk) void leaf_kernel(const RefitJob *__restrict__ jobs, const int32_t *__restrict__ first, int n) {
  __shared__ double s_red[kChunk];
  __shared__ int s_flag[kChunk];
  const int it = item_of_block(first, n, blockIdx.x);
  const RefitJob &J = jobs[it];
  const int c = blockIdx.x - first[it], t = threadIdx.x;
  const int D = J.D;
  const int64_t N = J.N, i = static_cast<int64_t>(c) * kChunk + t;
  double sq = 0.0;
  int fl = 0;
  if (i < N) {
    const int64_t o = value_index(J, i);
    double w = J.src_w[N + i];
    if (o < 0) fl |= kBadPerm;
    else if (J.kind == KDEHIP_REFIT_WEIGHTS) {
      w = J.values[o];
      if (!(w >= 0.0) || !(w < INFINITY)) fl |= kBadWeight;
    } else if (J.kind == KDEHIP_REFIT_LOGL) {
      w = bayes_term(w, J.values[o], J.scal[0]) / J.scal[1];
    }
    J.w[N + i] = w;
    sq = w * w;
    for (int k = 0; k < D; ++k) {
      double x = J.src_means[(N + i) * D + k];
      if (J.delta && o >= 0) {
        const double d = J.delta[o * D + k];
        if (!(fabs(d) < INFINITY)) fl |= kBadDelta;
        x = x + d;
        if ((J.circ >> k) & 1u) x = circ_wrap(x);  // addop
        J.means[(N + i) * D + k] = x;
      }
      if (J.centers) {  // a leaf's centre is its mean, its half-span 0 (buildTree!, BallTree01.jl:419-429)
        J.centers[(N + i) * D + k] = x;
        J.ranges[(N + i) * D + k] = 0.0;
      }
    }
  }
  s_flag[t] = fl;
  const double sum = chunk_tree_sum(sq, s_red);  // (its first barrier publishes s_flag too)
  for (int s = kChunk / 2; s >= 1; s >>= 1) {
    if (t < s) s_flag[t] |= s_flag[t + s];
    __syncthreads();
  }
  if (t == 0) {
    J.part[static_cast<int64_t>(c) * kPart + 2] = sum;
    J.part[static_cast<int64_t>(c) * kPart + 3] = static_cast<double>(s_flag[0]);
  }
}

// calcStatsBall! (src/BallTree01.jl:282-336) and calcStatsDensity! (src/BallTreeDensity01.jl:141-187) of internal node `id`
// from its children: the expressions of balltree.cpp summarize, operand for operand.
__device__ __forceinline__ void refit_node(const RefitJob &J, int64_t id, int64_t a, int64_t b) {
  const int D = J.D;
  if (J.centers) {
    for (int k = 0; k < D; ++k) {
      const double ca = J.centers[(a - 1) * D + k], ra = J.ranges[(a - 1) * D + k];
      const double cb = J.centers[(b - 1) * D + k], rb = J.ranges[(b - 1) * D + k];
      if ((J.circ >> k) & 1u) {  // getMiniMaxi / calcStatsBall! through addop / diffop (:249-321)
        const double upA = circ_wrap(ca + ra), upB = circ_wrap(cb + rb), dnA = circ_wrap(ca - ra), dnB = circ_wrap(cb - rb);
        const double top = (upA > upB) ? upA : upB, bottom = (dnA < dnB) ? dnA : dnB;
        const double half = circ_wrap(top - bottom) / 2.0;
        J.ranges[(id - 1) * D + k] = half;
        J.centers[(id - 1) * D + k] = circ_wrap(bottom + half);
        continue;
      }
      const double upA = ca + ra, upB = cb + rb, dnA = ca - ra, dnB = cb - rb;
      const double top = (upA > upB) ? upA : upB, bottom = (dnA < dnB) ? dnA : dnB;
      const double half = (top - bottom) / 2.0;
      J.ranges[(id - 1) * D + k] = half;
      J.centers[(id - 1) * D + k] = bottom + half;
    }
  }
  double wa = J.w[a - 1], wb = J.w[b - 1];
  J.w[id - 1] = (a != b) ? wa + wb : wa;
  const double wt = wa + wb + DBL_EPSILON;  // eps(Float64), BallTreeDensity01.jl:161
  wa /= wt;
  wb /= wt;
  for (int k = 0; k < D; ++k) {
    const double ma = J.means[(a - 1) * D + k], mb = J.means[(b - 1) * D + k];
    const double m = wa * ma + wb * mb;
    J.means[(id - 1) * D + k] = m;
    J.bw[(id - 1) * D + k] = wa * (J.bw[(a - 1) * D + k] + ma * ma) + wb * (J.bw[(b - 1) * D + k] + mb * mb) - m * m;
  }
}

// one height of every item whose height h is wider than a workgroup
__global__ __launch_bounds__(kNodeThreads) void node_kernel(const RefitJob *__restrict__ jobs, const int32_t *__restrict__ first, int n,
                                                             int h) {
  const int it = item_of_block(first, n, blockIdx.x);
  const RefitJob &J = jobs[it];
  const int64_t t = static_cast<int64_t>(J.hoff[h - 1]) + static_cast<int64_t>(blockIdx.x - first[it]) * kNodeThreads + threadIdx.x;
  if (t < J.hoff[h]) refit_node(J, J.nodes[t], J.lc[t], J.rc[t]);
}

// the heights h_top .. H of one item, each at most a workgroup wide
__global__ __launch_bounds__(kNodeThreads) void top_kernel(const RefitJob *__restrict__ jobs) {
  const RefitJob &J = jobs[blockIdx.x];
  for (int h = J.h_top; h <= J.H; ++h) {
    for (int t = J.hoff[h - 1] + threadIdx.x; t < J.hoff[h]; t += kNodeThreads) refit_node(J, J.nodes[t], J.lc[t], J.rc[t]);
    __threadfence_block();
    __syncthreads();
  }
}

template <typename Op>
__device__ __forceinline__ double block_fold(double v, Op op, double *s_w) {
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_xor(v, s, 64);
    v = op(v, o);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = s_w[0];
  for (int q = 1; q < 4; ++q) r = op(r, s_w[q]);
  return r;
}

// examine_frontiers (pack_levels.cpp) on the new values, one block per (level, kFactNodes of its frontier)
__global__ __launch_bounds__(256) void facts_kernel(const RefitJob *__restrict__ jobs, const FactJob *__restrict__ fjobs,
                                                    double *__restrict__ recs) {
  __shared__ double s_w[4];
  const FactJob F = fjobs[blockIdx.x];
  const RefitJob &J = jobs[F.item];
  const int D = J.D;
  const int64_t N = J.N;
  double lo[KDEHIP_MAX_DIMS], hi[KDEHIP_MAX_DIMS], amax[KDEHIP_MAX_DIMS], bw0[KDEHIP_MAX_DIMS];
  int64_t id0 = J.src_front[F.level_begin];
  if (id0 < 1 || id0 > 2 * N) id0 = 1;
#pragma unroll
  for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) {
    lo[d] = INFINITY; hi[d] = 0.0; amax[d] = 0.0;
    bw0[d] = d < D ? J.bw[(id0 - 1) * D + d] : 0.0;
  }
  double uni = 1.0, bad = 0.0;
  for (int z = F.begin + threadIdx.x; z < F.begin + F.count; z += 256) {
    const int64_t id = J.src_front[z];
    if (id < 1 || id > 2 * N) continue;
#pragma unroll
    for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) {
      if (d < D) {
        const double mu = J.means[(id - 1) * D + d], v = J.bw[(id - 1) * D + d], a = fabs(mu);
        if (!(a < 1e100) || !(v > 0.0) || !(v < INFINITY)) bad = 1.0;
        lo[d] = v < lo[d] ? v : lo[d];
        hi[d] = v > hi[d] ? v : hi[d];
        amax[d] = a > amax[d] ? a : amax[d];
        if (v != bw0[d]) uni = 0.0;
      }
    }
    const double w = J.w[id - 1];
    if (!(w >= 0.0) || !(w < INFINITY)) bad = 1.0;
  }
  auto mn = [](double a, double b) { return b < a ? b : a; };
  auto mx = [](double a, double b) { return b > a ? b : a; };
  double *rec = recs + static_cast<int64_t>(blockIdx.x) * kFactDoubles;
  const double r_uni = block_fold(uni, mn, s_w), r_bad = block_fold(bad, mx, s_w);
  if (threadIdx.x == 0) { rec[0] = r_uni; rec[1] = r_bad; }
#pragma unroll
  for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) {
    const double a = block_fold(lo[d], mn, s_w), b = block_fold(hi[d], mx, s_w), c = block_fold(amax[d], mx, s_w);
    if (threadIdx.x == 0) {
      rec[2 + d] = a;
      rec[2 + KDEHIP_MAX_DIMS + d] = b;
      rec[2 + 2 * KDEHIP_MAX_DIMS + d] = c;
      rec[2 + 3 * KDEHIP_MAX_DIMS + d] = bw0[d];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// The table of p's topology, made once (the device is current).
int ensure_table(const kdehip_device_density *p, std::shared_ptr<RefitTable> &out) {
  std::lock_guard<std::mutex> lock(p->refit_mu);
  if (p->refit) { out = p->refit; return KDEHIP_OK; }
  const int64_t N = p->N;
  std::vector<int64_t> kl, kr;
  const int64_t *left = nullptr, *right = nullptr;
  if (p->built && p->m.left && p->m.right) { left = p->m.left; right = p->m.right; }
  else if (p->kids.size() == static_cast<size_t>(2 * N)) {
    kl.assign(p->kids.begin(), p->kids.begin() + N);
    kr.assign(p->kids.begin() + N, p->kids.end());
    left = kl.data(); right = kr.data();
  } else {
    return set_error(KDEHIP_ERR_UNSUPPORTED, "refit: this density has no child arrays");
  }
  const char *no_tree = "refit: the density's child arrays are no tree";
  auto child_ok = [N](int64_t a) { return a >= 1 && a <= 2 * N && a != N; };
  std::vector<int64_t> order;
  if (N == 1) {
    if (left[0] != 2) return set_error(KDEHIP_ERR_ARG, no_tree);
    order.push_back(1);
  } else {
    KDEHIP_CHECK_RC(children_first_order(N, left, right, order));
    if (static_cast<int64_t>(order.size()) != N - 1) return set_error(KDEHIP_ERR_ARG, no_tree);
  }
  const int64_t nI = static_cast<int64_t>(order.size());
  std::vector<int32_t> height(static_cast<size_t>(N) + 1, -1);
  int32_t H = 0;
  for (size_t t = order.size(); t-- > 0;) {  // reverse pre-order: every node after its descendants
    const int64_t id = order[t];
    const int64_t a = left[id - 1], b = (N == 1) ? a : right[id - 1];
    if (!child_ok(a) || !child_ok(b) || height[id] >= 0) return set_error(KDEHIP_ERR_ARG, no_tree);
    const int32_t ha = a > N ? 0 : height[a], hb = b > N ? 0 : height[b];
    if (ha < 0 || hb < 0) return set_error(KDEHIP_ERR_ARG, no_tree);
    height[id] = 1 + (ha > hb ? ha : hb);
    H = height[id] > H ? height[id] : H;
  }
  std::shared_ptr<RefitTable> tab = std::make_shared<RefitTable>();
  tab->device = p->device;
  tab->nI = nI;
  tab->hoff.assign(static_cast<size_t>(H) + 1, 0);
  for (int64_t id : order) tab->hoff[static_cast<size_t>(height[id])]++;
  for (int32_t h = 1; h <= H; ++h) tab->hoff[h] += tab->hoff[h - 1];  // hoff[h] = nodes of height <= h
  std::vector<int64_t> at(tab->hoff.begin(), tab->hoff.end());         // at[h - 1]: the next slot of height h
  const size_t bytes = align256(sizeof(int32_t) * 3 * static_cast<size_t>(nI));
  void *pin = nullptr;
  KDEHIP_CHECK(cached_host_malloc(&pin, bytes));
  int32_t *nodes = static_cast<int32_t *>(pin), *lc = nodes + nI, *rc = lc + nI;
  for (size_t t = order.size(); t-- > 0;) {
    const int64_t id = order[t];
    const int64_t slot = at[static_cast<size_t>(height[id]) - 1]++;
    nodes[slot] = static_cast<int32_t>(id);
    lc[slot] = static_cast<int32_t>(left[id - 1]);
    rc[slot] = static_cast<int32_t>(N == 1 ? left[id - 1] : right[id - 1]);
  }
  hipError_t e = cached_malloc(&tab->d_tab, bytes);
  if (e != hipSuccess) {
    tab->d_tab = nullptr;
    cached_host_free(pin, bytes);
    return set_error(KDEHIP_ERR_HIP, std::string("refit table: ") + hipGetErrorString(e));
  }
  tab->bytes = bytes;
  e = hipMemcpyAsync(tab->d_tab, pin, bytes, hipMemcpyHostToDevice, hipStreamPerThread);
  const hipError_t se = hipStreamSynchronize(hipStreamPerThread);
  cached_host_free(pin, bytes);
  if (e != hipSuccess || se != hipSuccess)
    return set_error(KDEHIP_ERR_HIP, std::string("refit table: ") + hipGetErrorString(e != hipSuccess ? e : se));
  p->refit = tab;
  out = tab;
  return KDEHIP_OK;
}

// The device block of a result: the block of every resident density, [means | bandwidth | weights | permutation | frontier
// ids], and for a result that keeps the twelve arrays [centers | ranges] behind it -- the whole block then comes down into
// the head of the mirror in ONE copy.
struct ResultLayout {
  size_t o_mean = 0, o_bw = 0, o_w = 0, o_perm = 0, o_front = 0, o_ctr = 0, o_rng = 0, total = 0, nd = 0, n2 = 0;
  ResultLayout(int64_t N, int64_t D, size_t nfront, bool boxes) {
    nd = sizeof(double) * 2 * N * D;
    n2 = sizeof(double) * 2 * N;
    Carve c;
    o_mean = c.take(nd); o_bw = c.take(nd); o_w = c.take(n2); o_perm = c.take(sizeof(int64_t) * 2 * N);
    o_front = c.take(sizeof(int32_t) * nfront);
    if (boxes) { o_ctr = c.take(nd); o_rng = c.take(nd); }
    total = c.mark();
  }
};

struct Plan {  // one item of a call
  const kdehip_device_density *p = nullptr;
  std::shared_ptr<RefitTable> tab;
  kdehip_device_density *h = nullptr;
  int nchunks = 0, H = 0, h_top = 1;
  size_t nfront = 0, o_hoff = 0, o_part = 0;
  int fact0 = 0;                 // its first FactJob; level l has fact_of[l] .. fact_of[l + 1]
  std::vector<int> fact_of;
};

void destroy(kdehip_device_density *h) {  // (the device is current; nothing is in flight)
  if (!h) return;
  if (h->d_blob) cached_free(h->d_blob, h->blob_bytes);
  if (h->mirror) cached_host_free(h->mirror, h->mirror_bytes);
  delete h;
}

int refit_impl(int n, const kdehip_refit_item *items, kdehip_device_density **out) {
  const int device = items[0].p->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  hipStream_t st = hipStreamPerThread;
  std::vector<Plan> plans(static_cast<size_t>(n));
  struct Cleanup {
    std::vector<Plan> &plans;
    bool keep = false;
    ~Cleanup() { if (!keep) for (Plan &q : plans) { destroy(q.h); q.h = nullptr; } }
  } cl{plans};

  // ---- tables, result handles, the layout of the call's block ----
  Carve cv;
  const size_t o_jobs = cv.take(sizeof(RefitJob) * n), o_scal = cv.take(sizeof(double) * kScal * n);
  int maxHw = 0, nseg = 0, nfact = 0;
  std::vector<FactJob> fjobs;
  for (int i = 0; i < n; ++i) {
    Plan &q = plans[i];
    const kdehip_device_density *p = q.p = items[i].p;
    KDEHIP_CHECK_RC(ensure_table(p, q.tab));
    const int64_t N = p->N;
    const int L = p->Lown;
    if (p->fr.off.size() != static_cast<size_t>(L) + 2) return set_error(KDEHIP_ERR_ARG, "refit: the density has no frontiers");
    q.nfront = static_cast<size_t>(p->fr.off[static_cast<size_t>(L) + 1]);
    q.nchunks = static_cast<int>((N + kChunk - 1) / kChunk);
    q.H = static_cast<int>(q.tab->hoff.size()) - 1;
    q.h_top = q.H + 1;  // the smallest height from which on every height fits a workgroup
    while (q.h_top > 1 && q.tab->hoff[q.h_top - 1] - q.tab->hoff[q.h_top - 2] <= kNodeThreads) --q.h_top;
    maxHw = (q.h_top - 1 > maxHw) ? q.h_top - 1 : maxHw;
    nseg += 5;
    q.o_hoff = cv.take(sizeof(int32_t) * (q.H + 1));
    q.fact0 = nfact;
    q.fact_of.assign(static_cast<size_t>(L) + 2, 0);
    for (int l = 0; l <= L; ++l) {
      q.fact_of[l] = nfact;
      const int64_t b = p->fr.off[l], e = p->fr.off[l + 1];
      for (int64_t z = b; z < e; z += kFactNodes) {
        fjobs.push_back(FactJob{i, static_cast<int32_t>(b), static_cast<int32_t>(z),
                                static_cast<int32_t>(e - z < kFactNodes ? e - z : kFactNodes)});
        ++nfact;
      }
    }
    q.fact_of[static_cast<size_t>(L) + 1] = nfact;

    kdehip_device_density *h = new (std::nothrow) kdehip_device_density();
    if (!h) return set_error(KDEHIP_ERR_ALLOC, "out of host memory");
    q.h = h;
    h->device = device; h->N = N; h->D = p->D; h->Lown = L;
    const ResultLayout rl(N, p->D, q.nfront, p->built);
    KDEHIP_CHECK(cached_malloc(&h->d_blob, rl.total));
    h->blob_bytes = rl.total;
    if (p->built) {  // the twelve arrays: [image of the device block | bwmin | bwmax | left | right | lowest | highest]
      const size_t nd = static_cast<size_t>(2 * N * p->D), n2 = static_cast<size_t>(2 * N);
      h->mirror_bytes = align256(rl.total + sizeof(double) * nd + sizeof(int64_t) * 4 * n2);
      const hipError_t e = cached_host_malloc(&h->mirror, h->mirror_bytes);
      if (e != hipSuccess) { h->mirror = nullptr; return set_error(KDEHIP_ERR_HIP, std::string("refit mirror: ") + hipGetErrorString(e)); }
    }
  }
  const size_t o_segs = cv.take(sizeof(CopySeg) * nseg), o_first_copy = cv.take(sizeof(int32_t) * (nseg + 1));
  const size_t o_first_logl = cv.take(sizeof(int32_t) * (n + 1)), o_which_logl = cv.take(sizeof(int32_t) * n);
  const size_t o_first_leaf = cv.take(sizeof(int32_t) * (n + 1)), o_which_all = cv.take(sizeof(int32_t) * n);
  const size_t o_first_h = cv.take(sizeof(int32_t) * (n + 1) * (maxHw > 0 ? maxHw : 1));
  const size_t o_fjobs = cv.take(sizeof(FactJob) * (nfact > 0 ? nfact : 1));
  const size_t up_bytes = cv.mark();
  const size_t o_recs = cv.take(sizeof(double) * kFactDoubles * (nfact > 0 ? nfact : 1));
  const size_t host_bytes = cv.mark();
  for (Plan &q : plans) q.o_part = cv.take(sizeof(double) * kPart * q.nchunks);
  CallBlock blk;
  KDEHIP_CHECK(blk.alloc(cv.mark(), host_bytes));
  blk.touch(st);
  unsigned char *hb = blk.host(), *db = blk.dev();
  std::memset(hb, 0, up_bytes);
  RefitJob *jobs = reinterpret_cast<RefitJob *>(hb + o_jobs);
  CopySeg *segs = reinterpret_cast<CopySeg *>(hb + o_segs);
  int32_t *first_copy = reinterpret_cast<int32_t *>(hb + o_first_copy), *first_logl = reinterpret_cast<int32_t *>(hb + o_first_logl);
  int32_t *which_logl = reinterpret_cast<int32_t *>(hb + o_which_logl), *first_leaf = reinterpret_cast<int32_t *>(hb + o_first_leaf);
  int32_t *which_all = reinterpret_cast<int32_t *>(hb + o_which_all), *first_h = reinterpret_cast<int32_t *>(hb + o_first_h);
  if (nfact) std::memcpy(hb + o_fjobs, fjobs.data(), sizeof(FactJob) * nfact);
  int ncopy = 0, nl = 0, nlb = 0, nleaf = 0;
  for (int i = 0; i < n; ++i) {
    Plan &q = plans[i];
    const kdehip_device_density *p = q.p;
    kdehip_device_density *h = q.h;
    const int64_t N = p->N;
    const int D = p->D;
    const ResultLayout rl(N, D, q.nfront, p->built);
    unsigned char *rb = static_cast<unsigned char *>(h->d_blob);
    const RefitTable &tab = *q.tab;
    const int32_t *d_nodes = static_cast<const int32_t *>(tab.d_tab);
    RefitJob &J = jobs[i];
    J.src_means = p->means; J.src_bw = p->bandwidth; J.src_w = p->weights; J.src_perm = p->perm; J.src_front = p->front;
    J.means = reinterpret_cast<double *>(rb + rl.o_mean); J.bw = reinterpret_cast<double *>(rb + rl.o_bw);
    J.w = reinterpret_cast<double *>(rb + rl.o_w);
    J.centers = p->built ? reinterpret_cast<double *>(rb + rl.o_ctr) : nullptr;
    J.ranges = p->built ? reinterpret_cast<double *>(rb + rl.o_rng) : nullptr;
    J.values = items[i].d_values; J.delta = items[i].d_delta;
    J.nodes = d_nodes; J.lc = d_nodes + tab.nI; J.rc = d_nodes + 2 * tab.nI;
    J.hoff = reinterpret_cast<const int32_t *>(db + q.o_hoff);
    J.scal = reinterpret_cast<double *>(db + o_scal) + static_cast<size_t>(i) * kScal;
    J.part = reinterpret_cast<double *>(db + q.o_part);
    J.N = N; J.D = D; J.kind = items[i].kind; J.leaf_order = items[i].leaf_order ? 1 : 0; J.nchunks = q.nchunks;
    J.H = q.H; J.h_top = q.h_top; J.circ = items[i].circular_mask;
    int32_t *hoff = reinterpret_cast<int32_t *>(hb + q.o_hoff);
    for (int t = 0; t <= q.H; ++t) hoff[t] = static_cast<int32_t>(tab.hoff[t]);
    const struct { size_t off; const void *src; size_t bytes; } pieces[5] = {
        {rl.o_mean, p->means, rl.nd}, {rl.o_bw, p->bandwidth, rl.nd}, {rl.o_w, p->weights, rl.n2},
        {rl.o_perm, p->perm, sizeof(int64_t) * 2 * N}, {rl.o_front, p->front, sizeof(int32_t) * q.nfront}};
    for (int s = 0; s < 5; ++s) {
      const int64_t words = static_cast<int64_t>(pieces[s].bytes / 4);
      segs[i * 5 + s] = CopySeg{reinterpret_cast<uint32_t *>(rb + pieces[s].off), static_cast<const uint32_t *>(pieces[s].src), words};
      first_copy[i * 5 + s] = ncopy;
      ncopy += static_cast<int>((words + kCopyWords - 1) / kCopyWords);
    }
    first_logl[i] = nlb;
    if (items[i].kind == KDEHIP_REFIT_LOGL) { which_logl[nl++] = i; nlb += q.nchunks; }
    first_leaf[i] = nleaf;
    nleaf += q.nchunks;
    which_all[i] = i;
  }
  first_copy[nseg] = ncopy; first_logl[n] = nlb; first_leaf[n] = nleaf;
  std::vector<int> nblocks_h(static_cast<size_t>(maxHw) + 1, 0);
  for (int hgt = 1; hgt <= maxHw; ++hgt) {
    int32_t *f = first_h + static_cast<size_t>(hgt - 1) * (n + 1);
    int acc = 0;
    for (int i = 0; i < n; ++i) {
      f[i] = acc;
      const Plan &q = plans[i];
      if (hgt < q.h_top) acc += static_cast<int>((q.tab->hoff[hgt] - q.tab->hoff[hgt - 1] + kNodeThreads - 1) / kNodeThreads);
    }
    f[n] = acc;
    nblocks_h[hgt] = acc;
  }

  // ---- the passes ----
  KDEHIP_CHECK(blk.upload(up_bytes, st));
  PhaseTimer device_time(kPhaseRefit, st);
  const RefitJob *d_jobs = reinterpret_cast<const RefitJob *>(db + o_jobs);
  auto d_i32 = [db](size_t o) { return reinterpret_cast<const int32_t *>(db + o); };
  if (ncopy > 0)
    hipLaunchKernelGGL(copy_kernel, dim3(ncopy), dim3(256), 0, st, reinterpret_cast<const CopySeg *>(db + o_segs), d_i32(o_first_copy), nseg);
  if (nlb > 0) {
    hipLaunchKernelGGL(bayes_max_kernel, dim3(nlb), dim3(kChunk), 0, st, d_jobs, d_i32(o_first_logl), n);
    hipLaunchKernelGGL(bayes_sum_kernel, dim3(nlb), dim3(kChunk), 0, st, d_jobs, d_i32(o_first_logl), n);
    hipLaunchKernelGGL(fold_kernel, dim3(nl), dim3(256), 0, st, d_jobs, d_i32(o_which_logl), 1, 1, 1);
  }
  hipLaunchKernelGGL(leaf_kernel, dim3(nleaf), dim3(kChunk), 0, st, d_jobs, d_i32(o_first_leaf), n);
  hipLaunchKernelGGL(fold_kernel, dim3(n), dim3(256), 0, st, d_jobs, d_i32(o_which_all), 2, 2, 0);
  for (int hgt = 1; hgt <= maxHw; ++hgt)
    if (nblocks_h[hgt] > 0)
      hipLaunchKernelGGL(node_kernel, dim3(nblocks_h[hgt]), dim3(kNodeThreads), 0, st, d_jobs,
                         d_i32(o_first_h + sizeof(int32_t) * static_cast<size_t>(hgt - 1) * (n + 1)), n, hgt);
  hipLaunchKernelGGL(top_kernel, dim3(n), dim3(kNodeThreads), 0, st, d_jobs);
  if (nfact > 0)
    hipLaunchKernelGGL(facts_kernel, dim3(nfact), dim3(256), 0, st, d_jobs, reinterpret_cast<const FactJob *>(db + o_fjobs),
                       reinterpret_cast<double *>(db + o_recs));
  KDEHIP_CHECK(hipGetLastError());
  device_time.stop();
  // ONE readback of the call's results; a result that keeps the twelve arrays fetches its block here as well
  KDEHIP_CHECK(blk.download(o_scal, sizeof(double) * kScal * n, st));
  KDEHIP_CHECK(blk.download(o_recs, sizeof(double) * kFactDoubles * (nfact > 0 ? nfact : 1), st));
  for (Plan &q : plans)
    if (q.h->mirror) KDEHIP_CHECK(hipMemcpyAsync(q.h->mirror, q.h->d_blob, q.h->blob_bytes, hipMemcpyDeviceToHost, st));
  // (under the transfer) what does not change: the topology arrays of the twelve, the frontiers' sizes
  for (Plan &q : plans) {
    const kdehip_device_density *p = q.p;
    kdehip_device_density *h = q.h;
    const int64_t N = p->N;
    const ResultLayout rl(N, p->D, q.nfront, p->built);
    h->fr.off = p->fr.off;
    h->fr.nodes = p->fr.nodes;
    for (int k = 0; k < KDEHIP_MAX_DIMS; ++k) h->bw[k] = p->bw[k];
    h->built = p->built;
    h->refit = q.tab;  // (the same tree)
    if (h->mirror) {
      const size_t nd = static_cast<size_t>(2 * N * p->D), n2 = static_cast<size_t>(2 * N);
      unsigned char *mb = static_cast<unsigned char *>(h->mirror);
      double *bwmin = reinterpret_cast<double *>(mb + rl.total), *bwmax = bwmin + nd / 2;
      int64_t *left = reinterpret_cast<int64_t *>(bwmax + nd / 2), *right = left + n2, *lowest = right + n2, *highest = lowest + n2;
      h->m = {reinterpret_cast<double *>(mb + rl.o_ctr), reinterpret_cast<double *>(mb + rl.o_rng),
              reinterpret_cast<double *>(mb + rl.o_mean), reinterpret_cast<double *>(mb + rl.o_bw), bwmin, bwmax,
              reinterpret_cast<double *>(mb + rl.o_w), left, right, lowest, highest, reinterpret_cast<int64_t *>(mb + rl.o_perm)};
      std::memcpy(bwmin, p->m.bwmin, sizeof(double) * nd / 2);
      std::memcpy(bwmax, p->m.bwmax, sizeof(double) * nd / 2);
      std::memcpy(left, p->m.left, sizeof(int64_t) * n2);
      std::memcpy(right, p->m.right, sizeof(int64_t) * n2);
      std::memcpy(lowest, p->m.lowest, sizeof(int64_t) * n2);
      std::memcpy(highest, p->m.highest, sizeof(int64_t) * n2);
    }
    unsigned char *rb = static_cast<unsigned char *>(h->d_blob);
    h->means = reinterpret_cast<const double *>(rb + rl.o_mean);
    h->bandwidth = reinterpret_cast<const double *>(rb + rl.o_bw);
    h->weights = reinterpret_cast<const double *>(rb + rl.o_w);
    h->perm = reinterpret_cast<const int64_t *>(rb + rl.o_perm);
    h->front = reinterpret_cast<const int32_t *>(rb + rl.o_front);
  }
  KDEHIP_CHECK(blk.wait());
  device_time.collect();
  // slot N is no node: no pass writes its box, the twelve arrays keep the source's.  (A density of ONE point has no such
  // slot: id 1 = N is its root, whose box the top kernel has just recomputed.)
  for (Plan &q : plans)
    if (q.h->mirror && q.p->N > 1) {
      const size_t D = static_cast<size_t>(q.p->D), at = static_cast<size_t>(q.p->N - 1) * D;
      std::memcpy(q.h->m.centers + at, q.p->m.centers + at, sizeof(double) * D);
      std::memcpy(q.h->m.ranges + at, q.p->m.ranges + at, sizeof(double) * D);
    }

  // ---- verdicts, the packers' facts, the host results ----
  const double *scal = reinterpret_cast<const double *>(hb + o_scal), *recs = reinterpret_cast<const double *>(hb + o_recs);
  for (int i = 0; i < n; ++i) {
    const double *sc = scal + static_cast<size_t>(i) * kScal;
    const int fl = static_cast<int>(sc[3]);
    const std::string who = n > 1 ? "refit item " + std::to_string(i) + ": " : "refit: ";
    if (fl & kBadPerm) return set_error(KDEHIP_ERR_ARG, who + "the density's permutation leaves 1..npts");
    if (fl & kBadWeight) return set_error(KDEHIP_ERR_ARG, who + "a weight is negative or not finite");
    if (fl & kBadDelta) return set_error(KDEHIP_ERR_ARG, who + "delta is not finite");
    if (items[i].kind == KDEHIP_REFIT_LOGL) {
      if (fl & kBadLogl) return set_error(KDEHIP_ERR_ARG, who + "a log-likelihood is NaN or +Inf");
      if (!(fl & kHasPositive)) return set_error(KDEHIP_ERR_ARG, who + "no leaf of the density has a positive weight");
      if (!(sc[1] > 0.0) || !(sc[1] < INFINITY))
        return set_error(KDEHIP_ERR_ARG, who + "the evidence sum_i w_i exp(l_i - m) is 0 or not finite (every log-likelihood -Inf?)");
    }
  }
  for (int i = 0; i < n; ++i) {
    Plan &q = plans[i];
    kdehip_device_density *h = q.h;
    const int L = h->Lown, D = h->D;
    Frontiers &fr = h->fr;
    fr.uniform.assign(static_cast<size_t>(L) + 1, 1);
    fr.uratio.assign(static_cast<size_t>(L) + 1, 0.0);
    bool bad = false;
    for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) { fr.lo[d] = INFINITY; fr.hi[d] = 0.0; }
    for (int l = 0; l <= L; ++l) {
      bool uni = true;
      double amax[KDEHIP_MAX_DIMS] = {};
      const double *bw0 = nullptr;
      for (int f = q.fact_of[l]; f < q.fact_of[l + 1]; ++f) {
        const double *r = recs + static_cast<size_t>(f) * kFactDoubles;
        uni = uni && r[0] != 0.0;
        bad = bad || r[1] != 0.0;
        for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) {
          const double lo = r[2 + d], hi = r[2 + KDEHIP_MAX_DIMS + d], am = r[2 + 2 * KDEHIP_MAX_DIMS + d];
          fr.lo[d] = lo < fr.lo[d] ? lo : fr.lo[d];
          fr.hi[d] = hi > fr.hi[d] ? hi : fr.hi[d];
          amax[d] = am > amax[d] ? am : amax[d];
        }
        bw0 = r + 2 + 3 * KDEHIP_MAX_DIMS;
      }
      fr.uniform[l] = uni ? 1 : 0;
      if (uni && bw0) {  // examine_frontiers: the largest |mean_d| over sqrt(2 bandwidth_d), on the host as there
        double ratio = 0.0;
        for (int d = 0; d < D; ++d) {
          const double r = amax[d] / std::sqrt(2.0 * bw0[d]);
          ratio = r > ratio ? r : ratio;
        }
        fr.uratio[l] = ratio;
      }
    }
    fr.bad = bad;
    const double *sc = scal + static_cast<size_t>(i) * kScal;
    if (items[i].kind == KDEHIP_REFIT_LOGL) {
      if (items[i].log_evidence) *items[i].log_evidence = sc[0] + std::log(sc[1]);
      if (items[i].ess) *items[i].ess = 1.0 / sc[2];
    }
  }
  cl.keep = true;
  for (int i = 0; i < n; ++i) out[i] = plans[i].h;
  return KDEHIP_OK;
}

int check_item(const kdehip_refit_item &it) {
  if (!it.p) return set_error(KDEHIP_ERR_ARG, "refit: null density");
  const int64_t N = it.p->N;
  const int D = it.p->D;
  if (N < 1) return set_error(KDEHIP_ERR_ARG, "density with no points");
  if (N > (int64_t(1) << 26))  // (the frontier ids of all levels are counted in 32 bits)
    return set_error(KDEHIP_ERR_UNSUPPORTED, "refit: density too large");
  if (D < 1 || D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (it.kind != KDEHIP_REFIT_KEEP && it.kind != KDEHIP_REFIT_WEIGHTS && it.kind != KDEHIP_REFIT_LOGL)
    return set_error(KDEHIP_ERR_ARG, "refit: kind is KDEHIP_REFIT_KEEP, KDEHIP_REFIT_WEIGHTS or KDEHIP_REFIT_LOGL");
  if (it.kind == KDEHIP_REFIT_KEEP && it.d_values) return set_error(KDEHIP_ERR_ARG, "refit: d_values must be null with KDEHIP_REFIT_KEEP");
  if (it.kind != KDEHIP_REFIT_KEEP && !it.d_values) return set_error(KDEHIP_ERR_ARG, "refit: null d_values");
  if (it.kind == KDEHIP_REFIT_KEEP && !it.d_delta) return set_error(KDEHIP_ERR_ARG, "refit: d_values and d_delta are both null: nothing to do");
  if (D < 32 && (it.circular_mask >> D)) return set_error(KDEHIP_ERR_ARG, "refit: circular_mask has a bit at or above ndims");
  return KDEHIP_OK;
}

}  // namespace
}  // namespace kdehip

using namespace kdehip;

extern "C" int kdehip_density_refit_device_batch(int n, const kdehip_refit_item *items, kdehip_device_density **out) {
  if (n < 0) return set_error(KDEHIP_ERR_ARG, "refit: negative item count");
  if (n == 0) return KDEHIP_OK;
  if (!items || !out) return set_error(KDEHIP_ERR_ARG, "refit: null items or out");
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  for (int i = 0; i < n; ++i) {
    KDEHIP_CHECK_RC(check_item(items[i]));
    if (items[i].p->device != items[0].p->device) return set_error(KDEHIP_ERR_ARG, "refit: the items are on different devices");
  }
  try {
    return refit_impl(n, items, out);
  } catch (const std::exception &e) {
    return set_error(KDEHIP_ERR_ALLOC, std::string("refit: ") + e.what());
  }
}

extern "C" int kdehip_density_refit_device(kdehip_device_density **out, const kdehip_device_density *p, const double *d_values,
                                           int kind, int leaf_order, const double *d_delta, const uint8_t *tree_manifold,
                                           double *log_evidence, double *ess) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null out pointer");
  *out = nullptr;
  if (!p) return set_error(KDEHIP_ERR_ARG, "refit: null density");
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(tree_manifold, p->D, &circ, kTreeManifold));
  const kdehip_refit_item item{p, d_values, d_delta, log_evidence, ess, kind, leaf_order, circ, 0u};
  return kdehip_density_refit_device_batch(1, &item, out);
}
