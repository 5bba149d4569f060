// conditional.hip -- a density conditioned on some of its dimensions (include/kdehip.h section 5i; the library's own: the
// reference has `marginal` and no counterpart of this).  For a density with leaves c_i, weights w_i and ONE bandwidth vector
// v, the given dimensions G (a bit mask), the free ones F and a query y (|G| values),
//   a_i = sum_{k in G} diff(y_k, c_ik)^2 * (-0.5 / v_k),  S = { i : w_i > 0 },  m = max_S a_i,  t_i = w_i exp(a_i - m)
//   logz = m + log sum_S t_i - log norm_G,  omega_i = t_i / sum_S t_j,  mean and variance of x_F under sum_i omega_i N(c_iF, v_F),
//   and ONE draw per query: the leaf by the inverse CDF of omega in leaf order, the point c_iF + sqrt(v_F) n.
// Host densities (uploaded for the call, blocking) and resident ones (single, or batched and enqueue-only) run ONE path, any
// number of items described in device memory by CondItem and driven by CondRun:
//   cond_expand_kernel          a query row becomes D values: y in the given dimensions, the reference point r (the root
//                               node's mean) in the free ones;
//   cond_partial_kernel<D>      one launch per distinct D (one more for its items with a circular dimension): the sweep of
//                               pair_sweep.hpp with nhib = 0 in the free dimensions -- the exponent ignores them, their
//                               differences are r_k - c_ik -- and the step of moments_partial_kernel (modes.hip), carrying
//                               (m, s_0) and, for the items that ask for moments, the first and second moments of the
//                               differences; scratch [2 (+ 2 D)][ngroups][Nq];
//   cond_finish_kernel          the groups combined in group order: M, S_0, logz, mean, var; a drawing item walks the groups
//                               to the first whose running total exceeds u S_0, keeps that group and the residual in the
//                               group's own scale, and marks (query block, group) as chosen;
//   cond_select_kernel<D>       the geometry of the partial sweep; a block nobody chose returns before any barrier; the
//                               others walk their chunks with m = m_g fixed and keep the first leaf of S whose running sum
//                               exceeds the lane's residual (or the group's last leaf of S); the lane forms the point;
//   cond_weights_kernel         one thread per (query, leaf): omega scattered to the ORIGINAL point order.
// No atomics; at most two exp per (query, leaf) pair; the group split (split_chunks(N, Nq, 1)) depends on the item's sizes
// alone, so the host entry, a resident call and any batch give the same bits.
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
#include "philox.hpp"

using namespace kdehip;

namespace {


constexpr int kFinishThreads = kEvalThreads;  // a finish block is a query block: its chosen flags are that block's

// One item: a density (N leaves in leaf order, one bandwidth vector) and Nq queries of ng values each.
struct CondItem : PairHead {
  const double *bw;      // [D] the density's first leaf's variances
  const double *ref;     // [D] the reference point r of the moments: the root node's mean
  const double *given;   // [Nq][ng] the caller's queries
  const int64_t *perm;   // [N] 1-based original position of leaf i
  double *xq;            // [Nq][D] the expanded queries (== qry)
  double *logz;          // [Nq], or null
  double *mean, *var;    // [Nq][nf], or null
  double *pts;           // [Nq][nf] and
  int64_t *ind;          // [Nq] the draw, or both null
  double *wout;          // [Nq][N] omega in original order (the weights entries), or null
  double *partial;       // [2 + 2 D (moments) or 2][ngroups][Nq]: m, s_0, s1_k, s2_k
  double *ms;            // [2][Nq]: M, S_0
  double *resid;         // [Nq] the draw's residual in the chosen group's scale
  int32_t *cgrp;         // [Nq] the chosen group, -1: S is empty
  int32_t *chosen;       // [qblocks][ngroups] some lane of the query block chose the group
  uint64_t seed;
  int64_t offset;
  double norm0;          // (2 pi)^(ng/2)
  uint32_t gmask;
  int32_t ngroups, nfb, D, ng, mom;
};

__device__ __forceinline__ bool is_given(const CondItem &it, int k) { return (it.gmask >> k) & 1u; }

// Items [0, n), item i owns (finish) blocks [first[i], first[i+1]): xq[q] = y in G, r in F
__global__ __launch_bounds__(kFinishThreads) void cond_expand_kernel(const CondItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n) {
  const ItemBlock ib = item_block(first, n);
  const CondItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  if (q >= it.Nq) return;
  int j = 0;
  for (int k = 0; k < it.D; ++k) it.xq[q * it.D + k] = is_given(it, k) ? it.given[q * it.ng + j++] : it.ref[k];
}

// partial[0][g][q] = m, partial[1][g][q] = s_0 and, for an item with moments, partial[2 + k][g][q] = sum t d_k,
// partial[2 + D + k][g][q] = sum t d_k^2 over the source chunks of group g in chunk order, d_k = xq_k - c_ik (the free
// dimensions' are r_k - c_ik; the given dimensions' are carried and not read).  The step is moments_partial_kernel's: per
// staged chunk the maximum of a_i over S, ONE rescale of the carried sums, then t = w_i exp_nonpos(a_i - m).
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void cond_partial_kernel(const CondItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n,
                                                                    const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const CondItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double nhib[D];  // -1/(2 bw_k) in G, 0 in F
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = is_given(pb, k) ? -0.5 / pb.bw[k] : 0.0;
  const int64_t row = static_cast<int64_t>(pb.ngroups) * pb.Nq, o = at.grp * pb.Nq + at.q;
  double m = -INFINITY, s0 = 0.0;
  if (pb.mom) {  // block-uniform
    double s1[D], s2[D];
#pragma unroll
    for (int k = 0; k < D; ++k) s1[k] = s2[k] = 0.0;
    pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
      double cm = -INFINITY;
      each([&](int64_t, double w, double a) { cm = (w > 0.0) ? fmax(cm, a) : cm; });
      if (cm > m) {  // (m == -Inf: the sums are still 0)
        const double r = exp_nonpos(m - cm, sExpTab);
        s0 *= r;
#pragma unroll
        for (int k = 0; k < D; ++k) { s1[k] *= r; s2[k] *= r; }
        m = cm;
      }
      double c0 = 0.0, c1[D], c2[D];
#pragma unroll
      for (int k = 0; k < D; ++k) c1[k] = c2[k] = 0.0;
      each([&](int64_t, double w, double a, const double (&d)[D]) {
        const double t = (w > 0.0) ? w * exp_nonpos(a - m, sExpTab) : 0.0;  // in S: a <= m
        c0 += t;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          c1[k] = fma(d[k], t, c1[k]);
          c2[k] = fma(d[k] * d[k], t, c2[k]);
        }
      });
      s0 += c0;
#pragma unroll
      for (int k = 0; k < D; ++k) { s1[k] += c1[k]; s2[k] += c2[k]; }
    });
    if (at.q < pb.Nq) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        pb.partial[(2 + k) * row + o] = s1[k];
        pb.partial[(2 + D + k) * row + o] = s2[k];
      }
    }
  } else {
    pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
      double cm = -INFINITY;
      each([&](int64_t, double w, double a) { cm = (w > 0.0) ? fmax(cm, a) : cm; });
      if (cm > m) {
        s0 *= exp_nonpos(m - cm, sExpTab);
        m = cm;
      }
      double c0 = 0.0;
      each([&](int64_t, double w, double a) { c0 += (w > 0.0) ? w * exp_nonpos(a - m, sExpTab) : 0.0; });
      s0 += c0;
    });
  }
  if (at.q < pb.Nq) {
    pb.partial[o] = m;
    pb.partial[row + o] = s0;
  }
}

// Items [0, n), item i owns blocks [first[i], first[i+1]).  The groups in group order: M = max m_g, S_j = sum_g s_jg
// exp(m_g - M); logz = M + log S_0 - log norm_G; mean_k = r_k - S1_k / S_0, var_k = v_k + max(0, S2_k / S_0 - (S1_k / S_0)^2)
// (k in F).  No leaf in S: logz = -Inf, mean and var NaN, the draw's point NaN and ind = 0.  A NaN among the given values:
// logz NaN as well, the rest likewise, and no group marked as chosen.  The draw: T = u S_0, the first
// group whose running total (the very additions that formed S_0) exceeds T, the residual T - (the total before it) divided
// by exp(m_g - M); none: the last group with s_0g > 0 and an infinite residual.
__global__ __launch_bounds__(kFinishThreads) void cond_finish_kernel(const CondItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n) {
  __shared__ int32_t sChosen[kEvalMaxGroups];
  const ItemBlock ib = item_block(first, n);
  const CondItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  const bool draw = it.pts != nullptr;  // block-uniform
  if (draw) {
    if (threadIdx.x < kEvalMaxGroups) sChosen[threadIdx.x] = 0;
    __syncthreads();
  }
  if (q < it.Nq) {
    const int D = it.D, nf = D - it.ng;
    const int64_t row = static_cast<int64_t>(it.ngroups) * it.Nq;
    const double *pm = it.partial + q;
    double M = -INFINITY;
    for (int g = 0; g < it.ngroups; ++g) M = fmax(M, pm[static_cast<int64_t>(g) * it.Nq]);
    bool bad = false;  // a NaN among the given values (the sweep drops it: pair_sweep.hpp): every output of the query is NaN
    for (int k = 0; k < D; ++k) bad = bad || (is_given(it, k) && it.xq[q * D + k] != it.xq[q * D + k]);
    const bool some = M > -INFINITY;
    const int nsum = it.mom ? 1 + 2 * D : 1;
    double S[2 * KDEHIP_MAX_DIMS + 1];
    for (int j = 0; j < nsum; ++j) S[j] = 0.0;
    if (some) {
      for (int g = 0; g < it.ngroups; ++g) {
        const double mg = pm[static_cast<int64_t>(g) * it.Nq];
        if (mg > -INFINITY) {
          const double e = exp(mg - M);
          for (int j = 0; j < nsum; ++j) S[j] += pm[(j + 1) * row + static_cast<int64_t>(g) * it.Nq] * e;
        }
      }
    }
    it.ms[q] = M;
    it.ms[it.Nq + q] = S[0];
    if (it.logz) {
      const double norm = gauss_norm(it.norm0, D, [&](int k) { return is_given(it, k) ? it.bw[k] : 1.0; });
      it.logz[q] = bad ? __builtin_nan("") : some ? M + log(S[0]) - log(norm) : -INFINITY;
    }
    if (it.mom) {
      int j = 0;
      for (int k = 0; k < D; ++k) {
        if (is_given(it, k)) continue;
        double mu = __builtin_nan(""), va = __builtin_nan("");
        if (some && !bad) {
          const double a1 = S[1 + k] / S[0], a2 = S[1 + D + k] / S[0];
          mu = it.ref[k] - a1;
          va = it.bw[k] + fmax(a2 - a1 * a1, 0.0);
        }
        if (it.mean) it.mean[q * nf + j] = mu;
        if (it.var) it.var[q * nf + j] = va;
        ++j;
      }
    }
    if (draw) {
      int cg = -1;
      double res = INFINITY;
      if (some && !bad) {  // (a NaN query chooses no group)
        const double T = philox_uniform(it.seed, static_cast<uint64_t>(it.offset + q), 1u) * S[0];
        double run = 0.0;
        int last = -1;
        for (int g = 0; g < it.ngroups; ++g) {
          const double mg = pm[static_cast<int64_t>(g) * it.Nq];
          if (!(mg > -INFINITY)) continue;
          const double e = exp(mg - M), s0g = pm[row + static_cast<int64_t>(g) * it.Nq];
          if (s0g > 0.0) last = g;
          const double next = run + s0g * e;
          if (next > T) {  // (then e > 0)
            cg = g;
            res = (T - run) / e;
            break;
          }
          run = next;
        }
        if (cg < 0) cg = last;
      }
      it.cgrp[q] = cg;
      it.resid[q] = res;
      if (cg >= 0) {
        sChosen[cg] = 1;  // (every writer writes 1)
      } else {
        for (int j = 0; j < nf; ++j) it.pts[q * nf + j] = __builtin_nan("");
        it.ind[q] = 0;
      }
    }
  }
  if (draw) {
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < it.ngroups)
      it.chosen[static_cast<int64_t>(ib.k) * it.ngroups + threadIdx.x] = sChosen[threadIdx.x];
  }
}

// The blocks of the partial sweep once more.  A block whose (query block, group) no lane chose returns before any barrier;
// in the others the lanes that chose the group add t_i = w_i exp_nonpos(a_i - m_g) over the group's leaves of S in leaf order
// and keep the first whose running sum exceeds their residual, or the group's last leaf of S.  Such a lane then forms its
// query's point, c_iF + sqrt(v_F) n with the multiply and the add rounded on their own (wrapped where F_j is circular),
// and ind = the leaf's original index.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void cond_select_kernel(const CondItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n,
                                                                   const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const CondItem pb = items[ib.item];
  if (!pb.pts) return;  // block-uniform: the item draws nothing
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;
  const int64_t qblocks = (pb.Nq + kEvalThreads - 1) / kEvalThreads;
  if (pb.chosen[(ib.k % qblocks) * pb.ngroups + at.grp] == 0) return;  // block-uniform, before any barrier
  const bool mine = at.q < pb.Nq && pb.cgrp[at.q] == static_cast<int32_t>(at.grp);
  const double mg = mine ? pb.partial[at.grp * pb.Nq + at.q] : 0.0;
  const double res = mine ? pb.resid[at.q] : 0.0;
  double nhib[D];
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = is_given(pb, k) ? -0.5 / pb.bw[k] : 0.0;
  double run = 0.0;
  int64_t found = -1, last = -1;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    each([&](int64_t i, double w, double a) {
      if (mine && found < 0 && w > 0.0) {  // in S: a <= m_g
        run += w * exp_nonpos(a - mg, sExpTab);
        last = i;
        if (run > res) found = i;
      }
    });
  });
  if (!mine) return;
  const int64_t lab = found >= 0 ? found : last;
  const int nf = D - pb.ng;
  if (lab < 0 || lab >= pb.N) {  // (a chosen group has a leaf in S)
    for (int j = 0; j < nf; ++j) pb.pts[at.q * nf + j] = __builtin_nan("");
    pb.ind[at.q] = 0;
    return;
  }
  const uint64_t g = static_cast<uint64_t>(pb.offset + at.q);
  double even = 0.0, odd = 0.0;
  int j = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if (is_given(pb, k)) continue;
    if ((j & 1) == 0) philox_normal_pair(pb.seed, g, static_cast<uint32_t>(j >> 1), even, odd);
    const double nj = (j & 1) ? odd : even;
    double x = __dadd_rn(pb.src[lab * D + k], __dmul_rn(__dsqrt_rn(pb.bw[k]), nj));
    if constexpr (CIRC) {
      if ((circ >> k) & 1u) x = circ_wrap(x);
    }
    pb.pts[at.q * nf + j] = x;
    ++j;
  }
  pb.ind[at.q] = pb.perm[lab];
}

// ONE item; thread t is (query t / N, leaf t % N): omega = w_i exp_nonpos(a_i - M) / S_0 -- a_i by the sweep's expression
// over the given dimensions (the free ones add +0 there) -- to w_out[q][original index of the leaf]; a leaf outside S: 0;
// a query whose S_0 is 0 (an infinite given value): 0; a query with a NaN among its given values: NaN.
__global__ __launch_bounds__(256) void cond_weights_kernel(const CondItem *__restrict__ items, uint32_t circ) {
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  __syncthreads();
  const CondItem it = items[0];
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= it.N * it.Nq) return;
  const int64_t q = t / it.N, i = t - q * it.N;
  const int64_t o = it.perm[i] - 1;
  if (o < 0 || o >= it.N) return;  // (an uploaded density's permutation is the caller's)
  const double w = it.w[i];
  bool bad = false;  // a NaN among the given values: the whole row is NaN
  for (int k = 0; k < it.D; ++k) bad = bad || (is_given(it, k) && it.xq[q * it.D + k] != it.xq[q * it.D + k]);
  double om = bad ? __builtin_nan("") : 0.0;
  if (!bad && w > 0.0 && it.ms[it.Nq + q] > 0.0) {  // (S_0 == 0: no leaf of S in reach of an infinite value -- the row is 0)
    double acc = 0.0;
    for (int k = 0; k < it.D; ++k) {
      if (!is_given(it, k)) continue;
      double d = it.xq[q * it.D + k] - it.src[i * it.D + k];
      if ((circ >> k) & 1u) d = circ_wrap(d);
      acc = fma(d * d, -0.5 / it.bw[k], acc);
    }
    om = w * exp_nonpos(acc - it.ms[q], sExpTab) / it.ms[it.Nq + q];  // acc <= M
  }
  it.wout[q * it.N + o] = om;
}

// The run of one call (pair_sweep.hpp PairRun) with the conditional's scratch, per item
// [xq | partial | ms | resid | cgrp | chosen], and its launches.  Protocol: fill `items` (sizes, D, ng, gmask, mom, seed,
// offset, norm0) and `circ` -> alloc(prefix bytes of caller data, result doubles of the caller) -> the caller writes its data
// into host() and points the items at dev() -> run(stream) -> (the weights entries) weights() -> wait() or defer(device).
class CondRun : public PairRun<CondItem> {
 public:
  int alloc(size_t prefix, size_t nresults) {
    const size_t n = items.size();
    int64_t pblocks = 0, fblocks = 0;
    for (CondItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      fblocks += it.nfb;
    }
    if (pblocks > INT32_MAX / 2 || fblocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many queries for one launch");
    Carve c;
    carve_head(c, prefix, 2, 0, nresults);  // first[] of the sweeps and of the expand / finish kernels
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) scratch[k] = c.take(scratch_bytes(items[k]));
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) {
      CondItem &it = items[k];
      it.xq = reinterpret_cast<double *>(dev() + scratch[k]);
      it.qry = it.xq;
      it.partial = it.xq + it.Nq * it.D;
      it.ms = it.partial + static_cast<int64_t>(nrows(it)) * it.ngroups * it.Nq;
      it.resid = it.ms + 2 * it.Nq;
      it.cgrp = reinterpret_cast<int32_t *>(it.resid + it.Nq);
      it.chosen = it.cgrp + it.Nq;
    }
    return KDEHIP_OK;
  }
  int run(hipStream_t st) {
    bool draws = false;
    for (const CondItem &it : items) draws = draws || it.pts;
    prepare([&](size_t k) { return 2 * items[k].D + (circ[k] ? 1 : 0); });  // by D; Euclidean items before circular ones
    const size_t n = items.size();
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    for (size_t k = 0; k < n; ++k) ffirst[k + 1] = ffirst[k] + items[k].nfb;
    KDEHIP_CHECK(send(st));
    if (ffirst[n] <= 0) return KDEHIP_OK;
    hipLaunchKernelGGL(cond_expand_kernel, dim3(static_cast<unsigned>(ffirst[n])), dim3(kFinishThreads), 0, st, d_items(),
                       d_first(1), static_cast<int>(n));
    KDEHIP_CHECK(hipGetLastError());
    KDEHIP_CHECK_RC(sweep(false));
    hipLaunchKernelGGL(cond_finish_kernel, dim3(static_cast<unsigned>(ffirst[n])), dim3(kFinishThreads), 0, st, d_items(),
                       d_first(1), static_cast<int>(n));
    KDEHIP_CHECK(hipGetLastError());
    if (draws) KDEHIP_CHECK_RC(sweep(true));
    return KDEHIP_OK;
  }
  // (a run of ONE item) omega of every (query, leaf) to the item's wout
  int weights() {
    const CondItem &it = items[0];
    const int64_t blocks = (it.N * it.Nq + 255) / 256;
    if (blocks > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many (query, point) pairs for one launch");
    hipLaunchKernelGGL(cond_weights_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream(), d_items(), circ[0]);
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }

 private:
  static int nrows(const CondItem &it) { return it.mom ? 2 + 2 * it.D : 2; }
  static size_t scratch_bytes(const CondItem &it) {
    return sizeof(double) * (it.Nq * it.D + static_cast<int64_t>(nrows(it)) * it.ngroups * it.Nq + 3 * it.Nq) +
           sizeof(int32_t) * (it.Nq + static_cast<int64_t>(it.nfb) * it.ngroups);
  }
  // one launch per distinct (D, circular): the partial sweep, or the select sweep of the runs in which an item draws
  int sweep(bool select) {
    const hipStream_t st = stream();
    return for_each_run([&](const CondItem &it, const CondItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                            const uint32_t *d_masks) -> int {
      if (select) {
        const CondItem *a = items.data() + (d_it - d_items());
        if (std::none_of(a, a + cnt, [](const CondItem &x) { return x.pts != nullptr; })) return KDEHIP_OK;
      }
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        if (select)
          launch_pair<CondItem>(cond_select_kernel<kD, false>, cond_select_kernel<kD, true>, blocks, st, d_it, d_pfirst, cnt, d_masks);
        else
          launch_pair<CondItem>(cond_partial_kernel<kD, false>, cond_partial_kernel<kD, true>, blocks, st, d_it, d_pfirst, cnt, d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    });
  }
};

// ---- arguments ------------------------------------------------------------------------------------------------------------

int popcount32(uint32_t x) { return __builtin_popcount(x); }

// the given dimensions of a D-dimensional density: 1 <= ng <= D - 1 and no bit at or above D
int check_mask(uint32_t gmask, int D) {
  if (D < 2) return set_error(KDEHIP_ERR_ARG, "conditional: a 1-D density has no dimension left to condition on");
  if (gmask >> D) return set_error(KDEHIP_ERR_ARG, "conditional: given_mask names a dimension the density does not have");
  const int ng = popcount32(gmask);
  if (ng < 1 || ng > D - 1) return set_error(KDEHIP_ERR_ARG, "conditional: between 1 and ndims - 1 dimensions can be given");
  return KDEHIP_OK;
}

int check_free_moments(bool moments, uint32_t circ, uint32_t gmask) {
  if (moments && (circ & ~gmask))
    return set_error(KDEHIP_ERR_UNSUPPORTED, "conditional: mean and var over a circular free dimension are not supported");
  return KDEHIP_OK;
}

int check_outputs(const void *logz, const void *mean, const void *var, const void *pts, const void *ind) {
  if (!logz && !mean && !var && !pts && !ind) return set_error(KDEHIP_ERR_ARG, "null argument");
  if ((pts == nullptr) != (ind == nullptr)) return set_error(KDEHIP_ERR_ARG, "conditional: pts and ind are given together");
  return KDEHIP_OK;
}

const char kGiven[] = "given must hold Nq >= 0 queries", kDeviceGiven[] = "d_given must hold Nq >= 0 queries";

CondItem base_item(int64_t N, int D, int64_t Nq, uint32_t gmask, bool moments, uint64_t seed, int64_t offset) {
  CondItem it{};
  it.N = N; it.Nq = Nq; it.D = D; it.gmask = gmask; it.ng = popcount32(gmask);
  it.norm0 = gauss_norm0(it.ng);
  it.mom = moments ? 1 : 0; it.seed = seed; it.offset = offset;
  return it;
}

void point_resident(CondItem &it, const kdehip_device_density *bd) {
  const LeafRows leaf = leaf_rows(bd);
  it.src = leaf.src; it.w = leaf.w; it.bw = leaf.bw; it.perm = leaf.perm; it.ref = leaf.ref;
}

// a host density at offset 0 of the call's image: the plain form (density_args.hpp), then [r | permutation]
size_t cond_density_bytes(const kdehip_density *bd) {
  return host_density_bytes(bd) + sizeof(double) * bd->ndim + sizeof(int64_t) * bd->npts;
}
void pack_cond_density(CondRun &run, CondItem &it, const kdehip_density *bd) {
  const int64_t N = bd->npts, D = bd->ndim;
  const size_t o_ref = host_density_bytes(bd), o_perm = o_ref + sizeof(double) * D;
  it.bw = pack_host_density(run, it, bd);
  std::memcpy(run.host() + o_ref, bd->means, sizeof(double) * D);
  std::memcpy(run.host() + o_perm, bd->permutation + N, sizeof(int64_t) * N);
  it.ref = reinterpret_cast<const double *>(run.dev() + o_ref);
  it.perm = reinterpret_cast<const int64_t *>(run.dev() + o_perm);
}

}  // namespace

extern "C" int kdehip_conditional(const kdehip_density *bd, uint32_t given_mask, const double *given, int64_t Nq, uint64_t seed,
                                  int64_t sample_offset, double *logz, double *mean, double *var, double *pts, int64_t *ind,
                                  int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!bd) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_outputs(logz, mean, var, pts, ind));
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  KDEHIP_CHECK_RC(check_mask(given_mask, D));
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(given, Nq, kGiven));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  KDEHIP_CHECK_RC(check_free_moments(mean || var, circ, given_mask));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  CondRun run;
  run.items.push_back(base_item(bd->npts, D, Nq, given_mask, mean || var, seed, sample_offset));
  run.circ.push_back(circ);
  const int ng = run.items[0].ng, nf = D - ng;
  // caller data: [the density | queries]; results: [logz (Nq) | mean (Nq nf) | var (Nq nf) | pts (Nq nf) | ind (Nq int64)]
  const size_t o_q = cond_density_bytes(bd), prefix = o_q + sizeof(double) * Nq * ng;
  const size_t r_mean = static_cast<size_t>(Nq), r_var = r_mean + static_cast<size_t>(Nq) * nf,
               r_pts = r_var + static_cast<size_t>(Nq) * nf, r_ind = r_pts + static_cast<size_t>(Nq) * nf;
  KDEHIP_CHECK_RC(run.alloc(prefix, r_ind + static_cast<size_t>(Nq)));
  CondItem &ri = run.items[0];
  pack_cond_density(run, ri, bd);
  std::memcpy(run.host() + o_q, given, sizeof(double) * Nq * ng);
  ri.given = reinterpret_cast<const double *>(run.dev() + o_q);
  ri.logz = logz ? run.result(0) : nullptr;
  ri.mean = mean ? run.result(r_mean) : nullptr;
  ri.var = var ? run.result(r_var) : nullptr;
  ri.pts = pts ? run.result(r_pts) : nullptr;
  ri.ind = ind ? reinterpret_cast<int64_t *>(run.result(r_ind)) : nullptr;
  KDEHIP_CHECK_RC(run.run(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  if (logz) std::memcpy(logz, run.host_result(0), sizeof(double) * Nq);
  if (mean) std::memcpy(mean, run.host_result(r_mean), sizeof(double) * Nq * nf);
  if (var) std::memcpy(var, run.host_result(r_var), sizeof(double) * Nq * nf);
  if (pts) std::memcpy(pts, run.host_result(r_pts), sizeof(double) * Nq * nf);
  if (ind) std::memcpy(ind, run.host_result(r_ind), sizeof(int64_t) * Nq);
  return KDEHIP_OK;
}

extern "C" int kdehip_conditional_device_batch(int n, const kdehip_conditional_item *items, void *stream) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "conditional batch: "));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_conditional_item &c = items[i];
    KDEHIP_CHECK_RC(check_resident_density(c.bd, false));
    KDEHIP_CHECK_RC(check_outputs(c.d_logz, c.d_mean, c.d_var, c.d_pts, c.d_ind));
    KDEHIP_CHECK_RC(check_same_device(c.bd, items[0].bd, "conditional batch: "));
    KDEHIP_CHECK_RC(check_mask(c.given_mask, c.bd->D));
    KDEHIP_CHECK_RC(check_circular_mask(c.circular_mask, c.bd->D, "conditional batch: "));
    KDEHIP_CHECK_RC(check_query_count(c.d_given, c.Nq, kDeviceGiven));
    if (!leaves_share_bandwidth(c.bd)) return set_error(KDEHIP_ERR_UNSUPPORTED, kOneBandwidth);
    KDEHIP_CHECK_RC(check_free_moments(c.d_mean || c.d_var, c.circular_mask, c.given_mask));
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  CondRun run;
  std::vector<int> which;
  for (int i = 0; i < n; ++i) {
    const kdehip_conditional_item &c = items[i];
    if (c.Nq == 0) continue;
    run.items.push_back(base_item(c.bd->N, c.bd->D, c.Nq, c.given_mask, c.d_mean || c.d_var, c.seed, c.sample_offset));
    run.circ.push_back(c.circular_mask);
    which.push_back(i);
  }
  if (run.items.empty()) return KDEHIP_OK;
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  for (size_t k = 0; k < which.size(); ++k) {
    const kdehip_conditional_item &c = items[which[k]];
    CondItem &ri = run.items[k];
    point_resident(ri, c.bd);
    ri.given = c.d_given;
    ri.logz = c.d_logz; ri.mean = c.d_mean; ri.var = c.d_var; ri.pts = c.d_pts; ri.ind = c.d_ind;
  }
  KDEHIP_CHECK_RC(run.run(static_cast<hipStream_t>(stream)));
  return finish_enqueue(run, nullptr, device);
}

extern "C" int kdehip_conditional_device(const kdehip_device_density *bd, uint32_t given_mask, const double *d_given, int64_t Nq,
                                         uint64_t seed, int64_t sample_offset, double *d_logz, double *d_mean, double *d_var,
                                         double *d_pts, int64_t *d_ind, const uint8_t *manifold, void *stream) {
  if (!bd) return set_error(KDEHIP_ERR_ARG, "null density");
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(check_resident_density(bd, false));
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  kdehip_conditional_item c{};
  c.bd = bd; c.d_given = d_given; c.Nq = Nq; c.seed = seed; c.sample_offset = sample_offset;
  c.d_logz = d_logz; c.d_mean = d_mean; c.d_var = d_var; c.d_pts = d_pts; c.d_ind = d_ind;
  c.given_mask = given_mask; c.circular_mask = circ;
  return kdehip_conditional_device_batch(1, &c, stream);
}

extern "C" int kdehip_condition_weights(const kdehip_density *bd, uint32_t given_mask, const double *given, int64_t Nq,
                                        double *w_out, double *logz, int device, const uint8_t *manifold) {
  if (!bd || !w_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  const int64_t N = bd->npts;
  KDEHIP_CHECK_RC(check_mask(given_mask, D));
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(given, Nq, kGiven));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  CondRun run;
  run.items.push_back(base_item(N, D, Nq, given_mask, false, 0, 0));
  run.circ.push_back(circ);
  const int ng = run.items[0].ng;
  // caller data: [the density | queries]; results: [w_out (Nq N) | logz (Nq)]
  const size_t o_q = cond_density_bytes(bd), prefix = o_q + sizeof(double) * Nq * ng;
  const size_t r_logz = static_cast<size_t>(Nq) * N;
  KDEHIP_CHECK_RC(run.alloc(prefix, r_logz + static_cast<size_t>(Nq)));
  CondItem &ri = run.items[0];
  pack_cond_density(run, ri, bd);
  std::memcpy(run.host() + o_q, given, sizeof(double) * Nq * ng);
  ri.given = reinterpret_cast<const double *>(run.dev() + o_q);
  ri.wout = run.result(0);
  ri.logz = logz ? run.result(r_logz) : nullptr;
  KDEHIP_CHECK_RC(run.run(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.weights());
  KDEHIP_CHECK_RC(run.wait());
  std::memcpy(w_out, run.host_result(0), sizeof(double) * Nq * N);
  if (logz) std::memcpy(logz, run.host_result(r_logz), sizeof(double) * Nq);
  return KDEHIP_OK;
}

extern "C" int kdehip_condition_weights_device(const kdehip_device_density *bd, uint32_t given_mask, const double *d_given,
                                               int64_t Nq, double *d_w_out, double *d_logz, const uint8_t *manifold,
                                               void *stream) {
  if (!bd || !d_w_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, false));
  KDEHIP_CHECK_RC(check_mask(given_mask, bd->D));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(d_given, Nq, kDeviceGiven));
  if (!leaves_share_bandwidth(bd)) return set_error(KDEHIP_ERR_UNSUPPORTED, kOneBandwidth);
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  CondRun run;
  run.items.push_back(base_item(bd->N, bd->D, Nq, given_mask, false, 0, 0));
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  CondItem &ri = run.items[0];
  point_resident(ri, bd);
  ri.given = d_given;
  ri.wout = d_w_out;
  ri.logz = d_logz;
  KDEHIP_CHECK_RC(run.run(static_cast<hipStream_t>(stream)));
  KDEHIP_CHECK_RC(run.weights());
  return finish_enqueue(run, nullptr, bd->device);
}
