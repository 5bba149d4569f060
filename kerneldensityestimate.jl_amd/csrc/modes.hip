// modes.hip -- the gradient of a Gaussian-kernel density and its joint modes by mean shift (include/kdehip.h section 5h; no
// reference counterpart: getKDEMax, src/DualTree01.jl:558-570, is the grid argmax of every 1-D marginal on its own).
// For a query x, with a_i the exponent of pair_sweep.hpp and d_ik the differences it is formed from,
//   S_0 = sum_{i in S} w_i exp(a_i - m),  S_k = sum_{i in S} w_i exp(a_i - m) d_ik,   S = { i : w_i > 0 },  m = max_S a_i
//   log p = m + log S_0 - log norm,   grad log p (x)_k = -S_k / (S_0 v_k),   the mean-shift step x_k <- x_k - S_k / S_0.
// Host densities (uploaded for the call, blocking) and resident ones (single, or batched and enqueue-only) run ONE path, any
// number of items described in device memory by MomentItem and driven by MomentRun:
//   moments_init_kernel        the starts copied to x (or the density's own points scattered to their original order), the
//                              step counts and frozen flags cleared, every query block's live count set;
//   moments_partial_kernel<D>  one launch per distinct D (one more for its items with a circular dimension): the sweep of
//                              pair_sweep.hpp with the step of eval_partial_log_kernel, carrying (m, s_0, s_1..s_D) -- D more
//                              fmas per pair beside the one exp; scratch [D + 2][ngroups][Nq];
//   moments_finish_kernel      the groups combined in group order; an evaluate item stores the value and the gradient, a step
//                              item moves its query in place, counts the step, freezes the query at convergence and writes
//                              the block's number of live queries -- which the next sweep's partial blocks of that query block
//                              read to return at once when it is 0;
//   moments_live_kernel        one thread per item: the live counts in block order into one int32.
// A mean-shift call holds every item twice, as a step item and as an evaluate item (the closing log p) on the same scratch.
// No atomics; the in-place update is ordered by the stream.  The group split (split_chunks(N, Nq, 1)) depends on the item's
// sizes alone and a frozen query is never written again, so a query's trajectory depends on the density, its start and tol
// alone: the host entry, a resident call and any batch give the same bits, however the sweeps are grouped into rounds.
// The curvature (section 5k: the Hessian of log p and the covariance of a mode) is the same sweep with the second moments
// carried too, on a run of its own (CurvItem, CurvRun): see "curvature" below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
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

constexpr int kFinishThreads = kEvalThreads;  // a finish block is a query block: its live count is that block's
constexpr int kRound = 8;                     // step sweeps between two reads of the live count (blocking calls)

enum : int32_t { kModeEvaluate = 0, kModeStep = 1 };

// One item: a density (N source points in leaf order, one bandwidth vector) and Nq queries.  The head's qry IS x for a step
// item (moved in place) and the caller's positions for a plain evaluation.
struct MomentItem : PairHead {
  const double *bw;      // [D] the density's first leaf's variances
  const double *start;   // step items: [Nq][D] the starts, or null: the sources through perm
  const int64_t *perm;   // [N] 1-based original position of leaf i (start == null)
  double *x;             // step items: [Nq][D], == qry
  double *val;           // [Nq] log p (or p), or null
  double *grad;          // [Nq][D], or null (evaluate items)
  int32_t *iters;        // [Nq] steps taken, negative while the last one was above tol (null: a plain evaluation)
  int32_t *frozen;       // [Nq] the query moves no more
  int32_t *live;         // [qblocks] queries of the block that still move
  int32_t *nlive;        // their sum over the item
  double *partial;       // [D + 2][ngroups][Nq]: m, s_0, s_1..s_D
  double norm0, tol;
  int32_t ngroups, nfb, D, mode, logdom, pad_;
};

__device__ __forceinline__ double moment_norm(const MomentItem &it) {
  return gauss_norm(it.norm0, it.D, [&](int k) { return it.bw[k]; });
}

// step items [0, n), item i owns (finish) blocks [first[i], first[i+1]): x from the starts, the state cleared
__global__ __launch_bounds__(kFinishThreads) void moments_init_kernel(const MomentItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n) {
  const ItemBlock ib = item_block(first, n);
  const MomentItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  bool bad = false;  // a start with a NaN coordinate is frozen from the outset: it never counts as live
  if (q < it.Nq) {
    if (it.start) {
      bad = query_has_nan(it.start, q, it.D);
      if (it.start != it.x)
        for (int k = 0; k < it.D; ++k) it.x[q * it.D + k] = it.start[q * it.D + k];
    } else {  // (Nq == N) leaf q is original point perm[q]
      const int64_t o = it.perm[q] - 1;
      if (o >= 0 && o < it.Nq)
        for (int k = 0; k < it.D; ++k) it.x[o * it.D + k] = it.src[q * it.D + k];
    }
    it.iters[q] = 0;
    it.frozen[q] = bad ? 1 : 0;
  }
  const int cnt = __syncthreads_count(q < it.Nq && !bad);
  if (threadIdx.x == 0) it.live[ib.k] = cnt;
}

// partial[0][g][q] = m, partial[1][g][q] = s_0, partial[2 + k][g][q] = s_{k+1} over the source chunks of group g in chunk
// order: per staged chunk, pass one takes the chunk's maximum of a_i over S, the carried sums are rescaled ONCE by
// exp_nonpos(m_old - m_new), pass two adds t = w_i exp_nonpos(a_i - m) to s_0 and d_k t to s_k (one exp per pair).  A
// group with S empty leaves (-Inf, 0, ..).  A block whose query block has no live query (step items) returns at once.
// CIRC as in evaluate.hip: data in which no difference wraps gives the bits of the Euclidean instantiation.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void moments_partial_kernel(const MomentItem *__restrict__ items,
                                                                       const int32_t *__restrict__ first, int n,
                                                                       const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const MomentItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  if (pb.mode == kModeStep) {          // block-uniform, before any barrier: nothing of this query block moves any more
    const int64_t qblocks = (pb.Nq + kEvalThreads - 1) / kEvalThreads;
    if (pb.live[ib.k % qblocks] == 0) return;
  }
  double nhib[D];  // -1/(2 bw_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.bw[k];
  double m = -INFINITY, s[D + 1];
#pragma unroll
  for (int j = 0; j <= D; ++j) s[j] = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t, double w, double a) { cm = (w > 0.0) ? fmax(cm, a) : cm; });
    if (cm > m) {  // (m == -Inf: the sums are still 0)
      const double r = exp_nonpos(m - cm, sExpTab);
#pragma unroll
      for (int j = 0; j <= D; ++j) s[j] *= r;
      m = cm;
    }
    double c[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) c[j] = 0.0;
    each([&](int64_t, double w, double a, const double (&d)[D]) {
      const double t = (w > 0.0) ? w * exp_nonpos(a - m, sExpTab) : 0.0;  // in S: a <= m
      c[0] += t;
#pragma unroll
      for (int k = 0; k < D; ++k) c[k + 1] = fma(d[k], t, c[k + 1]);
    });
#pragma unroll
    for (int j = 0; j <= D; ++j) s[j] += c[j];
  });
  if (at.q < pb.Nq) {
    const int64_t row = static_cast<int64_t>(pb.ngroups) * pb.Nq, o = at.grp * pb.Nq + at.q;
    pb.partial[o] = m;
#pragma unroll
    for (int j = 0; j <= D; ++j) pb.partial[(j + 1) * row + o] = s[j];
  }
}

// Items [0, n) of one mode, item i owns blocks [first[i], first[i+1]).  The groups in group order: M = max m_g,
// S_j = sum_g s_jg exp(m_g - M); then
//   evaluate: val = log p = M + log S_0 - log norm (or p = exp(M) S_0 / norm), grad_k = -S_k / (S_0 v_k) (times p); no
//             source in S: -Inf (0) and 0; a query with a NaN coordinate: NaN, all of them
//   step:     val = log p HERE, then x_k <- x_k - S_k / S_0 (wrapped in a circular dimension), one more step counted, and the
//             query frozen once max_k |S_k / S_0| / sqrt(v_k) <= tol; no source in S: frozen where it is.  A frozen query
//             is not touched, and a start with a NaN coordinate is frozen by moments_init_kernel: it stays where it is with
//             0 steps, and the closing evaluation gives it log p = NaN.  live[block] = the block's queries that still move.
__global__ __launch_bounds__(kFinishThreads) void moments_finish_kernel(const MomentItem *__restrict__ items,
                                                                      const int32_t *__restrict__ first, int n,
                                                                      const uint32_t *__restrict__ masks) {
  const ItemBlock ib = item_block(first, n);
  const MomentItem it = items[ib.item];
  const unsigned circ = masks[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  const bool step = it.mode == kModeStep;
  int alive = 0;
  if (q < it.Nq && !(step && it.frozen[q])) {
    const int D = it.D;
    const int64_t row = static_cast<int64_t>(it.ngroups) * it.Nq;
    const double *pm = it.partial + q;
    double M = -INFINITY;
    for (int g = 0; g < it.ngroups; ++g) M = fmax(M, pm[static_cast<int64_t>(g) * it.Nq]);
    double S[KDEHIP_MAX_DIMS + 1];
    for (int j = 0; j <= D; ++j) S[j] = 0.0;
    if (M > -INFINITY) {
      for (int g = 0; g < it.ngroups; ++g) {
        const double mg = pm[static_cast<int64_t>(g) * it.Nq];
        if (mg > -INFINITY) {
          const double e = exp(mg - M);
          for (int j = 0; j <= D; ++j) S[j] += pm[(j + 1) * row + static_cast<int64_t>(g) * it.Nq] * e;
        }
      }
    }
    const double lp = (M > -INFINITY) ? M + log(S[0]) - log(moment_norm(it)) : -INFINITY;
    const bool bad = query_has_nan(it.qry, q, D);  // (the sweep drops a NaN: pair_sweep.hpp)
    if (!step) {
      const double p = (M > -INFINITY) ? exp(M) * S[0] / moment_norm(it) : 0.0;
      if (it.val) it.val[q] = bad ? __builtin_nan("") : it.logdom ? lp : p;
      if (it.grad)
        for (int k = 0; k < D; ++k) {
          const double g = (M > -INFINITY) ? -S[k + 1] / (S[0] * it.bw[k]) : 0.0;
          it.grad[q * D + k] = bad ? __builtin_nan("") : it.logdom ? g : g * p;
        }
    } else if (bad) {  // (a start is caught by moments_init_kernel; this is a query that has become NaN on its way)
      it.val[q] = __builtin_nan("");
      it.frozen[q] = 1;
    } else if (M > -INFINITY) {
      it.val[q] = lp;
      double reach = 0.0;
      for (int k = 0; k < D; ++k) {
        const double dx = S[k + 1] / S[0];
        double xn = it.x[q * D + k] - dx;
        if ((circ >> k) & 1u) xn = circ_wrap(xn);
        it.x[q * D + k] = xn;
        reach = fmax(reach, fabs(dx) / sqrt(it.bw[k]));
      }
      const int32_t cnt = abs(it.iters[q]) + 1;
      if (reach <= it.tol) {
        it.iters[q] = cnt;
        it.frozen[q] = 1;
      } else {
        it.iters[q] = -cnt;
        alive = 1;
      }
    } else {
      it.val[q] = lp;
      it.frozen[q] = 1;  // (no step taken: iters stays 0)
    }
  }
  if (!step) return;  // (block-uniform)
  const int cnt = __syncthreads_count(alive);
  if (threadIdx.x == 0) it.live[ib.k] = cnt;
}

// one thread per step item: the live counts in block order
__global__ void moments_live_kernel(const MomentItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const MomentItem it = items[i];
  int32_t s = 0;
  for (int b = 0; b < it.nfb; ++b) s += it.live[b];
  *it.nlive = s;
}

// ---- curvature (include/kdehip.h section 5k) ------------------------------------------------------------------------------
// The second moments S_kl = sum_{i in S} t_i d_ik d_il (k <= l) beside (m, S_0, S_k), the Hessian of log p and, where -H is
// positive definite, its inverse: the covariance of the Gaussian that has the density's curvature at x.
//   curvature_partial_kernel<D>  the sweep and the two passes of moments_partial_kernel, carrying 2 + D + D(D+1)/2 values
//                                per lane: per pair D multiplies (u = d_k t) and D(D+1)/2 fmas (fma(u, d_l, c_kl)) beside
//                                the moments' work; scratch [2 + D + D(D+1)/2][ngroups][Nq];
//   curvature_finish_kernel      ONE launch for all items, one thread per query: the groups combined in group order, then g,
//                                H, the Cholesky factor of -H and the inverse, instantiated per D (compile-time indices).
constexpr int tri_count(int D) { return D * (D + 1) / 2; }
constexpr int tri_index(int D, int k, int l) { return k * D - k * (k - 1) / 2 + (l - k); }  // k <= l, row-major upper triangle

struct CurvItem : PairHead {
  const double *bw;   // [D] the density's first leaf's variances
  double *logp;       // [Nq], or null
  double *grad;       // [Nq][D], or null
  double *hess;       // [Nq][D][D], or null
  double *cov;        // [Nq][D][D], or null
  int32_t *definite;  // [Nq], or null
  double *partial;    // [2 + D + D(D+1)/2][ngroups][Nq]: m, s_0, s_1..s_D, s_kl (k <= l, row by row)
  double norm0;
  int32_t ngroups, nfb, D, pad_;
};

// partial[0][g][q] = m, [1] = s_0, [2 + k] = s_{k+1}, [2 + D + tri_index(k, l)] = s_kl over the source chunks of group g in
// chunk order, exactly as moments_partial_kernel words it: per staged chunk the chunk's maximum over S, the carried sums
// rescaled ONCE by exp_nonpos(m_old - m_new), then the chunk's own sums (from 0, in source order) added to the carried ones.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void curvature_partial_kernel(const CurvItem *__restrict__ items,
                                                                         const int32_t *__restrict__ first, int n,
                                                                         const uint32_t *__restrict__ masks) {
  constexpr int T = tri_count(D), W = 1 + D + T;
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const CurvItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform, before any barrier
  double nhib[D];  // -1/(2 bw_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.bw[k];
  double m = -INFINITY, s[W];
#pragma unroll
  for (int j = 0; j < W; ++j) s[j] = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t, double w, double a) { cm = (w > 0.0) ? fmax(cm, a) : cm; });
    if (cm > m) {  // (m == -Inf: the sums are still 0)
      const double r = exp_nonpos(m - cm, sExpTab);
#pragma unroll
      for (int j = 0; j < W; ++j) s[j] *= r;
      m = cm;
    }
    double c[W];
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = 0.0;
    each([&](int64_t, double w, double a, const double (&d)[D]) {
      const double t = (w > 0.0) ? w * exp_nonpos(a - m, sExpTab) : 0.0;  // in S: a <= m
      c[0] += t;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        c[k + 1] = fma(d[k], t, c[k + 1]);
        const double u = d[k] * t;
#pragma unroll
        for (int l = k; l < D; ++l) c[1 + D + tri_index(D, k, l)] = fma(u, d[l], c[1 + D + tri_index(D, k, l)]);
      }
    });
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] += c[j];
  });
  if (at.q < pb.Nq) {
    const int64_t row = static_cast<int64_t>(pb.ngroups) * pb.Nq, o = at.grp * pb.Nq + at.q;
    pb.partial[o] = m;
#pragma unroll
    for (int j = 0; j < W; ++j) pb.partial[(j + 1) * row + o] = s[j];
  }
}

// One query of an item of dimension D.  The groups in group order: M = max m_g, S_j = sum_g s_jg exp(m_g - M); then
//   log p = M + log S_0 - log norm,  g_k = -S_k / (S_0 v_k),
//   H_kl  = fma(-g_k, g_l, S_kl / ((S_0 v_k) v_l) [- 1 / v_k if k == l])     (k <= l; both triangles store that one value)
//   -H = L L^T by Cholesky, column by column (pivot_j = -H_jj - sum_{i<j} L_ji^2 in ascending i); definite = every pivot
//   finite and > 0; then cov = L^-T L^-1 (k <= l, the products summed in ascending row), else all of cov NaN.
// No source in S: -Inf, 0, 0, definite 0, cov NaN.  A query with a NaN coordinate: NaN everywhere, definite 0.
template <int D>
__device__ __forceinline__ void curvature_finish_query(const CurvItem &it, int64_t q) {
  constexpr int T = tri_count(D), W = 1 + D + T;
  const int64_t row = static_cast<int64_t>(it.ngroups) * it.Nq;
  const double *pm = it.partial + q;
  double M = -INFINITY;
  for (int g = 0; g < it.ngroups; ++g) M = fmax(M, pm[static_cast<int64_t>(g) * it.Nq]);
  double S[W];
#pragma unroll
  for (int j = 0; j < W; ++j) S[j] = 0.0;
  const bool some = M > -INFINITY;
  if (some) {
    for (int g = 0; g < it.ngroups; ++g) {
      const double mg = pm[static_cast<int64_t>(g) * it.Nq];
      if (mg > -INFINITY) {
        const double e = exp(mg - M);
#pragma unroll
        for (int j = 0; j < W; ++j) S[j] += pm[(j + 1) * row + static_cast<int64_t>(g) * it.Nq] * e;
      }
    }
  }
  const bool bad = query_has_nan(it.qry, q, D);  // (the sweep drops a NaN: pair_sweep.hpp)
  const double nan = __builtin_nan("");
  double v[D], g[D], H[D][D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    v[k] = it.bw[k];
    g[k] = some ? -S[k + 1] / (S[0] * v[k]) : 0.0;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
#pragma unroll
    for (int l = k; l < D; ++l) {
      double h = 0.0;
      if (some) {
        h = S[1 + D + tri_index(D, k, l)] / ((S[0] * v[k]) * v[l]);
        if (k == l) h -= 1.0 / v[k];
        h = fma(-g[k], g[l], h);
      }
      H[k][l] = h;
      H[l][k] = h;
    }
  }
  if (it.logp) {
    double norm = it.norm0;
#pragma unroll
    for (int k = 0; k < D; ++k) norm *= __dsqrt_rn(v[k]);  // gauss_norm
    it.logp[q] = bad ? nan : some ? M + log(S[0]) - log(norm) : -INFINITY;
  }
  if (it.grad) {
#pragma unroll
    for (int k = 0; k < D; ++k) it.grad[q * D + k] = bad ? nan : g[k];
  }
  if (it.hess) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
      for (int l = 0; l < D; ++l) it.hess[(q * D + k) * D + l] = bad ? nan : H[k][l];
    }
  }
  if (!it.cov && !it.definite) return;
  // L in the lower triangle of A (A = -H), then its inverse in place of it
  double L[D][D];
  bool ok = some && !bad;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double p = -H[j][j];
#pragma unroll
    for (int i = 0; i < j; ++i) p = fma(-L[j][i], L[j][i], p);
    ok = ok && (p > 0.0) && (p < INFINITY);  // (a NaN pivot fails the first comparison)
    const double d = __dsqrt_rn(p);
    L[j][j] = d;
#pragma unroll
    for (int r = j + 1; r < D; ++r) {
      double a = -H[r][j];
#pragma unroll
      for (int i = 0; i < j; ++i) a = fma(-L[r][i], L[j][i], a);
      L[r][j] = a / d;
    }
  }
  if (it.definite) it.definite[q] = ok ? 1 : 0;
  if (!it.cov) return;
  double R[D][D];  // R = L^-1 (lower triangular), column by column: R_jj = 1 / L_jj, R_rj = -(sum_{i=j}^{r-1} L_ri R_ij) / L_rr
#pragma unroll
  for (int j = 0; j < D; ++j) {
    R[j][j] = 1.0 / L[j][j];
#pragma unroll
    for (int r = j + 1; r < D; ++r) {
      double a = 0.0;
#pragma unroll
      for (int i = j; i < r; ++i) a = fma(L[r][i], R[i][j], a);
      R[r][j] = -a / L[r][r];
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
#pragma unroll
    for (int l = k; l < D; ++l) {
      double c = 0.0;
#pragma unroll
      for (int r = l; r < D; ++r) c = fma(R[r][k], R[r][l], c);  // (L^-T L^-1)_kl, rows r >= max(k, l) = l
      c = ok ? c : nan;
      it.cov[(q * D + k) * D + l] = c;
      it.cov[(q * D + l) * D + k] = c;
    }
  }
}

// items [0, n), item i owns blocks [first[i], first[i+1]); the item's D is block-uniform
__global__ __launch_bounds__(kFinishThreads) void curvature_finish_kernel(const CurvItem *__restrict__ items,
                                                                        const int32_t *__restrict__ first, int n) {
  const ItemBlock ib = item_block(first, n);
  const CurvItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  if (q >= it.Nq) return;
  static_assert(KDEHIP_MAX_DIMS == 8, "one case per dimension count");
  switch (it.D) {
    case 1: curvature_finish_query<1>(it, q); break;
    case 2: curvature_finish_query<2>(it, q); break;
    case 3: curvature_finish_query<3>(it, q); break;
    case 4: curvature_finish_query<4>(it, q); break;
    case 5: curvature_finish_query<5>(it, q); break;
    case 6: curvature_finish_query<6>(it, q); break;
    case 7: curvature_finish_query<7>(it, q); break;
    case 8: curvature_finish_query<8>(it, q); break;
    default: break;
  }
}

// (CaptureScope, what a call does while its stream is being captured into a graph, is pair_sweep.hpp: mass.hip shares it)
// The run of one call (pair_sweep.hpp PairRun) with the moments' scratch, per item [partial | frozen | live], and its
// launches.  Protocol: fill `items` (evaluate items: sizes, D, logdom) and `circ` -> alloc(prefix bytes of caller data,
// result doubles of the caller, steps?) -> the caller writes its data into host() and points the items at dev() ->
// start(stream) (with steps: every item once more as a step item; the upload; the state cleared) -> sweep() any number of
// times, count() before the host reads live() -> close() (the evaluate items) -> wait(), defer(device) or keep(device).
class MomentRun : public PairRun<MomentItem> {
 public:
  int alloc(size_t prefix, size_t nresults, bool steps) {
    const size_t n = items.size();
    steps_ = steps;
    int64_t pblocks = 0, fblocks = 0;
    for (MomentItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      fblocks += it.nfb;
    }
    if (pblocks > INT32_MAX / 2 || fblocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many queries for one launch");
    if (steps) {  // the descriptors hold every item twice
      items.resize(2 * n);
      circ.resize(n, 0u);
      circ.resize(2 * n);
      for (size_t k = 0; k < n; ++k) circ[n + k] = circ[k];
    }
    own_ = nresults;
    Carve c;
    carve_head(c, prefix, 2, 0, nresults + (n + 1) / 2);  // first[] of the partial and of the finish kernels; the live counts
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) {
      const MomentItem &it = items[k];
      scratch[k] = c.take(sizeof(double) * (it.D + 2) * it.ngroups * it.Nq + sizeof(int32_t) * (it.Nq + it.nfb));
    }
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) {
      MomentItem &it = items[k];
      it.partial = reinterpret_cast<double *>(dev() + scratch[k]);
      it.frozen = reinterpret_cast<int32_t *>(it.partial + static_cast<int64_t>(it.D + 2) * it.ngroups * it.Nq);
      it.live = it.frozen + it.Nq;
      it.nlive = reinterpret_cast<int32_t *>(result(nresults)) + k;
      it.mode = kModeEvaluate;
    }
    nbase_ = n;
    return KDEHIP_OK;
  }
  const int32_t *host_live() const { return reinterpret_cast<const int32_t *>(host_result(own_)); }
  int start(hipStream_t st) {
    const size_t n = nbase_;
    if (steps_)
      for (size_t k = 0; k < n; ++k) {  // the step twin: x in place, log p to val, no gradient
        MomentItem &s = items[n + k];
        s = items[k];
        s.mode = kModeStep;
        s.grad = nullptr;
        s.logdom = 1;
      }
    // the step items first; by D; Euclidean items before circular ones
    prepare([&](size_t k) { return (items[k].mode == kModeStep ? 0 : 1024) + 2 * items[k].D + (circ[k] ? 1 : 0); });
    const size_t all = items.size();
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    for (size_t k = 0; k < all; ++k) ffirst[k + 1] = ffirst[k] + items[k].nfb;
    nsteps_ = steps_ ? n : 0;
    KDEHIP_CHECK(send(st));
    if (nsteps_ && ffirst[nsteps_] > 0) {
      hipLaunchKernelGGL(moments_init_kernel, dim3(static_cast<unsigned>(ffirst[nsteps_])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(1), static_cast<int>(nsteps_));
      KDEHIP_CHECK(hipGetLastError());
    }
    return KDEHIP_OK;
  }
  int sweep() { return pass(kModeStep, 0, nsteps_); }             // one mean-shift step of every live query
  int close() { return pass(kModeEvaluate, nsteps_, items.size()); }  // the evaluate items
  int count() {                                                   // the live counts, item by item
    if (!nsteps_) return KDEHIP_OK;
    hipLaunchKernelGGL(moments_live_kernel, dim3(static_cast<unsigned>((nsteps_ + 63) / 64)), dim3(64), 0, stream(), d_items(),
                       static_cast<int>(nsteps_));
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  // (blocking calls) count(), and the sum of the live counts on the host
  int live(int64_t *total) {
    KDEHIP_CHECK_RC(count());
    const hipStream_t st = stream();
    const size_t off = reinterpret_cast<unsigned char *>(result(own_)) - dev();
    KDEHIP_CHECK(hipMemcpyAsync(host() + off, dev() + off, sizeof(int32_t) * nbase_, hipMemcpyDeviceToHost, st));
    KDEHIP_CHECK(hipStreamSynchronize(st));
    *total = 0;
    for (size_t k = 0; k < nbase_; ++k) *total += host_live()[k];
    return KDEHIP_OK;
  }
  // (a captured call ends with keep(device), pair_sweep.hpp: the graph's nodes read and write the blocks at every replay)

 private:
  // the partial launches of the runs of `mode`, then ONE finish launch for its items [a, e)
  int pass(int32_t mode, size_t a, size_t e) {
    if (a >= e) return KDEHIP_OK;
    const hipStream_t st = stream();
    KDEHIP_CHECK_RC(for_each_run([&](const MomentItem &it, const MomentItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *d_masks) -> int {
      if (it.mode != mode) return KDEHIP_OK;
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<MomentItem>(moments_partial_kernel<kD, false>, moments_partial_kernel<kD, true>, blocks, st, d_it, d_pfirst,
                                cnt, d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    const int32_t *ffirst = first(1);
    if (ffirst[e] > ffirst[a]) {
      hipLaunchKernelGGL(moments_finish_kernel, dim3(static_cast<unsigned>(ffirst[e] - ffirst[a])), dim3(kFinishThreads), 0, st,
                         d_items() + a, d_first(1) + a, static_cast<int>(e - a), d_masks() + a);
      KDEHIP_CHECK(hipGetLastError());
    }
    return KDEHIP_OK;
  }
  bool steps_ = false;
  size_t nbase_ = 0, nsteps_ = 0, own_ = 0;
};

// The run of one curvature call: per item the scratch [2 + D + D(D+1)/2][ngroups][Nq].  Protocol: fill `items` (sizes, D)
// and `circ` -> alloc(prefix bytes of caller data, result doubles of the caller) -> point the items at their data ->
// start(stream) -> run() (one partial launch per distinct (D, circular), ONE finish launch) -> wait(), defer() or keep().
class CurvRun : public PairRun<CurvItem> {
 public:
  int alloc(size_t prefix, size_t nresults) {
    const size_t n = items.size();
    int64_t pblocks = 0, fblocks = 0;
    for (CurvItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      fblocks += it.nfb;
    }
    if (pblocks > INT32_MAX / 2 || fblocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many queries for one launch");
    Carve c;
    carve_head(c, prefix, 2, 0, nresults);  // first[] of the partial and of the finish kernel
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) scratch[k] = c.take(sizeof(double) * rows(items[k].D) * items[k].ngroups * items[k].Nq);
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) items[k].partial = reinterpret_cast<double *>(dev() + scratch[k]);
    return KDEHIP_OK;
  }
  int start(hipStream_t st) {
    prepare([&](size_t k) { return 2 * items[k].D + (circ[k] ? 1 : 0); });  // by D; Euclidean items before circular ones
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    for (size_t k = 0; k < items.size(); ++k) ffirst[k + 1] = ffirst[k] + items[k].nfb;
    KDEHIP_CHECK(send(st));
    return KDEHIP_OK;
  }
  int run() {
    const hipStream_t st = stream();
    KDEHIP_CHECK_RC(for_each_run([&](const CurvItem &it, const CurvItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *d_masks) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<CurvItem>(curvature_partial_kernel<kD, false>, curvature_partial_kernel<kD, true>, blocks, st, d_it, d_pfirst,
                              cnt, d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    const int32_t *ffirst = first(1);
    const size_t n = items.size();
    if (ffirst[n] > 0) {
      hipLaunchKernelGGL(curvature_finish_kernel, dim3(static_cast<unsigned>(ffirst[n])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(1), static_cast<int>(n));
      KDEHIP_CHECK(hipGetLastError());
    }
    return KDEHIP_OK;
  }

 private:
  static size_t rows(int D) { return static_cast<size_t>(2 + D + tri_count(D)); }
};

// ---- arguments ------------------------------------------------------------------------------------------------------------

const char kPositions[] = "pos must hold Nq >= 0 points", kDevicePositions[] = "d_pos must hold Nq >= 0 points";

int check_iteration(const double *tol, int maxiter) {
  if (!tol) return set_error(KDEHIP_ERR_ARG, "null argument");
  if (!(std::isfinite(*tol) && *tol >= 0.0)) return set_error(KDEHIP_ERR_ARG, "mean shift: tol must be finite and >= 0");
  if (maxiter < 0) return set_error(KDEHIP_ERR_ARG, "mean shift: the number of steps must be >= 0");
  return KDEHIP_OK;
}

int check_starts(const void *start, int64_t nstart, int64_t npts) {
  if (nstart < 0) return set_error(KDEHIP_ERR_ARG, "mean shift: nstart must be >= 0");
  if (!start && nstart != npts) return set_error(KDEHIP_ERR_ARG, "mean shift: start == NULL starts from the density's own points, nstart must be npts");
  return KDEHIP_OK;
}

MomentItem resident_item(const kdehip_device_density *bd, int64_t Nq, int logdom) {
  const LeafRows leaf = leaf_rows(bd);
  MomentItem it{};
  it.src = leaf.src; it.w = leaf.w; it.bw = leaf.bw; it.perm = leaf.perm;
  it.norm0 = gauss_norm0(bd->D);
  it.N = bd->N; it.Nq = Nq; it.D = bd->D; it.logdom = logdom ? 1 : 0;
  return it;
}

CurvItem resident_curv_item(const kdehip_device_density *bd, int64_t Nq) {
  const LeafRows leaf = leaf_rows(bd);
  CurvItem it{};
  it.src = leaf.src; it.w = leaf.w; it.bw = leaf.bw;
  it.norm0 = gauss_norm0(bd->D);
  it.N = bd->N; it.Nq = Nq; it.D = bd->D;
  return it;
}

// The rounds of a blocking mean shift: kRound sweeps (fewer at the end), then one look at the number of live starts.
int run_rounds(MomentRun &run, int maxiter) {
  for (int done = 0; done < maxiter;) {
    const int r = std::min(kRound, maxiter - done);
    for (int s = 0; s < r; ++s) KDEHIP_CHECK_RC(run.sweep());
    done += r;
    if (done >= maxiter) break;
    int64_t live = 0;
    KDEHIP_CHECK_RC(run.live(&live));
    if (live == 0) break;
  }
  return run.close();
}

// results of a blocking mean shift, in the run's result doubles: [x (Nq D) | logp (Nq) | iters (Nq int32)]
size_t shift_results(int64_t Nq, int D) { return static_cast<size_t>(Nq) * (D + 1) + static_cast<size_t>(Nq + 1) / 2; }
void point_shift_item(MomentRun &run, MomentItem &it) {
  it.x = run.result(0);
  it.qry = it.x;
  it.val = run.result(static_cast<size_t>(it.Nq) * it.D);
  it.iters = reinterpret_cast<int32_t *>(run.result(static_cast<size_t>(it.Nq) * (it.D + 1)));
}
void read_shift_results(const MomentRun &run, int64_t Nq, int D, double *x, double *logp, int32_t *iters) {
  std::memcpy(x, run.host_result(0), sizeof(double) * Nq * D);
  std::memcpy(logp, run.host_result(static_cast<size_t>(Nq) * D), sizeof(double) * Nq);
  std::memcpy(iters, run.host_result(static_cast<size_t>(Nq) * (D + 1)), sizeof(int32_t) * Nq);
}

}  // namespace

extern "C" int kdehip_evaluate_grad(const kdehip_density *bd, const double *pos, int64_t Nq, int log_domain, double *val,
                                    double *grad, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!bd || (!val && !grad)) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(pos, Nq, kPositions));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  // caller data: [the density | queries]; results: [val (Nq) | grad (Nq D)]
  const size_t o_q = host_density_bytes(bd), prefix = o_q + sizeof(double) * Nq * D;
  MomentRun run;
  MomentItem it{};
  it.norm0 = gauss_norm0(D);
  it.N = bd->npts; it.Nq = Nq; it.D = D; it.logdom = log_domain ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix, static_cast<size_t>(Nq) * (D + 1), false));
  MomentItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  std::memcpy(run.host() + o_q, pos, sizeof(double) * Nq * D);
  ri.qry = reinterpret_cast<const double *>(run.dev() + o_q);
  ri.val = val ? run.result(0) : nullptr;
  ri.grad = grad ? run.result(static_cast<size_t>(Nq)) : nullptr;
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.close());
  KDEHIP_CHECK_RC(run.wait());
  if (val) std::memcpy(val, run.host_result(0), sizeof(double) * Nq);
  if (grad) std::memcpy(grad, run.host_result(static_cast<size_t>(Nq)), sizeof(double) * Nq * D);
  return KDEHIP_OK;
}

extern "C" int kdehip_evaluate_grad_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int log_domain,
                                           double *d_val, double *d_grad, const uint8_t *manifold, void *stream) {
  if (!bd || (!d_val && !d_grad)) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(d_pos, Nq, kDevicePositions));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  MomentRun run;
  run.items.push_back(resident_item(bd, Nq, log_domain));
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0, 0, false));
  MomentItem &ri = run.items[0];
  ri.qry = d_pos;
  ri.val = d_val;
  ri.grad = d_grad;
  KDEHIP_CHECK_RC(run.start(static_cast<hipStream_t>(stream)));
  KDEHIP_CHECK_RC(run.close());
  return finish_enqueue(run, nullptr, bd->device);
}

extern "C" int kdehip_meanshift(const kdehip_density *bd, const double *start, int64_t nstart, const double *tol, int maxiter, double *x,
                                double *logp, int32_t *iters, int device, const uint8_t *manifold) {
  if (!bd || !x || !logp || !iters) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  const int64_t N = bd->npts;
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_starts(start, nstart, N));
  KDEHIP_CHECK_RC(check_iteration(tol, maxiter));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  if (nstart == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  // caller data: [the density | the starts, or the leaf row of the permutation]
  const size_t o_s = host_density_bytes(bd), prefix = o_s + (start ? sizeof(double) * nstart * D : sizeof(int64_t) * N);
  MomentRun run;
  MomentItem it{};
  it.norm0 = gauss_norm0(D);
  it.N = N; it.Nq = nstart; it.D = D; it.logdom = 1; it.tol = *tol;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix, shift_results(nstart, D), true));
  MomentItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  if (start) {
    std::memcpy(run.host() + o_s, start, sizeof(double) * nstart * D);
    ri.start = reinterpret_cast<const double *>(run.dev() + o_s);
  } else {
    std::memcpy(run.host() + o_s, bd->permutation + N, sizeof(int64_t) * N);
    ri.perm = reinterpret_cast<const int64_t *>(run.dev() + o_s);
  }
  point_shift_item(run, ri);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run_rounds(run, maxiter));
  KDEHIP_CHECK_RC(run.wait());
  read_shift_results(run, nstart, D, x, logp, iters);
  return KDEHIP_OK;
}

extern "C" int kdehip_meanshift_device(const kdehip_device_density *bd, const double *d_start, int64_t nstart, const double *tol,
                                       int maxiter, double *x, double *logp, int32_t *iters, const uint8_t *manifold) {
  if (!bd || !x || !logp || !iters) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_starts(d_start, nstart, bd->N));
  KDEHIP_CHECK_RC(check_iteration(tol, maxiter));
  if (nstart == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  MomentRun run;
  run.items.push_back(resident_item(bd, nstart, 1));
  run.items[0].tol = *tol;
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0, shift_results(nstart, bd->D), true));
  MomentItem &ri = run.items[0];
  ri.start = d_start;
  point_shift_item(run, ri);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run_rounds(run, maxiter));
  KDEHIP_CHECK_RC(run.wait());
  read_shift_results(run, nstart, bd->D, x, logp, iters);
  return KDEHIP_OK;
}

extern "C" int kdehip_meanshift_device_batch(int n, const kdehip_meanshift_item *items, const double *tol, int niter, void *stream) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "mean shift batch: "));
  KDEHIP_CHECK_RC(check_iteration(tol, niter));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_meanshift_item &m = items[i];
    KDEHIP_CHECK_RC(check_resident_density(m.bd, true));
    KDEHIP_CHECK_RC(check_same_device(m.bd, items[0].bd, "mean shift batch: "));
    KDEHIP_CHECK_RC(check_circular_mask(m.circular_mask, m.bd->D, "mean shift batch: "));
    KDEHIP_CHECK_RC(check_starts(m.d_start, m.nstart, m.bd->N));
    if (m.nstart > 0 && (!m.d_x || !m.d_logp || !m.d_iters)) return set_error(KDEHIP_ERR_ARG, "null argument");
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);
  MomentRun run;
  for (int i = 0; i < n; ++i) {
    if (items[i].nstart == 0) continue;
    run.items.push_back(resident_item(items[i].bd, items[i].nstart, 1));
    run.items.back().tol = *tol;
    run.circ.push_back(items[i].circular_mask);
  }
  if (run.items.empty()) return KDEHIP_OK;
  KDEHIP_CHECK_RC(run.alloc(0, 0, true));
  for (int i = 0, k = 0; i < n; ++i) {
    if (items[i].nstart == 0) continue;
    MomentItem &ri = run.items[k++];
    ri.start = items[i].d_start;
    ri.x = items[i].d_x;
    ri.qry = ri.x;
    ri.val = items[i].d_logp;
    ri.iters = items[i].d_iters;
  }
  KDEHIP_CHECK_RC(run.start(st));
  for (int s = 0; s < niter; ++s) KDEHIP_CHECK_RC(run.sweep());
  KDEHIP_CHECK_RC(run.close());
  return finish_enqueue(run, &scope, device);
}

extern "C" int kdehip_evaluate_hess(const kdehip_density *bd, const double *pos, int64_t Nq, double *logp, double *grad, double *hess,
                                    double *cov, int32_t *definite, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!bd || (!logp && !grad && !hess && !cov && !definite)) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(pos, Nq, kPositions));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  // caller data: [the density | queries]; results, those asked for only: [logp (Nq) | grad (Nq D) | hess (Nq D D) | cov (Nq D D) |
  // definite (Nq int32)]
  const size_t o_q = host_density_bytes(bd), prefix = o_q + sizeof(double) * Nq * D;
  const size_t n = static_cast<size_t>(Nq);
  size_t nres = 0;
  auto take = [&](bool asked, size_t doubles) { const size_t at = nres; if (asked) nres += doubles; return at; };
  const size_t r_logp = take(logp, n), r_grad = take(grad, n * D), r_hess = take(hess, n * D * D), r_cov = take(cov, n * D * D),
               r_def = take(definite, (n + 1) / 2);
  CurvRun run;
  CurvItem it{};
  it.norm0 = gauss_norm0(D);
  it.N = bd->npts; it.Nq = Nq; it.D = D;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix, nres));
  CurvItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  std::memcpy(run.host() + o_q, pos, sizeof(double) * Nq * D);
  ri.qry = reinterpret_cast<const double *>(run.dev() + o_q);
  ri.logp = logp ? run.result(r_logp) : nullptr;
  ri.grad = grad ? run.result(r_grad) : nullptr;
  ri.hess = hess ? run.result(r_hess) : nullptr;
  ri.cov = cov ? run.result(r_cov) : nullptr;
  ri.definite = definite ? reinterpret_cast<int32_t *>(run.result(r_def)) : nullptr;
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.run());
  KDEHIP_CHECK_RC(run.wait());
  if (logp) std::memcpy(logp, run.host_result(r_logp), sizeof(double) * n);
  if (grad) std::memcpy(grad, run.host_result(r_grad), sizeof(double) * n * D);
  if (hess) std::memcpy(hess, run.host_result(r_hess), sizeof(double) * n * D * D);
  if (cov) std::memcpy(cov, run.host_result(r_cov), sizeof(double) * n * D * D);
  if (definite) std::memcpy(definite, run.host_result(r_def), sizeof(int32_t) * n);
  return KDEHIP_OK;
}

extern "C" int kdehip_evaluate_hess_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, double *d_logp,
                                           double *d_grad, double *d_hess, double *d_cov, int32_t *d_definite,
                                           const uint8_t *manifold, void *stream) {
  if (!bd || (!d_logp && !d_grad && !d_hess && !d_cov && !d_definite)) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(d_pos, Nq, kDevicePositions));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  CurvRun run;
  run.items.push_back(resident_curv_item(bd, Nq));
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  CurvItem &ri = run.items[0];
  ri.qry = d_pos;
  ri.logp = d_logp; ri.grad = d_grad; ri.hess = d_hess; ri.cov = d_cov; ri.definite = d_definite;
  KDEHIP_CHECK_RC(run.start(static_cast<hipStream_t>(stream)));
  KDEHIP_CHECK_RC(run.run());
  return finish_enqueue(run, nullptr, bd->device);
}

extern "C" int kdehip_evaluate_hess_device_batch(int n, const kdehip_hess_item *items, void *stream) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "curvature batch: "));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_hess_item &h = items[i];
    KDEHIP_CHECK_RC(check_resident_density(h.bd, true));
    KDEHIP_CHECK_RC(check_same_device(h.bd, items[0].bd, "curvature batch: "));
    KDEHIP_CHECK_RC(check_circular_mask(h.circular_mask, h.bd->D, "curvature batch: "));
    KDEHIP_CHECK_RC(check_query_count(h.d_pos, h.Nq, kDevicePositions));
    if (!h.d_logp && !h.d_grad && !h.d_hess && !h.d_cov && !h.d_definite) return set_error(KDEHIP_ERR_ARG, "null argument");
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);
  CurvRun run;
  for (int i = 0; i < n; ++i) {
    const kdehip_hess_item &h = items[i];
    if (h.Nq == 0) continue;
    CurvItem it = resident_curv_item(h.bd, h.Nq);
    it.qry = h.d_pos;
    it.logp = h.d_logp; it.grad = h.d_grad; it.hess = h.d_hess; it.cov = h.d_cov; it.definite = h.d_definite;
    run.items.push_back(it);
    run.circ.push_back(h.circular_mask);
  }
  if (run.items.empty()) return KDEHIP_OK;
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  KDEHIP_CHECK_RC(run.start(st));
  KDEHIP_CHECK_RC(run.run());
  return finish_enqueue(run, &scope, device);
}
