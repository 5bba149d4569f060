// sinkhorn.hip -- entropic optimal transport between two densities by Sinkhorn's iteration in the log domain, and the
// barycentric map of the plan it reaches (include/kdehip.h section 5s; no reference counterpart).  With x_i, a_i the leaves
// and weights of p (N of them), y_j, b_j those of q (M), a positive scale vector s, eps = reg and
//   A_ij = -c_ij / eps = sum_k diff_k(x_i, y_j)^2 * nhib[k],  nhib[k] = -1 / (2 eps s_k^2)   (the exponent of pair_sweep.hpp)
// the potentials are kept divided by eps (phi_i, gamma_j) and a half-step is a log-sum-exp over all pairs,
//   T_x(gamma)_i = -LSE_{j : b_j > 0} (log b_j + gamma_j + A_ij),
// the sweep of eval_partial_log_kernel with ONE extra number per source: log b_j + gamma_j (-Inf for a weightless leaf) rides
// in the slot where pair_sweep stages the weight -- PairHead.w points at it; pair_sweep itself is what it was.
// Any number of items described in device memory by OtItem, each with an OtState, driven by OtRun as bwjoint.hip drives its
// fixed point:
//   ot_init_kernel            phi = gamma = 0, la_phi = log a, lb_gam = log b; the default scale v_p + v_q to the state;
//   ot_partial_kernel<D>      one launch per distinct D per half-step (one more for the items with a circular dimension):
//                             `side` 0 has p's leaves as queries and q's as sources, side 1 the roles exchanged (a self item
//                             idles there); the running maximum and the rescaled sum of evaluate_log; scratch [2][ngroups][Nq];
//   ot_finish_kernel          one thread per query: the groups in group order; side 0: tau, r = exp(phi - tau) and the shares
//                             of err, mass and sum a phi; side 1: gamma = T_y(phi), lb_gam and the share of sum b gamma; each
//                             share summed over the block in a fixed tree;
//   ot_update_kernel          one block per item: the block shares in block order; side 0 makes the stop decision and either
//                             freezes the item with the potentials whose err it has just read, or adopts tau (a self item:
//                             the average) into phi / la_phi; side 1 counts the step;
//   ot_map_kernel<D>          once, when every item has stopped: the sweep with the step that takes the differences, carrying
//                             (m, s_0, sum e d_k, sum e A); ot_map_finish_kernel: m_i = the barycentric displacement, the
//                             share of <pi, c>, and the outputs in their orders; ot_close_kernel sums the shares.
// No atomics.  The group split (split_chunks of the two sizes with one problem) depends on the item's sizes alone, so an
// item's bits depend on the two densities, scale, reg, tol and maxiter alone: the host entry, the resident entry and any
// batch give the same bits, however the iterations are grouped into rounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "density_args.hpp"
#include "device_density.hpp"
#include "entry_helpers.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"
#include "manifold_arg.hpp"
#include "pair_sweep.hpp"

using namespace kdehip;

namespace {

constexpr int kFinishThreads = kEvalThreads;  // queries per finish block
constexpr int kUpdateThreads = 256;
constexpr int kShares = 5;   // err, mass, sum a phi, leaves of positive weight, queries without a source
constexpr int kRound = 8;    // iterations between two reads of the states (the round length changes no bit)

enum : int32_t { kStepping = 0, kFinished = 1 };

// The state of one item, in device memory: written by ot_init_kernel, ot_update_kernel and ot_close_kernel alone.
struct OtState {
  double v[KDEHIP_MAX_DIMS];  // s_k^2
  double err, mass, sap, sbg, cost, value;
  int32_t steps, done, iters, status;  // status 1: a side has no leaf of positive weight
};
static_assert(sizeof(OtState) == 8 * (KDEHIP_MAX_DIMS + 8), "OtState layout");

// One item.  The head describes side 0: src = q's leaves (N of them), w = lb_gam, qry = p's leaves (Nq).  A self item has
// q = p throughout: src == qry, b == a, gamma == phi and lb_gam == la_phi are the same arrays.
struct OtItem : PairHead {
  const double *a, *b;             // [Nq], [N] the weights
  double *phi, *gamma;             // [Nq], [N] leaf order
  double *la_phi, *lb_gam;         // log a + phi, log b + gamma: -Inf for a weightless leaf
  double *tau;                     // [Nq] T_x of the current half-step
  OtState *state;
  double *partial;                 // stepping: [2][groups][queries] of the side; map: [D + 3][ngroups][Nq]
  double *bpart;                   // [max(nfb, nfb_y)][kShares]
  const double *bwp, *bwq;         // the two densities' variances: the default scale; null with a scale from the caller
  const int64_t *perm_p, *perm_q;  // leaf -> original point (1-based), or null: outputs in leaf order
  double *phi_out, *gamma_out, *delta_out, *map_out;  // or null; delta_out [Nq][D] is ALWAYS in leaf order
  double eps, tol;
  int64_t cpg_y;                   // chunks_per_group of side 1
  int32_t ngroups, ngroups_y, nfb, nfb_y, D, maxiter, self, pad_;
};

// the head of side 1: the roles exchanged
__device__ __forceinline__ PairHead side_head(const OtItem &it, int side) {
  PairHead h = it;
  if (side) {
    h.src = it.qry; h.w = it.la_phi; h.qry = it.src;
    h.N = it.Nq; h.Nq = it.N; h.chunks_per_group = it.cpg_y;
  }
  return h;
}

__device__ __forceinline__ double log_weight(double w, double pot) { return w > 0.0 ? log(w) + pot : -INFINITY; }

// one block per item, strided over its leaves
__global__ __launch_bounds__(kUpdateThreads) void ot_init_kernel(const OtItem *__restrict__ items) {
  const OtItem it = items[blockIdx.x];
  if (threadIdx.x == 0 && it.bwp)
    for (int k = 0; k < it.D; ++k) it.state->v[k] = it.bwp[k] + it.bwq[k];
  for (int64_t i = threadIdx.x; i < it.Nq; i += kUpdateThreads) {
    it.phi[i] = 0.0;
    it.la_phi[i] = log_weight(it.a[i], 0.0);
  }
  if (it.self) return;
  for (int64_t j = threadIdx.x; j < it.N; j += kUpdateThreads) {
    it.gamma[j] = 0.0;
    it.lb_gam[j] = log_weight(it.b[j], 0.0);
  }
}

template <int D>
__device__ __forceinline__ void load_nhib(const OtItem &it, double (&nhib)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -1.0 / (2.0 * it.eps * it.state->v[k]);
}

// partial[g][q] = m, partial[groups + g][q] = s of query q over the source chunks of group g in chunk order, as
// eval_partial_log_kernel words it with t_j = l_j + A_qj in the place of a_i, l_j the staged value: per staged chunk, pass
// one takes the chunk's maximum of t over S = { j : l_j > -Inf }, the carried sum is rescaled ONCE by
// exp_nonpos(m_old - m_new), pass two adds exp_nonpos(t - m).  A group with S empty leaves (-Inf, 0).  The blocks of a
// finished item, and on side 1 those of a self item (it has none), return at once, before any barrier.
// CIRC as in evaluate.hip: data in which no difference wraps gives the bits of the Euclidean instantiation.
template <int D, bool CIRC, int SIDE>
__global__ __launch_bounds__(kEvalThreads) void ot_partial_kernel(const OtItem *__restrict__ items,
                                                                  const int32_t *__restrict__ first, int n,
                                                                  const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const OtItem it = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairHead pb = side_head(it, SIDE);
  const int64_t groups = SIDE ? it.ngroups_y : it.ngroups;
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;          // block-uniform
  if (it.state->done == kFinished) return;     // block-uniform, before any barrier
  double nhib[D];
  load_nhib<D>(it, nhib);
  double m = -INFINITY, total = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t, double l, double a) { cm = (l > -INFINITY) ? fmax(cm, l + a) : cm; });
    if (cm > m) {  // (m == -Inf: total is still 0)
      total *= exp_nonpos(m - cm, sExpTab);
      m = cm;
    }
    double sum = 0.0;
    each([&](int64_t, double l, double a) { sum += (l > -INFINITY) ? exp_nonpos((l + a) - m, sExpTab) : 0.0; });
    total += sum;
  });
  if (at.q < pb.Nq) {
    it.partial[at.grp * pb.Nq + at.q] = m;
    it.partial[(groups + at.grp) * pb.Nq + at.q] = total;
  }
}

// -LSE of query q from the groups' (m, s) in group order: M = max m_g, S = sum s_g exp(m_g - M); +Inf when no group has a source
__device__ __forceinline__ double neg_lse(const double *partial, int64_t groups, int64_t Nq, int64_t q) {
  double M = -INFINITY;
  for (int64_t g = 0; g < groups; ++g) M = fmax(M, partial[g * Nq + q]);
  if (!(M > -INFINITY)) return INFINITY;
  double S = 0.0;
  for (int64_t g = 0; g < groups; ++g) {
    const double mg = partial[g * Nq + q];
    if (mg > -INFINITY) S += partial[(groups + g) * Nq + q] * exp(mg - M);
  }
  return -(M + log(S));
}

// the kShares columns of a block through the tree of block_tree_sum (halving strides) together; thread j < kShares writes
// column j of the block's row
__device__ __forceinline__ void block_shares(const double (&term)[kShares], double (*red)[kFinishThreads], double *row) {
  for (int j = 0; j < kShares; ++j) red[j][threadIdx.x] = term[j];
  __syncthreads();
  for (int off = kFinishThreads / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off)
      for (int j = 0; j < kShares; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < kShares) row[threadIdx.x] = red[threadIdx.x][0];
}

// Items [0, n), item i owns blocks [first[i], first[i+1]) of its side.  Side 0, query i: tau_i = T_x(gamma)_i is kept,
// r_i = exp(phi_i - tau_i); bpart[block] = [ sum a_i |r_i - 1| | sum a_i r_i | sum a_i phi_i | leaves with a_i > 0 | queries
// that found no source ], the sums over a_i > 0.  Side 1, query j: gamma_j = T_y(phi)_j and lb_gam_j are WRITTEN (this half
// never stops an item); bpart[block] = [ sum b_j gamma_j over b_j > 0 | 0 .. ].
template <int SIDE>
__global__ __launch_bounds__(kFinishThreads) void ot_finish_kernel(const OtItem *__restrict__ items,
                                                                 const int32_t *__restrict__ first, int n) {
  __shared__ double red[kShares][kFinishThreads];
  const ItemBlock ib = item_block(first, n);
  const OtItem it = items[ib.item];
  if (it.state->done == kFinished) return;  // block-uniform, before any barrier
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  double term[kShares] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (SIDE == 0) {
    if (q < it.Nq) {
      const double tau = neg_lse(it.partial, it.ngroups, it.Nq, q);
      it.tau[q] = tau;
      const double aq = it.a[q];
      if (!(tau < INFINITY)) term[4] = 1.0;
      if (aq > 0.0) {
        const double ph = it.phi[q], r = exp(ph - tau);
        term[0] = aq * fabs(r - 1.0);
        term[1] = aq * r;
        term[2] = aq * ph;
        term[3] = 1.0;
      }
    }
  } else {
    if (q < it.N) {
      const double g = neg_lse(it.partial, it.ngroups_y, it.N, q);
      const double bq = it.b[q];
      it.gamma[q] = g;
      it.lb_gam[q] = log_weight(bq, g);
      if (bq > 0.0) term[0] = bq * g;
    }
  }
  block_shares(term, red, it.bpart + static_cast<int64_t>(ib.k) * kShares);
}

// One block per item.  Thread j sums column j of the block shares in block order.
// Side 0: err, mass and sum a phi at the current (phi, gamma).  (steps >= 1 and err <= tol) or steps == maxiter: the item is
// finished with THESE potentials -- nothing is adopted on the stopping pass.  Otherwise phi = tau (a self item:
// (phi + tau) / 2, one more step counted) and la_phi follows.  A side without a leaf of positive weight: status = 1, finished.
// Side 1 (cross items): sum b gamma is kept and one more step counted.
template <int SIDE>
__global__ __launch_bounds__(kUpdateThreads) void ot_update_kernel(const OtItem *__restrict__ items) {
  __shared__ double sum[kShares];
  const OtItem it = items[blockIdx.x];
  OtState *st = it.state;
  if (st->done == kFinished) return;  // block-uniform, before the barrier
  if (SIDE == 1 && it.self) return;
  const int nfb = SIDE ? it.nfb_y : it.nfb;
  if (threadIdx.x < kShares) {
    double s = 0.0;
    for (int b = 0; b < nfb; ++b) s += it.bpart[static_cast<int64_t>(b) * kShares + threadIdx.x];
    sum[threadIdx.x] = s;
  }
  const int32_t steps = st->steps;  // (read by every thread before thread 0 may write it)
  __syncthreads();
  if (SIDE == 1) {
    if (threadIdx.x == 0) {
      st->sbg = sum[0];
      st->steps = steps + 1;
    }
    return;
  }
  const double err = sum[0], mass = sum[1], sap = sum[2];
  const bool empty = !(sum[3] > 0.0) || sum[4] > 0.0;
  const bool conv = err <= it.tol;
  const bool stop = empty || (steps >= 1 && conv) || steps >= it.maxiter;
  if (stop) {
    if (threadIdx.x == 0) {
      const double sbg = it.self ? sap : st->sbg;
      st->err = err; st->mass = mass; st->sap = sap; st->sbg = sbg;
      st->value = it.eps * (sap + sbg - (mass - 1.0));
      st->iters = conv ? steps : -steps;
      st->status = empty ? 1 : 0;
      st->done = kFinished;
    }
    return;
  }
  for (int64_t i = threadIdx.x; i < it.Nq; i += kUpdateThreads) {
    const double ph = it.self ? 0.5 * (it.phi[i] + it.tau[i]) : it.tau[i];
    it.phi[i] = ph;
    it.la_phi[i] = log_weight(it.a[i], ph);
  }
  if (it.self && threadIdx.x == 0) st->steps = steps + 1;
}

// The map pass of a stopped item, side 0: partial[0] = m, [1] = s_0 = sum e, [2 + k] = sum e d_k (d_k = diff_k(x_i, y_j), the
// values A_ij was formed from), [D + 2] = sum e A_ij, with e = exp_nonpos(t - m) over S as in ot_partial_kernel; the carried
// sums are rescaled once per chunk.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void ot_map_kernel(const OtItem *__restrict__ items, const int32_t *__restrict__ first,
                                                              int n, const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const OtItem it = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(it, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double nhib[D];
  load_nhib<D>(it, nhib);
  double m = -INFINITY, s[D + 2];
#pragma unroll
  for (int j = 0; j < D + 2; ++j) s[j] = 0.0;
  pair_sweep<D, CIRC>(it, at, circ, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t, double l, double a) { cm = (l > -INFINITY) ? fmax(cm, l + a) : cm; });
    if (cm > m) {
      const double r = exp_nonpos(m - cm, sExpTab);
#pragma unroll
      for (int j = 0; j < D + 2; ++j) s[j] *= r;
      m = cm;
    }
    double c[D + 2];
#pragma unroll
    for (int j = 0; j < D + 2; ++j) c[j] = 0.0;
    each([&](int64_t, double l, double a, const double (&d)[D]) {
      const double e = (l > -INFINITY) ? exp_nonpos((l + a) - m, sExpTab) : 0.0;
      c[0] += e;
#pragma unroll
      for (int k = 0; k < D; ++k) c[k + 1] = fma(e, d[k], c[k + 1]);
      c[D + 1] = fma(e, a, c[D + 1]);
    });
#pragma unroll
    for (int j = 0; j < D + 2; ++j) s[j] += c[j];
  });
  if (at.q < it.Nq) {
    const int64_t row = static_cast<int64_t>(it.ngroups) * it.Nq, o = at.grp * it.Nq + at.q;
    it.partial[o] = m;
#pragma unroll
    for (int j = 0; j < D + 2; ++j) it.partial[(j + 1) * row + o] = s[j];
  }
}

// One thread per leaf i of p.  The groups in group order: M, S_0, S_k, S_A.  m_ik = -S_k / S_0 is the barycentric
// displacement (diff(y_j, x_i) = -d_k); the leaf's share of <pi, c> is a_i r_i (-eps S_A / S_0), r_i = exp(phi_i + M + log S_0),
// summed over the block into bpart[block][0].  Outputs: delta_out[i][k] = m_ik in LEAF order; map_out, phi_out through the
// permutation (column-major D x N by original point); a self item's gamma_out is its phi.
__global__ __launch_bounds__(kFinishThreads) void ot_map_finish_kernel(const OtItem *__restrict__ items,
                                                                     const int32_t *__restrict__ first, int n,
                                                                     const uint32_t *__restrict__ masks) {
  __shared__ double red[kFinishThreads];
  const ItemBlock ib = item_block(first, n);
  const OtItem it = items[ib.item];
  const unsigned circ = masks[ib.item];
  const int D = it.D;
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  double share = 0.0;
  if (q < it.Nq) {
    const int64_t row = static_cast<int64_t>(it.ngroups) * it.Nq;
    const double *pm = it.partial + q;
    double M = -INFINITY;
    for (int g = 0; g < it.ngroups; ++g) M = fmax(M, pm[static_cast<int64_t>(g) * it.Nq]);
    double S[KDEHIP_MAX_DIMS + 2];
    for (int j = 0; j < D + 2; ++j) S[j] = 0.0;
    for (int g = 0; g < it.ngroups; ++g) {
      const double mg = pm[static_cast<int64_t>(g) * it.Nq];
      if (mg > -INFINITY) {
        const double e = exp(mg - M);
        for (int j = 0; j < D + 2; ++j) S[j] += pm[(j + 1) * row + static_cast<int64_t>(g) * it.Nq] * e;
      }
    }
    const int64_t o = it.perm_p ? it.perm_p[q] - 1 : q;
    const bool there = o >= 0 && o < it.Nq;  // (an uploaded density's permutation is the caller's)
    for (int k = 0; k < D; ++k) {
      const double mk = -S[k + 1] / S[0];
      if (it.delta_out) it.delta_out[q * D + k] = mk;
      if (it.map_out && there) {
        double t = it.qry[q * D + k] + mk;
        if ((circ >> k) & 1u) t = circ_wrap(t);
        it.map_out[o * D + k] = t;
      }
    }
    const double ph = it.phi[q], aq = it.a[q];
    if (aq > 0.0) share = aq * exp(ph + M + log(S[0])) * (-it.eps * (S[D + 1] / S[0]));
    if (it.phi_out && there) it.phi_out[o] = ph;
    if (it.self && it.gamma_out && there) it.gamma_out[o] = ph;
  }
  red[threadIdx.x] = share;
  __syncthreads();
  const double total = block_tree_sum<kFinishThreads>(red);
  if (threadIdx.x == 0) it.bpart[static_cast<int64_t>(ib.k) * kShares] = total;
}

// a cross item's gamma through q's permutation: one thread per leaf of q, over the blocks of side 1's finish
__global__ __launch_bounds__(kFinishThreads) void ot_gamma_out_kernel(const OtItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n) {
  const ItemBlock ib = item_block(first, n);
  const OtItem it = items[ib.item];
  const int64_t j = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  if (!it.gamma_out || j >= it.N) return;
  const int64_t o = it.perm_q ? it.perm_q[j] - 1 : j;
  if (o >= 0 && o < it.N) it.gamma_out[o] = it.gamma[j];
}

// one thread per item: <pi, c> from the map's block shares in block order
__global__ void ot_close_kernel(const OtItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const OtItem it = items[i];
  double s = 0.0;
  for (int b = 0; b < it.nfb; ++b) s += it.bpart[static_cast<int64_t>(b) * kShares];
  it.state->cost = s;
}

// The run of one call (pair_sweep.hpp PairRun).  The block: [caller's data | descriptors | four first[] arrays, masks |
// states | results | per item: phi, gamma, la_phi, lb_gam, tau, partial, block shares].  first[0] / first[1]: the sweep and
// the finish blocks of side 0, first[2] / first[3] those of side 1 (a self item has none).
// Protocol: add() every item -> alloc(prefix bytes, result doubles) -> the caller points the items at their data and
// outputs and writes the scales (state()) -> start() -> rounds() -> wait(); then state(k) holds the answer of the item added k-th.
class OtRun : public PairRun<OtItem> {
 public:
  int add(const OtItem &it, uint32_t mask) {
    items.push_back(it);
    circ.push_back(mask);
    return static_cast<int>(items.size()) - 1;
  }
  int alloc(size_t prefix, size_t nresults) {
    const size_t n = items.size();
    n_ = n;
    int64_t blocks = 0;
    for (OtItem &it : items) {
      blocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      it.cpg_y = 0; it.ngroups_y = 0; it.nfb_y = 0;
      if (!it.self) {
        const GroupSplit gs = split_chunks(it.Nq, it.N, 1);
        it.cpg_y = gs.chunks_per_group;
        it.ngroups_y = gs.ngroups;
        it.nfb_y = static_cast<int32_t>((it.N + kFinishThreads - 1) / kFinishThreads);
        blocks += sweep_blocks_y(it);
      }
      blocks += it.nfb + it.nfb_y;
    }
    if (blocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many points for one launch");
    Carve c;
    o_state_ = carve_head(c, prefix, 4, sizeof(OtState) * n, nresults);
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) scratch[k] = c.take(sizeof(double) * scratch_doubles(items[k]));
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) {
      OtItem &it = items[k];
      double *p = reinterpret_cast<double *>(dev() + scratch[k]);
      it.phi = p; p += it.Nq;
      it.la_phi = p; p += it.Nq;
      it.tau = p; p += it.Nq;
      if (it.self) { it.gamma = it.phi; it.lb_gam = it.la_phi; }
      else { it.gamma = p; p += it.N; it.lb_gam = p; p += it.N; }
      it.w = it.lb_gam;
      it.bpart = p; p += static_cast<int64_t>(std::max(it.nfb, it.nfb_y)) * kShares;
      it.partial = p;
      it.state = reinterpret_cast<OtState *>(dev() + o_state_) + k;
      state(k) = OtState{};
    }
    return KDEHIP_OK;
  }
  OtState &state(size_t k) const { return reinterpret_cast<OtState *>(host() + o_state_)[k]; }
  int start(hipStream_t st) {
    maxiter_ = 0;
    for (const OtItem &it : items) maxiter_ = std::max(maxiter_, it.maxiter);
    prepare([&](size_t k) { return 2 * items[k].D + (circ[k] ? 1 : 0); });  // by D; Euclidean items before circular ones
    keys_.resize(n_);
    for (size_t k = 0; k < n_; ++k) keys_[k] = 2 * items[k].D + (circ[k] ? 1 : 0);
    int32_t *f1 = first(1), *f2 = first(2), *f3 = first(3);
    f1[0] = f2[0] = f3[0] = 0;
    for (size_t k = 0; k < n_; ++k) {
      f1[k + 1] = f1[k] + items[k].nfb;
      f2[k + 1] = f2[k] + static_cast<int32_t>(sweep_blocks_y(items[k]));
      f3[k + 1] = f3[k] + items[k].nfb_y;
    }
    KDEHIP_CHECK(send(st));
    hipLaunchKernelGGL(ot_init_kernel, dim3(static_cast<unsigned>(n_)), dim3(kUpdateThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  // The rounds of a call: `round` iterations (fewer at the end), then one read of the states.  An item stops at the latest in
  // the first half of iteration maxiter + 1; when all have stopped, the map pass and the last read.
  int rounds(int round) {
    const int64_t total = static_cast<int64_t>(maxiter_) + 1;
    for (int64_t done = 0; done < total;) {
      const int64_t r = std::min<int64_t>(round, total - done);
      for (int64_t s = 0; s < r; ++s) KDEHIP_CHECK_RC(iteration());
      done += r;
      KDEHIP_CHECK_RC(read_states());
      bool live = false;
      for (size_t k = 0; k < n_; ++k) live = live || state(k).done != kFinished;
      if (!live) break;
    }
    KDEHIP_CHECK_RC(map_pass());
    return read_states();
  }

 private:
  static int64_t sweep_blocks_y(const OtItem &it) { return ((it.N + kEvalThreads - 1) / kEvalThreads) * it.ngroups_y; }
  static size_t scratch_doubles(const OtItem &it) {
    const size_t step_x = 2 * static_cast<size_t>(it.ngroups) * it.Nq, step_y = 2 * static_cast<size_t>(it.ngroups_y) * it.N;
    const size_t map = static_cast<size_t>(it.D + 3) * it.ngroups * it.Nq;
    return 3 * static_cast<size_t>(it.Nq) + (it.self ? 0 : 2 * static_cast<size_t>(it.N)) +
           static_cast<size_t>(std::max(it.nfb, it.nfb_y)) * kShares + std::max(map, std::max(step_x, step_y));
  }
  // launch(D, items of the run, its first[], count, blocks, its masks or null) per run of equal key, on the blocks of first[which]
  template <typename Launch>
  int for_runs(int which, Launch launch) {
    const int32_t *f = first(which);
    for (size_t a = 0; a < n_;) {
      size_t e = a;
      while (e < n_ && keys_[e] == keys_[a]) ++e;
      const int blocks = f[e] - f[a];
      if (blocks > 0) {
        KDEHIP_CHECK_RC(launch(items[a].D, d_items() + a, d_first(which) + a, static_cast<int>(e - a), blocks,
                               circ[a] ? d_masks() + a : nullptr));
        KDEHIP_CHECK(hipGetLastError());
      }
      a = e;
    }
    return KDEHIP_OK;
  }
  template <int SIDE>
  int half_step() {
    const hipStream_t st = stream();
    KDEHIP_CHECK_RC(for_runs(SIDE ? 2 : 0, [&](int D, const OtItem *d_it, const int32_t *d_f, int cnt, int blocks,
                                               const uint32_t *d_m) -> int {
      return dispatch_dims(D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<OtItem>(ot_partial_kernel<kD, false, SIDE>, ot_partial_kernel<kD, true, SIDE>, blocks, st, d_it, d_f, cnt, d_m);
      });
    }));
    const int32_t *ff = first(SIDE ? 3 : 1);
    if (ff[n_] == 0) return KDEHIP_OK;  // (side 1 of a run of self items)
    hipLaunchKernelGGL(ot_finish_kernel<SIDE>, dim3(static_cast<unsigned>(ff[n_])), dim3(kFinishThreads), 0, st, d_items(),
                       d_first(SIDE ? 3 : 1), static_cast<int>(n_));
    KDEHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ot_update_kernel<SIDE>, dim3(static_cast<unsigned>(n_)), dim3(kUpdateThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  int iteration() {
    KDEHIP_CHECK_RC(half_step<0>());
    return half_step<1>();
  }
  int map_pass() {
    const hipStream_t st = stream();
    KDEHIP_CHECK_RC(for_runs(0, [&](int D, const OtItem *d_it, const int32_t *d_f, int cnt, int blocks, const uint32_t *d_m) -> int {
      return dispatch_dims(D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<OtItem>(ot_map_kernel<kD, false>, ot_map_kernel<kD, true>, blocks, st, d_it, d_f, cnt, d_m);
      });
    }));
    hipLaunchKernelGGL(ot_map_finish_kernel, dim3(static_cast<unsigned>(first(1)[n_])), dim3(kFinishThreads), 0, st, d_items(),
                       d_first(1), static_cast<int>(n_), d_masks());
    KDEHIP_CHECK(hipGetLastError());
    if (first(3)[n_] > 0) {
      hipLaunchKernelGGL(ot_gamma_out_kernel, dim3(static_cast<unsigned>(first(3)[n_])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(3), static_cast<int>(n_));
      KDEHIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ot_close_kernel, dim3(static_cast<unsigned>((n_ + 63) / 64)), dim3(64), 0, st, d_items(), static_cast<int>(n_));
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  int read_states() {
    const hipStream_t st = stream();
    KDEHIP_CHECK(hipMemcpyAsync(host() + o_state_, dev() + o_state_, sizeof(OtState) * n_, hipMemcpyDeviceToHost, st));
    KDEHIP_CHECK(hipStreamSynchronize(st));
    return KDEHIP_OK;
  }

  size_t n_ = 0, o_state_ = 0;
  int maxiter_ = 0;
  std::vector<int> keys_;
};

// ---- arguments ------------------------------------------------------------------------------------------------------------

constexpr char kWords[] = "sinkhorn: ";
static_assert(sizeof(kdehip_sinkhorn_item) == 136, "kdehip_sinkhorn_item layout (_lib.CSinkhornItem mirrors it)");

int check_ot_numbers(const double *scale, int D, double reg, double tol, int maxiter) {
  if (!(std::isfinite(reg) && reg > 0.0)) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "reg must be finite and > 0");
  if (scale)
    for (int k = 0; k < D; ++k) {
      const double v = scale[k] * scale[k];
      if (!(std::isfinite(scale[k]) && scale[k] > 0.0 && std::isfinite(v) && v > 0.0))
        return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "every scale entry must be finite and > 0");
    }
  if (!(tol >= 0.0)) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "tol must be >= 0");
  if (maxiter < 0) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "maxiter must be >= 0");
  return KDEHIP_OK;
}

int check_ot_dims(int64_t Dp, int64_t Dq) {
  if (Dp != Dq) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "the two densities must have the same ndims");
  if (Dp < 1 || Dp > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "ndims outside 1..KDEHIP_MAX_DIMS");
  return KDEHIP_OK;
}

int check_ot_sizes(int64_t N, int64_t M) {
  if (N > INT32_MAX || M > INT32_MAX) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "a density has 2^31 points or more");
  return KDEHIP_OK;
}

int no_weight() { return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "a density has no leaf of positive weight"); }

bool has_positive_weight(const double *w, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (w[i] > 0.0) return true;
  return false;
}

// p's leaves are the queries of side 0, q's its sources
OtItem ot_item(int64_t N, int64_t M, int D, double reg, double tol, int maxiter, bool self) {
  OtItem it{};
  it.Nq = N; it.N = M; it.D = D; it.eps = reg; it.tol = tol; it.maxiter = maxiter; it.self = self ? 1 : 0;
  return it;
}

// sp, sq: the densities whose variances give the default scale (p and q, or those a batch item names), or null
OtItem resident_ot_item(const kdehip_device_density *p, const kdehip_device_density *q, double reg, double tol, int maxiter,
                        const kdehip_device_density *sp, const kdehip_device_density *sq) {
  const LeafRows lp = leaf_rows(p), lq = leaf_rows(q);
  OtItem it = ot_item(p->N, q->N, p->D, reg, tol, maxiter, p == q);
  it.qry = lp.src; it.a = lp.w; it.perm_p = lp.perm;
  it.src = lq.src; it.b = lq.w; it.perm_q = lq.perm;
  if (sp) { it.bwp = leaf_rows(sp).bw; it.bwq = leaf_rows(sq).bw; }
  return it;
}

// the scale of item k from the caller: the squares of its entries (the densities' bandwidths are then not read)
void write_scale(OtRun &run, size_t k, const double *scale) {
  if (!scale) return;
  OtItem &it = run.items[k];
  it.bwp = it.bwq = nullptr;
  for (int d = 0; d < it.D; ++d) run.state(k).v[d] = scale[d] * scale[d];
}

struct OtAnswer { double *value, *cost, *err, *mass; int32_t *iters; };

int read_answer(const OtRun &run, size_t k, const OtAnswer &o) {
  const OtState &s = run.state(k);
  if (s.status) return no_weight();
  *o.value = s.value; *o.cost = s.cost; *o.err = s.err; *o.mass = s.mass; *o.iters = s.iters;
  return KDEHIP_OK;
}

// sp, sq: where the default scale comes from when `scale` is null
int check_resident_pair(const kdehip_device_density *p, const kdehip_device_density *q, const double *scale, double reg, double tol,
                        int maxiter, const kdehip_device_density *first, const kdehip_device_density *sp,
                        const kdehip_device_density *sq) {
  if (!p || !q) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_ot_dims(p->D, q->D));
  KDEHIP_CHECK_RC(check_ot_numbers(scale, p->D, reg, tol, maxiter));
  KDEHIP_CHECK_RC(check_ot_sizes(p->N, q->N));
  if (p->device != q->device || p->device != first->device)
    return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "densities on different devices");
  if (scale) return KDEHIP_OK;
  if (sp->D != p->D || sq->D != p->D) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "the scale's densities must have the items' ndims");
  if (sp->device != p->device || sq->device != p->device)
    return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "densities on different devices");
  if (!(leaves_share_bandwidth(sp) && leaves_share_bandwidth(sq)))
    return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "a density with per-point bandwidths needs an explicit scale");
  return KDEHIP_OK;
}

}  // namespace

extern "C" int kdehip_sinkhorn(const kdehip_density *p, const kdehip_density *q, const double *scale, const double *reg_p,
                               const double *tol_p, int maxiter, double *value, double *transport_cost, double *err, double *mass, int32_t *iters,
                               double *phi, double *gamma, double *delta, double *map, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!p || !q || !reg_p || !tol_p || !value || !transport_cost || !err || !mass || !iters)
    return set_error(KDEHIP_ERR_ARG, "null argument");
  const double reg = *reg_p, tol = *tol_p;
  KDEHIP_CHECK_RC(check_ot_dims(p->ndim, q->ndim));
  KDEHIP_CHECK_RC(check_host_density(p));
  KDEHIP_CHECK_RC(check_host_density(q));
  const int D = static_cast<int>(p->ndim);
  const int64_t N = p->npts, M = q->npts;
  const bool self = p == q;
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_ot_numbers(scale, D, reg, tol, maxiter));
  KDEHIP_CHECK_RC(check_ot_sizes(N, M));
  if (!has_positive_weight(p->weights + N, N) || !has_positive_weight(q->weights + M, M)) return no_weight();
  if (!scale && (check_one_bandwidth(p, kOneBandwidth) != KDEHIP_OK || check_one_bandwidth(q, kOneBandwidth) != KDEHIP_OK))
    return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "a density with per-point bandwidths needs an explicit scale");
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  OtRun run;  // caller data: [p: means | weights | bw][q: the same], results: [phi | gamma | delta | map] in leaf order
  run.add(ot_item(N, M, D, reg, tol, maxiter, self), circ);
  const size_t bytes_p = align256(host_density_bytes(p)), bytes_q = self ? 0 : align256(host_density_bytes(q));
  const size_t o_phi = 0, o_gamma = o_phi + N, o_delta = o_gamma + M, o_map = o_delta + static_cast<size_t>(N) * D;
  KDEHIP_CHECK_RC(run.alloc(bytes_p + bytes_q, o_map + static_cast<size_t>(N) * D));
  OtItem &it = run.items[0];
  auto pack = [&](const kdehip_density *bd, size_t at, const double *&pts, const double *&w, const double *&bw) {
    const LeafArrays la = pack_leaves(run, at, bd);
    const size_t o_bw = at + sizeof(double) * bd->npts * (D + 1);
    std::memcpy(run.host() + o_bw, bd->bandwidth + bd->npts * D, sizeof(double) * D);
    pts = la.means; w = la.weights; bw = reinterpret_cast<const double *>(run.dev() + o_bw);
  };
  pack(p, 0, it.qry, it.a, it.bwp);
  if (self) { it.src = it.qry; it.b = it.a; it.bwq = it.bwp; }
  else pack(q, bytes_p, it.src, it.b, it.bwq);
  it.phi_out = run.result(o_phi); it.gamma_out = run.result(o_gamma);
  it.delta_out = run.result(o_delta); it.map_out = run.result(o_map);
  write_scale(run, 0, scale);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.rounds(kRound));
  KDEHIP_CHECK_RC(run.wait());
  KDEHIP_CHECK_RC(read_answer(run, 0, {value, transport_cost, err, mass, iters}));
  // leaf order -> the order of getPoints / getWeights
  const int64_t *pp = p->permutation + N, *pq = q->permutation + M;
  for (int64_t i = 0; i < N; ++i) {
    const int64_t o = pp[i] - 1;
    if (o < 0 || o >= N) continue;
    if (phi) phi[o] = run.host_result(o_phi)[i];
    for (int k = 0; k < D; ++k) {
      if (delta) delta[o * D + k] = run.host_result(o_delta)[i * D + k];
      if (map) map[o * D + k] = run.host_result(o_map)[i * D + k];
    }
  }
  if (gamma)
    for (int64_t j = 0; j < M; ++j) {
      const int64_t o = pq[j] - 1;
      if (o >= 0 && o < M) gamma[o] = run.host_result(o_gamma)[j];
    }
  return KDEHIP_OK;
}

extern "C" int kdehip_sinkhorn_device(const kdehip_device_density *p, const kdehip_device_density *q, const double *scale,
                                      const double *reg_p, const double *tol_p, int maxiter, double *value, double *transport_cost, double *err, double *mass,
                                      int32_t *iters, double *d_phi, double *d_gamma, double *d_delta, double *d_map,
                                      const uint8_t *manifold) {
  if (!p || !q || !reg_p || !tol_p || !value || !transport_cost || !err || !mass || !iters)
    return set_error(KDEHIP_ERR_ARG, "null argument");
  const double reg = *reg_p, tol = *tol_p;
  KDEHIP_CHECK_RC(check_resident_pair(p, q, scale, reg, tol, maxiter, p, p, q));
  uint32_t circ = 0;
  if (manifold_arg(manifold, p->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(p->device));
  OtRun run;
  run.add(resident_ot_item(p, q, reg, tol, maxiter, scale ? nullptr : p, q), circ);
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  OtItem &it = run.items[0];
  it.phi_out = d_phi; it.gamma_out = d_gamma; it.delta_out = d_delta; it.map_out = d_map;
  write_scale(run, 0, scale);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.rounds(kRound));
  KDEHIP_CHECK_RC(run.wait());
  return read_answer(run, 0, {value, transport_cost, err, mass, iters});
}

extern "C" int kdehip_sinkhorn_device_batch(int n, const kdehip_sinkhorn_item *items) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "sinkhorn batch: "));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_sinkhorn_item &b = items[i];
    if (!b.p || !b.q || !b.value || !b.transport_cost || !b.err || !b.mass || !b.iters) return set_error(KDEHIP_ERR_ARG, "null argument");
    if ((b.scale_p == nullptr) != (b.scale_q == nullptr)) return set_error(KDEHIP_ERR_ARG, "sinkhorn batch: scale_p and scale_q go together");
    KDEHIP_CHECK_RC(check_resident_pair(b.p, b.q, b.scale, b.reg, b.tol, b.maxiter, items[0].p, b.scale_p ? b.scale_p : b.p,
                                        b.scale_q ? b.scale_q : b.q));
    KDEHIP_CHECK_RC(check_circular_mask(b.circular_mask, b.p->D, "sinkhorn batch: "));
  }
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(items[0].p->device));
  OtRun run;
  for (int i = 0; i < n; ++i) {
    const kdehip_sinkhorn_item &b = items[i];
    run.add(resident_ot_item(b.p, b.q, b.reg, b.tol, b.maxiter, b.scale ? nullptr : (b.scale_p ? b.scale_p : b.p),
                             b.scale_q ? b.scale_q : b.q),
            b.circular_mask);
  }
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  for (int i = 0; i < n; ++i) {
    OtItem &it = run.items[i];
    it.phi_out = items[i].d_phi; it.gamma_out = items[i].d_gamma; it.delta_out = items[i].d_delta; it.map_out = items[i].d_map;
    write_scale(run, i, items[i].scale);
  }
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.rounds(kRound));
  KDEHIP_CHECK_RC(run.wait());
  for (int i = 0; i < n; ++i)
    KDEHIP_CHECK_RC(read_answer(run, i, {items[i].value, items[i].transport_cost, items[i].err, items[i].mass, items[i].iters}));
  return KDEHIP_OK;
}
