// bwjoint.hip -- joint bandwidth selection: the leave-one-out likelihood maximised over the whole bandwidth vector by a
// fixed-point iteration (include/kdehip.h section 5q; no reference counterpart: kde!(points), src/KDE01.jl:17-24, searches
// every 1-D marginal on its own).  For a density with leaves c_i, weights w_i and a current variance vector v, with a_ij the
// exponent of pair_sweep.hpp between leaves i and j and d_ijk the differences it is formed from,
//   S_i  = { j : w_j > 0, j != i },  m_i = max_{S_i} a_ij,
//   S0_i = sum_{S_i} w_j exp(a_ij - m_i),  T_ik = sum_{S_i} w_j exp(a_ij - m_i) d_ijk^2,
//   Q    = { i : w_i > 0, S_i not empty },  W = sum_Q w_i,
//   L(v) = sum_{w_i > 0} w_i (m_i + log S0_i - log norm - log(1 - w_i))      (log-domain evalAvgLogL(bd, bd), section 5f)
//   v_new_k = (sum_Q w_i T_ik / S0_i) / W
// -- EM for a mixture with fixed centres and one shared diagonal covariance, so L(v_new) >= L(v).
// Host densities (uploaded for the call) and resident ones (single or batched) run ONE path, any number of items described
// in device memory by BwItem, each with a BwState in device memory that holds its current iterate, driven by BwRun:
//   bwjoint_init_kernel          items that start from the density's own bandwidth: its variances copied to the state;
//   bwjoint_partial_kernel<D>    one launch per distinct D (one more for its items with a circular dimension): the sweep of
//                                pair_sweep.hpp, the queries being the density's own leaves, with the two-pass step of
//                                moments_partial_kernel carrying (m, s_0, t_1..t_D) and the self term skipped by index;
//                                nhib is read from the STATE; scratch [D + 2][ngroups][N];
//   bwjoint_finish_kernel        one thread per leaf: the groups combined in group order, then the leaf's w_i log p_-i, its
//                                w_i if in Q and its w_i T_ik / S0_i summed over the block in a fixed tree: D + 2 values a block;
//   bwjoint_update_kernel        one block per item: the block shares in block order, L(v_t), v_new, the convergence test and
//                                the degenerate test; it writes the state and trace[t].
// An item's state goes 0 (stepping) -> 1 (the next sweep is the closing one: it only reads L at the final iterate) -> 2
// (finished: its blocks return at once and it is never written again).  No atomics.  The group split (split_chunks(N, N, 1))
// depends on the item's size alone, so an item's result depends on the density, the start, tol and maxiter alone: the host
// entry, the resident entry and any batch give the same bits, however the sweeps are grouped into rounds.
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

constexpr int kFinishThreads = kEvalThreads;  // leaves per finish block
constexpr int kUpdateThreads = 64;            // >= KDEHIP_MAX_DIMS + 2: one thread per column of the block shares
constexpr int kRound = 8;              // sweeps between two reads of the states (the round length changes no bit)

enum : int32_t { kStepping = 0, kClosing = 1, kFinished = 2 };

// The iterate of one item, in device memory: written by bwjoint_update_kernel (and bwjoint_init_kernel) alone.
struct BwState {
  double v[KDEHIP_MAX_DIMS];  // the current variances
  double logl;                // L at v, once finished
  int32_t iters;              // steps taken, negative while the last one was above tol
  int32_t done;               // kStepping, kClosing, kFinished
  int32_t status;             // 1: a step gave a variance that was 0 or not finite, the iteration froze
  int32_t pad_;
};
static_assert(sizeof(BwState) == 8 * (KDEHIP_MAX_DIMS + 3), "BwState layout");

// One item: a density (N leaves in leaf order) whose leaves are also the queries (qry == src, Nq == N).
struct BwItem : PairHead {
  const double *bw0;  // [D] the density's first leaf's variances: the start, or null (the host wrote the start to the state)
  BwState *state;
  double *trace;      // [maxiter + 1], or null
  double *partial;    // [D + 2][ngroups][N]: m, s_0, t_1..t_D
  double *bpart;      // [nfb][D + 2]: the finish blocks' shares of L, W and the D numerators
  double norm0, tol;
  int32_t ngroups, nfb, D, maxiter;
};

// one thread per item
__global__ void bwjoint_init_kernel(const BwItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const BwItem it = items[i];
  if (!it.bw0) return;
  for (int k = 0; k < it.D; ++k) it.state->v[k] = it.bw0[k];
}

// partial[0][g][i] = m, partial[1][g][i] = s_0, partial[2 + k][g][i] = t_{k+1} of leaf i over the source chunks of group g in
// chunk order, as moments_partial_kernel words it: per staged chunk, pass one takes the chunk's maximum of a_ij over S_i, the
// carried sums are rescaled ONCE by exp_nonpos(m_old - m_new), pass two adds e = w_j exp_nonpos(a_ij - m) to s_0 and
// (e d_k) d_k to t_k (one exp per pair); the self term enters both passes with weight 0, which keeps their loops free of a
// second condition.  A group with S_i empty leaves (-Inf, 0, ..).  The variances are the STATE's (the
// read is block-uniform); the blocks of a finished item return at once.
// CIRC as in evaluate.hip: data in which no difference wraps gives the bits of the Euclidean instantiation.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void bwjoint_partial_kernel(const BwItem *__restrict__ items,
                                                                       const int32_t *__restrict__ first, int n,
                                                                       const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const BwItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;        // block-uniform
  if (pb.state->done == kFinished) return;   // block-uniform, before any barrier
  double nhib[D];  // -1/(2 v_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.state->v[k];
  // leave-one-out by INDEX (a duplicate of leaf i is in S_i); N < 2^31 (BwRun::alloc), so the low words decide
  const uint32_t skip = static_cast<uint32_t>(at.q);
  double m = -INFINITY, s[D + 1];
#pragma unroll
  for (int j = 0; j <= D; ++j) s[j] = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t i, double w, double a) {
      const double ws = (static_cast<uint32_t>(i) == skip) ? 0.0 : w;  // (the self term counts as weightless)
      cm = (ws > 0.0) ? fmax(cm, a) : cm;
    });
    if (cm > m) {  // (m == -Inf: the sums are still 0)
      const double r = exp_nonpos(m - cm, sExpTab);
#pragma unroll
      for (int j = 0; j <= D; ++j) s[j] *= r;
      m = cm;
    }
    double c[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) c[j] = 0.0;
    each([&](int64_t i, double w, double a, const double (&d)[D]) {
      const double ws = (static_cast<uint32_t>(i) == skip) ? 0.0 : w;
      const double e = (ws > 0.0) ? ws * exp_nonpos(a - m, sExpTab) : 0.0;  // in S_i: a <= m
      c[0] += e;
#pragma unroll
      for (int k = 0; k < D; ++k) c[k + 1] = fma(e * d[k], d[k], c[k + 1]);
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

// Items [0, n), item i owns blocks [first[i], first[i+1]).  Per leaf q the groups in group order: M = max m_g,
// S0 = sum_g s_0g exp(m_g - M), T_k likewise; log p_-q = M + log S0 - log norm - log(1 - w_q), -Inf with S_q empty, NaN for a
// leaf with a NaN coordinate.  bpart[block] = [ sum w_q log p_-q over w_q > 0 (-Inf if one of them is -Inf: evalAvgLogL, 5f) |
// sum_Q w_q | sum_Q w_q T_k / S0, k = 0..D-1 ], each summed over the block in the fixed tree of block_tree_sum.
__global__ __launch_bounds__(kFinishThreads) void bwjoint_finish_kernel(const BwItem *__restrict__ items,
                                                                      const int32_t *__restrict__ first, int n) {
  __shared__ double red[KDEHIP_MAX_DIMS + 2][kFinishThreads];
  const ItemBlock ib = item_block(first, n);
  const BwItem it = items[ib.item];
  if (it.state->done == kFinished) return;  // block-uniform, before any barrier
  const int D = it.D;
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  double term[KDEHIP_MAX_DIMS + 2];
  for (int j = 0; j < D + 2; ++j) term[j] = 0.0;
  int zero = 0;
  if (q < it.Nq && it.w[q] > 0.0) {
    const double wq = it.w[q];
    const int64_t row = static_cast<int64_t>(it.ngroups) * it.Nq;
    const double *pm = it.partial + q;
    double M = -INFINITY;
    for (int g = 0; g < it.ngroups; ++g) M = fmax(M, pm[static_cast<int64_t>(g) * it.Nq]);
    if (M > -INFINITY) {
      double S[KDEHIP_MAX_DIMS + 1];
      for (int j = 0; j <= D; ++j) S[j] = 0.0;
      for (int g = 0; g < it.ngroups; ++g) {
        const double mg = pm[static_cast<int64_t>(g) * it.Nq];
        if (mg > -INFINITY) {
          const double e = exp(mg - M);
          for (int j = 0; j <= D; ++j) S[j] += pm[(j + 1) * row + static_cast<int64_t>(g) * it.Nq] * e;
        }
      }
      const double lognorm = log(gauss_norm(it.norm0, D, [&](int k) { return it.state->v[k]; }));
      double lp = M + log(S[0]) - lognorm - log(1.0 - wq);
      if (query_has_nan(it.qry, q, D)) lp = __builtin_nan("");  // (the sweep drops a NaN: pair_sweep.hpp)
      term[0] = wq * lp;
      term[1] = wq;
      for (int k = 0; k < D; ++k) term[2 + k] = wq * S[k + 1] / S[0];
    } else {
      zero = 1;  // a weighted leaf with no other weighted leaf: L = -Inf
    }
  }
  const int anyzero = __syncthreads_or(zero);
  // the D + 2 columns through the tree of block_tree_sum (halving strides) together: one barrier a stride for all of them
  for (int j = 0; j < D + 2; ++j) red[j][threadIdx.x] = term[j];  // (D is block-uniform)
  __syncthreads();
  for (int off = kFinishThreads / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off)
      for (int j = 0; j < D + 2; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + off];
    __syncthreads();
  }
  const int j = threadIdx.x;
  if (j < D + 2) it.bpart[static_cast<int64_t>(ib.k) * (D + 2) + j] = (j == 0 && anyzero) ? -INFINITY : red[j][0];
}

// One block per item.  Thread j sums column j of the block shares in block order; thread 0 then takes the item one state on:
//   L = L(v_t), t = |iters|: trace[t] = L;
//   closing:  logl = L, finished;
//   stepping: v_new_k = numerator_k / W.  One of them 0 or not finite: status = 1, logl = L, finished, nothing else changes.
//             Else v = v_new, one more step counted, negative while max_k |log(v_new_k / v_k)| / 2 > tol; at convergence or
//             with maxiter steps taken the next sweep is the closing one.
__global__ __launch_bounds__(kUpdateThreads) void bwjoint_update_kernel(const BwItem *__restrict__ items) {
  __shared__ double sum[KDEHIP_MAX_DIMS + 2];
  const BwItem it = items[blockIdx.x];
  BwState *st = it.state;
  if (st->done == kFinished) return;  // block-uniform, before the barrier
  const int D = it.D;
  if (static_cast<int>(threadIdx.x) < D + 2) {
    double s = 0.0;
    for (int b = 0; b < it.nfb; ++b) s += it.bpart[static_cast<int64_t>(b) * (D + 2) + threadIdx.x];
    sum[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double L = sum[0], W = sum[1];
  const int32_t t = abs(st->iters);
  if (it.trace) it.trace[t] = L;
  if (st->done == kClosing) {
    st->logl = L;
    st->done = kFinished;
    return;
  }
  double vn[KDEHIP_MAX_DIMS];
  bool ok = true;
  double reach = 0.0;
  for (int k = 0; k < D; ++k) {
    vn[k] = sum[2 + k] / W;
    ok = ok && vn[k] > 0.0 && vn[k] < INFINITY;  // (a NaN fails the first comparison)
    reach = fmax(reach, 0.5 * fabs(log(vn[k] / st->v[k])));
  }
  if (!ok) {
    st->status = 1;
    st->logl = L;
    st->done = kFinished;
    return;
  }
  for (int k = 0; k < D; ++k) st->v[k] = vn[k];
  const int32_t cnt = t + 1;
  const bool conv = reach <= it.tol;
  st->iters = conv ? cnt : -cnt;
  st->done = (conv || cnt >= it.maxiter) ? kClosing : kStepping;
}

// The run of one call (pair_sweep.hpp PairRun): the states in the run's own part of the block (they go up with their
// starts), per item the scratch [partial | block shares], the traces in the results.  Protocol: add() every item ->
// alloc(prefix bytes of caller data) -> the caller points the items at their data and writes the starts (state()) ->
// start() -> rounds() -> wait(); then state(k) and trace(k) hold the answers of the item added k-th (an item keeps the
// state and the trace it was given in alloc(), wherever start()'s sort moves its descriptor).
class BwRun : public PairRun<BwItem> {
 public:
  std::vector<char> traced;   // per item: it asks for a trace
  int add(const BwItem &it, uint32_t mask, bool trace) {
    items.push_back(it);
    circ.push_back(mask);
    traced.push_back(trace ? 1 : 0);
    return static_cast<int>(items.size()) - 1;
  }
  int alloc(size_t prefix, int maxiter) {
    const size_t n = items.size();
    n_ = n;
    int64_t pblocks = 0, fblocks = 0;
    for (BwItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      fblocks += it.nfb;
    }
    for (const BwItem &it : items)  // (the partial kernel compares the low 32 bits of the leaf indices)
      if (it.N > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many points for one launch");
    if (pblocks > INT32_MAX / 2 || fblocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many points for one launch");
    size_t ntrace = 0;
    std::vector<size_t> o_trace(n);
    for (size_t k = 0; k < n; ++k) {
      o_trace[k] = ntrace;
      if (traced[k]) ntrace += static_cast<size_t>(maxiter) + 1;
    }
    Carve c;
    o_state_ = carve_head(c, prefix, 2, sizeof(BwState) * n, ntrace);  // first[] of the partial and of the finish kernel
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) {
      const BwItem &it = items[k];
      scratch[k] = c.take(sizeof(double) * (it.D + 2) * (static_cast<size_t>(it.ngroups) * it.Nq + it.nfb));
    }
    KDEHIP_CHECK(alloc_block(c));
    o_trace_ = o_trace;
    for (size_t k = 0; k < n; ++k) {
      BwItem &it = items[k];
      it.partial = reinterpret_cast<double *>(dev() + scratch[k]);
      it.bpart = it.partial + static_cast<int64_t>(it.D + 2) * it.ngroups * it.Nq;
      it.state = reinterpret_cast<BwState *>(dev() + o_state_) + k;
      it.trace = traced[k] ? result(o_trace[k]) : nullptr;
      it.maxiter = maxiter;
      BwState &s = state(k);
      s = BwState{};
      s.done = maxiter == 0 ? kClosing : kStepping;
    }
    maxiter_ = maxiter;
    return KDEHIP_OK;
  }
  BwState &state(size_t k) const { return reinterpret_cast<BwState *>(host() + o_state_)[k]; }
  const double *trace(size_t k) const { return host_result(o_trace_[k]); }
  int start(hipStream_t st) {
    bool init = false;
    for (const BwItem &it : items) init = init || it.bw0;
    prepare([&](size_t k) { return 2 * items[k].D + (circ[k] ? 1 : 0); });  // by D; Euclidean items before circular ones
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    for (size_t k = 0; k < n_; ++k) ffirst[k + 1] = ffirst[k] + items[k].nfb;
    KDEHIP_CHECK(send(st));
    if (init) {
      hipLaunchKernelGGL(bwjoint_init_kernel, dim3(static_cast<unsigned>((n_ + 63) / 64)), dim3(64), 0, st, d_items(), static_cast<int>(n_));
      KDEHIP_CHECK(hipGetLastError());
    }
    return KDEHIP_OK;
  }
  // one sweep of every item that is not finished: the partial launches, ONE finish launch, ONE update launch
  int sweep() {
    const hipStream_t st = stream();
    KDEHIP_CHECK_RC(for_each_run([&](const BwItem &it, const BwItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *d_masks) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<BwItem>(bwjoint_partial_kernel<kD, false>, bwjoint_partial_kernel<kD, true>, blocks, st, d_it, d_pfirst, cnt,
                            d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    const int32_t *ffirst = first(1);
    if (ffirst[n_] > 0) {
      hipLaunchKernelGGL(bwjoint_finish_kernel, dim3(static_cast<unsigned>(ffirst[n_])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(1), static_cast<int>(n_));
      KDEHIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(bwjoint_update_kernel, dim3(static_cast<unsigned>(n_)), dim3(kUpdateThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  // The rounds of a call: `round` sweeps (fewer at the end), then one read of the states.  An item takes at most maxiter
  // step sweeps and the closing one, so after maxiter + 1 sweeps every item is finished and the last read has its answer.
  int rounds(int round) {
    const int64_t total = static_cast<int64_t>(maxiter_) + 1;
    for (int64_t swept = 0; swept < total;) {
      const int64_t r = std::min<int64_t>(round, total - swept);
      for (int64_t s = 0; s < r; ++s) KDEHIP_CHECK_RC(sweep());
      swept += r;
      const hipStream_t st = stream();
      KDEHIP_CHECK(hipMemcpyAsync(host() + o_state_, dev() + o_state_, sizeof(BwState) * n_, hipMemcpyDeviceToHost, st));
      KDEHIP_CHECK(hipStreamSynchronize(st));
      bool live = false;
      for (size_t k = 0; k < n_; ++k) live = live || state(k).done != kFinished;
      if (!live) break;
    }
    return KDEHIP_OK;
  }

 private:
  size_t n_ = 0, o_state_ = 0;
  int maxiter_ = 0;
  std::vector<size_t> o_trace_;
};

// ---- arguments ------------------------------------------------------------------------------------------------------------

int check_bw_iteration(const double *tol, int maxiter) {
  if (!tol) return set_error(KDEHIP_ERR_ARG, "null argument");
  if (!(std::isfinite(*tol) && *tol >= 0.0)) return set_error(KDEHIP_ERR_ARG, "joint bandwidth: tol must be finite and >= 0");
  if (maxiter < 0) return set_error(KDEHIP_ERR_ARG, "joint bandwidth: the number of steps must be >= 0");
  return KDEHIP_OK;
}

// D standard deviations whose squares are finite and > 0, or NULL
int check_bw_start(const double *start, int D) {
  if (!start) return KDEHIP_OK;
  for (int k = 0; k < D; ++k) {
    const double v = start[k] * start[k];
    if (!(std::isfinite(start[k]) && start[k] > 0.0 && std::isfinite(v) && v > 0.0))
      return set_error(KDEHIP_ERR_ARG, "joint bandwidth: every start entry must be finite and > 0");
  }
  return KDEHIP_OK;
}

int check_bw_size(int64_t npts) {
  if (npts < 2) return set_error(KDEHIP_ERR_ARG, "joint bandwidth: the density must have at least two points");
  return KDEHIP_OK;
}

BwItem bw_item(int64_t N, int D, double tol) {
  BwItem it{};
  it.norm0 = gauss_norm0(D);
  it.N = N; it.Nq = N; it.D = D; it.tol = tol;
  return it;
}

BwItem resident_bw_item(const kdehip_device_density *bd, double tol) {
  const LeafRows leaf = leaf_rows(bd);
  BwItem it = bw_item(bd->N, bd->D, tol);
  it.src = leaf.src; it.w = leaf.w; it.qry = leaf.src; it.bw0 = leaf.bw;
  return it;
}

// the start of item k: the squares of the caller's standard deviations (bw0 is then not read)
void write_start(BwRun &run, size_t k, const double *start) {
  if (!start) return;
  BwItem &it = run.items[k];
  it.bw0 = nullptr;
  for (int d = 0; d < it.D; ++d) run.state(k).v[d] = start[d] * start[d];
}

void read_answer(const BwRun &run, size_t k, int D, double *bw_out, double *logl, int32_t *iters, int32_t *status, double *trace) {
  const BwState &s = run.state(k);
  for (int d = 0; d < D; ++d) bw_out[d] = std::sqrt(s.v[d]);
  *logl = s.logl;
  *iters = s.iters;
  *status = s.status;
  if (trace) std::memcpy(trace, run.trace(k), sizeof(double) * (static_cast<size_t>(std::abs(s.iters)) + 1));
}

}  // namespace

extern "C" int kdehip_bandwidth_joint(const kdehip_density *bd, const double *start, const double *tol, int maxiter, double *bw_out,
                                      double *logl, int32_t *iters, int32_t *status, double *trace, int device,
                                      const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!bd || !bw_out || !logl || !iters || !status) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  const int64_t N = bd->npts;
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_bw_iteration(tol, maxiter));
  KDEHIP_CHECK_RC(check_bw_size(N));
  KDEHIP_CHECK_RC(check_bw_start(start, D));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  BwRun run;  // caller data: [the density]
  run.add(bw_item(N, D, *tol), circ, trace != nullptr);
  KDEHIP_CHECK_RC(run.alloc(host_density_bytes(bd), maxiter));
  BwItem &ri = run.items[0];
  ri.bw0 = pack_host_density(run, ri, bd);
  ri.qry = ri.src;
  write_start(run, 0, start);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.rounds(kRound));
  KDEHIP_CHECK_RC(run.wait());
  read_answer(run, 0, D, bw_out, logl, iters, status, trace);
  return KDEHIP_OK;
}

extern "C" int kdehip_bandwidth_joint_device(const kdehip_device_density *bd, const double *start, const double *tol, int maxiter,
                                             double *bw_out, double *logl, int32_t *iters, int32_t *status, double *trace,
                                             const uint8_t *manifold) {
  if (!bd || !bw_out || !logl || !iters || !status) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, false));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_bw_iteration(tol, maxiter));
  KDEHIP_CHECK_RC(check_bw_size(bd->N));
  KDEHIP_CHECK_RC(check_bw_start(start, bd->D));
  KDEHIP_CHECK_RC(check_resident_density(bd, true));
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  BwRun run;
  run.add(resident_bw_item(bd, *tol), circ, trace != nullptr);
  KDEHIP_CHECK_RC(run.alloc(0, maxiter));
  write_start(run, 0, start);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.rounds(kRound));
  KDEHIP_CHECK_RC(run.wait());
  read_answer(run, 0, bd->D, bw_out, logl, iters, status, trace);
  return KDEHIP_OK;
}

extern "C" int kdehip_bandwidth_joint_device_batch(int n, const kdehip_bwjoint_item *items, const double *tol, int maxiter) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "joint bandwidth batch: "));
  KDEHIP_CHECK_RC(check_bw_iteration(tol, maxiter));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_bwjoint_item &b = items[i];
    if (!b.bd || !b.bw_out || !b.logl || !b.iters || !b.status) return set_error(KDEHIP_ERR_ARG, "null argument");
    KDEHIP_CHECK_RC(check_resident_density(b.bd, false));
    KDEHIP_CHECK_RC(check_same_device(b.bd, items[0].bd, "joint bandwidth batch: "));
    KDEHIP_CHECK_RC(check_circular_mask(b.circular_mask, b.bd->D, "joint bandwidth batch: "));
    KDEHIP_CHECK_RC(check_bw_size(b.bd->N));
    KDEHIP_CHECK_RC(check_bw_start(b.start, b.bd->D));
    KDEHIP_CHECK_RC(check_resident_density(b.bd, true));
  }
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(items[0].bd->device));
  BwRun run;
  for (int i = 0; i < n; ++i) run.add(resident_bw_item(items[i].bd, *tol), items[i].circular_mask, false);
  KDEHIP_CHECK_RC(run.alloc(0, maxiter));
  for (int i = 0; i < n; ++i) write_start(run, i, items[i].start);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.rounds(kRound));
  KDEHIP_CHECK_RC(run.wait());
  for (int i = 0; i < n; ++i)
    read_answer(run, i, items[i].bd->D, items[i].bw_out, items[i].logl, items[i].iters, items[i].status, nullptr);
  return KDEHIP_OK;
}
