// evaluate.hip -- direct KDE evaluation and log-likelihoods on gfx950 (include/kdehip.h sections 5, 5b).
//
// Replaces, for the default configuration of the reference (FORCE_EVAL_DIRECT = true,
// src/KernelDensityEstimate.jl:54, so `evaluate` always ends in `evalDirect`):
//   evaluateDualTree(bd, pos) / bd(pos)         src/DualTree01.jl:370-446 -> evaluate :303-346 -> evalDirect :130-162
//   evalAvgLogL(bd1, bd2)                       src/DualTree01.jl:450-470 = sum_q W_q log p_q with p = bd1 at bd2's points
//                                               (leave-one-out when bd1 === bd2) and W = bd2's weights; a p_q == 0 with
//                                               W_q != 0 makes it -Inf
// for host densities (arrays in and out, blocking) and for resident ones (enqueue-only, single or batched).  ONE path serves
// all of them: any number of items (a density, a set of query points, what to compute) of any sizes, described in device
// memory by EvalItem and driven by EvalRun:
//   eval_partial_kernel<D>  one launch per distinct D (one more for its items with a circular dimension): the all-pairs
//                           Gaussian sum of pair_sweep.hpp, one partial sum per (group of source chunks, query);
//   eval_finish_kernel      the groups summed in a fixed order (deterministic, no atomics), / norm, / (1 - w) for
//                           leave-one-out, the value stored (through the item's permutation, if any) when asked for, then
//                           W_q log p_q and the block's share in a fixed LDS tree; a weighted zero raises the block's flag
//                           instead of adding -Inf; a query with a NaN coordinate gets NaN;
//   logl_reduce_kernel      only when an item asks for a log-likelihood: per item, the block shares summed in block order
//                           (or -Inf if a flag is up) into one double.
// Log-domain items (kdehip.h section 5f: log p by log-sum-exp, finite where p underflows) run eval_partial_log_kernel<D> and
// eval_finish_log_kernel in launches of their own, with the same sweep, split and reduction.
// Evaluation within a tolerance (kdehip.h section 5m: kdehip_evaluate_tol, kdehip_evaluate_device_at_tol) is the same run
// with the three passes of evaltol.hip in the place of eval_partial_kernel; the finish kernel does not know the difference.
// The group split (split_chunks(N, Nq, 1)) depends on the item's (N, Nq) alone, so nothing depends on the launch or the
// batch: the host entry, a single device call and any batch give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "density_args.hpp"
#include "device_density.hpp"
#include "entry_helpers.hpp"
#include "evaltol.hpp"
#include "manifold_arg.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"
#include "pair_sweep.hpp"
#include "phase_timer.hpp"

using namespace kdehip;

namespace {

// (kEvalThreads, kEvalChunk and split_chunks, the mapping of the all-pairs sum, are in entry_helpers.hpp; the sum itself is
// pair_sweep.hpp: ksum.hip shares them)
constexpr int kFinishThreads = 256;  // queries per finish block

// One evaluation: a density (N source points in tree / leaf order, one bandwidth vector) at Nq query points.
struct EvalItem : PairHead {
  const double *bw;     // [D] the density's first leaf's variances (every leaf has them: checked on the host)
  const double *qw;     // [Nq] query weights (the `at` density's leaf weights), or null: no log-likelihood
  const int64_t *perm;  // [Nq] 1-based output position of query q, or null: query order
  double *out;          // [Nq] p, or null
  double *partial;      // [ngroups][Nq]
  double *bpart;        // [nfb] the finish blocks' shares of sum W log p
  int32_t *bzero;       // [nfb] the finish block met a p == 0 with W != 0
  double *logl;         // the result, or null
  double norm0;         // (2 pi)^(D/2) as the host's libm rounds it
  int32_t ngroups, nfb, D, loo;
  int32_t logdom, pad_;  // log-domain item (kdehip.h section 5f): partial is [2][ngroups][Nq], the maxima m then the sums s
};

// partial[g][q] = sum over the source chunks c of group g, in chunk order, of
//   sum_{i in chunk c, (i != q if loo)} w_i exp(-1/2 sum_k (x_qk - c_ik)^2 / bw_k)
// (the kernel value of distGauss!, src/DualTree01.jl:14-47, with leaf ranges 0 and uniform bandwidth), for the items [0, n)
// of one D, by the sweep of pair_sweep.hpp with the running sum in a register: the scratch is [ngroups][Nq] with
// ngroups <= kEvalMaxGroups whatever N is, and the summation order is fixed by (N, ngroups).
// CIRC: bit k of masks[i] makes dimension k of item i circular; nothing else changes, so data in which no difference wraps
// gives the bits of the Euclidean instantiation (circ_wrap(t) == t for -pi <= t < pi).  The host launches the items that
// have a circular dimension with this instantiation and all others with the Euclidean one.
template <int D, bool CIRC = false>
__global__ __launch_bounds__(kEvalThreads) void eval_partial_kernel(const EvalItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n,
                                                                    const uint32_t *__restrict__ masks = nullptr) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const EvalItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double nhib[D];  // -1/(2 bw_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.bw[k];
  double total = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double sum = 0.0;
    each([&](int64_t i, double w, double a) {
      double v = w * exp_nonpos(a, sExpTab);
      if (pb.loo && i == at.q) v = 0.0;  // leave-one-out: skip the self term (:141)
      sum += v;
    });
    total += sum;
  });
  if (at.q < pb.Nq) pb.partial[at.grp * pb.Nq + at.q] = total;
}

// The log-domain step on the same sweep (kdehip.h section 5f): the same items, mapping and a_i, but the block carries
// (m, s) with
//   m = max a_i,  s = sum w_i exp(a_i - m)   over S = { i in the group : w_i > 0, (i != q if loo) }
// instead of the plain sum, so nothing underflows that matters to log p.  Per staged chunk: pass one takes the chunk's
// maximum over S (D fmas per source, no exp), the carried s is rescaled ONCE by exp_nonpos(m_old - m_new), pass two
// recomputes a_i and adds w_i exp_nonpos(a_i - m_new): one exp per pair, as the direct kernel.  A source outside S takes no
// part in the maximum (a near, weightless point would push every real term into underflow) and adds nothing.  A group
// with S empty leaves (m, s) = (-Inf, 0).
// partial[g][q] = m, partial[ngroups + g][q] = s.
template <int D, bool CIRC = false>
__global__ __launch_bounds__(kEvalThreads) void eval_partial_log_kernel(const EvalItem *__restrict__ items,
                                                                        const int32_t *__restrict__ first, int n,
                                                                        const uint32_t *__restrict__ masks = nullptr) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const EvalItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double nhib[D];  // -1/(2 bw_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.bw[k];
  const int64_t skip = pb.loo ? at.q : -1;  // leave-one-out: the self term is not in S
  double m = -INFINITY, total = 0.0;
  pair_sweep<D, CIRC>(pb, at, circ, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t i, double w, double a) { cm = (w > 0.0 && i != skip) ? fmax(cm, a) : cm; });
    if (cm > m) {  // (m == -Inf: total is still 0)
      total *= exp_nonpos(m - cm, sExpTab);
      m = cm;
    }
    double sum = 0.0;
    each([&](int64_t i, double w, double a) {
      const bool in = w > 0.0 && i != skip;  // in S: then a <= m
      sum += in ? w * exp_nonpos(a - m, sExpTab) : 0.0;
    });
    total += sum;
  });
  if (at.q < pb.Nq) {
    pb.partial[at.grp * pb.Nq + at.q] = m;
    pb.partial[(pb.ngroups + at.grp) * pb.Nq + at.q] = total;
  }
}

__device__ __forceinline__ double eval_norm(const EvalItem &it) {
  return gauss_norm(it.norm0, it.D, [&](int k) { return it.bw[k]; });
}

// The tail of both finish kernels, for query q of finish block fb (q < Nq: a live lane): the value stored (through the
// item's permutation, if any) when the item asks for values; when it asks for a log-likelihood, the lanes' terms summed in
// a fixed LDS tree into bpart[fb], and bzero[fb] raised if any lane's `zero` is.
__device__ __forceinline__ void finish_tail(const EvalItem &it, int fb, int64_t q, double value, double term, int zero,
                                            double *red /* LDS [kFinishThreads] */) {
  if (q < it.Nq && it.out) {
    const int64_t o = it.perm ? it.perm[q] - 1 : q;
    if (o >= 0 && o < it.Nq) it.out[o] = value;  // (an uploaded density's permutation is the caller's)
  }
  if (!it.logl) return;  // (block-uniform)
  red[threadIdx.x] = term;
  const int anyzero = __syncthreads_or(zero);
  const double share = block_tree_sum<kFinishThreads>(red);
  if (threadIdx.x == 0) {
    it.bpart[fb] = share;
    it.bzero[fb] = anyzero;
  }
}

// p[q] = (sum over the groups, in group order) / norm [/ (1 - w_q)]   (src/DualTree01.jl:325-340), then W log p and the
// block's share (items [0, n), item i owns blocks [first[i], first[i+1]), first[0] the launch's first block)
__global__ __launch_bounds__(kFinishThreads) void eval_finish_kernel(const EvalItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n) {
  __shared__ double red[kFinishThreads];
  const ItemBlock ib = item_block(first, n);
  const EvalItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  const double inv_norm = 1.0 / eval_norm(it);
  double p = 0.0, term = 0.0;
  int zero = 0;
  if (q < it.Nq) {
    double s = 0.0;
    for (int c = 0; c < it.ngroups; ++c) s += it.partial[static_cast<int64_t>(c) * it.Nq + q];
    p = s * inv_norm;
    if (it.loo) p = p / (1.0 - it.w[q]);
    if (query_has_nan(it.qry, q, it.D)) p = __builtin_nan("");  // (the sweep drops a NaN: pair_sweep.hpp)
    if (it.qw) {  // evalAvgLogL (:456-466): L == 0 counts as 1 when its weight is 0, and makes the result -Inf otherwise
      const double W = it.qw[q];
      double L = p;
      if (L == 0.0) { zero = W != 0.0; L = 1.0; }
      term = log(L) * W;
    }
  }
  finish_tail(it, ib.k, q, p, term, zero, red);
}

// The log-domain finish (section 5f): the groups combined in group order, M = max m_g, S = sum s_g exp(m_g - M),
//   log p = M + log S - log norm [- log(1 - w_q)],   -Inf when no group has a source in S;
// stored and reduced as eval_finish_kernel does, with W log p summed over the W != 0 only and the block's flag raised by a
// weighted -Inf.
__global__ __launch_bounds__(kFinishThreads) void eval_finish_log_kernel(const EvalItem *__restrict__ items,
                                                                       const int32_t *__restrict__ first, int n) {
  __shared__ double red[kFinishThreads];
  const ItemBlock ib = item_block(first, n);
  const EvalItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  const double lognorm = log(eval_norm(it));
  double lp = -INFINITY, term = 0.0;
  int zero = 0;
  if (q < it.Nq) {
    const double *pm = it.partial + q, *ps = pm + static_cast<int64_t>(it.ngroups) * it.Nq;
    double M = -INFINITY;
    for (int c = 0; c < it.ngroups; ++c) M = fmax(M, pm[static_cast<int64_t>(c) * it.Nq]);
    if (M > -INFINITY) {
      double S = 0.0;
      for (int c = 0; c < it.ngroups; ++c) {
        const double mg = pm[static_cast<int64_t>(c) * it.Nq];
        if (mg > -INFINITY) S += ps[static_cast<int64_t>(c) * it.Nq] * exp(mg - M);
      }
      lp = M + log(S) - lognorm;
      if (it.loo) lp -= log(1.0 - it.w[q]);
    }
    if (query_has_nan(it.qry, q, it.D)) lp = __builtin_nan("");  // (the sweep drops a NaN: pair_sweep.hpp)
    if (it.qw) {
      const double W = it.qw[q];
      if (W != 0.0) {
        if (lp == -INFINITY) zero = 1;
        else term = W * lp;
      }
    }
  }
  finish_tail(it, ib.k, q, lp, term, zero, red);
}

// one thread per item: the block shares in block order
__global__ void logl_reduce_kernel(const EvalItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const EvalItem it = items[i];
  if (!it.logl) return;
  double s = 0.0;
  int zero = 0;
  for (int b = 0; b < it.nfb; ++b) {
    s += it.bpart[b];
    zero |= it.bzero[b];
  }
  *it.logl = zero ? -INFINITY : s;
}

// The run of one call (pair_sweep.hpp PairRun) with the evaluation's scratch, per item [partial | shares | flags], and its
// launches.  Protocol: fill `items` (sizes, D, loo, what to compute) and `circ` (may be shorter: 0 for the rest) ->
// alloc(prefix bytes of caller data) -> the caller writes its data into host() and points the items at dev() ->
// enqueue(stream) (= upload + launch) -> wait() or defer(device).  The results are one double per item (an item's
// log-likelihood), or as many as a blocking caller asks alloc for (the host evaluation's Nq values).
class EvalRun : public PairRun<EvalItem> {
 public:
  // (`extra`: bytes of further scratch behind the items', for the passes of a tolerance-bounded evaluation)
  int alloc(size_t prefix, size_t nresults = 0, size_t extra = 0) {  // nresults == 0: one per item
    const size_t n = items.size();
    int64_t pblocks = 0, fblocks = 0;
    for (EvalItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      fblocks += it.nfb;
    }
    if (pblocks > INT32_MAX || fblocks > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "evaluation too large for one launch");
    Carve c;
    carve_head(c, prefix, 2, 0, nresults ? nresults : n);  // first[] of both kernels
    scratch_.resize(n);
    for (size_t k = 0; k < n; ++k) {
      const EvalItem &it = items[k];
      scratch_[k] = c.take(sizeof(double) * ((it.logdom ? 2 : 1) * it.ngroups * it.Nq + it.nfb) + sizeof(int32_t) * it.nfb);
    }
    o_extra_ = c.take(extra);
    KDEHIP_CHECK(alloc_block(c));
    return KDEHIP_OK;
  }
  unsigned char *extra() const { return dev() + o_extra_; }
  int enqueue(hipStream_t st) {
    KDEHIP_CHECK_RC(upload(st));
    return launch();
  }
  // scratch pointers, descriptors sorted (the direct items before the log-domain ones; by D; Euclidean items before circular
  // ones), one upload on `st`
  int upload(hipStream_t st) {
    const size_t n = items.size();
    for (size_t k = 0; k < n; ++k) {
      EvalItem &it = items[k];
      it.partial = reinterpret_cast<double *>(dev() + scratch_[k]);
      it.bpart = it.partial + static_cast<int64_t>(it.logdom ? 2 : 1) * it.ngroups * it.Nq;
      it.bzero = reinterpret_cast<int32_t *>(it.bpart + it.nfb);
    }
    prepare([&](size_t k) { return (items[k].logdom ? 1024 : 0) + 2 * items[k].D + (circ[k] ? 1 : 0); });
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    for (size_t k = 0; k < n; ++k) ffirst[k + 1] = ffirst[k] + items[k].nfb;
    KDEHIP_CHECK(send(st));
    return KDEHIP_OK;
  }
  // the launches behind the upload: two kernels (and their log-domain twins for the log-domain items), and the per-item
  // reduce when an item asks for a log-likelihood
  int launch() {
    KDEHIP_CHECK_RC(launch_sweep());
    return launch_finish();
  }
  int launch_sweep() {
    const hipStream_t st = stream();
    // one launch per distinct D, and one more for its circular and for its log-domain items
    KDEHIP_CHECK_RC(for_each_run([&](const EvalItem &it, const EvalItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *d_masks) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        if (it.logdom)
          launch_pair<EvalItem>(eval_partial_log_kernel<kD, false>, eval_partial_log_kernel<kD, true>, blocks, st, d_it, d_pfirst,
                                cnt, d_masks);
        else
          launch_pair<EvalItem>(eval_partial_kernel<kD, false>, eval_partial_kernel<kD, true>, blocks, st, d_it, d_pfirst, cnt,
                                d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    return KDEHIP_OK;
  }
  int launch_finish() {
    const hipStream_t st = stream();
    const size_t n = items.size();
    const int32_t *ffirst = first(1);
    size_t nd = 0;  // the direct items are the first nd
    while (nd < n && !items[nd].logdom) ++nd;
    if (ffirst[nd] > 0)
      hipLaunchKernelGGL(eval_finish_kernel, dim3(static_cast<unsigned>(ffirst[nd])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(1), static_cast<int>(nd));
    if (ffirst[n] > ffirst[nd])
      hipLaunchKernelGGL(eval_finish_log_kernel, dim3(static_cast<unsigned>(ffirst[n] - ffirst[nd])), dim3(kFinishThreads), 0,
                         st, d_items() + nd, d_first(1) + nd, static_cast<int>(n - nd));
    if (std::any_of(items.begin(), items.end(), [](const EvalItem &it) { return it.logl != nullptr; }))
      hipLaunchKernelGGL(logl_reduce_kernel, dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64), 0, st, d_items(),
                         static_cast<int>(n));
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }

 private:
  std::vector<size_t> scratch_;
  size_t o_extra_ = 0;
};

}  // namespace

// evaluateDualTree reads ONE bandwidth vector (bandwidthMin[1..D], BallTreeDensity01.jl:98): a resident density qualifies when
// its all-leaf frontier (level Lown) shares its first node's -- the flag the upload / the builders set (examine_frontiers)
bool kdehip::leaves_share_bandwidth(const kdehip_device_density *h) {
  const Frontiers &fr = h->fr;
  const size_t L = static_cast<size_t>(h->Lown);
  return fr.uniform.size() > L && fr.off.size() > L + 1 && fr.uniform[L] && fr.off[L + 1] - fr.off[L] == h->N;
}

namespace {

// bd at at's leaf points (tree order; out, if any, through at's permutation), W = at's leaf weights
EvalItem pair_item(const kdehip_device_density *bd, const kdehip_device_density *at, int loo, bool logl, bool logdom) {
  const LeafRows src = leaf_rows(bd), qry = leaf_rows(at);
  EvalItem it{};
  it.src = src.src; it.w = src.w; it.bw = src.bw;
  it.qry = qry.src;
  it.qw = logl ? qry.w : nullptr;
  it.perm = qry.perm;
  it.norm0 = gauss_norm0(bd->D);
  it.N = bd->N; it.Nq = at->N; it.D = bd->D; it.loo = loo ? 1 : 0; it.logdom = logdom ? 1 : 0;
  return it;
}

}  // namespace

extern "C" int kdehip_evaluate(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out,
                               double *p_out, int device) {
  return kdehip_evaluate_manifold(bd, pos, Nq, leave_one_out, p_out, device, nullptr);
}

namespace {

// The tolerances of an evaluation within a tolerance (section 5m), and where its tile counts go: a host int64[2] for the
// blocking entry, a device one for the resident entry, or null.
struct TolArgs {
  double rel_tol, abs_tol;
  int64_t *stats;
};

// NULL rel_tol: the reference's default errTol, 1e-3; NULL abs_tol: 0
int read_tolerances(const double *rel_tol, const double *abs_tol, TolArgs *out) {
  out->rel_tol = rel_tol ? *rel_tol : 1e-3;
  out->abs_tol = abs_tol ? *abs_tol : 0.0;
  if (!(out->rel_tol >= 0.0 && out->rel_tol < 1.0))
    return set_error(KDEHIP_ERR_ARG, "evaluate_tol: rel_tol must lie in [0, 1)");
  if (!(out->abs_tol >= 0.0 && out->abs_tol < INFINITY))
    return set_error(KDEHIP_ERR_ARG, "evaluate_tol: abs_tol must be finite and >= 0");
  return KDEHIP_OK;
}

// the passes that take the direct sweep's place for item 0 of a run that has been uploaded, with tol_scratch_bytes of `extra`
int enqueue_tol(const EvalRun &run, uint32_t circ, const TolArgs &tol, int64_t *d_stats, hipStream_t st,
                hipEvent_t *marks = nullptr) {
  const EvalItem &it = run.items[0];
  TolPass t{};
  t.src = it.src; t.w = it.w; t.qry = it.qry; t.bw = it.bw;
  t.N = it.N; t.Nq = it.Nq; t.chunks_per_group = it.chunks_per_group;
  t.ngroups = it.ngroups; t.D = it.D; t.loo = it.loo;
  t.circ = circ;
  t.norm0 = it.norm0; t.rel_tol = tol.rel_tol; t.abs_tol = tol.abs_tol;
  t.partial = it.partial;
  t.scratch = run.extra();
  t.stats = d_stats;
  return enqueue_tol_passes(t, st, marks);
}

}  // namespace

// The bodies of the entries: `logdom` selects the log-domain kernels (section 5f); everything else -- checks, layout of the
// call's block, streams -- is shared, so a log-domain entry refuses what its direct twin refuses, with the same words.
// `tol` (direct items only): the passes of section 5m in place of the sweep, the tile counts behind the Nq results.
static int evaluate_host(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, double *p_out, int device,
                         const uint8_t *manifold, bool logdom, const TolArgs *tol = nullptr) {
  if (!bd || !p_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  const int64_t N = bd->npts;
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (leave_one_out) Nq = N;
  else if (!pos || Nq < 0) return set_error(KDEHIP_ERR_ARG, "pos must hold Nq >= 0 points");
  if (Nq == 0) {
    if (tol && tol->stats) tol->stats[0] = tol->stats[1] = 0;
    return KDEHIP_OK;
  }
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));  // (the reference's evalDirect reads bandwidthMin[1..D])
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  hipStream_t st = hipStreamPerThread;  // the calling thread's own stream, like every blocking entry point (kdehip.h)
  // caller data: [the density (leaf means | leaf weights | leaf bandwidth: density_args.hpp) | queries, or
  // (leave-one-out) the leaf row of the permutation: p[getIndexOf(locations, j)] (:335), results in the caller's original
  // order].  ONE pinned image goes up in one DMA and the Nq results come back in one; everything is enqueued on the
  // calling thread's stream and the host waits once (pageable hipMemcpy calls, one per array, cost more than the kernel
  // for anything below ~10^8 kernel evaluations).
  const size_t o_q = host_density_bytes(bd);
  const size_t prefix = o_q + (leave_one_out ? sizeof(int64_t) * N : sizeof(double) * Nq * D);
  EvalRun run;
  EvalItem it{};
  it.norm0 = gauss_norm0(D);
  it.N = N; it.Nq = Nq; it.D = D; it.loo = leave_one_out ? 1 : 0; it.logdom = logdom ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  static_assert(sizeof(int64_t) == sizeof(double), "the tile counts take two result slots");
  KDEHIP_CHECK_RC(run.alloc(prefix, static_cast<size_t>(Nq) + (tol ? 2 : 0), tol ? tol_scratch_bytes(N, Nq, D) : 0));
  unsigned char *h = run.host(), *d = run.dev();
  EvalItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  if (leave_one_out) std::memcpy(h + o_q, bd->permutation + N, sizeof(int64_t) * N);
  else std::memcpy(h + o_q, pos, sizeof(double) * Nq * D);
  ri.qry = leave_one_out ? ri.src : reinterpret_cast<const double *>(d + o_q);
  ri.perm = leave_one_out ? reinterpret_cast<const int64_t *>(d + o_q) : nullptr;
  ri.out = run.result(0);
  KDEHIP_CHECK_RC(run.upload(st));
  PhaseTimer timer(kPhaseEvaluate, st);  // kdehip_profile_phase_read: the two launches, not the copies
  PassMarks marks(kPhaseTolBox, tol != nullptr);  // kdehip_profile_phase_read 3..5
  if (tol) {
    KDEHIP_CHECK_RC(enqueue_tol(run, circ, *tol, reinterpret_cast<int64_t *>(run.result(static_cast<size_t>(Nq))), st,
                                marks.events()));
    KDEHIP_CHECK_RC(run.launch_finish());
  } else {
    KDEHIP_CHECK_RC(run.launch());
  }
  timer.stop();
  KDEHIP_CHECK_RC(run.wait());
  timer.collect();
  marks.collect();
  std::memcpy(p_out, run.host_result(0), sizeof(double) * Nq);
  if (tol && tol->stats) std::memcpy(tol->stats, run.host_result(static_cast<size_t>(Nq)), sizeof(int64_t) * 2);
  return KDEHIP_OK;
}

extern "C" int kdehip_eval_avg_logl(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out,
                                    int device) {
  return kdehip_eval_avg_logl_manifold(bd, at, leave_one_out, out, device, nullptr);
}

static int eval_avg_logl_host(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out, int device,
                              const uint8_t *manifold, bool logdom) {
  // every check that needs no device comes first
  if (!bd || !out) return set_error(KDEHIP_ERR_ARG, "null argument");
  if (leave_one_out && at && at != bd) return set_error(KDEHIP_ERR_ARG, "leave_one_out needs at == bd (or at == NULL)");
  if (!leave_one_out && !at) return set_error(KDEHIP_ERR_ARG, "null argument");
  if (!at) at = bd;
  const int64_t D = bd->ndim, N = bd->npts, Nq = at->npts;
  if (D > KDEHIP_MAX_DIMS || at->ndim > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (D < 1 || at->ndim < 1) return set_error(KDEHIP_ERR_ARG, "density with no dimensions");
  if (at->ndim != D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "evaluate -- dimensions of two BallTreeDensities must match");
  if (N < 1 || !bd->means || !bd->bandwidth || !bd->weights || !bd->permutation) return set_error(KDEHIP_ERR_ARG, "malformed density");
  if (Nq < 0 || (Nq > 0 && (!at->means || !at->weights))) return set_error(KDEHIP_ERR_ARG, "malformed density");
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  hipStream_t st = hipStreamPerThread;
  const bool self = at == bd;
  // caller data: [bd leaf means | bd leaf weights | bd leaf bandwidth | at leaf means | at leaf weights] (at == bd: none)
  const size_t o_q = host_density_bytes(bd), prefix = o_q + (self ? 0 : sizeof(double) * Nq * (D + 1));
  EvalRun run;
  EvalItem it{};
  it.norm0 = gauss_norm0(static_cast<int>(D));
  it.N = N; it.Nq = Nq; it.D = static_cast<int32_t>(D); it.loo = leave_one_out ? 1 : 0; it.logdom = logdom ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix));
  EvalItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  const LeafArrays qry = self ? LeafArrays{ri.src, ri.w} : pack_leaves(run, o_q, at);
  ri.qry = qry.means;
  ri.qw = qry.weights;
  ri.logl = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(st));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}

extern "C" int kdehip_eval_avg_logl_device_batch(int n, const kdehip_logl_item *items, double *d_out, void *stream) {
  if (n < 0 || (n > 0 && (!items || !d_out))) return set_error(KDEHIP_ERR_ARG, "evalAvgLogL batch: bad item list");
  if (n == 0) return KDEHIP_OK;
  try {  // (the old entry forwards with mask 0; its reserved_ word stays unread)
    std::vector<kdehip_logl_manifold_item> mi(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) mi[i] = kdehip_logl_manifold_item{items[i].bd, items[i].at, items[i].leave_one_out, 0u};
    return kdehip_eval_avg_logl_device_batch_manifold(n, mi.data(), d_out, stream);
  } catch (const std::exception &e) {
    return set_error(KDEHIP_ERR_ALLOC, std::string("evalAvgLogL batch: ") + e.what());
  }
}

static int eval_avg_logl_batch(int n, const kdehip_logl_manifold_item *items, double *d_out, void *stream, bool logdom) {
  if (n < 0 || (n > 0 && (!items || !d_out))) return set_error(KDEHIP_ERR_ARG, "evalAvgLogL batch: bad item list");
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    KDEHIP_CHECK_RC(check_pair(items[i].bd, items[i].at, items[i].leave_one_out, true));
    KDEHIP_CHECK_RC(check_same_device(items[i].bd, items[0].bd, "evalAvgLogL batch: "));
    if (items[i].circular_mask >> items[i].bd->D)
      return set_error(KDEHIP_ERR_ARG, "evalAvgLogL batch: circular_mask names a dimension the densities do not have");
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  EvalRun run;
  for (int i = 0; i < n; ++i) {
    run.items.push_back(pair_item(items[i].bd, items[i].at, items[i].leave_one_out, true, logdom));
    run.items.back().logl = d_out + i;
    run.circ.push_back(items[i].circular_mask);
  }
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return finish_enqueue(run, nullptr, device);
}

extern "C" int kdehip_eval_avg_logl_device(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                           double *out) {
  return kdehip_eval_avg_logl_device_manifold(bd, at, leave_one_out, out, nullptr);
}

static int eval_avg_logl_resident(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                  double *out, const uint8_t *manifold, bool logdom) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_pair(bd, at, leave_one_out, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  EvalRun run;
  run.items.push_back(pair_item(bd, at, leave_one_out, true, logdom));
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0));
  run.items[0].logl = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}

extern "C" int kdehip_evaluate_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int leave_one_out,
                                      double *d_out, void *stream) {
  return kdehip_evaluate_device_manifold(bd, d_pos, Nq, leave_one_out, d_out, stream, nullptr);
}

static int evaluate_resident_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out, void *stream,
                                const uint8_t *manifold, bool logdom);

static int evaluate_resident(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int leave_one_out, double *d_out,
                             void *stream, const uint8_t *manifold, bool logdom) {
  if (!bd || !d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  if (leave_one_out) return evaluate_resident_at(bd, bd, d_out, stream, manifold, logdom);
  KDEHIP_CHECK_RC(check_query_count(d_pos, Nq, "d_pos must hold Nq >= 0 points"));
  KDEHIP_CHECK_RC(check_pair(bd, bd, 0, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  EvalRun run;
  EvalItem it = pair_item(bd, bd, 0, false, logdom);
  it.qry = d_pos; it.perm = nullptr; it.Nq = Nq; it.out = d_out;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return finish_enqueue(run, nullptr, bd->device);
}

extern "C" int kdehip_evaluate_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out,
                                         void *stream) {
  return kdehip_evaluate_device_at_manifold(bd, at, d_out, stream, nullptr);
}

static int evaluate_resident_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out, void *stream,
                                const uint8_t *manifold, bool logdom) {
  if (!d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_pair(bd, at, at == bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  EvalRun run;
  EvalItem it = pair_item(bd, at, at == bd, false, logdom);
  it.out = d_out;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return finish_enqueue(run, nullptr, bd->device);
}

// ---- evaluation within a tolerance (kdehip.h section 5m): the bodies above with the passes of evaltol.hip in the sweep's place
extern "C" int kdehip_evaluate_tol(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out,
                                   const double *rel_tol, const double *abs_tol, double *p_out, int64_t *stats, int device,
                                   const uint8_t *manifold) {
  TolArgs tol{};
  KDEHIP_CHECK_RC(read_tolerances(rel_tol, abs_tol, &tol));
  tol.stats = stats;
  return evaluate_host(bd, pos, Nq, leave_one_out, p_out, device, manifold, false, &tol);
}

extern "C" int kdehip_evaluate_device_at_tol(const kdehip_device_density *bd, const kdehip_device_density *at,
                                             const double *rel_tol, const double *abs_tol, double *d_out, int64_t *d_stats,
                                             void *stream, const uint8_t *manifold) {
  TolArgs tol{};
  KDEHIP_CHECK_RC(read_tolerances(rel_tol, abs_tol, &tol));
  if (!d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_pair(bd, at, at == bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);  // (a captured call's blocks are kept until kdehip_clear_cache: section 5h)
  EvalRun run;
  EvalItem it = pair_item(bd, at, at == bd, false, false);
  it.out = d_out;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0, 0, tol_scratch_bytes(it.N, it.Nq, it.D)));
  KDEHIP_CHECK_RC(run.upload(st));
  KDEHIP_CHECK_RC(enqueue_tol(run, circ, tol, d_stats, st));
  KDEHIP_CHECK_RC(run.launch_finish());
  return finish_enqueue(run, &scope, bd->device);
}

extern "C" int kdehip_evaluate_manifold(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out,
                                        double *p_out, int device, const uint8_t *manifold) {
  return evaluate_host(bd, pos, Nq, leave_one_out, p_out, device, manifold, false);
}
extern "C" int kdehip_eval_avg_logl_manifold(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out,
                                             int device, const uint8_t *manifold) {
  return eval_avg_logl_host(bd, at, leave_one_out, out, device, manifold, false);
}
extern "C" int kdehip_eval_avg_logl_device_batch_manifold(int n, const kdehip_logl_manifold_item *items, double *d_out,
                                                          void *stream) {
  return eval_avg_logl_batch(n, items, d_out, stream, false);
}
extern "C" int kdehip_eval_avg_logl_device_manifold(const kdehip_device_density *bd, const kdehip_device_density *at,
                                                    int leave_one_out, double *out, const uint8_t *manifold) {
  return eval_avg_logl_resident(bd, at, leave_one_out, out, manifold, false);
}
extern "C" int kdehip_evaluate_device_manifold(const kdehip_device_density *bd, const double *d_pos, int64_t Nq,
                                               int leave_one_out, double *d_out, void *stream, const uint8_t *manifold) {
  return evaluate_resident(bd, d_pos, Nq, leave_one_out, d_out, stream, manifold, false);
}
extern "C" int kdehip_evaluate_device_at_manifold(const kdehip_device_density *bd, const kdehip_device_density *at,
                                                  double *d_out, void *stream, const uint8_t *manifold) {
  return evaluate_resident_at(bd, at, d_out, stream, manifold, false);
}

// ---- log-domain entries (kdehip.h section 5f): the same bodies with the log-domain kernels
extern "C" int kdehip_evaluate_log(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, double *logp_out,
                                   int device, const uint8_t *manifold) {
  return evaluate_host(bd, pos, Nq, leave_one_out, logp_out, device, manifold, true);
}
extern "C" int kdehip_evaluate_log_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int leave_one_out,
                                          double *d_out, void *stream, const uint8_t *manifold) {
  return evaluate_resident(bd, d_pos, Nq, leave_one_out, d_out, stream, manifold, true);
}
extern "C" int kdehip_evaluate_log_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out,
                                             void *stream, const uint8_t *manifold) {
  return evaluate_resident_at(bd, at, d_out, stream, manifold, true);
}
extern "C" int kdehip_eval_avg_logl_log(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out,
                                        int device, const uint8_t *manifold) {
  return eval_avg_logl_host(bd, at, leave_one_out, out, device, manifold, true);
}
extern "C" int kdehip_eval_avg_logl_log_device(const kdehip_device_density *bd, const kdehip_device_density *at,
                                               int leave_one_out, double *out, const uint8_t *manifold) {
  return eval_avg_logl_resident(bd, at, leave_one_out, out, manifold, true);
}
extern "C" int kdehip_eval_avg_logl_log_device_batch(int n, const kdehip_logl_manifold_item *items, double *d_out, void *stream) {
  return eval_avg_logl_batch(n, items, d_out, stream, true);
}
