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
//                           Gaussian sum, one lane per query point, source points staged through LDS in chunks and read as
//                           broadcasts, one partial sum per (group of source chunks, query);
//   eval_finish_kernel      the groups summed in a fixed order (deterministic, no atomics), / norm, / (1 - w) for
//                           leave-one-out, the value stored (through the item's permutation, if any) when asked for, then
//                           W_q log p_q and the block's share in a fixed LDS tree; a weighted zero raises the block's flag
//                           instead of adding -Inf;
//   logl_reduce_kernel      only when an item asks for a log-likelihood: per item, the block shares summed in block order
//                           (or -Inf if a flag is up) into one double.
// Log-domain items (kdehip.h section 5f: log p by log-sum-exp, finite where p underflows) run eval_partial_log_kernel<D> and
// eval_finish_log_kernel in launches of their own, with the same mapping, split and reduction.
// The group split (split_chunks(N, Nq, 1)) depends on the item's (N, Nq) alone, so nothing depends on the launch or the
// batch: the host entry, a single device call and any batch give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "circ_wrap.hpp"
#include "device_density.hpp"
#include "call_block.hpp"
#include "entry_helpers.hpp"
#include "manifold_arg.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"
#include "phase_timer.hpp"

using namespace kdehip;

namespace {

// (kEvalThreads, kEvalChunk and split_chunks, the mapping of the all-pairs sum, are in entry_helpers.hpp: ksum.hip shares them)
constexpr int kFinishThreads = 256;  // queries per finish block

// One evaluation: a density (N source points in tree / leaf order, one bandwidth vector) at Nq query points.
struct EvalItem {
  const double *src;    // [N][D] leaf means of the evaluated density (tree order)
  const double *w;      // [N] its leaf weights
  const double *bw;     // [D] its first leaf's variances (every leaf has them: checked on the host)
  const double *qry;    // [Nq][D] query points
  const double *qw;     // [Nq] query weights (the `at` density's leaf weights), or null: no log-likelihood
  const int64_t *perm;  // [Nq] 1-based output position of query q, or null: query order
  double *out;          // [Nq] p, or null
  double *partial;      // [ngroups][Nq]
  double *bpart;        // [nfb] the finish blocks' shares of sum W log p
  int32_t *bzero;       // [nfb] the finish block met a p == 0 with W != 0
  double *logl;         // the result, or null
  double norm0;         // (2 pi)^(D/2) as the host's libm rounds it
  int64_t N, Nq, chunks_per_group;
  int32_t ngroups, nfb, D, loo;
  int32_t logdom, pad_;  // log-domain item (kdehip.h section 5f): partial is [2][ngroups][Nq], the maxima m then the sums s
};

// partial[g][q] = sum over the source chunks c of group g, in chunk order, of
//   sum_{i in chunk c, (i != q if loo)} w_i exp(-1/2 sum_k (x_qk - c_ik)^2 / bw_k)
// (the kernel value of distGauss!, src/DualTree01.jl:14-47, with leaf ranges 0 and uniform bandwidth), for the items [0, n)
// of one D: item i owns blocks [first[i], first[i+1]) - first[0], its block k is query block k % qblocks of source group
// k / qblocks.  A block owns kEvalThreads queries and ONE group of consecutive 128-point source chunks, which it walks in
// order with the running sum in a register: the scratch is [ngroups][Nq] with ngroups <= kEvalMaxGroups whatever N is,
// and the summation order is fixed by (N, ngroups).
// CIRC: bit k of masks[i] (uniform over the block) makes dimension k of item i circular -- its difference goes through
// circ_wrap before it is squared (diffop inside distGauss!); nothing else changes, so data in which no difference wraps
// gives the bits of the Euclidean instantiation (circ_wrap(t) == t for -pi <= t < pi).  The host launches the items that
// have a circular dimension with this instantiation and all others with the Euclidean one.
template <int D, bool CIRC = false>
__global__ __launch_bounds__(kEvalThreads) void eval_partial_kernel(const EvalItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n,
                                                                    const uint32_t *__restrict__ masks = nullptr) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const int b = static_cast<int>(blockIdx.x) + first[0];
  const int i = item_of_block(first, n, b);
  const EvalItem pb = items[i];
  unsigned circ = 0;
  if constexpr (CIRC) circ = __builtin_amdgcn_readfirstlane(masks[i]);
  const int64_t qblocks = (pb.Nq + kEvalThreads - 1) / kEvalThreads;
  const int64_t kb = b - first[i];
  const int64_t qb = kb % qblocks, grp = kb / qblocks;
  const int64_t q = qb * kEvalThreads + threadIdx.x;
  const int64_t c_begin = grp * pb.chunks_per_group;
  int64_t c_end = c_begin + pb.chunks_per_group;
  const int64_t nchunks = (pb.N + kEvalChunk - 1) / kEvalChunk;
  if (c_end > nchunks) c_end = nchunks;
  if (c_begin >= c_end) return;  // block-uniform
  double nhib[D];  // -1/(2 bw_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.bw[k];
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = (q < pb.Nq) ? pb.qry[q * D + k] : 0.0;
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((pb.N - i0 < kEvalChunk) ? (pb.N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * (D + 1); t += kEvalThreads) {
      const int i = t / (D + 1), f = t % (D + 1);
      sSrc[buf][t] = (f < D) ? pb.src[(i0 + i) * D + f] : pb.w[i0 + i];
    }
  };
  stage(c_begin, 0);
  double total = 0.0;
  for (int64_t c = c_begin; c < c_end; ++c) {
    const int buf = static_cast<int>((c - c_begin) & 1);
    __syncthreads();  // chunk c is staged; the other buffer is free again
    if (c + 1 < c_end) stage(c + 1, buf ^ 1);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((pb.N - i0 < kEvalChunk) ? (pb.N - i0) : kEvalChunk);
    double sum = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const double *s = sSrc[buf] + i * (D + 1);
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double d = x[k] - s[k];
        if constexpr (CIRC) {
          if ((circ >> k) & 1u) d = circ_wrap(d);
        }
        acc = fma(d * d, nhib[k], acc);
      }
      double v = s[D] * exp_nonpos(acc, sExpTab);  // acc <= 0
      if (pb.loo && i0 + i == q) v = 0.0;  // leave-one-out: skip the self term (:141)
      sum += v;
    }
    total += sum;
  }
  if (q < pb.Nq) pb.partial[grp * pb.Nq + q] = total;
}

// The log-domain twin (kdehip.h section 5f): the same items, block mapping, LDS double buffer and a_i (same fma order, same
// nhib[k]) as eval_partial_kernel, but the block carries (m, s) with
//   m = max a_i,  s = sum w_i exp(a_i - m)   over S = { i in the group : w_i > 0, (i != q if loo) }
// instead of the plain sum, so nothing underflows that matters to log p.  Per staged chunk: pass one takes the chunk's
// maximum over S (D fmas per source, no exp), the carried s is rescaled ONCE by exp_nonpos(m_old - m_new), pass two
// recomputes a_i and adds w_i exp_nonpos(a_i - m_new): one exp per pair, as the direct kernel.  A source outside S takes no
// part in the maximum (a near, weightless point would push every real term into underflow) and adds nothing.  A group
// with S empty leaves (m, s) = (-Inf, 0).  Every lane, those beyond Nq included, walks the same chunks and barriers.
// partial[g][q] = m, partial[ngroups + g][q] = s.
template <int D, bool CIRC = false>
__global__ __launch_bounds__(kEvalThreads) void eval_partial_log_kernel(const EvalItem *__restrict__ items,
                                                                        const int32_t *__restrict__ first, int n,
                                                                        const uint32_t *__restrict__ masks = nullptr) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const int b = static_cast<int>(blockIdx.x) + first[0];
  const int i = item_of_block(first, n, b);
  const EvalItem pb = items[i];
  unsigned circ = 0;
  if constexpr (CIRC) circ = __builtin_amdgcn_readfirstlane(masks[i]);
  const int64_t qblocks = (pb.Nq + kEvalThreads - 1) / kEvalThreads;
  const int64_t kb = b - first[i];
  const int64_t qb = kb % qblocks, grp = kb / qblocks;
  const int64_t q = qb * kEvalThreads + threadIdx.x;
  const int64_t c_begin = grp * pb.chunks_per_group;
  int64_t c_end = c_begin + pb.chunks_per_group;
  const int64_t nchunks = (pb.N + kEvalChunk - 1) / kEvalChunk;
  if (c_end > nchunks) c_end = nchunks;
  if (c_begin >= c_end) return;  // block-uniform
  double nhib[D];  // -1/(2 bw_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / pb.bw[k];
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = (q < pb.Nq) ? pb.qry[q * D + k] : 0.0;
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((pb.N - i0 < kEvalChunk) ? (pb.N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * (D + 1); t += kEvalThreads) {
      const int i = t / (D + 1), f = t % (D + 1);
      sSrc[buf][t] = (f < D) ? pb.src[(i0 + i) * D + f] : pb.w[i0 + i];
    }
  };
  auto exponent = [&](const double *s) {  // a_i
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double d = x[k] - s[k];
      if constexpr (CIRC) {
        if ((circ >> k) & 1u) d = circ_wrap(d);
      }
      acc = fma(d * d, nhib[k], acc);
    }
    return acc;
  };
  const int64_t skip = pb.loo ? q : -1;  // leave-one-out: the self term is not in S
  stage(c_begin, 0);
  double m = -INFINITY, total = 0.0;
  for (int64_t c = c_begin; c < c_end; ++c) {
    const int buf = static_cast<int>((c - c_begin) & 1);
    __syncthreads();  // chunk c is staged; the other buffer is free again
    if (c + 1 < c_end) stage(c + 1, buf ^ 1);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((pb.N - i0 < kEvalChunk) ? (pb.N - i0) : kEvalChunk);
    double cm = -INFINITY;
    for (int i = 0; i < cnt; ++i) {
      const double *s = sSrc[buf] + i * (D + 1);
      const double acc = exponent(s);
      cm = (s[D] > 0.0 && i0 + i != skip) ? fmax(cm, acc) : cm;
    }
    if (cm > m) {  // (m == -Inf: total is still 0)
      total *= exp_nonpos(m - cm, sExpTab);
      m = cm;
    }
    double sum = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const double *s = sSrc[buf] + i * (D + 1);
      const double acc = exponent(s);
      const bool in = s[D] > 0.0 && i0 + i != skip;  // in S: then acc <= m
      sum += in ? s[D] * exp_nonpos(acc - m, sExpTab) : 0.0;
    }
    total += sum;
  }
  if (q < pb.Nq) {
    pb.partial[grp * pb.Nq + q] = m;
    pb.partial[(pb.ngroups + grp) * pb.Nq + q] = total;
  }
}

// p[q] = (sum over the groups, in group order) / norm [/ (1 - w_q)]   (src/DualTree01.jl:325-340), then W log p and the
// block's share (items [0, n), item i owns blocks [first[i], first[i+1]))
__global__ __launch_bounds__(kFinishThreads) void eval_finish_kernel(const EvalItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n) {
  __shared__ double red[kFinishThreads];
  const int b = static_cast<int>(blockIdx.x);
  const int i = item_of_block(first, n, b);
  const EvalItem it = items[i];
  const int fb = b - first[i];
  const int64_t q = static_cast<int64_t>(fb) * kFinishThreads + threadIdx.x;
  double norm = it.norm0;  // (2 pi)^(D/2) * prod_k sqrt(bw_k)   (src/DualTree01.jl:325-330)
  for (int k = 0; k < it.D; ++k) norm *= __dsqrt_rn(it.bw[k]);
  const double inv_norm = 1.0 / norm;
  double term = 0.0;
  int zero = 0;
  if (q < it.Nq) {
    double s = 0.0;
    for (int c = 0; c < it.ngroups; ++c) s += it.partial[static_cast<int64_t>(c) * it.Nq + q];
    double p = s * inv_norm;
    if (it.loo) p = p / (1.0 - it.w[q]);
    if (it.out) {
      const int64_t o = it.perm ? it.perm[q] - 1 : q;
      if (o >= 0 && o < it.Nq) it.out[o] = p;  // (an uploaded density's permutation is the caller's)
    }
    if (it.qw) {  // evalAvgLogL (:456-466): L == 0 counts as 1 when its weight is 0, and makes the result -Inf otherwise
      const double W = it.qw[q];
      if (p == 0.0) { zero = W != 0.0; p = 1.0; }
      term = log(p) * W;
    }
  }
  if (!it.logl) return;  // (block-uniform)
  red[threadIdx.x] = term;
  const int anyzero = __syncthreads_or(zero);
  for (int off = kFinishThreads / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    it.bpart[fb] = red[0];
    it.bzero[fb] = anyzero;
  }
}

// The log-domain finish (section 5f), for the items [0, n) with block offsets first[] (first[0] is the launch's first
// block): the groups combined in group order, M = max m_g, S = sum s_g exp(m_g - M),
//   log p = M + log S - log norm [- log(1 - w_q)],   -Inf when no group has a source in S;
// stored and reduced as eval_finish_kernel does, with W log p summed over the W != 0 only and the block's flag raised by a
// weighted -Inf.
__global__ __launch_bounds__(kFinishThreads) void eval_finish_log_kernel(const EvalItem *__restrict__ items,
                                                                       const int32_t *__restrict__ first, int n) {
  __shared__ double red[kFinishThreads];
  const int b = static_cast<int>(blockIdx.x) + first[0];
  const int i = item_of_block(first, n, b);
  const EvalItem it = items[i];
  const int fb = b - first[i];
  const int64_t q = static_cast<int64_t>(fb) * kFinishThreads + threadIdx.x;
  double norm = it.norm0;  // as eval_finish_kernel
  for (int k = 0; k < it.D; ++k) norm *= __dsqrt_rn(it.bw[k]);
  const double lognorm = log(norm);
  double term = 0.0;
  int zero = 0;
  if (q < it.Nq) {
    const double *pm = it.partial + q, *ps = pm + static_cast<int64_t>(it.ngroups) * it.Nq;
    double M = -INFINITY;
    for (int c = 0; c < it.ngroups; ++c) M = fmax(M, pm[static_cast<int64_t>(c) * it.Nq]);
    double lp = -INFINITY;
    if (M > -INFINITY) {
      double S = 0.0;
      for (int c = 0; c < it.ngroups; ++c) {
        const double mg = pm[static_cast<int64_t>(c) * it.Nq];
        if (mg > -INFINITY) S += ps[static_cast<int64_t>(c) * it.Nq] * exp(mg - M);
      }
      lp = M + log(S) - lognorm;
      if (it.loo) lp -= log(1.0 - it.w[q]);
    }
    if (it.out) {
      const int64_t o = it.perm ? it.perm[q] - 1 : q;
      if (o >= 0 && o < it.Nq) it.out[o] = lp;
    }
    if (it.qw) {
      const double W = it.qw[q];
      if (W != 0.0) {
        if (lp == -INFINITY) zero = 1;
        else term = W * lp;
      }
    }
  }
  if (!it.logl) return;  // (block-uniform)
  red[threadIdx.x] = term;
  const int anyzero = __syncthreads_or(zero);
  for (int off = kFinishThreads / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    it.bpart[fb] = red[0];
    it.bzero[fb] = anyzero;
  }
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

// d_masks: the items' circular masks (all nonzero), or null: Euclidean items; logdom: log-domain items
int launch_partial(int D, const EvalItem *d_items, const int32_t *d_first, int n, int blocks, const uint32_t *d_masks,
                   bool logdom, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(blocks)), block(kEvalThreads);
  KDEHIP_CHECK_RC(dispatch_dims(D, [&](auto dim) {
    constexpr int kD = decltype(dim)::value;
    if (logdom) {
      if (d_masks) hipLaunchKernelGGL((eval_partial_log_kernel<kD, true>), grid, block, 0, st, d_items, d_first, n, d_masks);
      else hipLaunchKernelGGL((eval_partial_log_kernel<kD, false>), grid, block, 0, st, d_items, d_first, n,
                              static_cast<const uint32_t *>(nullptr));
    } else if (d_masks) hipLaunchKernelGGL((eval_partial_kernel<kD, true>), grid, block, 0, st, d_items, d_first, n, d_masks);
    else hipLaunchKernelGGL((eval_partial_kernel<kD, false>), grid, block, 0, st, d_items, d_first, n,
                            static_cast<const uint32_t *>(nullptr));
  }));
  KDEHIP_CHECK(hipGetLastError());
  return KDEHIP_OK;
}

// The blocks of one call: ONE device block [caller's data | descriptors | first[] | results | per item: partial, shares,
// flags] and ONE pinned image of everything up to and including the results; what precedes the results goes up in one copy.
// Protocol: fill `items` (sizes, D, loo, what to compute) -> alloc(prefix bytes of caller data) -> the caller writes its
// data into host() and points the items at dev() -> enqueue(stream) (= upload + launch) -> wait() (blocking calls) or
// defer(stream) (enqueue-only calls).  The results are one double per item (an item's log-likelihood), or as many as a
// blocking caller asks alloc for (the host evaluation's Nq values): wait() brings them back in one copy.
class EvalRun {
 public:
  std::vector<EvalItem> items;
  std::vector<uint32_t> circ;  // per item: its circular dimensions (bit k = dimension k); shorter than `items`: 0 for the rest
  int alloc(size_t prefix, size_t nresults = 0) {  // nresults == 0: one per item
    const size_t n = items.size();
    int64_t pblocks = 0, fblocks = 0;
    for (EvalItem &it : items) {
      const GroupSplit gs = split_chunks(it.N, it.Nq, 1);
      it.chunks_per_group = gs.chunks_per_group;
      it.ngroups = it.Nq > 0 ? gs.ngroups : 0;
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      pblocks += ((it.Nq + kEvalThreads - 1) / kEvalThreads) * it.ngroups;
      fblocks += it.nfb;
    }
    if (pblocks > INT32_MAX || fblocks > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "evaluation too large for one launch");
    Carve c;
    c.take(prefix);
    o_items_ = c.take(sizeof(EvalItem) * n);
    o_first_ = c.take(sizeof(int32_t) * 2 * (n + 1) + sizeof(uint32_t) * n);  // first[] of both kernels, then the masks
    o_masks_ = o_first_ + sizeof(int32_t) * 2 * (n + 1);
    nres_ = nresults ? nresults : n;
    o_res_ = c.take(sizeof(double) * nres_);
    scratch_.resize(n);
    for (size_t k = 0; k < n; ++k) {
      const EvalItem &it = items[k];
      scratch_[k] = c.take(sizeof(double) * ((it.logdom ? 2 : 1) * it.ngroups * it.Nq + it.nfb) + sizeof(int32_t) * it.nfb);
    }
    KDEHIP_CHECK(blk_.alloc(c.mark(), o_res_ + sizeof(double) * nres_));
    return KDEHIP_OK;
  }
  unsigned char *dev() const { return blk_.dev(); }
  unsigned char *host() const { return blk_.host(); }
  double *result(size_t k) const { return reinterpret_cast<double *>(dev() + o_res_) + k; }  // (device) result k: item k's own slot
  double *host_result(size_t k) const { return reinterpret_cast<double *>(host() + o_res_) + k; }

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
      unsigned char *s = dev() + scratch_[k];
      it.partial = reinterpret_cast<double *>(s);
      it.bpart = it.partial + static_cast<int64_t>(it.logdom ? 2 : 1) * it.ngroups * it.Nq;
      it.bzero = reinterpret_cast<int32_t *>(it.bpart + it.nfb);
    }
    circ.resize(n, 0u);
    {
      std::vector<size_t> ord(n);
      for (size_t k = 0; k < n; ++k) ord[k] = k;
      auto key = [&](size_t k) { return (items[k].logdom ? 1024 : 0) + 2 * items[k].D + (circ[k] ? 1 : 0); };
      std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return key(a) < key(b); });
      std::vector<EvalItem> si(n);
      std::vector<uint32_t> sc(n);
      for (size_t k = 0; k < n; ++k) { si[k] = items[ord[k]]; sc[k] = circ[ord[k]]; }
      items.swap(si);
      circ.swap(sc);
    }
    if (n) std::memcpy(host() + o_masks_, circ.data(), sizeof(uint32_t) * n);
    int32_t *pfirst = reinterpret_cast<int32_t *>(host() + o_first_), *ffirst = pfirst + (n + 1);
    pfirst[0] = ffirst[0] = 0;
    for (size_t k = 0; k < n; ++k) {
      const EvalItem &it = items[k];
      pfirst[k + 1] = pfirst[k] + static_cast<int32_t>(((it.Nq + kEvalThreads - 1) / kEvalThreads) * it.ngroups);
      ffirst[k + 1] = ffirst[k] + it.nfb;
    }
    if (n) std::memcpy(host() + o_items_, items.data(), sizeof(EvalItem) * n);
    KDEHIP_CHECK(blk_.upload(o_res_, st));
    return KDEHIP_OK;
  }
  // the launches behind the upload: two kernels (and their log-domain twins for the log-domain items), and the per-item
  // reduce when an item asks for a log-likelihood
  int launch() {
    const hipStream_t st = blk_.stream();
    const size_t n = items.size();
    const int32_t *pfirst = reinterpret_cast<const int32_t *>(host() + o_first_), *ffirst = pfirst + (n + 1);
    const EvalItem *d_items = reinterpret_cast<const EvalItem *>(dev() + o_items_);
    const int32_t *d_pfirst = reinterpret_cast<const int32_t *>(dev() + o_first_), *d_ffirst = d_pfirst + (n + 1);
    const uint32_t *d_masks = reinterpret_cast<const uint32_t *>(dev() + o_masks_);
    for (size_t a = 0; a < n;) {  // one launch per distinct D, and one more for its circular and for its log-domain items
      size_t e = a;
      while (e < n && items[e].D == items[a].D && !circ[e] == !circ[a] && items[e].logdom == items[a].logdom) ++e;
      const int blocks = pfirst[e] - pfirst[a];
      if (blocks > 0) {
        KDEHIP_CHECK_RC(launch_partial(items[a].D, d_items + a, d_pfirst + a, static_cast<int>(e - a), blocks,
                                       circ[a] ? d_masks + a : nullptr, items[a].logdom != 0, st));
      }
      a = e;
    }
    size_t nd = 0;  // the direct items are the first nd
    while (nd < n && !items[nd].logdom) ++nd;
    if (ffirst[nd] > 0)
      hipLaunchKernelGGL(eval_finish_kernel, dim3(static_cast<unsigned>(ffirst[nd])), dim3(kFinishThreads), 0, st, d_items,
                         d_ffirst, static_cast<int>(nd));
    if (ffirst[n] > ffirst[nd])
      hipLaunchKernelGGL(eval_finish_log_kernel, dim3(static_cast<unsigned>(ffirst[n] - ffirst[nd])), dim3(kFinishThreads), 0,
                         st, d_items + nd, d_ffirst + nd, static_cast<int>(n - nd));
    if (std::any_of(items.begin(), items.end(), [](const EvalItem &it) { return it.logl != nullptr; }))
      hipLaunchKernelGGL(logl_reduce_kernel, dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64), 0, st, d_items,
                         static_cast<int>(n));
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  // blocking calls: the results come back to host_result()
  int wait() {
    hipError_t e = hipSuccess;
    if (nres_) e = blk_.download(o_res_, sizeof(double) * nres_, blk_.stream());
    const hipError_t se = blk_.wait();
    KDEHIP_CHECK(e);
    KDEHIP_CHECK(se);
    return KDEHIP_OK;
  }
  // enqueue-only calls: both blocks go back once the work on the stream is done
  int defer(int device) {
    reap_deferred(device);
    return blk_.defer(device);
  }

 private:
  CallBlock blk_;
  size_t o_items_ = 0, o_first_ = 0, o_masks_ = 0, o_res_ = 0, nres_ = 0;
  std::vector<size_t> scratch_;
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

// the checks every resident entry makes; `at` may be bd
int check_pair(const kdehip_device_density *bd, const kdehip_device_density *at, int loo) {
  if (!bd || !at) return set_error(KDEHIP_ERR_ARG, "null density");
  if (loo && at != bd) return set_error(KDEHIP_ERR_ARG, "leave_one_out needs at == bd");
  if (bd->D < 1 || bd->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (at->D != bd->D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "evaluate -- dimensions of two BallTreeDensities must match");
  if (at->device != bd->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  if (!leaves_share_bandwidth(bd))
    return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths are not supported (the reference's kde! never builds them)");
  return KDEHIP_OK;
}

// bd at at's leaf points (tree order; out, if any, through at's permutation), W = at's leaf weights
EvalItem pair_item(const kdehip_device_density *bd, const kdehip_device_density *at, int loo, bool logl, bool logdom) {
  EvalItem it{};
  const int64_t N = bd->N, Nq = at->N;
  const int D = bd->D;
  it.src = bd->means + N * D; it.w = bd->weights + N; it.bw = bd->bandwidth + N * D;
  it.qry = at->means + Nq * D;
  it.qw = logl ? at->weights + Nq : nullptr;
  it.perm = at->perm + Nq;
  it.norm0 = std::pow(2.0 * M_PI, D / 2.0);
  it.N = N; it.Nq = Nq; it.D = D; it.loo = loo ? 1 : 0; it.logdom = logdom ? 1 : 0;
  return it;
}

}  // namespace

extern "C" int kdehip_evaluate(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out,
                               double *p_out, int device) {
  return kdehip_evaluate_manifold(bd, pos, Nq, leave_one_out, p_out, device, nullptr);
}

// The bodies of the entries: `logdom` selects the log-domain kernels (section 5f); everything else -- checks, layout of the
// call's block, streams -- is shared, so a log-domain entry refuses what its direct twin refuses, with the same words.
static int evaluate_host(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, double *p_out, int device,
                         const uint8_t *manifold, bool logdom) {
  if (!bd || !p_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  const int D = static_cast<int>(bd->ndim);
  const int64_t N = bd->npts;
  if (D < 1 || D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (N < 1 || !bd->means || !bd->bandwidth || !bd->weights || !bd->permutation)
    return set_error(KDEHIP_ERR_ARG, "malformed density");
  if (leave_one_out) Nq = N;
  else if (!pos || Nq < 0) return set_error(KDEHIP_ERR_ARG, "pos must hold Nq >= 0 points");
  if (Nq == 0) return KDEHIP_OK;
  // the reference's evalDirect reads ONE bandwidth vector (bandwidthMin[1..D], BallTreeDensity01.jl:98)
  const double *bw = bd->bandwidth + N * D;
  for (int64_t i = 0; i < N; ++i)
    for (int k = 0; k < D; ++k)
      if (bd->bandwidth[(N + i) * D + k] != bw[k])
        return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths are not supported (the reference's kde! never builds them)");
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != KDEHIP_OK) return rc;
  hipStream_t st = hipStreamPerThread;  // the calling thread's own stream, like every blocking entry point (kdehip.h)
  // caller data: [leaf means (leaf centres == the points, tree order) | leaf weights | leaf bandwidth | queries, or
  // (leave-one-out) the leaf row of the permutation: p[getIndexOf(locations, j)] (:335), results in the caller's original
  // order].  ONE pinned image goes up in one DMA and the Nq results come back in one; everything is enqueued on the
  // calling thread's stream and the host waits once (pageable hipMemcpy calls, one per array, cost more than the kernel
  // for anything below ~10^8 kernel evaluations).
  const size_t o_w = sizeof(double) * N * D, o_bw = o_w + sizeof(double) * N, o_q = o_bw + sizeof(double) * D;
  const size_t prefix = o_q + (leave_one_out ? sizeof(int64_t) * N : sizeof(double) * Nq * D);
  EvalRun run;
  EvalItem it{};
  it.norm0 = std::pow(2.0 * M_PI, D / 2.0);
  it.N = N; it.Nq = Nq; it.D = D; it.loo = leave_one_out ? 1 : 0; it.logdom = logdom ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix, static_cast<size_t>(Nq)));
  unsigned char *h = run.host(), *d = run.dev();
  std::memcpy(h, bd->means + N * D, sizeof(double) * N * D);
  std::memcpy(h + o_w, bd->weights + N, sizeof(double) * N);
  std::memcpy(h + o_bw, bw, sizeof(double) * D);
  if (leave_one_out) std::memcpy(h + o_q, bd->permutation + N, sizeof(int64_t) * N);
  else std::memcpy(h + o_q, pos, sizeof(double) * Nq * D);
  EvalItem &ri = run.items[0];
  ri.src = reinterpret_cast<const double *>(d);
  ri.w = reinterpret_cast<const double *>(d + o_w);
  ri.bw = reinterpret_cast<const double *>(d + o_bw);
  ri.qry = leave_one_out ? ri.src : reinterpret_cast<const double *>(d + o_q);
  ri.perm = leave_one_out ? reinterpret_cast<const int64_t *>(d + o_q) : nullptr;
  ri.out = run.result(0);
  KDEHIP_CHECK_RC(run.upload(st));
  PhaseTimer timer(kPhaseEvaluate, st);  // kdehip_profile_phase_read: the two launches, not the copies
  KDEHIP_CHECK_RC(run.launch());
  timer.stop();
  KDEHIP_CHECK_RC(run.wait());
  timer.collect();
  std::memcpy(p_out, run.host_result(0), sizeof(double) * Nq);
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
  const double *bw = bd->bandwidth + N * D;
  for (int64_t i = 0; i < N; ++i)
    for (int k = 0; k < D; ++k)
      if (bd->bandwidth[(N + i) * D + k] != bw[k])
        return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths are not supported (the reference's kde! never builds them)");
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != KDEHIP_OK) return rc;
  hipStream_t st = hipStreamPerThread;
  const bool self = at == bd;
  // caller data: [bd leaf means | bd leaf weights | bd leaf bandwidth | at leaf means | at leaf weights] (at == bd: none)
  const size_t o_w = sizeof(double) * N * D, o_bw = o_w + sizeof(double) * N, o_q = o_bw + sizeof(double) * D;
  const size_t o_qw = o_q + (self ? 0 : sizeof(double) * Nq * D), prefix = o_qw + (self ? 0 : sizeof(double) * Nq);
  EvalRun run;
  EvalItem it{};
  it.norm0 = std::pow(2.0 * M_PI, D / 2.0);
  it.N = N; it.Nq = Nq; it.D = static_cast<int32_t>(D); it.loo = leave_one_out ? 1 : 0; it.logdom = logdom ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix));
  unsigned char *h = run.host(), *d = run.dev();
  std::memcpy(h, bd->means + N * D, sizeof(double) * N * D);
  std::memcpy(h + o_w, bd->weights + N, sizeof(double) * N);
  std::memcpy(h + o_bw, bw, sizeof(double) * D);
  if (!self) {
    std::memcpy(h + o_q, at->means + Nq * D, sizeof(double) * Nq * D);
    std::memcpy(h + o_qw, at->weights + Nq, sizeof(double) * Nq);
  }
  EvalItem &ri = run.items[0];
  ri.src = reinterpret_cast<const double *>(d);
  ri.w = reinterpret_cast<const double *>(d + o_w);
  ri.bw = reinterpret_cast<const double *>(d + o_bw);
  ri.qry = self ? ri.src : reinterpret_cast<const double *>(d + o_q);
  ri.qw = self ? ri.w : reinterpret_cast<const double *>(d + o_qw);
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
    const int rc = check_pair(items[i].bd, items[i].at, items[i].leave_one_out);
    if (rc != KDEHIP_OK) return rc;
    if (items[i].bd->device != items[0].bd->device) return set_error(KDEHIP_ERR_ARG, "evalAvgLogL batch: densities on different devices");
    if (items[i].circular_mask >> items[i].bd->D)
      return set_error(KDEHIP_ERR_ARG, "evalAvgLogL batch: circular_mask names a dimension the densities do not have");
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != KDEHIP_OK) return rc;
  EvalRun run;
  for (int i = 0; i < n; ++i) {
    run.items.push_back(pair_item(items[i].bd, items[i].at, items[i].leave_one_out, true, logdom));
    run.items.back().logl = d_out + i;
    run.circ.push_back(items[i].circular_mask);
  }
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return run.defer(device);
}

extern "C" int kdehip_eval_avg_logl_device(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                           double *out) {
  return kdehip_eval_avg_logl_device_manifold(bd, at, leave_one_out, out, nullptr);
}

static int eval_avg_logl_resident(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                  double *out, const uint8_t *manifold, bool logdom) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  int rc = check_pair(bd, at, leave_one_out);
  if (rc != KDEHIP_OK) return rc;
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  rc = guard.enter(bd->device);
  if (rc != KDEHIP_OK) return rc;
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
  if (Nq < 0 || (Nq > 0 && !d_pos)) return set_error(KDEHIP_ERR_ARG, "d_pos must hold Nq >= 0 points");
  int rc = check_pair(bd, bd, 0);
  if (rc != KDEHIP_OK) return rc;
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  rc = guard.enter(bd->device);
  if (rc != KDEHIP_OK) return rc;
  EvalRun run;
  EvalItem it = pair_item(bd, bd, 0, false, logdom);
  it.qry = d_pos; it.perm = nullptr; it.Nq = Nq; it.out = d_out;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return run.defer(bd->device);
}

extern "C" int kdehip_evaluate_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out,
                                         void *stream) {
  return kdehip_evaluate_device_at_manifold(bd, at, d_out, stream, nullptr);
}

static int evaluate_resident_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out, void *stream,
                                const uint8_t *manifold, bool logdom) {
  if (!d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  int rc = check_pair(bd, at, at == bd);
  if (rc != KDEHIP_OK) return rc;
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  rc = guard.enter(bd->device);
  if (rc != KDEHIP_OK) return rc;
  EvalRun run;
  EvalItem it = pair_item(bd, at, at == bd, false, logdom);
  it.out = d_out;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return run.defer(bd->device);
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
