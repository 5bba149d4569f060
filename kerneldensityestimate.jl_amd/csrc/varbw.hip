// varbw.hip -- evaluation and log-likelihoods of densities whose points each have a bandwidth of their own, on gfx950
// (include/kdehip.h section 5o).  The reference's layout allows such densities (`bandwidth` is D x 2N, multibandwidth = 1,
// src/BallTreeDensity01.jl:11-24) and its evalDirect is written for one vector; here the sum is
//   p(x) = (2 pi)^(-D/2) sum_i w_i / prod_k sqrt(v_ik) exp(-1/2 sum_k diff_k(x_k, c_ik)^2 / v_ik)
// with the normaliser inside the sum, since it differs per source.  The skeleton is evaluate.hip's:
//   varbw_prepass_kernel     one thread per leaf, in leaf order, into the call's block: nh_ik = -0.5 / v_ik and the folded
//                            normaliser c_i = w_i / prod_k sqrt(v_ik), or (log-domain items) lc_i = log w_i - 1/2 sum_k log v_ik;
//   varbw_partial_kernel<D>  the sweep of pair_sweep.hpp (pair_sweep_var: 2D + 1 staged values per source), one partial per
//                            (group of source chunks, query): the plain sum, or (m, s) of the log-domain step;
//   varbw_finish_kernel      the groups combined in group order (no atomics), the norm, leave-one-out's 1 - w_q, the value
//                            stored (through the item's permutation, if any), W_q log p_q and the block's share in a fixed
//                            LDS tree; a query with a NaN coordinate gets NaN;
//   varbw_logl_kernel        only for a log-likelihood: the block shares in block order (or -Inf if a flag is up).
// The group split is split_chunks(N, Nq, 1), a function of (N, Nq) alone: the host entry, a resident call and a second run
// give the same bits.  A density with one bandwidth vector is accepted like any other; its values agree with evaluate.hip's
// to rounding, not bit for bit (there the normaliser is applied once, after the sum).
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
#include "phase_timer.hpp"

using namespace kdehip;

namespace {

constexpr int kFinishThreads = 256;  // queries per finish block
constexpr int kPrepassThreads = 256;

// One evaluation: a density (N source points in leaf order, N x D variances) at Nq query points.
struct VarItem : PairHead {
  const double *var;    // [N][D] the leaves' variances
  const double *qw;     // [Nq] query weights (the `at` density's leaf weights), or null: no log-likelihood
  const int64_t *perm;  // [Nq] 1-based output position of query q, or null: query order
  double *out;          // [Nq] p or log p, or null
  double *nh;           // [N][D] -1/(2 v_ik)                        (prepass)
  double *cc;           // [N] c_i, or lc_i for a log-domain item    (prepass)
  double *partial;      // [ngroups][Nq]; log-domain: [2][ngroups][Nq], the maxima m then the sums s
  double *bpart;        // [nfb] the finish blocks' shares of sum W log p
  int32_t *bzero;       // [nfb] the finish block met a p == 0 (log p == -Inf) with W != 0
  double *logl;         // the result, or null
  double norm0;         // (2 pi)^(D/2) as the host's libm rounds it
  double lognorm0;      // (D/2) log(2 pi), likewise
  int32_t ngroups, nfb, D, loo;
  int32_t logdom, pad_;
};

// nh, and c_i = w_i / prod_k sqrt(v_ik) (k ascending, correctly rounded roots: a product of the variances themselves would
// leave the range of fp64 for small bandwidths in 8-D) or lc_i = log w_i - 1/2 sum_k log v_ik (-Inf for w_i == 0)
__global__ __launch_bounds__(kPrepassThreads) void varbw_prepass_kernel(const VarItem *__restrict__ items) {
  const VarItem it = items[blockIdx.y];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kPrepassThreads + threadIdx.x;
  if (i >= it.N) return;
  double prod = 1.0, slog = 0.0;
  for (int k = 0; k < it.D; ++k) {
    const double v = it.var[i * it.D + k];
    it.nh[i * it.D + k] = -0.5 / v;
    prod *= __dsqrt_rn(v);
    slog += log(v);
  }
  const double w = it.w[i];
  it.cc[i] = it.logdom ? log(w) - 0.5 * slog : w / prod;
}

// partial[g][q] = sum over the chunks of group g, in chunk order, of sum_{i in chunk, (i != q if loo)} c_i exp(a_i)
template <int D, bool CIRC = false>
__global__ __launch_bounds__(kEvalThreads) void varbw_partial_kernel(const VarItem *__restrict__ items,
                                                                     const int32_t *__restrict__ first, int n,
                                                                     const uint32_t *__restrict__ masks = nullptr) {
  __shared__ double sSrc[2][kEvalChunk * (2 * D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const VarItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double total = 0.0;
  pair_sweep_var<D, CIRC>(pb, pb.nh, pb.cc, at, circ, sSrc, [&](auto &&each) {
    double sum = 0.0;
    each([&](int64_t i, double c, double a) {
      double v = c * exp_nonpos(a, sExpTab);
      if (pb.loo && i == at.q) v = 0.0;  // leave-one-out: skip the self term
      sum += v;
    });
    total += sum;
  });
  if (at.q < pb.Nq) pb.partial[at.grp * pb.Nq + at.q] = total;
}

// The log-domain step: t_i = a_i + lc_i, and the block carries
//   m = max t_i,  s = sum exp(t_i - m)   over S = { i in the group : w_i > 0, (i != q if loo) }
// with s rescaled once per chunk, as eval_partial_log_kernel does.  The maximum is over t_i, not a_i: the normalisers differ
// per source, so the largest a_i need not be the largest term.  w_i > 0 is read off lc_i > -Inf (a NaN fails it too).
// partial[g][q] = m, partial[ngroups + g][q] = s.
template <int D, bool CIRC = false>
__global__ __launch_bounds__(kEvalThreads) void varbw_partial_log_kernel(const VarItem *__restrict__ items,
                                                                         const int32_t *__restrict__ first, int n,
                                                                         const uint32_t *__restrict__ masks = nullptr) {
  __shared__ double sSrc[2][kEvalChunk * (2 * D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const VarItem pb = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  const int64_t skip = pb.loo ? at.q : -1;  // leave-one-out: the self term is not in S
  double m = -INFINITY, total = 0.0;
  pair_sweep_var<D, CIRC>(pb, pb.nh, pb.cc, at, circ, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t i, double lc, double a) { cm = (lc > -INFINITY && i != skip) ? fmax(cm, a + lc) : cm; });
    if (cm > m) {  // (m == -Inf: total is still 0)
      total *= exp_nonpos(m - cm, sExpTab);
      m = cm;
    }
    double sum = 0.0;
    each([&](int64_t i, double lc, double a) {
      const bool in = lc > -INFINITY && i != skip;  // in S: then a + lc <= m
      sum += in ? exp_nonpos((a + lc) - m, sExpTab) : 0.0;
    });
    total += sum;
  });
  if (at.q < pb.Nq) {
    pb.partial[at.grp * pb.Nq + at.q] = m;
    pb.partial[(pb.ngroups + at.grp) * pb.Nq + at.q] = total;
  }
}

// Both domains' finish, one thread per query (items [0, n), item i owns blocks [first[i], first[i+1])):
//   direct  p = (sum over the groups, in group order) / (2 pi)^(D/2) [/ (1 - w_q)]; evalAvgLogL's term as
//           src/DualTree01.jl:456-466: a p == 0 counts as 1 when its weight is 0 and makes the result -Inf otherwise;
//   log     M = max m_g, S = sum s_g exp(m_g - M), log p = M + log S - (D/2) log 2pi [- log(1 - w_q)], -Inf when no group
//           has a source in S; W log p summed over the W != 0 only, a weighted -Inf raises the block's flag.
__global__ __launch_bounds__(kFinishThreads) void varbw_finish_kernel(const VarItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n) {
  __shared__ double red[kFinishThreads];
  const ItemBlock ib = item_block(first, n);
  const VarItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  double value = it.logdom ? -INFINITY : 0.0, term = 0.0;
  int zero = 0;
  if (q < it.Nq) {
    const double *pm = it.partial + q;
    if (it.logdom) {
      const double *ps = pm + static_cast<int64_t>(it.ngroups) * it.Nq;
      double M = -INFINITY;
      for (int c = 0; c < it.ngroups; ++c) M = fmax(M, pm[static_cast<int64_t>(c) * it.Nq]);
      if (M > -INFINITY) {
        double S = 0.0;
        for (int c = 0; c < it.ngroups; ++c) {
          const double mg = pm[static_cast<int64_t>(c) * it.Nq];
          if (mg > -INFINITY) S += ps[static_cast<int64_t>(c) * it.Nq] * exp(mg - M);
        }
        value = M + log(S) - it.lognorm0;
        if (it.loo) value -= log(1.0 - it.w[q]);
      }
    } else {
      double s = 0.0;
      for (int c = 0; c < it.ngroups; ++c) s += pm[static_cast<int64_t>(c) * it.Nq];
      value = s / it.norm0;
      if (it.loo) value = value / (1.0 - it.w[q]);
    }
    if (query_has_nan(it.qry, q, it.D)) value = __builtin_nan("");  // (the sweep drops a NaN: pair_sweep.hpp)
    if (it.qw) {
      const double W = it.qw[q];
      if (it.logdom) {
        if (W != 0.0) {
          if (value == -INFINITY) zero = 1;
          else term = W * value;
        }
      } else {
        double L = value;
        if (L == 0.0) { zero = W != 0.0; L = 1.0; }
        term = log(L) * W;
      }
    }
    if (it.out) {
      const int64_t o = it.perm ? it.perm[q] - 1 : q;
      if (o >= 0 && o < it.Nq) it.out[o] = value;  // (an uploaded density's permutation is the caller's)
    }
  }
  if (!it.logl) return;  // (block-uniform)
  red[threadIdx.x] = term;
  const int anyzero = __syncthreads_or(zero);
  const double share = block_tree_sum<kFinishThreads>(red);
  if (threadIdx.x == 0) {
    it.bpart[ib.k] = share;
    it.bzero[ib.k] = anyzero;
  }
}

// one thread per item: the block shares in block order
__global__ void varbw_logl_kernel(const VarItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const VarItem it = items[i];
  if (!it.logl) return;
  double s = 0.0;
  int zero = 0;
  for (int b = 0; b < it.nfb; ++b) {
    s += it.bpart[b];
    zero |= it.bzero[b];
  }
  *it.logl = zero ? -INFINITY : s;
}

// The run of one call (pair_sweep.hpp PairRun) with the scratch of its item, [nh | cc | partial | shares | flags].  A call
// evaluates ONE item (there is no batched entry); the descriptors, first[] arrays and launches are the skeleton's all the
// same.  Protocol as EvalRun's: fill items[0] and circ -> alloc(prefix bytes of caller data, results) -> the caller writes
// its data into host() and points the item at dev() -> enqueue(stream) -> wait(), defer(device) or keep(device).
class VarRun : public PairRun<VarItem> {
 public:
  int alloc(size_t prefix, size_t nresults) {
    VarItem &it = items[0];
    const int64_t pblocks = split(it);
    it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
    if (pblocks > INT32_MAX || (it.N + kPrepassThreads - 1) / kPrepassThreads > INT32_MAX)
      return set_error(KDEHIP_ERR_UNSUPPORTED, "evaluation too large for one launch");
    Carve c;
    carve_head(c, prefix, 2, 0, nresults);  // first[] of the sweep and of the finish
    o_nh_ = c.take(sizeof(double) * it.N * (it.D + 1));
    o_scratch_ = c.take(sizeof(double) * ((it.logdom ? 2 : 1) * it.ngroups * it.Nq + it.nfb) + sizeof(int32_t) * it.nfb);
    KDEHIP_CHECK(alloc_block(c));
    return KDEHIP_OK;
  }
  int enqueue(hipStream_t st) {
    KDEHIP_CHECK_RC(upload(st));
    return launch();
  }
  // scratch pointers, descriptors and first[] arrays written, one upload on `st`
  int upload(hipStream_t st) {
    VarItem &it = items[0];
    it.nh = reinterpret_cast<double *>(dev() + o_nh_);
    it.cc = it.nh + it.N * it.D;
    it.partial = reinterpret_cast<double *>(dev() + o_scratch_);
    it.bpart = it.partial + static_cast<int64_t>(it.logdom ? 2 : 1) * it.ngroups * it.Nq;
    it.bzero = reinterpret_cast<int32_t *>(it.bpart + it.nfb);
    prepare([&](size_t k) { return (items[k].logdom ? 1024 : 0) + 2 * items[k].D + (circ[k] ? 1 : 0); });
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    ffirst[1] = items[0].nfb;
    KDEHIP_CHECK(send(st));
    return KDEHIP_OK;
  }
  // the launches behind the upload: prepass, sweep, finish, and the reduce when the item asks for a log-likelihood
  int launch() {
    const hipStream_t st = stream();
    const VarItem &it = items[0];
    const int32_t *ffirst = first(1);
    hipLaunchKernelGGL(varbw_prepass_kernel, dim3(static_cast<unsigned>((it.N + kPrepassThreads - 1) / kPrepassThreads), 1),
                       dim3(kPrepassThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    KDEHIP_CHECK_RC(for_each_run([&](const VarItem &ri, const VarItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *d_masks) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(ri.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        if (ri.logdom)
          launch_pair<VarItem>(varbw_partial_log_kernel<kD, false>, varbw_partial_log_kernel<kD, true>, blocks, st, d_it,
                               d_pfirst, cnt, d_masks);
        else
          launch_pair<VarItem>(varbw_partial_kernel<kD, false>, varbw_partial_kernel<kD, true>, blocks, st, d_it, d_pfirst,
                               cnt, d_masks);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    if (ffirst[1] > 0)
      hipLaunchKernelGGL(varbw_finish_kernel, dim3(static_cast<unsigned>(ffirst[1])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(1), 1);
    if (items[0].logl) hipLaunchKernelGGL(varbw_logl_kernel, dim3(1), dim3(64), 0, st, d_items(), 1);
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }

 private:
  size_t o_nh_ = 0, o_scratch_ = 0;
};

VarItem blank_item(int64_t N, int64_t Nq, int D, int loo, int logdom) {
  VarItem it{};
  it.norm0 = gauss_norm0(D);
  it.lognorm0 = 0.5 * D * std::log(2.0 * M_PI);
  it.N = N; it.Nq = Nq; it.D = D; it.loo = loo ? 1 : 0; it.logdom = logdom ? 1 : 0;
  return it;
}

// bd at at's leaf points (leaf order; out, if any, through at's permutation), W = at's leaf weights.  (The entries check the
// pair without the test of the bandwidths: they take any density.)
VarItem pair_item(const kdehip_device_density *bd, const kdehip_device_density *at, int loo, bool logl, int logdom) {
  const LeafRows src = leaf_rows(bd), qry = leaf_rows(at);
  VarItem it = blank_item(bd->N, at->N, bd->D, loo, logdom);
  it.src = src.src; it.w = src.w; it.var = src.bw;
  it.qry = qry.src;
  it.qw = logl ? qry.w : nullptr;
  it.perm = qry.perm;
  return it;
}

// one resident item on the caller's stream: enqueue only; on a capturing stream the call's blocks are kept (section 5h)
int enqueue_resident(const VarItem &it, uint32_t circ, int device, void *stream) {
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);
  VarRun run;
  run.items.push_back(it);
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(0, 1));
  KDEHIP_CHECK_RC(run.enqueue(st));
  return finish_enqueue(run, &scope, device);
}

}  // namespace

extern "C" int kdehip_density_uniform_bandwidth(const kdehip_device_density *h) {
  if (!h) {
    set_error(KDEHIP_ERR_ARG, "null density");
    return 0;
  }
  return leaves_share_bandwidth(h) ? 1 : 0;
}

extern "C" int kdehip_evaluate_varbw(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out,
                                     int log_domain, double *p_out, int device, const uint8_t *manifold) {
  if (!bd || !p_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  const int64_t N = bd->npts;
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (leave_one_out) Nq = N;
  else if (!pos || Nq < 0) return set_error(KDEHIP_ERR_ARG, "pos must hold Nq >= 0 points");
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  hipStream_t st = hipStreamPerThread;  // the calling thread's own stream, like every blocking entry point
  // caller data: [leaf means | leaf weights | leaf variances | queries, or (leave-one-out) the leaf row of the permutation]:
  // one pinned image up, the Nq results back, as kdehip_evaluate
  const size_t o_q = host_density_bytes(bd, true);
  const size_t prefix = o_q + (leave_one_out ? sizeof(int64_t) * N : sizeof(double) * Nq * D);
  VarRun run;
  run.items.push_back(blank_item(N, Nq, D, leave_one_out, log_domain));
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix, static_cast<size_t>(Nq)));
  unsigned char *h = run.host(), *d = run.dev();
  VarItem &ri = run.items[0];
  ri.var = pack_host_density(run, ri, bd, true);
  if (leave_one_out) std::memcpy(h + o_q, bd->permutation + N, sizeof(int64_t) * N);
  else std::memcpy(h + o_q, pos, sizeof(double) * Nq * D);
  ri.qry = leave_one_out ? ri.src : reinterpret_cast<const double *>(d + o_q);
  ri.perm = leave_one_out ? reinterpret_cast<const int64_t *>(d + o_q) : nullptr;
  ri.out = run.result(0);
  KDEHIP_CHECK_RC(run.upload(st));
  PhaseTimer timer(kPhaseEvaluate, st);  // kdehip_profile_phase_read: the launches, not the copies
  KDEHIP_CHECK_RC(run.launch());
  timer.stop();
  KDEHIP_CHECK_RC(run.wait());
  timer.collect();
  std::memcpy(p_out, run.host_result(0), sizeof(double) * Nq);
  return KDEHIP_OK;
}

extern "C" int kdehip_eval_avg_logl_varbw(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, int log_domain,
                                          double *out, int device, const uint8_t *manifold) {
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
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  hipStream_t st = hipStreamPerThread;
  const bool self = at == bd;
  // caller data: [bd leaf means | bd leaf weights | bd leaf variances | at leaf means | at leaf weights] (at == bd: none)
  const size_t o_q = host_density_bytes(bd, true), prefix = o_q + (self ? 0 : sizeof(double) * Nq * (D + 1));
  VarRun run;
  run.items.push_back(blank_item(N, Nq, static_cast<int>(D), leave_one_out, log_domain));
  run.circ.push_back(circ);
  KDEHIP_CHECK_RC(run.alloc(prefix, 1));
  VarItem &ri = run.items[0];
  ri.var = pack_host_density(run, ri, bd, true);
  const LeafArrays qry = self ? LeafArrays{ri.src, ri.w} : pack_leaves(run, o_q, at);
  ri.qry = qry.means;
  ri.qw = qry.weights;
  ri.logl = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(st));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}

extern "C" int kdehip_evaluate_varbw_device_at(const kdehip_device_density *bd, const kdehip_device_density *at,
                                               int leave_one_out, int log_domain, double *d_out, void *stream,
                                               const uint8_t *manifold) {
  if (!d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_pair(bd, at, leave_one_out, false));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (at->N == 0) return KDEHIP_OK;
  VarItem it = pair_item(bd, at, leave_one_out, false, log_domain);
  it.out = d_out;
  return enqueue_resident(it, circ, bd->device, stream);
}

extern "C" int kdehip_evaluate_varbw_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int log_domain,
                                            double *d_out, void *stream, const uint8_t *manifold) {
  if (!bd || !d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_query_count(d_pos, Nq, "d_pos must hold Nq >= 0 points"));
  KDEHIP_CHECK_RC(check_pair(bd, bd, 0, false));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (Nq == 0) return KDEHIP_OK;
  VarItem it = pair_item(bd, bd, 0, false, log_domain);
  it.qry = d_pos; it.perm = nullptr; it.Nq = Nq; it.out = d_out;
  return enqueue_resident(it, circ, bd->device, stream);
}

extern "C" int kdehip_eval_avg_logl_varbw_device(const kdehip_device_density *bd, const kdehip_device_density *at,
                                                 int leave_one_out, int log_domain, double *d_out, void *stream,
                                                 const uint8_t *manifold) {
  if (!d_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_pair(bd, at, leave_one_out, false));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  VarItem it = pair_item(bd, at, leave_one_out, true, log_domain);
  it.logl = d_out;
  return enqueue_resident(it, circ, bd->device, stream);
}
