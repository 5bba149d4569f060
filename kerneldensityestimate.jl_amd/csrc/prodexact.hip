// prodexact.hip -- the EXACT product of two densities (include/kdehip.h section 5p; the library's own: the reference has only
// the Gibbs samplers, the toolbox it descends from had productExact beside them).  For p (leaves a_i, weights alpha_i, ONE
// bandwidth vector u) and q (b_j, beta_j, v) the product is the mixture of the N1 N2 Gaussians
//   N(x; a_i + (b_j - a_i) u / s, u v / s),  s = u + v,  with weights alpha_i beta_j N(a_i - b_j; 0, s),
// so a draw is a label pair (i, j) by two inverse-CDF walks and one Gaussian; log int p q comes out of the same sums.
// Host densities (uploaded for the call, blocking) and resident ones (single, or batched and enqueue-only) run ONE path, any
// number of items described in device memory by ProdItem and driven by ProdRun:
//   prod_rows_kernel<D>     one launch per distinct D: the sweep of pair_sweep.hpp -- queries p's leaves, sources q's leaves
//                           and weights, nhib = -1 / (2 s_k) -- with the step of eval_partial_log_kernel: per (group, row) the
//                           maximum m and the rescaled sum; scratch [2][ngroups][N1];
//   prod_finish_kernel      per row the groups combined in group order: m_i, T_i, L_i = log alpha_i + m_i + log T_i;
//   prod_scan_kernel        ONE block per item: M = max L_i, R_i = exp(L_i - M), the inclusive scan of R_i in leaf order -- 256
//                           contiguous segments, each summed left to right, the segment totals summed left to right into
//                           offsets, cum_i = offset + the running sum: non-decreasing, and constant across a row with
//                           R_i = 0, whatever the launch --, R = the last value, logz;
//   prod_draw_kernel<D>     one lane per draw, blocks (draw block, group of q's chunks): the lane forms its two uniforms,
//                           finds its row i by bisection of the scan, walks the row's group partials to the group its second
//                           threshold falls into; a block none of whose lanes chose its group returns before the sweep, the
//                           others walk the group's chunks with a_i as the lane's query and m = m_g fixed and keep the first
//                           leaf of S_q whose running sum exceeds the lane's residual (or the group's last leaf of S_q); the
//                           lane writes the labels through the two permutations, and the point;
//   prod_components_kernel  one thread per (i, j): the component's mean and normalised weight to ORIGINAL order.
// No atomics; one exp per (i, j) pair for the rows, at most one per (draw, j) for the labels; the group split
// (split_chunks(N2, N1, 1)) depends on the item's sizes alone, so the host entry, a resident call and any batch give the
// same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "density_args.hpp"
#include "device_density.hpp"
#include "entry_helpers.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"
#include "pair_sweep.hpp"
#include "philox.hpp"

using namespace kdehip;

namespace {

constexpr int kRowThreads = kEvalThreads;  // rows per finish block
constexpr int kScanThreads = 256;          // segments of the scan: fixed, the result must not depend on a launch
constexpr int64_t kMaxComponents = int64_t(1) << 20;

// One item: the product of p (the sweep's queries: N1 = Nq leaves) and q (the sweep's sources: N2 = N leaves).
struct ProdItem : PairHead {
  const double *pw;       // [N1] alpha
  const double *bwp;      // [D] u: p's first leaf's variances
  const double *bwq;      // [D] v
  const int64_t *permp;   // [N1] 1-based original position of p's leaf i
  const int64_t *permq;   // [N2]
  double *partial;        // [2][ngroups][N1]: m, s of (group, row)
  double *rows;           // [3][N1]: m_i, T_i, L_i
  double *cum;            // [N1] the inclusive scan of R_i
  double *mr;             // [3]: M, R, the last leaf of S_p (as a double; -1: none)
  double *pts;            // [Np][D] and
  int64_t *ind;           // [Np][2] the draws, or both null
  double *logz;           // [1], or null
  double *cmeans;         // [N1 N2][D], with
  double *cweights;       // [N1 N2] and
  double *cvar;           // [D]: the mixture itself, or all null
  uint64_t seed;
  int64_t offset, Np;
  double norm0;           // (2 pi)^(D/2)
  int32_t ngroups, nfb, ndb, D;
};

// partial[g][i] = m, partial[ngroups + g][i] = s over the chunks of group g: eval_partial_log_kernel's step on p's leaf rows
template <int D>
__global__ __launch_bounds__(kEvalThreads) void prod_rows_kernel(const ProdItem *__restrict__ items,
                                                                 const int32_t *__restrict__ first, int n) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const ProdItem pb = items[ib.item];
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double nhib[D];  // -1/(2 s_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / (pb.bwp[k] + pb.bwq[k]);
  double m = -INFINITY, total = 0.0;
  pair_sweep<D, false>(pb, at, 0u, nhib, sSrc, [&](auto &&each) {
    double cm = -INFINITY;
    each([&](int64_t, double w, double a) { cm = (w > 0.0) ? fmax(cm, a) : cm; });
    if (cm > m) {  // (m == -Inf: total is still 0)
      total *= exp_nonpos(m - cm, sExpTab);
      m = cm;
    }
    double sum = 0.0;
    each([&](int64_t, double w, double a) { sum += (w > 0.0) ? w * exp_nonpos(a - m, sExpTab) : 0.0; });  // in S_q: a <= m
    total += sum;
  });
  if (at.q < pb.Nq) {
    pb.partial[at.grp * pb.Nq + at.q] = m;
    pb.partial[(pb.ngroups + at.grp) * pb.Nq + at.q] = total;
  }
}

// Items [0, n), item i owns blocks [first[i], first[i+1]).  Row i: m_i = max_g m_g, T_i = sum_g s_g exp(m_g - m_i) in group
// order, L_i = log alpha_i + m_i + log T_i; -Inf outside S_p or where S_q is empty.
__global__ __launch_bounds__(kRowThreads) void prod_finish_kernel(const ProdItem *__restrict__ items,
                                                                  const int32_t *__restrict__ first, int n) {
  const ItemBlock ib = item_block(first, n);
  const ProdItem it = items[ib.item];
  const int64_t i = static_cast<int64_t>(ib.k) * kRowThreads + threadIdx.x, N1 = it.Nq;
  if (i >= N1) return;
  const double *pm = it.partial + i, *ps = pm + static_cast<int64_t>(it.ngroups) * N1;
  double mi = -INFINITY, T = 0.0;
  for (int g = 0; g < it.ngroups; ++g) mi = fmax(mi, pm[static_cast<int64_t>(g) * N1]);
  if (mi > -INFINITY) {
    for (int g = 0; g < it.ngroups; ++g) {
      const double mg = pm[static_cast<int64_t>(g) * N1];
      if (mg > -INFINITY) T += ps[static_cast<int64_t>(g) * N1] * exp(mg - mi);
    }
  }
  const double al = it.pw[i];
  it.rows[i] = mi;
  it.rows[N1 + i] = T;
  it.rows[2 * N1 + i] = (al > 0.0 && T > 0.0) ? log(al) + mi + log(T) : -INFINITY;
}

// ONE block per item (blockIdx.x = the item).  Thread t owns the rows [t len, (t + 1) len), len = ceil(N1 / 256).
__global__ __launch_bounds__(kScanThreads) void prod_scan_kernel(const ProdItem *__restrict__ items) {
  __shared__ double red[kScanThreads];
  __shared__ long long slast[kScanThreads];
  const ProdItem it = items[blockIdx.x];
  const int64_t N1 = it.Nq;
  const double *L = it.rows + 2 * N1;
  const int tid = static_cast<int>(threadIdx.x);
  double m = -INFINITY;
  long long last = -1;
  for (int64_t i = tid; i < N1; i += kScanThreads) {
    m = fmax(m, L[i]);
    if (it.pw[i] > 0.0) last = i;  // (ascending i)
  }
  red[tid] = m;
  slast[tid] = last;
  __syncthreads();
  for (int off = kScanThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] = fmax(red[tid], red[tid + off]);
      slast[tid] = slast[tid] > slast[tid + off] ? slast[tid] : slast[tid + off];
    }
    __syncthreads();
  }
  const double M = red[0];
  last = slast[0];
  __syncthreads();
  const int64_t len = (N1 + kScanThreads - 1) / kScanThreads;
  int64_t b = tid * len, e = b + len;
  if (b > N1) b = N1;
  if (e > N1) e = N1;
  double run = 0.0;
  for (int64_t i = b; i < e; ++i) {
    const double r = (L[i] > -INFINITY) ? exp(L[i] - M) : 0.0;
    it.cum[i] = r;
    run += r;
  }
  red[tid] = run;
  __syncthreads();
  double off = 0.0;
  for (int k = 0; k < tid; ++k) off += red[k];  // (every thread the same additions: off_{t+1} == off_t + total_t)
  run = 0.0;
  for (int64_t i = b; i < e; ++i) {
    run += it.cum[i];
    it.cum[i] = off + run;
  }
  if (tid == kScanThreads - 1) {
    const double R = off + run;
    it.mr[0] = M;
    it.mr[1] = R;
    it.mr[2] = static_cast<double>(last);
    if (it.logz) {
      const double norm = gauss_norm(it.norm0, it.D, [&](int k) { return it.bwp[k] + it.bwq[k]; });
      *it.logz = (M > -INFINITY) ? M + log(R) - log(norm) : -INFINITY;
    }
  }
}

// Items [0, n), item i owns blocks [first[i], first[i+1]): block kb of an item is draw block kb % dblocks of group kb / dblocks.
template <int D>
__global__ __launch_bounds__(kEvalThreads) void prod_draw_kernel(const ProdItem *__restrict__ items,
                                                                 const int32_t *__restrict__ first, int n) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const ProdItem pb = items[ib.item];
  const int64_t N1 = pb.Nq, dblocks = (pb.Np + kEvalThreads - 1) / kEvalThreads;
  const int64_t db = ib.k % dblocks, grp = ib.k / dblocks;
  const int64_t t = db * kEvalThreads + threadIdx.x;
  const bool live = t < pb.Np;
  const int64_t nchunks = (pb.N + kEvalChunk - 1) / kEvalChunk;
  const int64_t c_begin = grp * pb.chunks_per_group;
  const int64_t c_end = (c_begin + pb.chunks_per_group < nchunks) ? c_begin + pb.chunks_per_group : nchunks;
  if (c_begin >= c_end) return;  // block-uniform
  const double M = pb.mr[0], R = pb.mr[1];
  const uint64_t g = static_cast<uint64_t>(pb.offset + t);
  int64_t i = -1;
  int cg = -1;
  double res = INFINITY, mg = 0.0;
  if (live && M > -INFINITY) {
    const double T0 = philox_uniform(pb.seed, g, 1u) * R;  // (uniforms 1 and 2: what kdehip_philox_fill_uniform with K = 2 returns)
    int64_t lo = 0, hi = N1;  // the first row whose scan value exceeds T0
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (pb.cum[mid] > T0) hi = mid; else lo = mid + 1;
    }
    i = (lo < N1) ? lo : static_cast<int64_t>(pb.mr[2]);
    if (i >= 0 && i < N1) {
      const double mi = pb.rows[i], T1 = philox_uniform(pb.seed, g, 2u) * pb.rows[N1 + i];
      const double *pm = pb.partial + i, *ps = pm + static_cast<int64_t>(pb.ngroups) * N1;
      double run = 0.0;
      int lastg = -1;
      for (int k = 0; k < pb.ngroups; ++k) {  // the very additions that formed T_i
        const double mk = pm[static_cast<int64_t>(k) * N1];
        if (!(mk > -INFINITY)) continue;
        const double e = exp(mk - mi), sk = ps[static_cast<int64_t>(k) * N1];
        if (sk > 0.0) lastg = k;
        const double next = run + sk * e;
        if (next > T1) {  // (then e > 0)
          cg = k;
          res = (T1 - run) / e;
          break;
        }
        run = next;
      }
      if (cg < 0) cg = lastg;
      if (cg >= 0) mg = pm[static_cast<int64_t>(cg) * N1];
    }
  }
  if (live && cg < 0 && grp == 0) {  // S_p or S_q empty
    for (int k = 0; k < D; ++k) pb.pts[t * D + k] = __builtin_nan("");
    pb.ind[2 * t] = 0;
    pb.ind[2 * t + 1] = 0;
  }
  const bool mine = live && cg == static_cast<int>(grp);
  if (!__syncthreads_or(mine ? 1 : 0)) return;  // block-uniform, before the sweep's barriers
  double nhib[D];
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / (pb.bwp[k] + pb.bwq[k]);
  const PairPlace at = {grp, mine ? i : N1, c_begin, c_end};  // (a lane that is not mine walks with x = 0)
  double run = 0.0;
  int64_t found = -1, lastj = -1;
  pair_sweep<D, false>(pb, at, 0u, nhib, sSrc, [&](auto &&each) {
    each([&](int64_t j, double w, double a) {
      if (mine && found < 0 && w > 0.0) {  // in S_q: a <= m_g
        run += w * exp_nonpos(a - mg, sExpTab);
        lastj = j;
        if (run > res) found = j;
      }
    });
  });
  if (!mine) return;
  const int64_t lab = found >= 0 ? found : lastj;
  if (lab < 0 || lab >= pb.N) {  // (a chosen group has a leaf in S_q)
    for (int k = 0; k < D; ++k) pb.pts[t * D + k] = __builtin_nan("");
    pb.ind[2 * t] = 0;
    pb.ind[2 * t + 1] = 0;
    return;
  }
  double even = 0.0, odd = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if ((k & 1) == 0) philox_normal_pair(pb.seed, g, static_cast<uint32_t>(k >> 1), even, odd);
    const double nk = (k & 1) ? odd : even;
    const double u = pb.bwp[k], v = pb.bwq[k], s = u + v;
    const double a = pb.qry[i * D + k], b = pb.src[lab * D + k];
    const double mean = fma(b - a, u / s, a);
    const double sd = __dsqrt_rn(__ddiv_rn(__dmul_rn(u, v), s));
    pb.pts[t * D + k] = __dadd_rn(mean, __dmul_rn(sd, nk));
  }
  pb.ind[2 * t] = pb.permp[i];
  pb.ind[2 * t + 1] = pb.permq[lab];
}

// ONE item; thread t is the leaf pair (i, j) = (t / N2, t % N2): component c = (original index of i) N2 + (original index
// of j) gets its mean and the weight exp((log alpha_i + log beta_j + e_ij) - (M + log R)); 0 outside S_p x S_q.
__global__ __launch_bounds__(256) void prod_components_kernel(const ProdItem *__restrict__ items) {
  const ProdItem it = items[0];
  const int D = it.D;
  const int64_t N1 = it.Nq, N2 = it.N;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t == 0)
    for (int k = 0; k < D; ++k) it.cvar[k] = it.bwp[k] * it.bwq[k] / (it.bwp[k] + it.bwq[k]);
  if (t >= N1 * N2) return;
  const int64_t i = t / N2, j = t - i * N2;
  const int64_t io = it.permp[i] - 1, jo = it.permq[j] - 1;
  if (io < 0 || io >= N1 || jo < 0 || jo >= N2) return;  // (an uploaded density's permutation is the caller's)
  const int64_t c = io * N2 + jo;
  double acc = 0.0;
  for (int k = 0; k < D; ++k) {
    const double u = it.bwp[k], s = u + it.bwq[k];
    const double a = it.qry[i * D + k], b = it.src[j * D + k];
    const double d = a - b;
    acc = fma(d * d, -0.5 / s, acc);
    it.cmeans[c * D + k] = fma(b - a, u / s, a);
  }
  const double al = it.pw[i], be = it.w[j], M = it.mr[0];
  it.cweights[c] = (al > 0.0 && be > 0.0 && M > -INFINITY) ? exp(((log(al) + log(be)) + acc) - (M + log(it.mr[1]))) : 0.0;
}

// The run of one call (pair_sweep.hpp PairRun) with the product's scratch, per item [partial | rows | cum | mr], and its
// launches.  Protocol: fill `items` (sizes, D, Np, seed, offset, norm0) -> alloc(prefix bytes of caller data, result doubles
// of the caller) -> the caller writes its data into host() and points the items at dev() -> run(stream) -> (ONE item)
// components() -> wait() or defer(device) / keep(device).
class ProdRun : public PairRun<ProdItem> {
 public:
  int alloc(size_t prefix, size_t nresults) {
    const size_t n = items.size();
    int64_t pblocks = 0, fblocks = 0, dblocks = 0;
    for (ProdItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kRowThreads - 1) / kRowThreads);
      fblocks += it.nfb;
      const int64_t nd = ((it.Np + kEvalThreads - 1) / kEvalThreads) * it.ngroups;
      if (nd > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many draws for one launch");
      it.ndb = static_cast<int32_t>(nd);
      dblocks += nd;
    }
    if (pblocks > INT32_MAX / 2 || fblocks > INT32_MAX / 2 || dblocks > INT32_MAX / 2)
      return set_error(KDEHIP_ERR_UNSUPPORTED, "too many points for one launch");
    Carve c;
    carve_head(c, prefix, 3, 0, nresults);  // first[] of the row sweep, of the finish kernel and of the draw kernel
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) scratch[k] = c.take(scratch_bytes(items[k]));
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) {
      ProdItem &it = items[k];
      it.partial = reinterpret_cast<double *>(dev() + scratch[k]);
      it.rows = it.partial + 2 * static_cast<int64_t>(it.ngroups) * it.Nq;
      it.cum = it.rows + 3 * it.Nq;
      it.mr = it.cum + it.Nq;
    }
    return KDEHIP_OK;
  }
  int run(hipStream_t st) {
    prepare([&](size_t k) { return items[k].D; });
    const size_t n = items.size();
    int32_t *ffirst = first(1), *dfirst = first(2);
    ffirst[0] = dfirst[0] = 0;
    for (size_t k = 0; k < n; ++k) {
      ffirst[k + 1] = ffirst[k] + items[k].nfb;
      dfirst[k + 1] = dfirst[k] + (items[k].pts ? items[k].ndb : 0);
    }
    KDEHIP_CHECK(send(st));
    if (n == 0) return KDEHIP_OK;
    KDEHIP_CHECK_RC(for_each_run([&](const ProdItem &it, const ProdItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        hipLaunchKernelGGL(prod_rows_kernel<kD>, dim3(static_cast<unsigned>(blocks)), dim3(kEvalThreads), 0, st, d_it, d_pfirst, cnt);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    hipLaunchKernelGGL(prod_finish_kernel, dim3(static_cast<unsigned>(ffirst[n])), dim3(kRowThreads), 0, st, d_items(), d_first(1),
                       static_cast<int>(n));
    KDEHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(prod_scan_kernel, dim3(static_cast<unsigned>(n)), dim3(kScanThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    for (size_t a = 0; a < n;) {  // the draws: one launch per distinct D (the items are sorted by D)
      size_t e = a;
      while (e < n && items[e].D == items[a].D) ++e;
      const int blocks = dfirst[e] - dfirst[a];
      if (blocks > 0) {
        KDEHIP_CHECK_RC(dispatch_dims(items[a].D, [&](auto dim) {
          constexpr int kD = decltype(dim)::value;
          hipLaunchKernelGGL(prod_draw_kernel<kD>, dim3(static_cast<unsigned>(blocks)), dim3(kEvalThreads), 0, st, d_items() + a,
                             d_first(2) + a, static_cast<int>(e - a));
        }));
        KDEHIP_CHECK(hipGetLastError());
      }
      a = e;
    }
    return KDEHIP_OK;
  }
  // (a run of ONE item) the mixture itself to the item's cmeans / cweights / cvar
  int components() {
    const ProdItem &it = items[0];
    const int64_t blocks = (it.N * it.Nq + 255) / 256;
    hipLaunchKernelGGL(prod_components_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream(), d_items());
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }

 private:
  static size_t scratch_bytes(const ProdItem &it) {
    return sizeof(double) * (2 * static_cast<int64_t>(it.ngroups) * it.Nq + 4 * it.Nq + 3);
  }
};

// ---- arguments ------------------------------------------------------------------------------------------------------------

int check_outputs(const void *pts, const void *ind, const void *logz) {
  if ((pts == nullptr) != (ind == nullptr)) return set_error(KDEHIP_ERR_ARG, "prod_exact: pts and ind are given together");
  if (!pts && !logz) return set_error(KDEHIP_ERR_ARG, "null argument");
  return KDEHIP_OK;
}

int check_count(int64_t Np) {
  if (Np < 0) return set_error(KDEHIP_ERR_ARG, "prod_exact: Np must be >= 0");
  return KDEHIP_OK;
}

const char kDims[] = "prod_exact -- dimensions of two BallTreeDensities must match";
const char kTooMany[] = "product_components: more than 2^20 components";

int check_host_pair(const kdehip_density *p, const kdehip_density *q) {
  KDEHIP_CHECK_RC(check_host_density(p));
  KDEHIP_CHECK_RC(check_host_density(q));
  if (p->ndim != q->ndim) return set_error(KDEHIP_ERR_DIM_MISMATCH, kDims);
  KDEHIP_CHECK_RC(check_one_bandwidth(p, kOneBandwidth));
  KDEHIP_CHECK_RC(check_one_bandwidth(q, kOneBandwidth));
  return KDEHIP_OK;
}

int check_resident_pair(const kdehip_device_density *p, const kdehip_device_density *q) {
  if (!p || !q) return set_error(KDEHIP_ERR_ARG, "null density");
  if (p->device != q->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  KDEHIP_CHECK_RC(check_resident_density(p, false));
  KDEHIP_CHECK_RC(check_resident_density(q, false));
  if (p->D != q->D) return set_error(KDEHIP_ERR_DIM_MISMATCH, kDims);
  if (!leaves_share_bandwidth(p) || !leaves_share_bandwidth(q)) return set_error(KDEHIP_ERR_UNSUPPORTED, kOneBandwidth);
  return KDEHIP_OK;
}

ProdItem base_item(int64_t N1, int64_t N2, int D, int64_t Np, uint64_t seed, int64_t offset) {
  ProdItem it{};
  it.Nq = N1; it.N = N2; it.D = D; it.Np = Np; it.seed = seed; it.offset = offset;
  it.norm0 = gauss_norm0(D);
  return it;
}

void point_resident(ProdItem &it, const kdehip_device_density *p, const kdehip_device_density *q) {
  const LeafRows lp = leaf_rows(p), lq = leaf_rows(q);
  it.qry = lp.src; it.pw = lp.w; it.bwp = lp.bw; it.permp = lp.perm;
  it.src = lq.src; it.w = lq.w; it.bwq = lq.bw; it.permq = lq.perm;
}

// two host densities in the call's image, each [means | weights | bw | permutation]
size_t host_leaf_bytes(const kdehip_density *bd) {
  return align256(sizeof(double) * (bd->npts * (bd->ndim + 1) + bd->ndim) + sizeof(int64_t) * bd->npts);
}
struct PackedLeaves { const double *means, *weights, *bw; const int64_t *perm; };
PackedLeaves pack_host_leaves(const ProdRun &run, size_t at, const kdehip_density *bd) {
  const int64_t N = bd->npts, D = bd->ndim;
  const LeafArrays la = pack_leaves(run, at, bd);
  const size_t o_bw = at + sizeof(double) * N * (D + 1), o_perm = o_bw + sizeof(double) * D;
  std::memcpy(run.host() + o_bw, bd->bandwidth + N * D, sizeof(double) * D);
  std::memcpy(run.host() + o_perm, bd->permutation + N, sizeof(int64_t) * N);
  return {la.means, la.weights, reinterpret_cast<const double *>(run.dev() + o_bw),
          reinterpret_cast<const int64_t *>(run.dev() + o_perm)};
}
void pack_host_pair(const ProdRun &run, ProdItem &it, const kdehip_density *p, const kdehip_density *q) {
  const PackedLeaves a = pack_host_leaves(run, 0, p), b = pack_host_leaves(run, host_leaf_bytes(p), q);
  it.qry = a.means; it.pw = a.weights; it.bwp = a.bw; it.permp = a.perm;
  it.src = b.means; it.w = b.weights; it.bwq = b.bw; it.permq = b.perm;
}

}  // namespace

extern "C" int kdehip_prod_exact(const kdehip_density *p, const kdehip_density *q, int64_t Np, uint64_t seed,
                                 int64_t sample_offset, double *pts, int64_t *ind, double *logz, int device) {
  // every check that needs no device comes first
  if (!p || !q) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_count(Np));
  KDEHIP_CHECK_RC(check_outputs(pts, ind, logz));
  KDEHIP_CHECK_RC(check_host_pair(p, q));
  const bool draws = pts && Np > 0;
  if (!draws && !logz) return KDEHIP_OK;
  const int D = static_cast<int>(p->ndim);
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  ProdRun run;
  run.items.push_back(base_item(p->npts, q->npts, D, draws ? Np : 0, seed, sample_offset));
  // caller data: [p | q]; results: [logz (1) | pts (Np D) | ind (2 Np int64)]
  const size_t prefix = host_leaf_bytes(p) + host_leaf_bytes(q);
  const size_t nd = draws ? static_cast<size_t>(Np) : 0, r_pts = 1, r_ind = r_pts + nd * D;
  KDEHIP_CHECK_RC(run.alloc(prefix, r_ind + 2 * nd));
  ProdItem &ri = run.items[0];
  pack_host_pair(run, ri, p, q);
  ri.logz = run.result(0);
  ri.pts = draws ? run.result(r_pts) : nullptr;
  ri.ind = draws ? reinterpret_cast<int64_t *>(run.result(r_ind)) : nullptr;
  KDEHIP_CHECK_RC(run.run(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  if (logz) *logz = *run.host_result(0);
  if (draws) {
    std::memcpy(pts, run.host_result(r_pts), sizeof(double) * nd * D);
    std::memcpy(ind, run.host_result(r_ind), sizeof(int64_t) * 2 * nd);
  }
  return KDEHIP_OK;
}

extern "C" int kdehip_prod_exact_device_batch(int n, const kdehip_prod_exact_item *items, void *stream) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "prod_exact batch: "));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_prod_exact_item &c = items[i];
    if (!c.p || !c.q) return set_error(KDEHIP_ERR_ARG, "null density");
    KDEHIP_CHECK_RC(check_count(c.Np));
    KDEHIP_CHECK_RC(check_outputs(c.d_pts, c.d_ind, c.d_logz));
    KDEHIP_CHECK_RC(check_resident_pair(c.p, c.q));
    KDEHIP_CHECK_RC(check_same_device(c.p, items[0].p, "prod_exact batch: "));
  }
  const int device = items[0].p->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);  // (a captured call's blocks are kept until kdehip_clear_cache: section 5h)
  ProdRun run;
  std::vector<int> which;
  for (int i = 0; i < n; ++i) {
    const kdehip_prod_exact_item &c = items[i];
    const bool draws = c.d_pts && c.Np > 0;
    if (!draws && !c.d_logz) continue;
    run.items.push_back(base_item(c.p->N, c.q->N, c.p->D, draws ? c.Np : 0, c.seed, c.sample_offset));
    which.push_back(i);
  }
  if (run.items.empty()) return KDEHIP_OK;
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  for (size_t k = 0; k < which.size(); ++k) {
    const kdehip_prod_exact_item &c = items[which[k]];
    ProdItem &ri = run.items[k];
    point_resident(ri, c.p, c.q);
    ri.logz = c.d_logz;
    ri.pts = ri.Np > 0 ? c.d_pts : nullptr;
    ri.ind = ri.Np > 0 ? c.d_ind : nullptr;
  }
  KDEHIP_CHECK_RC(run.run(st));
  return finish_enqueue(run, &scope, device);
}

extern "C" int kdehip_prod_exact_device(const kdehip_device_density *p, const kdehip_device_density *q, int64_t Np,
                                        uint64_t seed, int64_t sample_offset, double *d_pts, int64_t *d_ind, double *d_logz,
                                        void *stream) {
  kdehip_prod_exact_item c{};
  c.p = p; c.q = q; c.Np = Np; c.seed = seed; c.sample_offset = sample_offset;
  c.d_pts = d_pts; c.d_ind = d_ind; c.d_logz = d_logz;
  return kdehip_prod_exact_device_batch(1, &c, stream);
}

extern "C" int kdehip_product_components(const kdehip_density *p, const kdehip_density *q, double *means, double *weights,
                                         double *var, int device) {
  if (!p || !q || !means || !weights || !var) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_pair(p, q));
  const int64_t N1 = p->npts, N2 = q->npts, NC = N1 * N2;
  if (N1 > kMaxComponents || N2 > kMaxComponents || NC > kMaxComponents) return set_error(KDEHIP_ERR_UNSUPPORTED, kTooMany);
  const int D = static_cast<int>(p->ndim);
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  ProdRun run;
  run.items.push_back(base_item(N1, N2, D, 0, 0, 0));
  // caller data: [p | q]; results: [means (NC D) | weights (NC) | var (D)]
  const size_t r_w = static_cast<size_t>(NC) * D, r_var = r_w + static_cast<size_t>(NC);
  KDEHIP_CHECK_RC(run.alloc(host_leaf_bytes(p) + host_leaf_bytes(q), r_var + D));
  ProdItem &ri = run.items[0];
  pack_host_pair(run, ri, p, q);
  ri.cmeans = run.result(0);
  ri.cweights = run.result(r_w);
  ri.cvar = run.result(r_var);
  KDEHIP_CHECK_RC(run.run(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.components());
  KDEHIP_CHECK_RC(run.wait());
  std::memcpy(means, run.host_result(0), sizeof(double) * NC * D);
  std::memcpy(weights, run.host_result(r_w), sizeof(double) * NC);
  std::memcpy(var, run.host_result(r_var), sizeof(double) * D);
  return KDEHIP_OK;
}

extern "C" int kdehip_product_components_device(const kdehip_device_density *p, const kdehip_device_density *q, double *d_means,
                                                double *d_weights, double *d_var, void *stream) {
  if (!p || !q) return set_error(KDEHIP_ERR_ARG, "null density");
  if (!d_means || !d_weights || !d_var) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_pair(p, q));
  if (p->N > kMaxComponents || q->N > kMaxComponents || p->N * q->N > kMaxComponents)
    return set_error(KDEHIP_ERR_UNSUPPORTED, kTooMany);
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(p->device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);
  ProdRun run;
  run.items.push_back(base_item(p->N, q->N, p->D, 0, 0, 0));
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  ProdItem &ri = run.items[0];
  point_resident(ri, p, q);
  ri.cmeans = d_means;
  ri.cweights = d_weights;
  ri.cvar = d_var;
  KDEHIP_CHECK_RC(run.run(st));
  KDEHIP_CHECK_RC(run.components());
  return finish_enqueue(run, &scope, p->device);
}
