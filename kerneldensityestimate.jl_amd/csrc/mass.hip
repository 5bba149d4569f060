// mass.hip -- the probability mass of a density (include/kdehip.h section 5l; this library's own: the reference's only range
// summary is getKDERange, a support box): how much of a Gaussian-kernel density with ONE bandwidth vector lies inside an
// axis-aligned box, its marginal cdf and the marginal quantiles.
//   mass[q] = sum_i w_i prod_{k in B} f_ik,  f_ik = the mass of leaf i's kernel between lo_k and hi_k in dimension k,
// a difference of two normal cdfs written with erfc in the tail where that difference is relatively accurate (mass_factor).
// Host densities (uploaded for the call, blocking) and resident ones (single or batched, enqueue-only) run ONE path each:
//   mass_partial_kernel<NB>  one launch per distinct number NB of bounded dimensions: the mapping of pair_sweep.hpp (one lane
//                            per query, a block owns 256 queries and one group of 128-leaf chunks staged through a two-buffer
//                            LDS ring), but the ring holds the NB bounded coordinates and the weight only, gathered from the
//                            [N][D] leaf array, and the lane keeps lo[NB], hi[NB] and s[NB] in registers;
//   mass_finish_kernel       the groups summed in group order, NaN bounds answered, the value stored;
//   quantile_kernel          one 256-thread workgroup per (item, level): a bracketed Newton iteration on the marginal cdf,
//                            F and the pdf in one pass over the leaves (one erfc and one exp each), the whole iteration on the
//                            device.
// No atomics.  The group split (split_chunks(N, Nq, 1)) depends on the item's sizes alone and the quantile's sums have one
// fixed order, so the host entry, a resident call and any batch give the same bits.
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

constexpr int kFinishThreads = 256;    // queries per finish block
constexpr int kQuantileThreads = 256;  // lanes of the workgroup that solves one level

// One set of boxes: a density (N leaves in leaf order, one bandwidth vector) and Nq boxes over its nb bounded dimensions.
struct MassItem : PairHead {  // (qry is lo: what the head calls the queries)
  const double *hi;    // [Nq][nb]; lo = qry likewise
  const double *bw;    // [D] the density's first leaf's variances
  double *partial;     // [ngroups][Nq]
  double *out;         // [Nq]
  int32_t ngroups, nfb, D, nb;
  uint8_t dims[KDEHIP_MAX_DIMS];  // the bounded dimensions, ascending: dims[0 .. nb)
};

// 1 / sqrt(2 v): correctly rounded root and division, formed once per block and never per pair
__device__ __forceinline__ double mass_scale(double v) { return 1.0 / __dsqrt_rn(2.0 * v); }

// The mass of a unit kernel between a and b, both in units of sqrt(2 v) from the centre (section 5l).  The three forms keep
// each difference in the tail where it is relatively accurate; written as ONE pair of erfc calls whose arguments and whose
// combination are selected, so the lanes of a wave run the same instructions whichever form their box takes.
__device__ __forceinline__ double mass_factor(double a, double b) {
  const bool right = a >= 0.0, left = b <= 0.0;  // the box lies right / left of the centre
  const double e1 = erfc(right ? a : left ? -b : -a);
  const double e2 = erfc(right ? b : left ? -a : b);
  const double f = (right || left) ? (e1 - e2) / 2.0 : 1.0 - (e1 + e2) / 2.0;
  return (a < b) ? f : 0.0;  // empty, degenerate or a NaN bound (the finish kernel answers the NaN)
}

// partial[g][q] = sum over the leaf chunks c of group g, in chunk order, of (sum_{i in chunk c}, from 0 in leaf order, of
// w_i * prod_{k < NB} f_ik), for the items [0, n) of one NB.  Every lane, those at or beyond Nq included (their box is
// empty), walks the same chunks and barriers.
template <int NB>
__global__ __launch_bounds__(kEvalThreads) void mass_partial_kernel(const MassItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n) {
  __shared__ double sSrc[2][kEvalChunk * (NB + 1)];
  const ItemBlock ib = item_block(first, n);
  const MassItem pb = items[ib.item];
  const PairPlace at = pair_place(pb, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform, before any barrier
  const double *const src = pb.src, *const w = pb.w;
  const int64_t N = pb.N;
  const int D = pb.D;
  int dim[NB];
  double lo[NB], hi[NB], s[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    dim[k] = pb.dims[k];
    s[k] = mass_scale(pb.bw[dim[k]]);
    lo[k] = (at.q < pb.Nq) ? pb.qry[at.q * NB + k] : 0.0;
    hi[k] = (at.q < pb.Nq) ? pb.hi[at.q * NB + k] : 0.0;
  }
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * (NB + 1); t += kEvalThreads) {
      const int i = t / (NB + 1), f = t % (NB + 1);
      double val = w[i0 + i];
#pragma unroll
      for (int k = 0; k < NB; ++k) val = (f == k) ? src[(i0 + i) * D + dim[k]] : val;  // (dim[] stays in registers)
      sSrc[buf][t] = val;
    }
  };
  double total = 0.0;
  stage(at.c_begin, 0);
  for (int64_t c = at.c_begin; c < at.c_end; ++c) {
    const int buf = static_cast<int>((c - at.c_begin) & 1);
    __syncthreads();  // chunk c is staged; the other buffer is free again
    if (c + 1 < at.c_end) stage(c + 1, buf ^ 1);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    double sum = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const double *p = sSrc[buf] + i * (NB + 1);
      double prod = mass_factor((lo[0] - p[0]) * s[0], (hi[0] - p[0]) * s[0]);
#pragma unroll
      for (int k = 1; k < NB; ++k) prod *= mass_factor((lo[k] - p[k]) * s[k], (hi[k] - p[k]) * s[k]);
      sum += p[NB] * prod;
    }
    total += sum;
  }
  if (at.q < pb.Nq) pb.partial[at.grp * pb.Nq + at.q] = total;
}

// mass[q] = the groups in group order; NaN if any of the query's 2 nb bounds is one (the sweep gives such a box 0).
// Items [0, n), item i owns blocks [first[i], first[i+1]).
__global__ __launch_bounds__(kFinishThreads) void mass_finish_kernel(const MassItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n) {
  const ItemBlock ib = item_block(first, n);
  const MassItem it = items[ib.item];
  const int64_t q = static_cast<int64_t>(ib.k) * kFinishThreads + threadIdx.x;
  if (q >= it.Nq) return;
  double m = 0.0;
  for (int g = 0; g < it.ngroups; ++g) m += it.partial[static_cast<int64_t>(g) * it.Nq + q];
  if (query_has_nan(it.qry, q, it.nb) || query_has_nan(it.hi, q, it.nb)) m = __builtin_nan("");
  it.out[q] = m;
}

// The quantiles of one marginal: Nq levels of dimension `dim` of a density.
struct QuantItem : PairHead {  // (qry is alpha: what the head calls the queries; chunks_per_group is unused)
  const double *bw;     // [D] the density's first leaf's variances
  double *x;            // [Nq]
  double *resid;        // [Nq], or null
  int32_t *iters;       // [Nq], or null
  int32_t *converged;   // [Nq], or null
  double tol;
  int32_t max_iter, ngroups, D, dim;
};

// the block's minimum of red[0 .. W) (or its maximum, with MAX): red[t] was written by thread t and a barrier has passed
template <int W, bool MAX>
__device__ __forceinline__ double block_tree_extreme(double *red) {
  for (int off = W / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off)
      red[threadIdx.x] = MAX ? fmax(red[threadIdx.x], red[threadIdx.x + off]) : fmin(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();  // red is written again
  return r;
}

// x[j] solves F(x) = alpha[j], F the marginal cdf of dimension `dim` (section 5l), for level j = the block's index in its
// item; items [0, n), item i owns blocks [first[i], first[i+1]).  Every value that steers the iteration comes out of
// block_tree_sum, so the 256 lanes take every branch together.
__global__ __launch_bounds__(kQuantileThreads) void quantile_kernel(const QuantItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n) {
  __shared__ double sExpTab[32];
  __shared__ double redF[kQuantileThreads], redf[kQuantileThreads];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const QuantItem it = items[ib.item];
  const int64_t j = ib.k;
  const double alpha = it.qry[j];
  const double nan = __builtin_nan("");
  auto store = [&](double x, double r, int iters, int conv) {
    if (threadIdx.x != 0) return;
    it.x[j] = x;
    if (it.resid) it.resid[j] = r;
    if (it.iters) it.iters[j] = iters;
    if (it.converged) it.converged[j] = conv;
  };
  if (!(alpha > 0.0 && alpha < 1.0)) {  // (a NaN fails both; block-uniform, before any barrier)
    store(nan, nan, 0, 0);
    return;
  }
  const int64_t N = it.N;
  const int D = it.D;
  const double *const c = it.src + it.dim, *const w = it.w;
  const double v = it.bw[it.dim];
  const double s = mass_scale(v), sigma = __dsqrt_rn(v);
  const double pdf_scale = s * 0x1.20dd750429b6dp-1;  // s / sqrt(pi): d/dx of erfc(-(x - c) s) / 2 is this times exp(-t^2)
  // the leaves that carry weight lie in [cmin, cmax]
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < N; i += kQuantileThreads) {
    if (w[i] > 0.0) {
      mn = fmin(mn, c[i * D]);
      mx = fmax(mx, c[i * D]);
    }
  }
  redF[threadIdx.x] = mn;
  redf[threadIdx.x] = mx;
  __syncthreads();  // (also: the table is in place)
  const double cmin = block_tree_extreme<kQuantileThreads, false>(redF);
  const double cmax = block_tree_extreme<kQuantileThreads, true>(redf);
  if (!(cmin <= cmax)) {  // no leaf has weight: F is 0 everywhere
    store(nan, nan, 0, 0);
    return;
  }
  double xl = cmin - 39.0 * sigma, xh = cmax + 39.0 * sigma;  // F(xl) = 0 and F(xh) = sum w: erfc(39 / sqrt 2) underflows
  double x = 0.5 * (xl + xh);
  double dxold = xh - xl, dx = dxold;  // the step before last, the last step
  double r = nan;
  int iters = 0, conv = 0;
  for (;;) {
    double pF = 0.0, pf = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += kQuantileThreads) {
      const double t = (x - c[i * D]) * s, wi = w[i];
      pF += wi * erfc(-t);
      pf += wi * exp_nonpos(-(t * t), sExpTab);
    }
    redF[threadIdx.x] = pF;
    redf[threadIdx.x] = pf;
    __syncthreads();
    const double F = 0.5 * block_tree_sum<kQuantileThreads>(redF);
    const double f = pdf_scale * block_tree_sum<kQuantileThreads>(redf);
    __syncthreads();  // both sums are read: red is written again
    ++iters;
    r = F - alpha;
    if (fabs(r) <= it.tol) { conv = 1; break; }
    if (iters >= it.max_iter) break;
    if (r < 0.0) xl = x; else xh = x;
    const double step = r / f, xn = x - step;
    // Newton, if the pdf is positive, the point lies strictly inside the bracket and the step is at most half the step
    // before last (rtsafe); the midpoint otherwise
    const bool newton = f > 0.0 && xn > xl && xn < xh && fabs(2.0 * step) <= fabs(dxold);
    dxold = dx;
    if (newton) {
      dx = step;
      x = xn;
    } else {
      dx = 0.5 * (xh - xl);
      x = xl + dx;
    }
  }
  store(x, r, iters, conv);
}

// The run of one box-mass call (pair_sweep.hpp PairRun): per item the scratch [ngroups][Nq].  Protocol: fill `items` (sizes,
// D, nb, dims) -> alloc(prefix bytes of caller data, result doubles of the caller) -> point the items at their data ->
// start(stream) -> run() (one partial launch per distinct nb, ONE finish launch) -> wait(), defer() or keep().
class MassRun : public PairRun<MassItem> {
 public:
  int alloc(size_t prefix, size_t nresults) {
    const size_t n = items.size();
    int64_t pblocks = 0, fblocks = 0;
    for (MassItem &it : items) {
      pblocks += split(it);
      it.nfb = static_cast<int32_t>((it.Nq + kFinishThreads - 1) / kFinishThreads);
      fblocks += it.nfb;
    }
    if (pblocks > INT32_MAX / 2 || fblocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many boxes for one launch");
    Carve c;
    carve_head(c, prefix, 2, 0, nresults);  // first[] of the partial and of the finish kernel
    std::vector<size_t> scratch(n);
    for (size_t k = 0; k < n; ++k) scratch[k] = c.take(sizeof(double) * items[k].ngroups * items[k].Nq);
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) items[k].partial = reinterpret_cast<double *>(dev() + scratch[k]);
    return KDEHIP_OK;
  }
  int start(hipStream_t st) {
    prepare([&](size_t k) { return static_cast<int>(items[k].nb); });  // (no item is circular: a bounded circle is refused)
    int32_t *ffirst = first(1);
    ffirst[0] = 0;
    for (size_t k = 0; k < items.size(); ++k) ffirst[k + 1] = ffirst[k] + items[k].nfb;
    KDEHIP_CHECK(send(st));
    return KDEHIP_OK;
  }
  int run() {
    const hipStream_t st = stream();
    KDEHIP_CHECK_RC(for_each_run([&](const MassItem &it, const MassItem *d_it, const int32_t *d_pfirst, int cnt, int blocks,
                                     const uint32_t *) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.nb, [&](auto nb) {
        constexpr int kNB = decltype(nb)::value;
        hipLaunchKernelGGL(mass_partial_kernel<kNB>, dim3(static_cast<unsigned>(blocks)), dim3(kEvalThreads), 0, st, d_it,
                           d_pfirst, cnt);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    const int32_t *ffirst = first(1);
    const size_t n = items.size();
    if (ffirst[n] > 0) {
      hipLaunchKernelGGL(mass_finish_kernel, dim3(static_cast<unsigned>(ffirst[n])), dim3(kFinishThreads), 0, st, d_items(),
                         d_first(1), static_cast<int>(n));
      KDEHIP_CHECK(hipGetLastError());
    }
    return KDEHIP_OK;
  }
};

// The run of one quantile call: no scratch; first(1)[i] = the levels before item i, one workgroup per level, ONE launch.
class QuantRun : public PairRun<QuantItem> {
 public:
  int alloc(size_t prefix, size_t nresults) {
    int64_t blocks = 0;
    for (QuantItem &it : items) {
      it.ngroups = 1;
      blocks += it.Nq;
    }
    if (blocks > INT32_MAX / 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "too many levels for one launch");
    Carve c;
    carve_head(c, prefix, 2, 0, nresults);
    KDEHIP_CHECK(alloc_block(c));
    return KDEHIP_OK;
  }
  int start(hipStream_t st) {
    prepare([](size_t) { return 0; });
    int32_t *qfirst = first(1);
    qfirst[0] = 0;
    for (size_t k = 0; k < items.size(); ++k) qfirst[k + 1] = qfirst[k] + static_cast<int32_t>(items[k].Nq);
    KDEHIP_CHECK(send(st));
    return KDEHIP_OK;
  }
  int run() {
    const size_t n = items.size();
    const int32_t blocks = first(1)[n];
    if (blocks > 0) {
      hipLaunchKernelGGL(quantile_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kQuantileThreads), 0, stream(), d_items(),
                         d_first(1), static_cast<int>(n));
      KDEHIP_CHECK(hipGetLastError());
    }
    return KDEHIP_OK;
  }
};

// ---- arguments (none of these touches a device; the density's own checks are density_args.hpp) ---------------------------

const char kBoxes[] = "lo and hi must hold Nq >= 0 boxes", kDeviceBoxes[] = "d_lo and d_hi must hold Nq >= 0 boxes";
const char kLevels[] = "alpha must hold Nq >= 0 levels", kDeviceLevels[] = "d_alpha must hold Nq >= 0 levels";

// the bounded dimensions of a box: between 1 and D of them, none at or above D, none circular
int check_box(uint64_t dim_mask, uint32_t circ, int D) {
  if (dim_mask == 0u || (dim_mask >> D)) return set_error(KDEHIP_ERR_ARG, "box mass: dim_mask names between 1 and ndims dimensions of the density");
  if (dim_mask & circ) return set_error(KDEHIP_ERR_UNSUPPORTED, "box mass: a circular dimension cannot be bounded");
  return KDEHIP_OK;
}

int check_quantile_dim(int dim, uint32_t circ, int D) {
  if (dim < 0 || dim >= D) return set_error(KDEHIP_ERR_ARG, "quantile: dim is a dimension of the density, 0-based");
  if ((circ >> dim) & 1u) return set_error(KDEHIP_ERR_UNSUPPORTED, "quantile: the marginal of a circular dimension has no quantiles");
  return KDEHIP_OK;
}

// tol and max_iter as the entries take them (NULL, 0 = the default), resolved
int check_iteration(const double *tol_arg, double *tol, int *max_iter) {
  *tol = tol_arg ? *tol_arg : 0.0;
  if (*tol == 0.0) *tol = 1e-12;
  if (*max_iter == 0) *max_iter = 100;
  if (!(std::isfinite(*tol) && *tol >= 1e-14)) return set_error(KDEHIP_ERR_ARG, "quantile: tol must be finite and >= 1e-14 (0: the default 1e-12)");
  if (*max_iter < 1) return set_error(KDEHIP_ERR_ARG, "quantile: max_iter must be >= 1 (0: the default 100)");
  return KDEHIP_OK;
}

void set_dims(MassItem &it, uint64_t dim_mask) {
  it.nb = 0;
  for (int d = 0; d < it.D; ++d)
    if ((dim_mask >> d) & 1u) it.dims[it.nb++] = static_cast<uint8_t>(d);
}

}  // namespace

extern "C" int kdehip_box_mass(const kdehip_density *bd, uint64_t dim_mask, const double *lo, const double *hi, int64_t Nq,
                               double *mass, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!bd || !mass) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(lo && hi ? lo : nullptr, Nq, kBoxes));
  KDEHIP_CHECK_RC(check_box(dim_mask, circ, D));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  MassRun run;
  MassItem it{};
  it.N = bd->npts; it.Nq = Nq; it.D = D;
  set_dims(it, dim_mask);
  // caller data: [the density | lo | hi]; results: mass (Nq)
  const size_t bounds = sizeof(double) * Nq * it.nb;
  const size_t o_lo = host_density_bytes(bd), o_hi = o_lo + bounds, prefix = o_hi + bounds;
  run.items.push_back(it);
  KDEHIP_CHECK_RC(run.alloc(prefix, static_cast<size_t>(Nq)));
  MassItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  std::memcpy(run.host() + o_lo, lo, bounds);
  std::memcpy(run.host() + o_hi, hi, bounds);
  ri.qry = reinterpret_cast<const double *>(run.dev() + o_lo);
  ri.hi = reinterpret_cast<const double *>(run.dev() + o_hi);
  ri.out = run.result(0);
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.run());
  KDEHIP_CHECK_RC(run.wait());
  std::memcpy(mass, run.host_result(0), sizeof(double) * Nq);
  return KDEHIP_OK;
}

extern "C" int kdehip_box_mass_device_batch(int n, const kdehip_box_mass_item *items, void *stream) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "box mass batch: "));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_box_mass_item &b = items[i];
    KDEHIP_CHECK_RC(check_resident_density(b.bd, true));
    KDEHIP_CHECK_RC(check_same_device(b.bd, items[0].bd, "box mass batch: "));
    KDEHIP_CHECK_RC(check_circular_mask(b.circular_mask, b.bd->D, ""));
    KDEHIP_CHECK_RC(check_query_count(b.d_lo && b.d_hi ? b.d_lo : nullptr, b.Nq, kDeviceBoxes));
    if (!b.d_mass) return set_error(KDEHIP_ERR_ARG, "null argument");
    KDEHIP_CHECK_RC(check_box(b.dim_mask, b.circular_mask, b.bd->D));
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);
  MassRun run;
  for (int i = 0; i < n; ++i) {
    const kdehip_box_mass_item &b = items[i];
    if (b.Nq == 0) continue;
    const LeafRows leaf = leaf_rows(b.bd);
    MassItem it{};
    it.src = leaf.src; it.w = leaf.w; it.bw = leaf.bw;
    it.N = b.bd->N; it.Nq = b.Nq; it.D = b.bd->D;
    set_dims(it, b.dim_mask);
    it.qry = b.d_lo; it.hi = b.d_hi; it.out = b.d_mass;
    run.items.push_back(it);
  }
  if (run.items.empty()) return KDEHIP_OK;
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  KDEHIP_CHECK_RC(run.start(st));
  KDEHIP_CHECK_RC(run.run());
  return finish_enqueue(run, &scope, device);
}

// One item of the batch: the entry's own checks are those the batch does not make, or makes later than this entry always
// has; the boxes and the bounded dimensions are checked there, in this entry's order and words.
extern "C" int kdehip_box_mass_device(const kdehip_device_density *bd, uint64_t dim_mask, const double *d_lo, const double *d_hi,
                                      int64_t Nq, double *d_mass, const uint8_t *manifold, void *stream) {
  if (!bd || !d_mass) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  kdehip_box_mass_item b{};
  b.bd = bd; b.d_lo = d_lo; b.d_hi = d_hi; b.Nq = Nq; b.d_mass = d_mass;
  b.dim_mask = dim_mask; b.circular_mask = circ;
  return kdehip_box_mass_device_batch(1, &b, stream);
}

extern "C" int kdehip_quantile(const kdehip_density *bd, int dim, const double *alpha, int64_t Nq, const double *tol_arg, int max_iter,
                               double *x, double *resid, int32_t *iters, int32_t *converged, int device,
                               const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!bd || !x) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host_density(bd));
  const int D = static_cast<int>(bd->ndim);
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(alpha, Nq, kLevels));
  double tol = 0.0;
  KDEHIP_CHECK_RC(check_iteration(tol_arg, &tol, &max_iter));
  KDEHIP_CHECK_RC(check_quantile_dim(dim, circ, D));
  KDEHIP_CHECK_RC(check_one_bandwidth(bd, kOneBandwidth));
  if (Nq == 0) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  // caller data: [the density | alpha]; results, those asked for only: [x (Nq) | resid (Nq) | iters (Nq int32) | converged
  // (Nq int32)]
  const size_t n = static_cast<size_t>(Nq);
  const size_t o_alpha = host_density_bytes(bd), prefix = o_alpha + sizeof(double) * n;
  size_t nres = 0;
  auto take = [&](bool asked, size_t doubles) { const size_t at = nres; if (asked) nres += doubles; return at; };
  const size_t r_x = take(true, n), r_resid = take(resid, n), r_iters = take(iters, (n + 1) / 2), r_conv = take(converged, (n + 1) / 2);
  QuantRun run;
  QuantItem it{};
  it.N = bd->npts; it.Nq = Nq; it.D = D; it.dim = dim; it.tol = tol; it.max_iter = max_iter;
  run.items.push_back(it);
  KDEHIP_CHECK_RC(run.alloc(prefix, nres));
  QuantItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, bd);
  std::memcpy(run.host() + o_alpha, alpha, sizeof(double) * n);
  ri.qry = reinterpret_cast<const double *>(run.dev() + o_alpha);
  ri.x = run.result(r_x);
  ri.resid = resid ? run.result(r_resid) : nullptr;
  ri.iters = iters ? reinterpret_cast<int32_t *>(run.result(r_iters)) : nullptr;
  ri.converged = converged ? reinterpret_cast<int32_t *>(run.result(r_conv)) : nullptr;
  KDEHIP_CHECK_RC(run.start(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.run());
  KDEHIP_CHECK_RC(run.wait());
  std::memcpy(x, run.host_result(r_x), sizeof(double) * n);
  if (resid) std::memcpy(resid, run.host_result(r_resid), sizeof(double) * n);
  if (iters) std::memcpy(iters, run.host_result(r_iters), sizeof(int32_t) * n);
  if (converged) std::memcpy(converged, run.host_result(r_conv), sizeof(int32_t) * n);
  return KDEHIP_OK;
}

extern "C" int kdehip_quantile_device_batch(int n, const kdehip_quantile_item *items, const double *tol_arg, int max_iter,
                                            void *stream) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "quantile batch: "));
  double tol = 0.0;
  KDEHIP_CHECK_RC(check_iteration(tol_arg, &tol, &max_iter));
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_quantile_item &b = items[i];
    KDEHIP_CHECK_RC(check_resident_density(b.bd, true));
    KDEHIP_CHECK_RC(check_same_device(b.bd, items[0].bd, "quantile batch: "));
    KDEHIP_CHECK_RC(check_circular_mask(b.circular_mask, b.bd->D, ""));
    KDEHIP_CHECK_RC(check_query_count(b.d_alpha, b.Nq, kDeviceLevels));
    if (!b.d_x) return set_error(KDEHIP_ERR_ARG, "null argument");
    KDEHIP_CHECK_RC(check_quantile_dim(b.dim, b.circular_mask, b.bd->D));
  }
  const int device = items[0].bd->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);
  QuantRun run;
  for (int i = 0; i < n; ++i) {
    const kdehip_quantile_item &b = items[i];
    if (b.Nq == 0) continue;
    const LeafRows leaf = leaf_rows(b.bd);
    QuantItem it{};
    it.src = leaf.src; it.w = leaf.w; it.bw = leaf.bw;
    it.N = b.bd->N; it.Nq = b.Nq; it.D = b.bd->D; it.dim = b.dim; it.tol = tol; it.max_iter = max_iter;
    it.qry = b.d_alpha;
    it.x = b.d_x; it.resid = b.d_resid; it.iters = b.d_iters; it.converged = b.d_converged;
    run.items.push_back(it);
  }
  if (run.items.empty()) return KDEHIP_OK;
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  KDEHIP_CHECK_RC(run.start(st));
  KDEHIP_CHECK_RC(run.run());
  return finish_enqueue(run, &scope, device);
}

// one item of the batch, likewise
extern "C" int kdehip_quantile_device(const kdehip_device_density *bd, int dim, const double *d_alpha, int64_t Nq,
                                      const double *tol_arg, int max_iter, double *d_x, double *d_resid, int32_t *d_iters, int32_t *d_converged,
                                      const uint8_t *manifold, void *stream) {
  if (!bd || !d_x) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident_density(bd, true));
  uint32_t circ = 0;
  if (manifold_arg(manifold, bd->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  KDEHIP_CHECK_RC(check_query_count(d_alpha, Nq, kDeviceLevels));
  kdehip_quantile_item b{};
  b.bd = bd; b.d_alpha = d_alpha; b.Nq = Nq; b.d_x = d_x; b.d_resid = d_resid; b.d_iters = d_iters; b.d_converged = d_converged;
  b.dim = dim; b.circular_mask = circ;
  return kdehip_quantile_device_batch(1, &b, tol_arg, max_iter, stream);
}
