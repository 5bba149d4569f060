// summary.hip -- the density summaries of the reference's "misc" row on gfx950 (include/kdehip.h section 5c):
//   getKDERange, getKDEMean, getKDEfit         src/DualTree01.jl:512-578 (min / max, the sequential mean, the MLE covariance)
//   getKDEMax                                  src/DualTree01.jl:558-570 (1-D marginals on a grid, direct sum, first argmax)
//   intersIntgAppxIS                           src/DualTree01.jl:581-618 (a grid, the existing evaluation, a product-sum)
// Three kernels serve any number of items (resident densities of any D and N) in one call, described in device memory:
//   summary_moments_kernel  one workgroup per item: min, max and the weight total S from the leaves by block reductions
//                           (S in a fixed tree); when the mean or the covariance is asked for, the leaves scattered back to
//                           original order (getPoints order) and walked in LDS-staged chunks, one lane per dimension (per
//                           pair of dimensions) adding left to right -- a dependent chain of N adds, the reference's order;
//   grid_partial_kernel     for every (item, dimension, leaf group, block of 256 grid points): a lane owns a grid point and
//                           sums w_i / S * exp(-(x - m_i)^2 / (2 v)) over the group's leaves, staged through LDS in chunks
//                           (v = fl(sqrt(v_1))^2: the marginal's variance, see marginal());
//   grid_finish_kernel      one workgroup per (item, dimension): the group sums in order, / norm, and the first index of the
//                           maximum (a NaN wins, as Julia's maximum / isequal decide): wave shuffles, then LDS.
// The leaf groups depend on the item's (N, Ngrid) alone, never on the batch: a single call and any batch give the same bits.
// Circular dimensions (section 5e): every kernel has a compile-time CIRC instantiation -- the tangent offsets
// wrap(x - a0) at original point 1's angle for the range and the mean, wrapped residuals for the covariance, wrapped
// differences on the grid, the wrapped argmax.  Items with a circular bit run it, all others the plain one (the run keeps
// its Euclidean items first): a Euclidean item runs the code it always ran.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "device_density.hpp"
#include "call_block.hpp"
#include "circ_wrap.hpp"
#include "entry_helpers.hpp"
#include "manifold_arg.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"

namespace kdehip {
namespace {

constexpr int kSumThreads = 256;      // moments: one workgroup per item
constexpr int kGridThreads = 256;     // grid points per block
constexpr int kGridChunk = 256;       // leaves per staged chunk (one per lane)
constexpr int kGridMaxGroups = 256;   // at most this many partial sums per grid point
constexpr int64_t kMaxGrid = int64_t(1) << 24;
constexpr int64_t kMaxGrid2 = int64_t(1) << 14;  // intersIntgAppxIS in 2-D evaluates Ngrid^2 points

struct SumItem {
  const double *means, *bw, *w;  // leaf rows (tree order): [N][D] means, [N][D] variances, [N] weights
  const int64_t *perm;           // [N] 1-based original index of each leaf
  double *orig;                  // scratch [D][N]: the points by dimension in original order (mean / covariance only)
  double *stats;                 // scratch [3D + 1]: lo[D], hi[D] (extended), variances of original point 1 [D], weight total
  double *partial;               // scratch [D][ngroups][Ngrid]
  double *range, *mean, *cov, *argmax, *values;  // outputs (device, any may be null)
  double extend;
  double norm0;                  // sqrt(2 pi) as gauss_norm's libm rounds (2 pi)^(1/2)
  int64_t N, Ngrid, chunks_per_group;
  int32_t D, ngroups, gblocks, grid;  // grid: the grid kernels run for this item
  uint32_t circ;                 // bit k: dimension k is circular (section 5e); such an item runs the CIRC instantiations
};

constexpr double kPi = 3.141592653589793238462643383279, kTwoPi = 6.283185307179586476925286766559;  // circ_wrap's

// x_k of the grid over [lo, hi]: lo + k h with h = (hi - lo) / (Ngrid - 1), the last point hi; every operation rounded
// on its own (the build compiles with -ffp-contract=off)
__host__ __device__ __forceinline__ double grid_point(double lo, double hi, int64_t Ngrid, int64_t k) {
  if (k >= Ngrid - 1) return hi;
  const double h = (hi - lo) / static_cast<double>(Ngrid - 1);
  return lo + static_cast<double>(k) * h;
}

// (va, ka) comes before (vb, kb) in findfirst(isequal(maximum(y)), y): a NaN first, then the larger value, then the lower
// index; kb < 0 is "nothing yet"
__device__ __forceinline__ bool better(double va, int ka, double vb, int kb) {
  if (kb < 0) return ka >= 0;
  if (ka < 0) return false;
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return na;
  if (!na && va != vb) return va > vb;
  return ka < kb;
}

// min / max with Julia's NaN rule (a NaN sticks)
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a) ? a : (b != b) ? b : (b < a ? b : a); }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a) ? a : (b != b) ? b : (b > a ? b : a); }

template <bool CIRC>
__global__ __launch_bounds__(kSumThreads) void summary_moments_kernel(const SumItem *__restrict__ items) {
  __shared__ double sRow[KDEHIP_MAX_DIMS + 1][kSumThreads + 1];  // (+1: the lanes of a sequential walk hit distinct banks)
  __shared__ double sMean[KDEHIP_MAX_DIMS];
  __shared__ double sA0[KDEHIP_MAX_DIMS];  // CIRC: the reference angle a0 = original point 1 (NaN if no leaf claims it)
  const SumItem it = items[blockIdx.x];
  const int D = it.D;
  const int64_t N = it.N;
  const int tid = static_cast<int>(threadIdx.x);
  double *st = it.stats;
  if (tid < D) st[2 * D + tid] = NAN;  // (stays NaN if no leaf claims original point 1)
  if constexpr (CIRC)
    if (tid < D) sA0[tid] = NAN;
  __syncthreads();
  for (int64_t i = tid; i < N; i += kSumThreads)
    if (it.perm[i] == 1)
      for (int k = 0; k < D; ++k) {
        st[2 * D + k] = it.bw[i * D + k];
        if constexpr (CIRC) sA0[k] = it.means[i * D + k];
      }
  if constexpr (CIRC) __syncthreads();
  // (CIRC) x of a circular dimension d as its tangent offset at a0
  auto offset = [&](double x, int d) {
    if constexpr (CIRC)
      if ((it.circ >> d) & 1u) return circ_wrap(x - sA0[d]);
    return x;
  };
  // 1. per dimension min and max, and the weight total: straight from the leaves in ONE pass (min / max are exact in any
  //    order; the total is a fixed tree -- lane t sums leaves t, t + 256, ... in order, then the lanes pairwise in LDS)
  double lo[KDEHIP_MAX_DIMS], hi[KDEHIP_MAX_DIMS], wsum = 0.0;
#pragma unroll
  for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) { lo[d] = INFINITY; hi[d] = -INFINITY; }
  for (int64_t i = tid; i < N; i += kSumThreads) {
#pragma unroll
    for (int d = 0; d < KDEHIP_MAX_DIMS; ++d) {
      if (d < D) {
        const double x = offset(it.means[i * D + d], d);
        lo[d] = nan_min(lo[d], x);
        hi[d] = nan_max(hi[d], x);
      }
    }
    wsum += it.w[i];
  }
  for (int d = 0; d < 2 * D; d += 2) {  // two rows per round: (lo, hi) of one dimension; the weights last
    sRow[0][tid] = lo[0];
    sRow[1][tid] = hi[0];
#pragma unroll
    for (int k = 1; k < KDEHIP_MAX_DIMS; ++k)
      if (k == d / 2) { sRow[0][tid] = lo[k]; sRow[1][tid] = hi[k]; }
    __syncthreads();
    for (int off = kSumThreads / 2; off > 0; off >>= 1) {
      if (tid < off) {
        sRow[0][tid] = nan_min(sRow[0][tid], sRow[0][tid + off]);
        sRow[1][tid] = nan_max(sRow[1][tid], sRow[1][tid + off]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int k = d / 2;
      const double a = sRow[0][0], b = sRow[1][0];
      const double dr = it.extend * (b - a);
      double rlo = a - dr, rhi = b + dr;
      if constexpr (CIRC) {
        if ((it.circ >> k) & 1u) {  // the arc (a0 + lo_t, a0 + hi_t), extended, unwrapped; at most one turn
          const double alo = sA0[k] + a, ahi = sA0[k] + b;
          rlo = alo - dr;
          rhi = ahi + dr;
          if (rhi - rlo > kTwoPi) {
            const double mid = 0.5 * (alo + ahi);
            rlo = mid - kPi;
            rhi = mid + kPi;
          }
        }
      }
      st[k] = rlo;
      st[D + k] = rhi;
      if (it.range) { it.range[k] = rlo; it.range[D + k] = rhi; }
    }
    __syncthreads();
  }
  sRow[0][tid] = wsum;
  __syncthreads();
  for (int off = kSumThreads / 2; off > 0; off >>= 1) {
    if (tid < off) sRow[0][tid] += sRow[0][tid + off];
    __syncthreads();
  }
  if (tid == 0) st[3 * D] = sRow[0][0];
  if (!it.mean && !it.cov) return;  // (block-uniform)
  // 2. the mean (and the covariance) in ORIGINAL order: the leaves scattered back, then walked in 256-point chunks staged
  //    through LDS, one lane per dimension (per pair of dimensions) adding in order
  for (int64_t t = tid; t < N * D; t += kSumThreads) {
    const int64_t i = t / D;
    const int f = static_cast<int>(t - i * D);
    const int64_t o = it.perm[i] - 1;
    if (o >= 0 && o < N) it.orig[f * N + o] = it.means[i * D + f];  // (an uploaded density's permutation is the caller's)
  }
  // (CIRC: the wraps are done HERE, one point per lane, not in the one-lane walks below -- the same operations on the same
  // values, so the same bits: residual = false stages the tangent offsets, residual = true the residuals x - mu, wrapped in
  // a circular dimension)
  auto stage = [&](int64_t c0, int cnt, bool residual) {
    __syncthreads();  // the previous chunk is consumed; (first call) the scatter is complete; (residual) sMean is published
    if (tid < cnt)
      for (int f = 0; f < D; ++f) {
        double x = it.orig[f * N + c0 + tid];
        if constexpr (CIRC) {
          if (residual) {
            x -= sMean[f];
            if ((it.circ >> f) & 1u) x = circ_wrap(x);
          } else {
            x = offset(x, f);
          }
        }
        sRow[f][tid] = x;
      }
    __syncthreads();
  };
  double s = 0.0;
  for (int64_t c0 = 0; c0 < N; c0 += kSumThreads) {
    const int cnt = static_cast<int>(N - c0 < kSumThreads ? N - c0 : kSumThreads);
    stage(c0, cnt, false);
    if (tid < D)
      for (int j = 0; j < cnt; ++j) s += sRow[tid][j];
  }
  if (tid < D) {
    double mu = s / static_cast<double>(N);
    if constexpr (CIRC)
      if ((it.circ >> tid) & 1u) mu = circ_wrap(sA0[tid] + mu);
    sMean[tid] = mu;
    if (it.mean) it.mean[tid] = mu;
  }
  if (!it.cov) return;  // (block-uniform)
  int a = 0, b = 0;
  const bool pair = tid < D * (D + 1) / 2;
  if (pair) {
    int r = tid;
    while (r >= D - a) { r -= D - a; ++a; }
    b = a + r;
  }
  s = 0.0;
  for (int64_t c0 = 0; c0 < N; c0 += kSumThreads) {
    const int cnt = static_cast<int>(N - c0 < kSumThreads ? N - c0 : kSumThreads);
    stage(c0, cnt, true);  // (its first barrier also publishes sMean)
    if (pair) {
      if constexpr (CIRC) {
        for (int j = 0; j < cnt; ++j) s += sRow[a][j] * sRow[b][j];
      } else {
        const double ma = sMean[a], mb = sMean[b];
        for (int j = 0; j < cnt; ++j) s += (sRow[a][j] - ma) * (sRow[b][j] - mb);
      }
    }
  }
  if (pair) {
    const double c = s / static_cast<double>(N);
    it.cov[a * D + b] = c;
    it.cov[b * D + a] = c;
  }
}

// item i owns blocks [first[i], first[i+1]): D x ngroups x gblocks, dimension-major, then leaf group, then grid block
template <bool CIRC>
__global__ __launch_bounds__(kGridThreads) void grid_partial_kernel(const SumItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n) {
  __shared__ double sM[2][kGridChunk], sW[2][kGridChunk];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const int b = static_cast<int>(blockIdx.x);
  const int i = item_of_block(first, n, b);
  const SumItem it = items[i];
  const int64_t per_dim = static_cast<int64_t>(it.ngroups) * it.gblocks;
  const int64_t kb = b - first[i];
  const int d = static_cast<int>(kb / per_dim);
  const int64_t r = kb - d * per_dim;
  const int64_t grp = r / it.gblocks, gb = r - grp * it.gblocks;
  const int64_t k = gb * kGridThreads + threadIdx.x;
  const int D = it.D;
  const int64_t N = it.N;
  const double *st = it.stats;
  const double x = k < it.Ngrid ? grid_point(st[d], st[D + d], it.Ngrid, k) : 0.0;
  const double sd = sqrt(st[2 * D + d]);
  const double nhib = -0.5 / (sd * sd);  // the marginal's variance: getBW's sqrt, squared again by kde!
  const double S = st[3 * D];
  const bool wrapd = CIRC && ((it.circ >> d) & 1u);
  const int64_t nchunks = (N + kGridChunk - 1) / kGridChunk;
  const int64_t c_begin = grp * it.chunks_per_group;
  int64_t c_end = c_begin + it.chunks_per_group;
  if (c_end > nchunks) c_end = nchunks;
  auto stage = [&](int64_t c, int buf) {
    const int64_t l = c * kGridChunk + threadIdx.x;
    if (l < N) {
      sM[buf][threadIdx.x] = it.means[l * D + d];
      sW[buf][threadIdx.x] = it.w[l] / S;  // kde!'s normalisation of the marginal's weights
    }
  };
  stage(c_begin, 0);
  double total = 0.0;
  for (int64_t c = c_begin; c < c_end; ++c) {
    const int buf = static_cast<int>((c - c_begin) & 1);
    __syncthreads();  // chunk c is staged; the other buffer is free again
    if (c + 1 < c_end) stage(c + 1, buf ^ 1);
    const int64_t i0 = c * kGridChunk;
    const int cnt = static_cast<int>((N - i0 < kGridChunk) ? (N - i0) : kGridChunk);
    double sum = 0.0;
    if (CIRC && wrapd) {  // (block-uniform) the difference on the circle, then exactly the loop below
      for (int j = 0; j < cnt; ++j) {
        const double dd = circ_wrap(x - sM[buf][j]);
        const double acc = (dd * dd) * nhib;
        sum += sW[buf][j] * exp_nonpos(acc, sExpTab);
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        const double dd = x - sM[buf][j];
        const double acc = (dd * dd) * nhib;
        sum += sW[buf][j] * exp_nonpos(acc, sExpTab);  // acc <= 0
      }
    }
    total += sum;
  }
  if (k < it.Ngrid) it.partial[(static_cast<int64_t>(d) * it.ngroups + grp) * it.Ngrid + k] = total;
}

// item i owns blocks [first[i], first[i+1]): one per dimension
template <bool CIRC>
__global__ __launch_bounds__(kGridThreads) void grid_finish_kernel(const SumItem *__restrict__ items,
                                                                   const int32_t *__restrict__ first, int n) {
  constexpr int kWaves = kGridThreads / 64;
  __shared__ double sV[kWaves];
  __shared__ int sK[kWaves];
  const int b = static_cast<int>(blockIdx.x);
  const int i = item_of_block(first, n, b);
  const SumItem it = items[i];
  const int D = it.D, d = b - first[i];
  const int64_t Ng = it.Ngrid;
  const double lo = it.stats[d], hi = it.stats[D + d];
  const double sd = sqrt(it.stats[2 * D + d]);
  const double inv_norm = 1.0 / (it.norm0 * sqrt(sd * sd));  // gauss_norm of the 1-D marginal
  const double *part = it.partial + static_cast<int64_t>(d) * it.ngroups * Ng;
  double bv = 0.0;
  int bk = -1;
  for (int64_t k = threadIdx.x; k < Ng; k += kGridThreads) {
    double s = 0.0;
    for (int g = 0; g < it.ngroups; ++g) s += part[g * Ng + k];
    const double v = s * inv_norm;
    if (it.values) it.values[d * Ng + k] = v;
    if (better(v, static_cast<int>(k), bv, bk)) { bv = v; bk = static_cast<int>(k); }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off);
    const int ok = __shfl_xor(bk, off);
    if (better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
  }
  const int wave = static_cast<int>(threadIdx.x) / 64, lane = static_cast<int>(threadIdx.x) % 64;
  if (lane == 0) { sV[wave] = bv; sK[wave] = bk; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w)
      if (better(sV[w], sK[w], bv, bk)) { bv = sV[w]; bk = sK[w]; }
    if (it.argmax && bk >= 0) {
      double x = grid_point(lo, hi, Ng, bk);
      if constexpr (CIRC)
        if ((it.circ >> d) & 1u) x = circ_wrap(x);  // (the grid itself stays unwrapped: a monotone linspace)
      it.argmax[d] = x;
    }
  }
}

// intersIntgAppxIS's query points from the item's grid (stats lo / hi of dimensions 0 and 1): 1-D x_j at j; 2-D, row i
// (xx[2, :] = LD[2][i], :606-609) at i * Ngrid + j = (x1_j, x2_i).  [Nq][D] as the evaluation reads queries.
__global__ void inters_grid_kernel(const double *__restrict__ stats, int D, int64_t Ng, double *__restrict__ pts) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (D == 1) {
    if (t < Ng) pts[t] = grid_point(stats[0], stats[1], Ng, t);
    return;
  }
  if (t >= Ng * Ng) return;
  const int64_t i = t / Ng, j = t - i * Ng;
  pts[2 * t] = grid_point(stats[0], stats[2], Ng, j);
  pts[2 * t + 1] = grid_point(stats[1], stats[3], Ng, i);
}

// one workgroup: 1-D acc = 0 + (sum_k p_k q_k) dx1; 2-D, row i's sum_j p q (one lane per row, j in order), then
// acc += (dx1 row_i) dx2 over the rows in order -- the reference's loop (:604-612), its `sum` taken sequentially
__global__ __launch_bounds__(kSumThreads) void inters_reduce_kernel(const double *__restrict__ stats, int D, int64_t Ng,
                                                                    const double *__restrict__ pv, const double *__restrict__ qv,
                                                                    double *__restrict__ rows, double *__restrict__ out) {
  const double dx1 = grid_point(stats[0], stats[D], Ng, 1) - grid_point(stats[0], stats[D], Ng, 0);
  if (D == 1) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int64_t k = 0; k < Ng; ++k) s += pv[k] * qv[k];
      out[0] = 0.0 + s * dx1;
    }
    return;
  }
  const double dx2 = grid_point(stats[1], stats[3], Ng, 1) - grid_point(stats[1], stats[3], Ng, 0);
  for (int64_t i = threadIdx.x; i < Ng; i += kSumThreads) {
    double s = 0.0;
    for (int64_t j = 0; j < Ng; ++j) s += pv[i * Ng + j] * qv[i * Ng + j];
    rows[i] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int64_t i = 0; i < Ng; ++i) acc = acc + (dx1 * rows[i]) * dx2;
    out[0] = acc;
  }
}

// The blocks of one call: ONE device block [descriptors | first[] of the two grid kernels | caller's extra | per item:
// original-order rows, stats, partial sums] and ONE pinned image of everything up to the extra, which goes up in one copy.
// Protocol: fill `items` (densities' pointers, sizes, extend, outputs, circ; the Euclidean items first) -> alloc(extra bytes)
// -> enqueue(stream) -> wait() (blocking calls: the extra comes back to host_extra()) or defer(device) (enqueue-only calls).
// The Euclidean items [0, ne) and the circular ones [ne, n) each get their own launches and their own first[] arrays.
class SumRun {
 public:
  std::vector<SumItem> items;
  int alloc(size_t extra) {
    const size_t n = items.size();
    const int64_t cu = device_cu_count();
    int64_t pblocks = 0;
    for (SumItem &it : items) {
      it.ngroups = it.gblocks = 0;
      it.chunks_per_group = 1;
      if (!it.grid) continue;
      // the leaf split: groups for ~8 blocks per CU per dimension, from the item's (N, Ngrid) alone
      const int64_t nchunks = (it.N + kGridChunk - 1) / kGridChunk;
      const int64_t gblocks = (it.Ngrid + kGridThreads - 1) / kGridThreads;
      int64_t want = (8 * cu + gblocks - 1) / gblocks;
      want = std::max<int64_t>(1, std::min<int64_t>({want, kGridMaxGroups, nchunks}));
      it.chunks_per_group = (nchunks + want - 1) / want;
      it.ngroups = static_cast<int32_t>((nchunks + it.chunks_per_group - 1) / it.chunks_per_group);
      it.gblocks = static_cast<int32_t>(gblocks);
      pblocks += static_cast<int64_t>(it.D) * it.ngroups * it.gblocks;
    }
    if (pblocks > INT32_MAX || n > 65535) return set_error(KDEHIP_ERR_UNSUPPORTED, "summary too large for one launch");
    Carve c;
    o_items_ = c.take(sizeof(SumItem) * n);
    o_first_ = c.take(sizeof(int32_t) * 2 * (n + 2));
    o_extra_ = c.take(extra);
    extra_ = extra;
    scratch_.resize(n);
    for (size_t k = 0; k < n; ++k) {
      const SumItem &it = items[k];
      scratch_[k] = c.take(sizeof(double) * (it.D * it.N + 3 * it.D + 1 + static_cast<int64_t>(it.D) * it.ngroups * it.Ngrid));
    }
    KDEHIP_CHECK(blk_.alloc(c.mark(), o_extra_ + extra));
    for (size_t k = 0; k < n; ++k) {
      SumItem &it = items[k];
      it.orig = reinterpret_cast<double *>(dev() + scratch_[k]);
      it.stats = it.orig + it.D * it.N;
      it.partial = it.stats + 3 * it.D + 1;
    }
    return KDEHIP_OK;
  }
  unsigned char *dev() const { return blk_.dev(); }
  double *extra() const { return reinterpret_cast<double *>(dev() + o_extra_); }  // (device)
  const double *host_extra() const { return reinterpret_cast<const double *>(blk_.host() + o_extra_); }

  int enqueue(hipStream_t st) {
    const size_t n = items.size();
    size_t ne = 0;
    while (ne < n && items[ne].circ == 0) ++ne;
    for (size_t k = ne; k < n; ++k)
      if (items[k].circ == 0) return set_error(KDEHIP_ERR_ARG, "summary: Euclidean items come first");  // (internal)
    unsigned char *h = blk_.host();
    // [Euclidean partial first (ne + 1) | circular partial first (n - ne + 1) | the same two for the finish kernel]
    int32_t *pfirst = reinterpret_cast<int32_t *>(h + o_first_), *ffirst = pfirst + (n + 2);
    const auto fill = [&](size_t k0, size_t k1, int32_t *pf, int32_t *ff) {
      pf[0] = ff[0] = 0;
      for (size_t k = k0; k < k1; ++k) {
        const SumItem &it = items[k];
        pf[k - k0 + 1] = pf[k - k0] + it.D * it.ngroups * it.gblocks;
        ff[k - k0 + 1] = ff[k - k0] + (it.grid ? it.D : 0);
      }
    };
    fill(0, ne, pfirst, ffirst);
    fill(ne, n, pfirst + ne + 1, ffirst + ne + 1);
    if (n) std::memcpy(h + o_items_, items.data(), sizeof(SumItem) * n);
    KDEHIP_CHECK(blk_.upload(o_extra_, st));
    const SumItem *d_items = reinterpret_cast<const SumItem *>(dev() + o_items_);
    const int32_t *d_pfirst = reinterpret_cast<const int32_t *>(dev() + o_first_), *d_ffirst = d_pfirst + (n + 2);
    const auto launch = [&](auto circ, size_t k0, size_t cnt, size_t f0) {
      constexpr bool CIRC = decltype(circ)::value;
      if (!cnt) return;
      const int32_t np = pfirst[f0 + cnt], nf = ffirst[f0 + cnt];
      hipLaunchKernelGGL(summary_moments_kernel<CIRC>, dim3(static_cast<unsigned>(cnt)), dim3(kSumThreads), 0, st,
                         d_items + k0);
      if (np > 0)
        hipLaunchKernelGGL(grid_partial_kernel<CIRC>, dim3(static_cast<unsigned>(np)), dim3(kGridThreads), 0, st,
                           d_items + k0, d_pfirst + f0, static_cast<int>(cnt));
      if (nf > 0)
        hipLaunchKernelGGL(grid_finish_kernel<CIRC>, dim3(static_cast<unsigned>(nf)), dim3(kGridThreads), 0, st,
                           d_items + k0, d_ffirst + f0, static_cast<int>(cnt));
    };
    launch(std::false_type{}, 0, ne, 0);
    launch(std::true_type{}, ne, n - ne, ne + 1);
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  int wait() {
    hipError_t e = hipSuccess;
    if (extra_) e = blk_.download(o_extra_, extra_, blk_.stream());
    const hipError_t se = blk_.wait();
    KDEHIP_CHECK(e);
    KDEHIP_CHECK(se);
    return KDEHIP_OK;
  }
  int defer(int device) {
    reap_deferred(device);
    return blk_.defer(device);
  }

 private:
  CallBlock blk_;
  size_t o_items_ = 0, o_first_ = 0, o_extra_ = 0, extra_ = 0;
  std::vector<size_t> scratch_;
};

// the descriptor of a resident density (outputs, extend, grid set by the caller)
SumItem density_item(const kdehip_device_density *p, double extend, int64_t Ngrid, uint32_t circ = 0) {
  SumItem it{};
  const int64_t N = p->N;
  const int D = p->D;
  it.means = p->means + N * D; it.bw = p->bandwidth + N * D; it.w = p->weights + N; it.perm = p->perm + N;
  it.extend = extend;
  it.norm0 = std::pow(2.0 * M_PI, 1 / 2.0);
  it.N = N; it.Ngrid = Ngrid; it.D = D;
  it.circ = circ;
  return it;
}

int check_grid(int64_t Ngrid) {
  if (Ngrid < 2) return set_error(KDEHIP_ERR_ARG, "Ngrid must be at least 2");
  if (Ngrid > kMaxGrid) return set_error(KDEHIP_ERR_UNSUPPORTED, "Ngrid above 2^24");
  return KDEHIP_OK;
}

int check_resident(const kdehip_device_density *p) {
  if (!p) return set_error(KDEHIP_ERR_ARG, "null density");
  if (p->D < 1 || p->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (p->N < 1) return set_error(KDEHIP_ERR_ARG, "density with no points");
  return KDEHIP_OK;
}

// the checks of a host density the summaries read (leaf means, variances, weights, permutation)
int check_host(const kdehip_density *p) {
  if (!p) return set_error(KDEHIP_ERR_ARG, "null density");
  if (p->ndim > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (p->ndim < 1) return set_error(KDEHIP_ERR_ARG, "density with no dimensions");
  if (p->npts < 1 || !p->means || !p->bandwidth || !p->weights || !p->permutation || !p->left_child || !p->right_child)
    return set_error(KDEHIP_ERR_ARG, "malformed density");
  return KDEHIP_OK;
}

// an upload of a host density for the length of one call
struct Uploaded {
  kdehip_device_density *h = nullptr;
  ~Uploaded() { if (h) kdehip_density_free(h); }
};

// (manifold / circ: NULL / 0 or the same manifold as bytes and as a mask -- the grid over p's circular range, p and q by the
// kernels of kdehip_evaluate_manifold)
int inters_resident(const kdehip_device_density *p, const kdehip_device_density *q, int64_t Ngrid, double *out,
                    const uint8_t *manifold, uint32_t circ) {
  const int D = p->D;
  const int64_t Nq = D == 1 ? Ngrid : Ngrid * Ngrid;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(p->device));
  hipStream_t st = hipStreamPerThread;
  // extra: [result | query points Nq x D | p values | q values | row sums]
  Carve c;
  c.take(sizeof(double));
  const size_t o_pts = c.take(sizeof(double) * Nq * D), o_pv = c.take(sizeof(double) * Nq), o_qv = c.take(sizeof(double) * Nq);
  const size_t o_rows = c.mark(), extra = o_rows + sizeof(double) * Ngrid;
  SumRun run;
  run.items.push_back(density_item(p, 0.3, Ngrid, circ));  // LD[d] = getKDERangeLinspace(marginal(p, [d]), extend=0.3) (:599)
  KDEHIP_CHECK_RC(run.alloc(extra));
  unsigned char *x = reinterpret_cast<unsigned char *>(run.extra());
  double *d_res = reinterpret_cast<double *>(x), *d_pts = reinterpret_cast<double *>(x + o_pts);
  double *d_pv = reinterpret_cast<double *>(x + o_pv), *d_qv = reinterpret_cast<double *>(x + o_qv);
  double *d_rows = reinterpret_cast<double *>(x + o_rows);
  const double *d_stats = run.items[0].stats;
  KDEHIP_CHECK_RC(run.enqueue(st));
  hipLaunchKernelGGL(inters_grid_kernel, dim3(static_cast<unsigned>((Nq + 255) / 256)), dim3(256), 0, st, d_stats, D, Ngrid,
                     d_pts);
  KDEHIP_CHECK(hipGetLastError());
  // p and q at the grid by the existing direct evaluation: the values kdehip_evaluate returns at those points
  KDEHIP_CHECK_RC(kdehip_evaluate_device_manifold(p, d_pts, Nq, 0, d_pv, st, manifold));
  KDEHIP_CHECK_RC(kdehip_evaluate_device_manifold(q, d_pts, Nq, 0, d_qv, st, manifold));
  hipLaunchKernelGGL(inters_reduce_kernel, dim3(1), dim3(kSumThreads), 0, st, d_stats, D, Ngrid, d_pv, d_qv, d_rows, d_res);
  KDEHIP_CHECK(hipGetLastError());
  KDEHIP_CHECK_RC(run.wait());
  *out = run.host_extra()[0];
  return KDEHIP_OK;
}

int check_inters_shapes(int64_t Dp, int64_t Dq, int64_t Ngrid) {
  KDEHIP_CHECK_RC(check_grid(Ngrid));
  if (Dp != Dq) return set_error(KDEHIP_ERR_DIM_MISMATCH, "intersIntgAppxIS -- p and q must have the same dimension");
  if (Dp != 1 && Dp != 2) return set_error(KDEHIP_ERR_UNSUPPORTED, "intersIntgAppxIS: Can't do higher dimensions yet");
  if (Dp == 2 && Ngrid > kMaxGrid2) return set_error(KDEHIP_ERR_UNSUPPORTED, "intersIntgAppxIS: 2-D Ngrid above 2^14");
  return KDEHIP_OK;
}

}  // namespace
}  // namespace kdehip

using namespace kdehip;

namespace {

// the batch over items of either struct: item(i) = the kdehip_summary_item, mask(i) = its circular bits
template <typename Item, typename Mask>
int summary_batch(int n, Item item, Mask mask, void *stream) {
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_summary_item &s = item(i);
    KDEHIP_CHECK_RC(check_resident(s.density));
    KDEHIP_CHECK_RC(check_grid(s.Ngrid));
    if (s.density->device != item(0).density->device)
      return set_error(KDEHIP_ERR_ARG, "summary batch: densities on different devices");
    if (mask(i) >> s.density->D) return set_error(KDEHIP_ERR_ARG, "summary batch: a circular bit at or above the item's ndims");
  }
  const int device = item(0).density->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  SumRun run;
  for (int pass = 0; pass < 2; ++pass)  // the Euclidean items first (SumRun)
    for (int i = 0; i < n; ++i) {
      if ((mask(i) != 0) != (pass == 1)) continue;
      const kdehip_summary_item &s = item(i);
      SumItem it = density_item(s.density, s.extend, s.Ngrid, mask(i));
      it.range = s.d_range; it.mean = s.d_mean; it.cov = s.d_cov; it.argmax = s.d_argmax; it.values = s.d_values;
      it.grid = (s.d_argmax || s.d_values) ? 1 : 0;
      run.items.push_back(it);
    }
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return run.defer(device);
}

}  // namespace

extern "C" int kdehip_summary_device_batch(int n, const kdehip_summary_item *items, void *stream) {
  if (n < 0 || (n > 0 && !items)) return set_error(KDEHIP_ERR_ARG, "summary batch: bad item list");
  return summary_batch(n, [&](int i) -> const kdehip_summary_item & { return items[i]; }, [](int) { return 0u; }, stream);
}

extern "C" int kdehip_summary_device_batch_manifold(int n, const kdehip_summary_manifold_item *items, void *stream) {
  if (n < 0 || (n > 0 && !items)) return set_error(KDEHIP_ERR_ARG, "summary batch: bad item list");
  return summary_batch(n, [&](int i) -> const kdehip_summary_item & { return items[i].item; },
                       [&](int i) { return items[i].circular_mask; }, stream);
}

extern "C" int kdehip_density_summary(const kdehip_device_density *p, const double *extend, int64_t Ngrid, double *range,
                                      double *mean, double *cov, double *argmax, double *values) {
  return kdehip_density_summary_manifold(p, extend, Ngrid, range, mean, cov, argmax, values, nullptr);
}

extern "C" int kdehip_density_summary_manifold(const kdehip_device_density *p, const double *extend, int64_t Ngrid,
                                               double *range, double *mean, double *cov, double *argmax, double *values,
                                               const uint8_t *manifold) {
  KDEHIP_CHECK_RC(check_resident(p));
  KDEHIP_CHECK_RC(check_grid(Ngrid));
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->D, &circ));
  const int64_t D = p->D;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(p->device));
  // extra: [range 2D | mean D | cov D*D | argmax D | values D*Ngrid]
  const int64_t o_mean = 2 * D, o_cov = 3 * D, o_arg = o_cov + D * D, o_val = o_arg + D;
  const int64_t words = o_val + (values ? D * Ngrid : 0);
  SumRun run;
  run.items.push_back(density_item(p, extend ? *extend : 0.1, Ngrid, circ));
  run.items[0].grid = (argmax || values) ? 1 : 0;  // (alloc sizes the grid scratch from it)
  KDEHIP_CHECK_RC(run.alloc(sizeof(double) * words));
  double *x = run.extra();
  SumItem &it = run.items[0];
  if (range) it.range = x;
  if (mean) it.mean = x + o_mean;
  if (cov) it.cov = x + o_cov;
  if (argmax) it.argmax = x + o_arg;
  if (values) it.values = x + o_val;
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  const double *hx = run.host_extra();
  if (range) std::memcpy(range, hx, sizeof(double) * 2 * D);
  if (mean) std::memcpy(mean, hx + o_mean, sizeof(double) * D);
  if (cov) std::memcpy(cov, hx + o_cov, sizeof(double) * D * D);
  if (argmax) std::memcpy(argmax, hx + o_arg, sizeof(double) * D);
  if (values) std::memcpy(values, hx + o_val, sizeof(double) * D * Ngrid);
  return KDEHIP_OK;
}

extern "C" int kdehip_kde_max(const kdehip_density *p, int64_t Ngrid, double *out, double *grid_values, int device) {
  return kdehip_kde_max_manifold(p, Ngrid, out, grid_values, device, nullptr);
}

extern "C" int kdehip_kde_max_manifold(const kdehip_density *p, int64_t Ngrid, double *out, double *grid_values, int device,
                                       const uint8_t *manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host(p));
  KDEHIP_CHECK_RC(check_grid(Ngrid));
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->ndim, &circ));
  Uploaded up;
  KDEHIP_CHECK_RC(kdehip_density_upload(&up.h, p, device));
  return kdehip_density_summary_manifold(up.h, nullptr, Ngrid, nullptr, nullptr, nullptr, out, grid_values, manifold);
}

extern "C" int kdehip_inters_intg_appx_is_device(const kdehip_device_density *p, const kdehip_device_density *q,
                                                 int64_t Ngrid, double *out) {
  return kdehip_inters_intg_appx_is_device_manifold(p, q, Ngrid, out, nullptr);
}

extern "C" int kdehip_inters_intg_appx_is_device_manifold(const kdehip_device_density *p, const kdehip_device_density *q,
                                                          int64_t Ngrid, double *out, const uint8_t *manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident(p));
  KDEHIP_CHECK_RC(check_resident(q));
  KDEHIP_CHECK_RC(check_inters_shapes(p->D, q->D, Ngrid));
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->D, &circ));
  if (p->device != q->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  if (!leaves_share_bandwidth(p) || !leaves_share_bandwidth(q))
    return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths are not supported (the reference's kde! never builds them)");
  return inters_resident(p, q, Ngrid, out, circ ? manifold : nullptr, circ);
}

extern "C" int kdehip_inters_intg_appx_is(const kdehip_density *p, const kdehip_density *q, int64_t Ngrid, double *out,
                                          int device) {
  return kdehip_inters_intg_appx_is_manifold(p, q, Ngrid, out, device, nullptr);
}

extern "C" int kdehip_inters_intg_appx_is_manifold(const kdehip_density *p, const kdehip_density *q, int64_t Ngrid,
                                                   double *out, int device, const uint8_t *manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_host(p));
  KDEHIP_CHECK_RC(check_host(q));
  KDEHIP_CHECK_RC(check_inters_shapes(p->ndim, q->ndim, Ngrid));
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->ndim, &circ));
  for (const kdehip_density *d : {p, q}) {
    const int64_t N = d->npts, D = d->ndim;
    for (int64_t i = 0; i < N; ++i)
      for (int64_t k = 0; k < D; ++k)
        if (d->bandwidth[(N + i) * D + k] != d->bandwidth[N * D + k])
          return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths are not supported (the reference's kde! never builds them)");
  }
  Uploaded up, uq;
  KDEHIP_CHECK_RC(kdehip_density_upload(&up.h, p, device));
  KDEHIP_CHECK_RC(kdehip_density_upload(&uq.h, q, device));
  return inters_resident(up.h, uq.h, Ngrid, out, circ ? manifold : nullptr, circ);
}
