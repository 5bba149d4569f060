// sample.hip -- drawing from a density: `sample`, `rand`, `resample` (reference src/KDE01.jl:155-199,
// src/BallTreeDensity01.jl:312-334; semantics in include/kdehip.h section 2f).
//
// Two kernels.  The table build (one wavefront per density) scatters the leaf weights into original point order, forms
// the reference's C = cumsum(w) ./ C[end] -- a sequential fp64 sum by definition, so one dependent add per point -- and
// the inverse permutation (original index -> leaf row).  The draw kernel gives every sample one lane: the Philox uniform,
// a binary search of it in C (from LDS for up to 2048 points), a gather of the leaf's mean and variance through the inverse permutation, the Philox normals
// in Box-Muller pairs; the points of a workgroup's 256 samples are staged in LDS and written out as one contiguous block.
// The host entry (kdehip_sample) forms the same C on the host -- the same sequence of IEEE additions and divisions, so the
// same bits -- and uploads it with the leaves; every entry point then runs the same draw kernel.
// On a manifold (section 5e) the drawn coordinate of a circular dimension is wrapped on its way to the staging tile:
// circ_wrap of the very value the Euclidean call stores; labels and the other dimensions are untouched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "device_density.hpp"
#include "call_block.hpp"
#include "circ_wrap.hpp"
#include "entry_helpers.hpp"
#include "kdehip_internal.hpp"
#include "philox.hpp"
#include "manifold_arg.hpp"

using namespace kdehip;

namespace {

constexpr int kDrawBlock = 256;          // samples per workgroup and tile
constexpr int kMaxBlocksPerItem = 2048;  // workgroups of one item (8 per CU); larger items loop over their tiles

// table status bits (written by the build kernel)
constexpr int kBadPerm = 1, kBadWeight = 2, kBadTotal = 4;

// One draw: where its table and leaves are, what to draw, where the results go.  The leaf arrays start at the first LEAF
// (row N of the reference's node arrays): leaf k's mean of dimension d is means[k*D + d].
struct SampleItem {
  const double *cdf;     // N: C in original order, C[N-1] = 1
  const int32_t *inv;    // N: original index -> leaf k
  const double *means;   // N*D
  const double *var;     // N*D
  int64_t N, Npts;
  uint64_t seed;
  int64_t offset;
  const int64_t *ind_in;  // NULL = draw the labels
  double *pts;
  int64_t *ind;
  uint32_t circ;  // bit d: dimension d is circular, its coordinate is stored wrapped
};

// the table of one density: weights / permutation from the leaves (tree order), outputs in original order
struct TableJob {
  const double *weights;  // N leaf weights
  const int64_t *perm;    // N leaf permutation entries (1-based original index)
  int64_t N;
  double *cdf;
  int32_t *inv;
  int32_t *status;
};

struct CdfLayout {
  size_t o_inv = 0, o_status = 0, total = 0;
  explicit CdfLayout(int64_t N) {
    Carve c;
    c.take(sizeof(double) * N);
    o_inv = c.take(sizeof(int32_t) * N);
    o_status = c.take(sizeof(int32_t));
    total = c.mark();
  }
};

__device__ __forceinline__ double readlane_f64(double v, int k) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(b & 0xffffffffu), k));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(b >> 32), k));
  return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}

// One wavefront per density.  Every index it writes is checked against N first: an uploaded density's permutation is
// the caller's and may not be one.
__global__ __launch_bounds__(64) void cdf_build_kernel(const TableJob *__restrict__ jobs) {
  const TableJob j = jobs[blockIdx.x];
  const int ln = threadIdx.x;
  const int64_t N = j.N;
  for (int64_t i = ln; i < N; i += 64) j.inv[i] = -1;
  __syncthreads();
  int bad = 0;
  for (int64_t k = ln; k < N; k += 64) {
    const int64_t p = j.perm[k] - 1;
    const double w = j.weights[k];
    if (p < 0 || p >= N) { bad |= kBadPerm; continue; }
    if (!(w >= 0.0 && w <= DBL_MAX)) bad |= kBadWeight;  // negative, NaN, inf
    j.inv[p] = static_cast<int32_t>(k);
    j.cdf[p] = w;
  }
  __syncthreads();
  for (int64_t i = ln; i < N; i += 64)
    if (j.inv[i] < 0) bad |= kBadPerm;  // (a repeated entry leaves another one unset)
  // wave-wide OR
  for (int m = 32; m >= 1; m >>= 1) bad |= __shfl_xor(bad, m);
  if (bad) {
    if (ln == 0) *j.status = bad;
    return;
  }
  // C = cumsum(w): strictly left to right, the running sum passed from lane to lane through scalar registers (whole
  // chunks of 64 with constant lane indices: only the adds are dependent)
  double run = 0.0;
  int64_t base = 0;
  for (; base + 64 <= N; base += 64) {
    const double w = j.cdf[base + ln];
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      run = __dadd_rn(run, readlane_f64(w, k));
      c = ln == k ? run : c;
    }
    j.cdf[base + ln] = c;
  }
  if (base < N) {
    const int64_t i = base + ln;
    const double w = i < N ? j.cdf[i] : 0.0;
    const int cnt = static_cast<int>(N - base);
    double c = 0.0;
    for (int k = 0; k < cnt; ++k) {
      run = __dadd_rn(run, readlane_f64(w, k));
      if (ln == k) c = run;
    }
    if (i < N) j.cdf[i] = c;
  }
  if (!(run > 0.0 && run <= DBL_MAX)) {
    if (ln == 0) *j.status = kBadTotal;
    return;
  }
  __syncthreads();
  for (int64_t i = ln; i < N; i += 64) j.cdf[i] = __ddiv_rn(j.cdf[i], run);  // C ./ C[end]
  if (ln == 0) *j.status = 0;
}

// C of a density of up to kLdsCdf points is searched from LDS (the search is a chain of ~log2 N dependent loads: from L2
// it, not the arithmetic, bounded the draw); larger ones from global memory.
constexpr int kLdsCdf = 2048;

// (all threads of the workgroup) C into LDS when it fits; returns the array the search reads
__device__ __forceinline__ const double *stage_cdf(const SampleItem &it, double *lds_cdf) {
  if (it.N > kLdsCdf || it.ind_in) return it.cdf;
  for (int i = threadIdx.x; i < it.N; i += kDrawBlock) lds_cdf[i] = it.cdf[i];
  __syncthreads();
  return lds_cdf;
}

// The samples [base, base + 256) of one item: lane t draws sample base + t; its D values go through LDS so that the
// workgroup writes its D*256 doubles as one contiguous, coalesced block.
template <int D>
__device__ __forceinline__ void draw_tile(const SampleItem &it, const double *cdf, int64_t base, double *stage) {
  const int t = threadIdx.x;
  const int64_t s = base + t;
  if (s < it.Npts) {
    const uint64_t g = static_cast<uint64_t>(it.offset + s);
    int64_t lab;
    bool ok = true;
    if (it.ind_in) {
      lab = it.ind_in[s] - 1;
      ok = lab >= 0 && lab < it.N;
    } else {
      // the first i with C[i] > u (C[N-1] = 1 > u: always found)
      const double u = philox_uniform(it.seed, g, 1u);
      int64_t lo = 0, hi = it.N - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] > u) hi = mid; else lo = mid + 1;
      }
      lab = lo;
    }
    double n[D + 1];
#pragma unroll
    for (int b = 0; b < (D + 1) / 2; ++b) philox_normal_pair(it.seed, g, static_cast<uint32_t>(b), n[2 * b], n[2 * b + 1]);
    if (ok) {
      const int64_t k = it.inv[lab];
      const double *m = it.means + k * D, *v = it.var + k * D;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double x = __dadd_rn(m[d], __dmul_rn(__dsqrt_rn(v[d]), n[d]));
        stage[t * D + d] = ((it.circ >> d) & 1u) ? circ_wrap(x) : x;
      }
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) stage[t * D + d] = __builtin_nan("");
    }
    it.ind[s] = ok ? lab + 1 : 0;
  }
  __syncthreads();
  const int64_t rem = it.Npts - base;
  const int cnt = static_cast<int>((rem < kDrawBlock ? rem : kDrawBlock) * D);
  double *out = it.pts + base * D;
  for (int e = t; e < cnt; e += kDrawBlock) out[e] = stage[e];
  __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kDrawBlock) void sample_kernel(SampleItem it) {
  __shared__ double stage[kDrawBlock * D];
  __shared__ double lds_cdf[kLdsCdf];
  const double *cdf = stage_cdf(it, lds_cdf);
  for (int64_t tile = blockIdx.x; tile * kDrawBlock < it.Npts; tile += gridDim.x) draw_tile<D>(it, cdf, tile * kDrawBlock, stage);
}

// A batch of items of one D: item i owns workgroups [first[i], first[i+1]).
template <int D>
__global__ __launch_bounds__(kDrawBlock) void sample_batch_kernel(const SampleItem *__restrict__ items,
                                                                  const int32_t *__restrict__ first, int nitems) {
  __shared__ double stage[kDrawBlock * D];
  __shared__ double lds_cdf[kLdsCdf];
  const int b = blockIdx.x;
  const int lo = item_of_block(first, nitems, b);
  const SampleItem it = items[lo];
  const int64_t nb = first[lo + 1] - first[lo];
  const double *cdf = stage_cdf(it, lds_cdf);
  for (int64_t tile = b - first[lo]; tile * kDrawBlock < it.Npts; tile += nb) draw_tile<D>(it, cdf, tile * kDrawBlock, stage);
}

int blocks_for(int64_t Npts) {
  const int64_t t = (Npts + kDrawBlock - 1) / kDrawBlock;
  return static_cast<int>(t < kMaxBlocksPerItem ? t : kMaxBlocksPerItem);
}

int launch_draw(int D, const SampleItem &it, hipStream_t st) {
  KDEHIP_CHECK_RC(dispatch_dims(D, [&](auto dim) {
    hipLaunchKernelGGL(sample_kernel<decltype(dim)::value>, dim3(blocks_for(it.Npts)), dim3(kDrawBlock), 0, st, it);
  }));
  KDEHIP_CHECK(hipGetLastError());
  return KDEHIP_OK;
}

int launch_draw_batch(int D, const SampleItem *d_items, const int32_t *d_first, int n, int blocks, hipStream_t st) {
  KDEHIP_CHECK_RC(dispatch_dims(D, [&](auto dim) {
    hipLaunchKernelGGL(sample_batch_kernel<decltype(dim)::value>, dim3(blocks), dim3(kDrawBlock), 0, st, d_items, d_first, n);
  }));
  KDEHIP_CHECK(hipGetLastError());
  return KDEHIP_OK;
}

int table_error(int status) {
  if (status & kBadPerm) return set_error(KDEHIP_ERR_ARG, "sample: the density's permutation is not a permutation of 1..N");
  if (status & kBadWeight) return set_error(KDEHIP_ERR_ARG, "sample: a weight is negative or not finite");
  return set_error(KDEHIP_ERR_ARG, "sample: the weights do not have a positive finite total");
}

// Builds the tables of the handles in `hs` that have none yet (the device is current): one launch, one wait.  Every handle
// of `hs` is distinct; the caller holds their cdf_mu.
int build_tables(const std::vector<kdehip_device_density *> &hs) {
  std::vector<kdehip_device_density *> todo;
  for (kdehip_device_density *h : hs)
    if (!h->cdf_ready.load(std::memory_order_acquire)) todo.push_back(h);
  if (todo.empty()) return KDEHIP_OK;
  hipStream_t st = hipStreamPerThread;
  const size_t nj = todo.size();
  std::vector<TableJob> jobs(nj);
  for (size_t q = 0; q < nj; ++q) {
    kdehip_device_density *h = todo[q];
    const CdfLayout cl(h->N);
    const hipError_t me = cached_malloc(&h->d_cdf, cl.total);
    if (me != hipSuccess) {
      h->d_cdf = nullptr;
      for (size_t r = 0; r < q; ++r) { cached_free(todo[r]->d_cdf, todo[r]->cdf_bytes); todo[r]->d_cdf = nullptr; todo[r]->cdf_bytes = 0; }
      return set_error(KDEHIP_ERR_HIP, std::string("sample table: ") + hipGetErrorString(me));
    }
    h->cdf_bytes = cl.total;
    unsigned char *b = static_cast<unsigned char *>(h->d_cdf);
    jobs[q] = TableJob{h->weights + h->N, h->perm + h->N, h->N, reinterpret_cast<double *>(b),
                       reinterpret_cast<int32_t *>(b + cl.o_inv), reinterpret_cast<int32_t *>(b + cl.o_status)};
  }
  DevBuf sj;
  KDEHIP_CHECK(sj.alloc(sizeof(TableJob) * nj));
  std::vector<int32_t> status(nj, -1);
  hipError_t e = hipMemcpyAsync(sj.p, jobs.data(), sj.n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(cdf_build_kernel, dim3(static_cast<unsigned>(nj)), dim3(64), 0, st, static_cast<const TableJob *>(sj.p));
    e = hipGetLastError();
  }
  for (size_t q = 0; q < nj && e == hipSuccess; ++q)
    e = hipMemcpyAsync(&status[q], jobs[q].status, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t se = hipStreamSynchronize(st);  // (also keeps `jobs` alive until the upload has been served)
  if (e == hipSuccess) e = se;
  if (e != hipSuccess) {
    for (kdehip_device_density *h : todo) { cached_free(h->d_cdf, h->cdf_bytes); h->d_cdf = nullptr; h->cdf_bytes = 0; }
    return set_error(KDEHIP_ERR_HIP, std::string("sample table build: ") + hipGetErrorString(e));
  }
  int rc = KDEHIP_OK;
  for (size_t q = 0; q < nj; ++q) {
    kdehip_device_density *h = todo[q];
    if (status[q] != 0) {  // (the handle's arrays never change: the verdict is kept)
      cached_free(h->d_cdf, h->cdf_bytes);
      h->d_cdf = nullptr; h->cdf_bytes = 0;
      h->cdf_rc = KDEHIP_ERR_ARG;
      if (rc == KDEHIP_OK) rc = table_error(status[q]);
    }
    h->cdf_ready.store(true, std::memory_order_release);
  }
  return rc;
}

int ready_error(const kdehip_device_density *h) {
  return h->cdf_rc == KDEHIP_OK ? KDEHIP_OK
                                : set_error(h->cdf_rc, "sample: the density's weights or permutation cannot be drawn from");
}

// the table of one handle, built on first use (the device is current)
int ensure_table(kdehip_device_density *h) {
  if (h->cdf_ready.load(std::memory_order_acquire)) return ready_error(h);
  std::lock_guard<std::mutex> lock(h->cdf_mu);
  if (h->cdf_ready.load(std::memory_order_acquire)) return ready_error(h);
  return build_tables({h});
}

SampleItem item_of(const kdehip_device_density *h, int64_t Npts, uint64_t seed, int64_t offset, const int64_t *ind_in,
                   double *pts, int64_t *ind, uint32_t circ) {
  const CdfLayout cl(h->N);
  const unsigned char *b = static_cast<const unsigned char *>(h->d_cdf);
  return SampleItem{reinterpret_cast<const double *>(b), reinterpret_cast<const int32_t *>(b + cl.o_inv),
                    h->means + h->N * h->D, h->bandwidth + h->N * h->D, h->N, Npts, seed, offset, ind_in, pts, ind, circ};
}

bool weight_ok(double w) { return w >= 0.0 && w <= DBL_MAX; }

}  // namespace

extern "C" int kdehip_sample(const kdehip_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset,
                             const int64_t *ind_in, double *pts, int64_t *ind, int device) {
  return kdehip_sample_manifold(p, Npts, seed, sample_offset, ind_in, pts, ind, device, nullptr);
}

extern "C" int kdehip_sample_manifold(const kdehip_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset,
                                      const int64_t *ind_in, double *pts, int64_t *ind, int device,
                                      const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!p) return set_error(KDEHIP_ERR_ARG, "null density");
  if (Npts < 0) return set_error(KDEHIP_ERR_ARG, "sample: Npts < 0");
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->ndim, &circ));
  if (Npts == 0) return KDEHIP_OK;
  const int64_t N = p->npts, D = p->ndim;
  if (D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (D < 1 || N < 1) return set_error(KDEHIP_ERR_ARG, "sample: density with no points or no dimensions");
  if (N > (int64_t(1) << 30)) return set_error(KDEHIP_ERR_UNSUPPORTED, "density too large");
  if (!p->means || !p->bandwidth || !p->weights || !p->permutation) return set_error(KDEHIP_ERR_ARG, "density with a null array");
  if (!pts || !ind) return set_error(KDEHIP_ERR_ARG, "null output buffer");
  std::vector<double> C;
  std::vector<int32_t> inv;
  try {
    C.assign(static_cast<size_t>(N), 0.0);
    inv.assign(static_cast<size_t>(N), -1);
  } catch (const std::exception &e) {
    return set_error(KDEHIP_ERR_ALLOC, std::string("sample: ") + e.what());
  }
  for (int64_t k = 0; k < N; ++k) {
    const int64_t q = p->permutation[N + k] - 1;
    if (q < 0 || q >= N || inv[q] >= 0) return set_error(KDEHIP_ERR_ARG, "sample: the density's permutation is not a permutation of 1..N");
    inv[q] = static_cast<int32_t>(k);
    const double w = p->weights[N + k];
    if (!weight_ok(w)) return set_error(KDEHIP_ERR_ARG, "sample: a weight is negative or not finite");
    C[q] = w;
  }
  // C = cumsum(w) ./ C[end]: the table kernel's additions and divisions, in the same order
  double run = 0.0;
  for (int64_t i = 0; i < N; ++i) { run += C[i]; C[i] = run; }
  if (!(run > 0.0 && run <= DBL_MAX)) return set_error(KDEHIP_ERR_ARG, "sample: the weights do not have a positive finite total");
  for (int64_t i = 0; i < N; ++i) C[i] /= run;
  if (ind_in)
    for (int64_t s = 0; s < Npts; ++s)
      if (ind_in[s] < 1 || ind_in[s] > N) return set_error(KDEHIP_ERR_ARG, "sample: a label is outside 1..Npts(p)");
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != KDEHIP_OK) return rc;
  hipStream_t st = hipStreamPerThread;
  const size_t nd = sizeof(double) * N * D;
  Carve c;
  c.take(sizeof(double) * N);
  const size_t o_inv = c.take(sizeof(int32_t) * N), o_m = c.take(nd), o_v = c.take(nd),
               o_in = c.take(ind_in ? sizeof(int64_t) * Npts : 0), o_pts = c.take(sizeof(double) * Npts * D),
               o_ind = c.take(sizeof(int64_t) * Npts);
  CallBlock sc;
  KDEHIP_CHECK(sc.alloc(c.mark()));
  sc.touch(st);
  unsigned char *b = sc.dev();
  KDEHIP_CHECK(hipMemcpyAsync(b, C.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
  KDEHIP_CHECK(hipMemcpyAsync(b + o_inv, inv.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  KDEHIP_CHECK(hipMemcpyAsync(b + o_m, p->means + N * D, nd, hipMemcpyHostToDevice, st));
  KDEHIP_CHECK(hipMemcpyAsync(b + o_v, p->bandwidth + N * D, nd, hipMemcpyHostToDevice, st));
  if (ind_in) KDEHIP_CHECK(hipMemcpyAsync(b + o_in, ind_in, sizeof(int64_t) * Npts, hipMemcpyHostToDevice, st));
  const SampleItem it{reinterpret_cast<const double *>(b), reinterpret_cast<const int32_t *>(b + o_inv),
                      reinterpret_cast<const double *>(b + o_m), reinterpret_cast<const double *>(b + o_v), N, Npts, seed,
                      sample_offset, ind_in ? reinterpret_cast<const int64_t *>(b + o_in) : nullptr,
                      reinterpret_cast<double *>(b + o_pts), reinterpret_cast<int64_t *>(b + o_ind), circ};
  rc = launch_draw(static_cast<int>(D), it, st);
  if (rc != KDEHIP_OK) return rc;
  KDEHIP_CHECK(hipMemcpyAsync(pts, b + o_pts, sizeof(double) * Npts * D, hipMemcpyDeviceToHost, st));
  KDEHIP_CHECK(hipMemcpyAsync(ind, b + o_ind, sizeof(int64_t) * Npts, hipMemcpyDeviceToHost, st));
  KDEHIP_CHECK(sc.wait());
  return KDEHIP_OK;
}

extern "C" int kdehip_sample_device(kdehip_device_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset,
                                    const int64_t *d_ind_in, double *d_pts, int64_t *d_ind, void *stream) {
  return kdehip_sample_device_manifold(p, Npts, seed, sample_offset, d_ind_in, d_pts, d_ind, stream, nullptr);
}

extern "C" int kdehip_sample_device_manifold(kdehip_device_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset,
                                             const int64_t *d_ind_in, double *d_pts, int64_t *d_ind, void *stream,
                                             const uint8_t *manifold) {
  if (!p) return set_error(KDEHIP_ERR_ARG, "null density");
  if (Npts < 0) return set_error(KDEHIP_ERR_ARG, "sample: Npts < 0");
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->D, &circ));
  if (Npts == 0) return KDEHIP_OK;
  if (p->D < 1 || p->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (!d_pts || !d_ind) return set_error(KDEHIP_ERR_ARG, "null output buffer");
  DeviceGuard guard;
  int rc = guard.enter(p->device);
  if (rc == KDEHIP_OK) rc = ensure_table(p);
  if (rc != KDEHIP_OK) return rc;
  return launch_draw(p->D, item_of(p, Npts, seed, sample_offset, d_ind_in, d_pts, d_ind, circ),
                     static_cast<hipStream_t>(stream));
}

namespace {

// the batch over items of either struct: item(i) = the kdehip_sample_item, mask(i) = its circular bits
template <typename Item, typename Mask>
int sample_batch(int n, Item item, Mask mask, void *stream) {
  int device = -1;
  std::vector<kdehip_device_density *> hs;
  for (int i = 0; i < n; ++i) {
    const kdehip_sample_item &it = item(i);
    if (!it.density) return set_error(KDEHIP_ERR_ARG, "sample batch: null density");
    if (it.Npts < 0) return set_error(KDEHIP_ERR_ARG, "sample batch: Npts < 0");
    if (it.density->D >= 1 && it.density->D <= KDEHIP_MAX_DIMS && (mask(i) >> it.density->D))
      return set_error(KDEHIP_ERR_ARG, "sample batch: a circular bit at or above the item's ndims");
    if (it.Npts == 0) continue;
    if (it.density->D < 1 || it.density->D > KDEHIP_MAX_DIMS)
      return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
    if (!it.d_pts || !it.d_ind) return set_error(KDEHIP_ERR_ARG, "sample batch: null output buffer");
    if (device < 0) device = it.density->device;
    if (it.density->device != device) return set_error(KDEHIP_ERR_ARG, "sample batch: densities on different devices");
    hs.push_back(it.density);
  }
  if (hs.empty()) return KDEHIP_OK;
  std::sort(hs.begin(), hs.end());
  hs.erase(std::unique(hs.begin(), hs.end()), hs.end());
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != KDEHIP_OK) return rc;
  {
    // the handles' locks in address order (no deadlock with another batch), then one build for all that need it
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(hs.size());
    for (kdehip_device_density *h : hs)
      if (!h->cdf_ready.load(std::memory_order_acquire)) locks.emplace_back(h->cdf_mu);
    if (!locks.empty()) rc = build_tables(hs);
    if (rc != KDEHIP_OK) return rc;
  }
  for (kdehip_device_density *h : hs) {
    rc = ready_error(h);
    if (rc != KDEHIP_OK) return rc;
  }
  reap_deferred(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // per D: [items | first blocks], one upload through a pinned block, one launch
  for (int D = 1; D <= KDEHIP_MAX_DIMS; ++D) {
    std::vector<SampleItem> its;
    std::vector<int32_t> first(1, 0);
    for (int i = 0; i < n; ++i) {
      const kdehip_sample_item &it = item(i);
      if (it.Npts == 0 || it.density->D != D) continue;
      its.push_back(item_of(it.density, it.Npts, it.seed, it.sample_offset, it.d_ind_in, it.d_pts, it.d_ind, mask(i)));
      const int64_t nb = static_cast<int64_t>(first.back()) + blocks_for(it.Npts);
      if (nb > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "sample batch: too many workgroups");
      first.push_back(static_cast<int32_t>(nb));
    }
    if (its.empty()) continue;
    const int m = static_cast<int>(its.size());
    const size_t o_first = align256(sizeof(SampleItem) * m), bytes = o_first + sizeof(int32_t) * first.size();
    CallBlock blk;
    hipError_t e = blk.alloc(bytes, bytes);
    if (e != hipSuccess) return set_error(KDEHIP_ERR_HIP, std::string("sample batch: ") + hipGetErrorString(e));
    std::memcpy(blk.host(), its.data(), sizeof(SampleItem) * m);
    std::memcpy(blk.host() + o_first, first.data(), sizeof(int32_t) * first.size());
    e = blk.upload(bytes, st);
    if (e != hipSuccess) return set_error(KDEHIP_ERR_HIP, std::string("sample batch: ") + hipGetErrorString(e));
    KDEHIP_CHECK_RC(launch_draw_batch(D, reinterpret_cast<const SampleItem *>(blk.dev()),
                                      reinterpret_cast<const int32_t *>(blk.dev() + o_first), m, first.back(), st));
    KDEHIP_CHECK_RC(blk.defer(device));
  }
  return KDEHIP_OK;
}

}  // namespace

extern "C" int kdehip_sample_device_batch(int n, const kdehip_sample_item *items, void *stream) {
  if (n < 0 || (n > 0 && !items)) return set_error(KDEHIP_ERR_ARG, "sample batch: bad item list");
  return sample_batch(n, [&](int i) -> const kdehip_sample_item & { return items[i]; }, [](int) { return 0u; }, stream);
}

extern "C" int kdehip_sample_device_batch_manifold(int n, const kdehip_sample_manifold_item *items, void *stream) {
  if (n < 0 || (n > 0 && !items)) return set_error(KDEHIP_ERR_ARG, "sample batch: bad item list");
  return sample_batch(n, [&](int i) -> const kdehip_sample_item & { return items[i].item; },
                      [&](int i) { return items[i].circular_mask; }, stream);
}

extern "C" int kdehip_resample_device(kdehip_device_density **out, kdehip_device_density *p, int64_t Np, uint64_t seed,
                                      double *bw_out, int32_t *nevals) {
  return kdehip_resample_device_manifold(out, p, Np, seed, bw_out, nevals, nullptr, nullptr);
}

// (manifold: the draw is wrapped and the bandwidth search takes circular differences; tree_manifold: the builder's operators)
extern "C" int kdehip_resample_device_manifold(kdehip_device_density **out, kdehip_device_density *p, int64_t Np,
                                               uint64_t seed, double *bw_out, int32_t *nevals, const uint8_t *manifold,
                                               const uint8_t *tree_manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null out pointer");
  *out = nullptr;
  if (!p) return set_error(KDEHIP_ERR_ARG, "null density");
  if (Np <= 0) Np = p->N;
  if (Np < 2) return set_error(KDEHIP_ERR_ARG, "resample: kde!(points) needs at least two points");
  uint32_t circ = 0;
  KDEHIP_CHECK_RC(manifold_arg(manifold, p->D, &circ));
  KDEHIP_CHECK_RC(manifold_arg(tree_manifold, p->D, nullptr, kTreeManifold));
  DeviceGuard guard;
  int rc = guard.enter(p->device);
  if (rc != KDEHIP_OK) return rc;
  hipStream_t cs = hipStreamPerThread;
  const int D = p->D;
  const size_t o_ind = align256(sizeof(double) * Np * D);
  CallBlock sc;
  KDEHIP_CHECK(sc.alloc(o_ind + sizeof(int64_t) * Np));
  sc.touch(cs);
  double *d_pts = reinterpret_cast<double *>(sc.dev());
  int64_t *d_ind = reinterpret_cast<int64_t *>(sc.dev() + o_ind);
  rc = kdehip_sample_device_manifold(p, Np, seed, 0, nullptr, d_pts, d_ind, cs, manifold);
  if (rc != KDEHIP_OK) return rc;
  return kdehip_density_from_device_points_tree(out, d_pts, D, Np, p->device, cs, bw_out, nevals, manifold, tree_manifold);
}
