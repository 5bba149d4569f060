// pair_sweep.hpp -- the all-pairs Gaussian sum behind evaluate.hip (eval_partial_kernel, eval_partial_log_kernel) and
// ksum.hip (ksum_partial_kernel), written ONCE: the head both descriptors start with, a block's place in an item, the sweep
// over the staged source chunks, the block reduction and the norm on the device; the skeleton of a call's run (EvalRun,
// KsumRun) and the scope of a call on a capturing stream on the host.  Included by the files of entry points that run the
// sweep or its mapping (evaluate, evaltol, knn, ksum, modes, conditional, mass), and by varbw.hip, whose sweep over sources
// with variances of their own (pair_sweep_var) stands beside it.  What those entries do with a density ARGUMENT -- its
// checks, its leaf rows, its image in the call's block, the keep-or-defer ending -- is density_args.hpp, on top of this file.
//
// The sweep: one lane per query point, a block owns kEvalThreads queries and ONE group of consecutive kEvalChunk-point source
// chunks, which it stages through a two-buffer LDS ring ([point][D coordinates, weight], read back as broadcasts) and walks
// in order.  For every pair it forms the exponent
//   a_i = -1/2 sum_k diff_k(x_qk, c_ik)^2 / v_k     (k ascending, one fma per dimension; diff_k is the plain difference,
//                                                    or circ_wrap of it in a circular dimension)
// and hands (i, w_i, a_i) to the kernel's own step: the plain sum, the sum without the self term, or a running maximum and
// a rescaled sum.  A step that also takes the D differences, f(i, w_i, a_i, d) with d[k] = diff_k -- the values a_i was
// formed from --, gets them (modes.hip: the first moments); the others compile to what they were without them.
// What the variances v_k are is the kernel's business: it passes nhib[k] = -1/(2 v_k).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "call_block.hpp"
#include "circ_wrap.hpp"
#include "entry_helpers.hpp"
#include "kdehip_internal.hpp"

namespace kdehip {

// What the sweep reads of an item: EvalItem and KsumItem begin with it.
struct PairHead {
  const double *src;  // [N][D] source points (leaf means, tree order)
  const double *w;    // [N] their weights
  const double *qry;  // [Nq][D] query points
  int64_t N, Nq, chunks_per_group;
};

// A launch covers the items [0, n) of a longer sorted list: first[0] is the launch's first block in that list's count, item
// i owns blocks [first[i], first[i+1]).  The block's item and its index among the item's blocks.
struct ItemBlock { int item, k; };
__device__ __forceinline__ ItemBlock item_block(const int32_t *__restrict__ first, int n) {
  const int b = static_cast<int>(blockIdx.x) + first[0];
  const int i = item_of_block(first, n, b);
  return {i, b - first[i]};
}

// bit k set: dimension k of item i is circular (uniform over the block); 0 in the Euclidean instantiation
template <bool CIRC>
__device__ __forceinline__ unsigned circ_mask(const uint32_t *__restrict__ masks, int i) {
  if constexpr (CIRC) return __builtin_amdgcn_readfirstlane(masks[i]);
  else return 0u;
}

// Block kb of an item is query block kb % qblocks of source group kb / qblocks: the lane's query q (may lie at or beyond
// Nq) and the group's chunks [c_begin, c_end) (empty for a group past the last chunk: block-uniform).
struct PairPlace { int64_t grp, q, c_begin, c_end; };
__device__ __forceinline__ PairPlace pair_place(const PairHead &h, int64_t kb) {
  const int64_t qblocks = (h.Nq + kEvalThreads - 1) / kEvalThreads;
  const int64_t qb = kb % qblocks, grp = kb / qblocks;
  const int64_t c_begin = grp * h.chunks_per_group;
  int64_t c_end = c_begin + h.chunks_per_group;
  const int64_t nchunks = (h.N + kEvalChunk - 1) / kEvalChunk;
  if (c_end > nchunks) c_end = nchunks;
  return {grp, qb * kEvalThreads + threadIdx.x, c_begin, c_end};
}

// The walk over the chunks of the block's group.  Per staged chunk, in chunk order, step(each) is called once; each(f)
// calls f(i, w_i, a_i) -- or f(i, w_i, a_i, d), d the D differences, if f takes four arguments -- for the chunk's sources in
// order and may be called more than once (a second pass recomputes a_i).
// Every lane, those at or beyond Nq included (their x is 0), walks the same chunks and barriers.
template <int D, bool CIRC, typename Step>
__device__ __forceinline__ void pair_sweep(const PairHead &h, const PairPlace &at, unsigned circ, const double (&nhib)[D],
                                           double (&sSrc)[2][kEvalChunk * (D + 1)], Step &&step) {
  const double *const src = h.src, *const w = h.w;  // (values, not members: stage's choice between them must not index h)
  const int64_t N = h.N;
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = (at.q < h.Nq) ? h.qry[at.q * D + k] : 0.0;
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * (D + 1); t += kEvalThreads) {
      const int i = t / (D + 1), f = t % (D + 1);
      sSrc[buf][t] = (f < D) ? src[(i0 + i) * D + f] : w[i0 + i];
    }
  };
  if (at.c_begin < at.c_end) stage(at.c_begin, 0);
  for (int64_t c = at.c_begin; c < at.c_end; ++c) {
    const int buf = static_cast<int>((c - at.c_begin) & 1);
    __syncthreads();  // chunk c is staged; the other buffer is free again
    if (c + 1 < at.c_end) stage(c + 1, buf ^ 1);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    step([&](auto &&f) {
      constexpr bool kDiffs = std::is_invocable_v<decltype(f), int64_t, double, double, const double (&)[D]>;
      for (int i = 0; i < cnt; ++i) {
        const double *s = sSrc[buf] + i * (D + 1);
        double acc = 0.0;
        [[maybe_unused]] double diff[kDiffs ? D : 1];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          double d = x[k] - s[k];
          if constexpr (CIRC) {
            if ((circ >> k) & 1u) d = circ_wrap(d);
          }
          if constexpr (kDiffs) diff[k] = d;
          acc = fma(d * d, nhib[k], acc);
        }
        if constexpr (kDiffs) f(i0 + i, s[D], acc, diff);
        else f(i0 + i, s[D], acc);  // acc <= 0
      }
    });
  }
}

// The same walk for sources that each have variances of their own (varbw.hip; kdehip.h section 5o): a second function, so
// that pair_sweep above stays what it was.  Per source the ring holds [D coordinates | D values nh_ik = -1/(2 v_ik) | c_i]
// (2D + 1 doubles, read back as broadcasts), c_i being whatever the kernel's step wants next to the exponent -- the folded
// normaliser w_i / prod_k sqrt(v_ik) or its logarithm.  Same mapping, same chunks, same barriers; the exponent is
//   a_i = sum_k diff_k(x_qk, c_ik)^2 nh_ik     (k ascending, one fma per dimension)
// and each(f) calls f(i, c_i, a_i).
template <int D, bool CIRC, typename Step>
__device__ __forceinline__ void pair_sweep_var(const PairHead &h, const double *__restrict__ nh /* [N][D] */,
                                               const double *__restrict__ cc /* [N] */, const PairPlace &at, unsigned circ,
                                               double (&sSrc)[2][kEvalChunk * (2 * D + 1)], Step &&step) {
  constexpr int kRow = 2 * D + 1;
  const double *const src = h.src;
  const int64_t N = h.N;
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = (at.q < h.Nq) ? h.qry[at.q * D + k] : 0.0;
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * kRow; t += kEvalThreads) {
      const int i = t / kRow, f = t % kRow;
      sSrc[buf][t] = (f < D) ? src[(i0 + i) * D + f] : (f < 2 * D) ? nh[(i0 + i) * D + (f - D)] : cc[i0 + i];
    }
  };
  if (at.c_begin < at.c_end) stage(at.c_begin, 0);
  for (int64_t c = at.c_begin; c < at.c_end; ++c) {
    const int buf = static_cast<int>((c - at.c_begin) & 1);
    __syncthreads();  // chunk c is staged; the other buffer is free again
    if (c + 1 < at.c_end) stage(c + 1, buf ^ 1);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    step([&](auto &&f) {
      for (int i = 0; i < cnt; ++i) {
        const double *s = sSrc[buf] + i * kRow;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          double d = x[k] - s[k];
          if constexpr (CIRC) {
            if ((circ >> k) & 1u) d = circ_wrap(d);
          }
          acc = fma(d * d, s[D + k], acc);
        }
        f(i0 + i, s[2 * D], acc);  // acc <= 0
      }
    });
  }
}

// A query with a NaN in one of its D coordinates.  The sweep cannot tell: exp_nonpos's clamp and the running maxima (fmax)
// drop a NaN, so such a query comes out of it like one with no source in reach.  The kernels that finish a query (one thread
// per query) ask this of the position itself and answer NaN.
__device__ __forceinline__ bool query_has_nan(const double *__restrict__ qry, int64_t q, int D) {
  bool bad = false;
  for (int k = 0; k < D; ++k) bad = bad || (qry[q * D + k] != qry[q * D + k]);
  return bad;
}

// The sum of red[0 .. W) in a fixed tree (halving strides), for a block of W threads; red[t] was written by thread t and a
// barrier has passed since.  Every thread returns the sum.
template <int W>
__device__ __forceinline__ double block_tree_sum(double *red) {
  for (int off = W / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

// (2 pi)^(D/2) prod_k sqrt(v_k), norm0 the first factor: the product over k ascending, correctly rounded roots (a product
// of the variances themselves would leave the range of fp64 for small bandwidths in 8-D)   (src/DualTree01.jl:325-330)
template <typename Var>
__device__ __forceinline__ double gauss_norm(double norm0, int D, Var var) {
  double norm = norm0;
  for (int k = 0; k < D; ++k) norm *= __dsqrt_rn(var(k));
  return norm;
}

// ---- host ------------------------------------------------------------------------------------------------------------

// One launch of a sweep kernel over `blocks` blocks: the Euclidean instantiation, or with masks the circular one.
template <typename Item>
using PairKernel = void (*)(const Item *, const int32_t *, int, const uint32_t *);
template <typename Item>
void launch_pair(PairKernel<Item> euclidean, PairKernel<Item> circular, int blocks, hipStream_t st, const Item *d_items,
                 const int32_t *d_first, int n, const uint32_t *d_masks) {
  hipLaunchKernelGGL(d_masks ? circular : euclidean, dim3(static_cast<unsigned>(blocks)), dim3(kEvalThreads), 0, st, d_items,
                     d_first, n, d_masks);
}

// The blocks of one call and what every run of sweep items does with them: ONE device block [caller's data | descriptors |
// first[] arrays, masks | (the run's own) | results | (the run's scratch)] and ONE pinned image of everything up to and
// including the results; what precedes the results goes up in one copy.  Item begins with a PairHead and has D and ngroups.
// A run fills `items` and `circ`, carves (carve_head, its scratch, alloc_block), points the items at their data, then
// prepare -> send -> for_each_run and its own further launches -> wait() (blocking calls) or defer() (enqueue-only calls).
template <typename Item>
class PairRun {
 public:
  std::vector<Item> items;
  std::vector<uint32_t> circ;  // per item: its circular dimensions (bit k = dimension k)
  unsigned char *dev() const { return blk_.dev(); }
  unsigned char *host() const { return blk_.host(); }
  double *result(size_t k) const { return reinterpret_cast<double *>(dev() + o_res_) + k; }  // (device) result k
  double *host_result(size_t k) const { return reinterpret_cast<double *>(host() + o_res_) + k; }
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

  // enqueue-only calls on a stream that is being captured into a graph: both blocks stay until kdehip_clear_cache
  int keep(int device) { return blk_.keep(device); }

 protected:
  // the item's group split (a function of its sizes alone); returns its number of sweep blocks
  static int64_t split(Item &it) {
    const GroupSplit gs = split_chunks(it.N, it.Nq, 1);
    it.chunks_per_group = gs.chunks_per_group;
    it.ngroups = it.Nq > 0 ? gs.ngroups : 0;
    return sweep_blocks(it);
  }
  static int64_t sweep_blocks(const Item &it) { return ((it.Nq + kEvalThreads - 1) / kEvalThreads) * it.ngroups; }
  // the block up to the results, with nfirst first[] arrays and `own` bytes of the run's own; returns the offset of those
  size_t carve_head(Carve &c, size_t prefix, int nfirst, size_t own, size_t nresults) {
    const size_t n = items.size();
    c.take(prefix);
    o_items_ = c.take(sizeof(Item) * n);
    o_first_ = c.take(sizeof(int32_t) * nfirst * (n + 1) + sizeof(uint32_t) * n);
    o_masks_ = o_first_ + sizeof(int32_t) * nfirst * (n + 1);
    const size_t o_own = c.take(own);
    nres_ = nresults;
    o_res_ = c.take(sizeof(double) * nres_);
    return o_own;
  }
  hipError_t alloc_block(const Carve &c) { return blk_.alloc(c.mark(), o_res_ + sizeof(double) * nres_); }
  int32_t *first(int which = 0) const { return reinterpret_cast<int32_t *>(host() + o_first_) + which * (items.size() + 1); }
  // The descriptors sorted by key(k) (stable; the masks go along), then masks, the sweep's first[] and descriptors written
  // to the image.  Items with equal keys share a launch.
  template <typename Key>
  void prepare(Key key) {
    const size_t n = items.size();
    circ.resize(n, 0u);
    std::vector<size_t> ord(n);
    for (size_t k = 0; k < n; ++k) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return key(a) < key(b); });
    std::vector<Item> si(n);
    std::vector<uint32_t> sc(n);
    keys_.resize(n);
    for (size_t k = 0; k < n; ++k) { si[k] = items[ord[k]]; sc[k] = circ[ord[k]]; keys_[k] = key(ord[k]); }
    items.swap(si);
    circ.swap(sc);
    int32_t *f = first();
    f[0] = 0;
    for (size_t k = 0; k < n; ++k) f[k + 1] = f[k] + static_cast<int32_t>(sweep_blocks(items[k]));
    if (n) std::memcpy(host() + o_masks_, circ.data(), sizeof(uint32_t) * n);
    if (n) std::memcpy(host() + o_items_, items.data(), sizeof(Item) * n);
  }
  hipError_t send(hipStream_t st) { return blk_.upload(o_res_, st); }
  hipStream_t stream() const { return blk_.stream(); }
  const Item *d_items() const { return reinterpret_cast<const Item *>(dev() + o_items_); }
  const int32_t *d_first(int which = 0) const { return reinterpret_cast<const int32_t *>(dev() + o_first_) + which * (items.size() + 1); }
  const uint32_t *d_masks() const { return reinterpret_cast<const uint32_t *>(dev() + o_masks_); }  // one word per item
  // launch(first item of the run, its descriptors, its first[], items, blocks, its masks or null) per run of equal key
  template <typename Launch>
  int for_each_run(Launch launch) {
    const size_t n = items.size();
    const int32_t *f = first();
    const uint32_t *d_masks = reinterpret_cast<const uint32_t *>(dev() + o_masks_);
    for (size_t a = 0; a < n;) {
      size_t e = a;
      while (e < n && keys_[e] == keys_[a]) ++e;
      const int blocks = f[e] - f[a];
      if (blocks > 0)
        KDEHIP_CHECK_RC(launch(items[a], d_items() + a, d_first() + a, static_cast<int>(e - a), blocks,
                               circ[a] ? d_masks + a : nullptr));
      a = e;
    }
    return KDEHIP_OK;
  }

 private:
  CallBlock blk_;
  size_t o_items_ = 0, o_first_ = 0, o_masks_ = 0, o_res_ = 0, nres_ = 0;
  std::vector<int> keys_;
};

// While the stream is being captured into a graph the calling thread's capture mode is relaxed (the call allocates and
// copies), and the call's blocks must outlive the call: they are kept until kdehip_clear_cache (kdehip.h 5h: one pair of
// blocks per capture, and clearing the cache invalidates the graph).  A call that fails after its upload leaves through
// ~CallBlock, which synchronises the stream: on a capturing stream that is an error and ends the capture as invalid --
// what a failed capture should be; the blocks go back to the cache, no node of a usable graph refers to them.
class CaptureScope {
 public:
  explicit CaptureScope(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) {
      mode_ = hipStreamCaptureModeRelaxed;
      on_ = hipThreadExchangeStreamCaptureMode(&mode_) == hipSuccess;
      capturing_ = true;
    }
    (void)hipGetLastError();
  }
  ~CaptureScope() {
    if (on_) (void)hipThreadExchangeStreamCaptureMode(&mode_);
  }
  bool capturing() const { return capturing_; }

 private:
  hipStreamCaptureMode mode_ = hipStreamCaptureModeGlobal;
  bool on_ = false, capturing_ = false;
};

}  // namespace kdehip
