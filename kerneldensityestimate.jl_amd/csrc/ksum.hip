// ksum.hip -- exact overlap measures of two Gaussian-kernel densities by ONE primitive (include/kdehip.h section 5g; no
// reference counterpart: intersIntgAppxIS, src/DualTree01.jl:581-618, approximates the first of them on a grid in 1-D and 2-D):
//   S(A, B; v) = sum_{j<M} b_j sum_{i<N} a_i exp(-1/2 sum_k diff_k(y_jk, x_ik)^2 / v_k)
// with A = (x_i, a_i), B = (y_j, b_j) the leaf points and leaf weights of two densities, v a variance vector (explicit, or
// the sum of the two densities' leaf variances) and diff_k the plain difference, or circ_wrap of it in a circular dimension.
// With normalize, S / ((2 pi)^(D/2) prod_k sqrt(v_k)):
//   integral p q     = S(p, q; v_p + v_q) normalised           (intersIntg)
//   integral (p-q)^2 = the three such integrals                (ise)
//   MMD^2(p, q; h)   = S(p,p;h^2) - 2 S(p,q;h^2) + S(q,q;h^2)  (mmd)
// Host densities (uploaded for the call, blocking) and resident ones (single and blocking, or batched and enqueue-only) run
// ONE path, any number of items described in device memory by KsumItem:
//   ksum_partial_kernel<D>  one launch per distinct D (one more for its items with a circular dimension): the all-pairs sum
//                           of evaluate.hip's eval_partial_kernel -- one lane per point of B, A staged through LDS in chunks
//                           and read as broadcasts, same exponent, same exponential --, then b_j times the lane's sum reduced
//                           over the block in a fixed LDS tree: ONE double per block, no per-query scratch, no atomics;
//   ksum_reduce_kernel      one thread per item: the block shares in block order, times the scale.
// The full square is summed: no leave-one-out, no triangular shortcut for A == B.  The group split (split_chunks(N, M, 1))
// depends on the pair's sizes alone, so the host entry, a single device call and any batch give the same bits, and S(p, p)
// is S(p, an equal copy of p).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "circ_wrap.hpp"
#include "device_density.hpp"
#include "call_block.hpp"
#include "entry_helpers.hpp"
#include "manifold_arg.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"

using namespace kdehip;

namespace {

// One sum: the N leaves of A against the M leaves of B.
struct KsumItem {
  const double *src;   // [N][D] A's leaf means (tree order)
  const double *w;     // [N] A's leaf weights
  const double *qry;   // [M][D] B's leaf means
  const double *qw;    // [M] B's leaf weights
  const double *va;    // [D] the variances v, or A's first leaf's when vb is set
  const double *vb;    // null, or [D] B's first leaf's variances: v_k = va[k] + vb[k]
  double *bpart;       // [ngroups * qblocks] the blocks' shares
  double *out;         // the result
  double norm0;        // (2 pi)^(D/2) as the host's libm rounds it
  int64_t N, M, chunks_per_group;
  int32_t ngroups, D, normalize, pad_;
};

__device__ __forceinline__ double ksum_var(const KsumItem &it, int k) { return it.vb ? it.va[k] + it.vb[k] : it.va[k]; }

// bpart[grp * qblocks + qb] = sum over the lanes j of query block qb, in a fixed tree, of
//   b_j * (sum over the source chunks c of group grp, in chunk order, of sum_{i in chunk c} a_i exp(-1/2 sum_k d_k^2 / v_k))
// for the items [0, n) of one D: item i owns blocks [first[i], first[i+1]) - first[0], its block k is query block
// k % qblocks of source group k / qblocks -- eval_partial_kernel's mapping (256 query lanes, ONE group of consecutive
// 128-point source chunks walked in order, LDS double buffer, broadcast reads) and its arithmetic (the same fma order, the
// same -0.5 / v_k, exp_nonpos).  Every lane, those at or beyond M included, walks the same chunks and barriers; a lane at or
// beyond M contributes exactly 0.
// CIRC: bit k of masks[i] (made uniform over the wave) sends dimension k's difference through circ_wrap before it is
// squared; data in which no difference wraps gives the bits of the Euclidean instantiation.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void ksum_partial_kernel(const KsumItem *__restrict__ items,
                                                                    const int32_t *__restrict__ first, int n,
                                                                    const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  __shared__ double red[kEvalThreads];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const int b = static_cast<int>(blockIdx.x) + first[0];
  const int i = item_of_block(first, n, b);
  const KsumItem pb = items[i];
  unsigned circ = 0;
  if constexpr (CIRC) circ = __builtin_amdgcn_readfirstlane(masks[i]);
  const int64_t qblocks = (pb.M + kEvalThreads - 1) / kEvalThreads;
  const int64_t kb = b - first[i];  // < ngroups * qblocks: the item's blocks are exactly its shares
  const int64_t qb = kb % qblocks, grp = kb / qblocks;
  const int64_t q = qb * kEvalThreads + threadIdx.x;
  const int64_t c_begin = grp * pb.chunks_per_group;
  int64_t c_end = c_begin + pb.chunks_per_group;
  const int64_t nchunks = (pb.N + kEvalChunk - 1) / kEvalChunk;
  if (c_end > nchunks) c_end = nchunks;
  double nhib[D];  // -1/(2 v_k)
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / ksum_var(pb, k);
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = (q < pb.M) ? pb.qry[q * D + k] : 0.0;
  const double bq = (q < pb.M) ? pb.qw[q] : 0.0;
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((pb.N - i0 < kEvalChunk) ? (pb.N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * (D + 1); t += kEvalThreads) {
      const int i = t / (D + 1), f = t % (D + 1);
      sSrc[buf][t] = (f < D) ? pb.src[(i0 + i) * D + f] : pb.w[i0 + i];
    }
  };
  if (c_begin < c_end) stage(c_begin, 0);  // (block-uniform; split_chunks leaves no group empty)
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
      sum += s[D] * exp_nonpos(acc, sExpTab);  // acc <= 0
    }
    total += sum;
  }
  red[threadIdx.x] = (q < pb.M) ? total * bq : 0.0;
  __syncthreads();
  for (int off = kEvalThreads / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) pb.bpart[kb] = red[0];
}

// one thread per item: the block shares in block order, times the scale -- 1, or with normalize
// 1 / ((2 pi)^(D/2) prod_k sqrt(v_k)), the product over k ascending as eval_finish_kernel forms its norm (a product of the
// variances themselves would leave the range of fp64 for small bandwidths in 8-D).  Formed HERE for every route.
__global__ void ksum_reduce_kernel(const KsumItem *__restrict__ items, int n) {
  const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const KsumItem it = items[i];
  const int64_t nb = ((it.M + kEvalThreads - 1) / kEvalThreads) * it.ngroups;
  double s = 0.0;
  int64_t b = 0;
  for (; b + 16 <= nb; b += 16) {  // sixteen loads in flight, added in block order: the bits of the plain loop
    double t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = it.bpart[b + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += t[u];
  }
  for (; b < nb; ++b) s += it.bpart[b];
  double scale = 1.0;
  if (it.normalize) {
    double norm = it.norm0;
    for (int k = 0; k < it.D; ++k) norm *= __dsqrt_rn(ksum_var(it, k));
    scale = 1.0 / norm;
  }
  *it.out = s * scale;
}

int launch_ksum_partial(int D, const KsumItem *d_items, const int32_t *d_first, int n, int blocks, const uint32_t *d_masks,
                        hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(blocks)), block(kEvalThreads);
  KDEHIP_CHECK_RC(dispatch_dims(D, [&](auto dim) {
    constexpr int kD = decltype(dim)::value;
    if (d_masks) hipLaunchKernelGGL((ksum_partial_kernel<kD, true>), grid, block, 0, st, d_items, d_first, n, d_masks);
    else hipLaunchKernelGGL((ksum_partial_kernel<kD, false>), grid, block, 0, st, d_items, d_first, n,
                            static_cast<const uint32_t *>(nullptr));
  }));
  KDEHIP_CHECK(hipGetLastError());
  return KDEHIP_OK;
}

// The blocks of one call, as evaluate.hip's EvalRun lays them out: ONE device block [caller's data | descriptors | first[],
// masks | explicit variances | results | per item: block shares] and ONE pinned image of everything before the results,
// which goes up in one copy.  Protocol: fill `items` (sizes, D, normalize), `circ` and `var` -> alloc(prefix bytes of caller
// data) -> point the items at their data (and at result(k), or at the caller's output) -> enqueue(stream) -> wait()
// (blocking calls) or defer(device) (enqueue-only calls).
class KsumRun {
 public:
  std::vector<KsumItem> items;
  std::vector<uint32_t> circ;        // per item: its circular dimensions (bit k = dimension k)
  std::vector<const double *> var;   // per item: the caller's D explicit variances (host), or null: the leaf variances
  int alloc(size_t prefix) {
    const size_t n = items.size();
    int64_t blocks = 0;
    for (KsumItem &it : items) {
      const GroupSplit gs = split_chunks(it.N, it.M, 1);
      it.chunks_per_group = gs.chunks_per_group;
      it.ngroups = gs.ngroups;
      blocks += ((it.M + kEvalThreads - 1) / kEvalThreads) * it.ngroups;
    }
    if (blocks > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "kernel sum too large for one launch");
    Carve c;
    c.take(prefix);
    o_items_ = c.take(sizeof(KsumItem) * n);
    o_first_ = c.take(sizeof(int32_t) * (n + 1) + sizeof(uint32_t) * n);  // first[], then the masks
    o_masks_ = o_first_ + sizeof(int32_t) * (n + 1);
    o_var_ = c.take(sizeof(double) * KDEHIP_MAX_DIMS * n);
    o_res_ = c.take(sizeof(double) * n);
    shares_.resize(n);
    for (size_t k = 0; k < n; ++k)
      shares_[k] = c.take(sizeof(double) * ((items[k].M + kEvalThreads - 1) / kEvalThreads) * items[k].ngroups);
    KDEHIP_CHECK(blk_.alloc(c.mark(), o_res_ + sizeof(double) * n));
    for (size_t k = 0; k < n; ++k) {
      KsumItem &it = items[k];
      it.bpart = reinterpret_cast<double *>(dev() + shares_[k]);
      if (!var[k]) continue;
      std::memcpy(host() + o_var_ + sizeof(double) * KDEHIP_MAX_DIMS * k, var[k], sizeof(double) * it.D);
      it.va = reinterpret_cast<const double *>(dev() + o_var_) + KDEHIP_MAX_DIMS * k;
      it.vb = nullptr;
    }
    return KDEHIP_OK;
  }
  unsigned char *dev() const { return blk_.dev(); }
  unsigned char *host() const { return blk_.host(); }
  double *result(size_t k) const { return reinterpret_cast<double *>(dev() + o_res_) + k; }
  double *host_result(size_t k) const { return reinterpret_cast<double *>(host() + o_res_) + k; }

  // descriptors sorted (by D; Euclidean items before circular ones), one upload, one launch per run of equal (D, circular),
  // one reduce
  int enqueue(hipStream_t st) {
    const size_t n = items.size();
    {
      std::vector<size_t> ord(n);
      for (size_t k = 0; k < n; ++k) ord[k] = k;
      auto key = [&](size_t k) { return 2 * items[k].D + (circ[k] ? 1 : 0); };
      std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return key(a) < key(b); });
      std::vector<KsumItem> si(n);
      std::vector<uint32_t> sc(n);
      for (size_t k = 0; k < n; ++k) { si[k] = items[ord[k]]; sc[k] = circ[ord[k]]; }
      items.swap(si);
      circ.swap(sc);
    }
    std::memcpy(host() + o_masks_, circ.data(), sizeof(uint32_t) * n);
    int32_t *first = reinterpret_cast<int32_t *>(host() + o_first_);
    first[0] = 0;
    for (size_t k = 0; k < n; ++k)
      first[k + 1] = first[k] + static_cast<int32_t>(((items[k].M + kEvalThreads - 1) / kEvalThreads) * items[k].ngroups);
    std::memcpy(host() + o_items_, items.data(), sizeof(KsumItem) * n);
    KDEHIP_CHECK(blk_.upload(o_res_, st));
    const KsumItem *d_items = reinterpret_cast<const KsumItem *>(dev() + o_items_);
    const int32_t *d_first = reinterpret_cast<const int32_t *>(dev() + o_first_);
    const uint32_t *d_masks = reinterpret_cast<const uint32_t *>(dev() + o_masks_);
    for (size_t a = 0; a < n;) {
      size_t e = a;
      while (e < n && items[e].D == items[a].D && !circ[e] == !circ[a]) ++e;
      KDEHIP_CHECK_RC(launch_ksum_partial(items[a].D, d_items + a, d_first + a, static_cast<int>(e - a), first[e] - first[a],
                                          circ[a] ? d_masks + a : nullptr, st));
      a = e;
    }
    hipLaunchKernelGGL(ksum_reduce_kernel, dim3(static_cast<unsigned>((n + 63) / 64)), dim3(64), 0, st, d_items,
                       static_cast<int>(n));
    KDEHIP_CHECK(hipGetLastError());
    return KDEHIP_OK;
  }
  // blocking calls: the results come back to host_result()
  int wait() {
    const hipError_t e = blk_.download(o_res_, sizeof(double) * items.size(), blk_.stream());
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
  size_t o_items_ = 0, o_first_ = 0, o_masks_ = 0, o_var_ = 0, o_res_ = 0;
  std::vector<size_t> shares_;
};

// explicit variances: D of them, each finite and > 0
int check_var(const double *var, int64_t D) {
  for (int64_t k = 0; var && k < D; ++k)
    if (!(std::isfinite(var[k]) && var[k] > 0.0)) return set_error(KDEHIP_ERR_ARG, "kernel sum: every variance must be finite and > 0");
  return KDEHIP_OK;
}

// the checks every resident entry makes on one item; none touches a device
int check_resident(const kdehip_device_density *a, const kdehip_device_density *b, const double *var, uint32_t mask) {
  if (!a || !b) return set_error(KDEHIP_ERR_ARG, "null density");
  if (a->D > KDEHIP_MAX_DIMS || b->D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (a->D < 1 || b->D < 1) return set_error(KDEHIP_ERR_ARG, "density with no dimensions");
  if (a->D != b->D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "kernel sum -- dimensions of two BallTreeDensities must match");
  if (a->device != b->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  if (!var && !(leaves_share_bandwidth(a) && leaves_share_bandwidth(b)))
    return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths need explicit variances (the sum of the leaf variances is one vector)");
  KDEHIP_CHECK_RC(check_var(var, a->D));
  if (mask >> a->D) return set_error(KDEHIP_ERR_ARG, "kernel sum: circular_mask names a dimension the densities do not have");
  return KDEHIP_OK;
}

KsumItem resident_item(const kdehip_device_density *a, const kdehip_device_density *b, int normalize) {
  KsumItem it{};
  const int64_t N = a->N, M = b->N;
  const int D = a->D;
  it.src = a->means + N * D; it.w = a->weights + N; it.va = a->bandwidth + N * D;
  it.qry = b->means + M * D; it.qw = b->weights + M; it.vb = b->bandwidth + M * D;
  it.norm0 = std::pow(2.0 * M_PI, D / 2.0);
  it.N = N; it.M = M; it.D = D; it.normalize = normalize ? 1 : 0;
  return it;
}

// a host density as the sum reads it: leaves, weights and (without explicit variances) ONE bandwidth vector
int check_host(const kdehip_density *p, bool need_bw) {
  const int64_t N = p->npts, D = p->ndim;
  if (N < 1 || !p->means || !p->weights || (need_bw && !p->bandwidth)) return set_error(KDEHIP_ERR_ARG, "malformed density");
  if (!need_bw) return KDEHIP_OK;
  const double *bw = p->bandwidth + N * D;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t k = 0; k < D; ++k)
      if (p->bandwidth[(N + i) * D + k] != bw[k])
        return set_error(KDEHIP_ERR_UNSUPPORTED, "per-point bandwidths need explicit variances (the sum of the leaf variances is one vector)");
  return KDEHIP_OK;
}

}  // namespace

extern "C" int kdehip_kernel_sum_device_batch(int n, const kdehip_ksum_item *items, double *d_out, void *stream) {
  if (n < 0 || (n > 0 && (!items || !d_out))) return set_error(KDEHIP_ERR_ARG, "kernel sum batch: bad item list");
  if (n == 0) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    KDEHIP_CHECK_RC(check_resident(items[i].a, items[i].b, items[i].var, items[i].circular_mask));
    if (items[i].a->device != items[0].a->device) return set_error(KDEHIP_ERR_ARG, "kernel sum batch: densities on different devices");
  }
  const int device = items[0].a->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  KsumRun run;
  for (int i = 0; i < n; ++i) {
    run.items.push_back(resident_item(items[i].a, items[i].b, items[i].normalize));
    run.items.back().out = d_out + i;
    run.circ.push_back(items[i].circular_mask);
    run.var.push_back(items[i].var);
  }
  KDEHIP_CHECK_RC(run.alloc(0));
  KDEHIP_CHECK_RC(run.enqueue(static_cast<hipStream_t>(stream)));
  return run.defer(device);
}

extern "C" int kdehip_kernel_sum_device(const kdehip_device_density *a, const kdehip_device_density *b, const double *var,
                                        int normalize, double *out, const uint8_t *manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KDEHIP_CHECK_RC(check_resident(a, b, var, 0u));
  uint32_t circ = 0;
  if (manifold_arg(manifold, a->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(a->device));
  KsumRun run;
  run.items.push_back(resident_item(a, b, normalize));
  run.circ.push_back(circ);
  run.var.push_back(var);
  KDEHIP_CHECK_RC(run.alloc(0));
  run.items[0].out = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}

extern "C" int kdehip_kernel_sum(const kdehip_density *a, const kdehip_density *b, const double *var, int normalize,
                                 double *out, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!a || !b || !out) return set_error(KDEHIP_ERR_ARG, "null argument");
  const int64_t D = a->ndim, N = a->npts, M = b->npts;
  if (D > KDEHIP_MAX_DIMS || b->ndim > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims above KDEHIP_MAX_DIMS");
  if (D < 1 || b->ndim < 1) return set_error(KDEHIP_ERR_ARG, "density with no dimensions");
  if (b->ndim != D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "kernel sum -- dimensions of two BallTreeDensities must match");
  KDEHIP_CHECK_RC(check_host(a, !var));
  if (b != a) KDEHIP_CHECK_RC(check_host(b, !var));
  KDEHIP_CHECK_RC(check_var(var, D));
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const bool self = a == b;
  // caller data: [a leaf means | a leaf weights | b leaf means | b leaf weights (a == b: neither) | a's, b's first-leaf
  // variances (explicit variances: neither)]
  const size_t o_w = sizeof(double) * N * D, o_q = o_w + sizeof(double) * N;
  const size_t o_qw = o_q + (self ? 0 : sizeof(double) * M * D), o_va = o_qw + (self ? 0 : sizeof(double) * M);
  const size_t o_vb = o_va + (var ? 0 : sizeof(double) * D), prefix = o_vb + (var ? 0 : sizeof(double) * D);
  KsumRun run;
  KsumItem it{};
  it.norm0 = std::pow(2.0 * M_PI, D / 2.0);
  it.N = N; it.M = M; it.D = static_cast<int32_t>(D); it.normalize = normalize ? 1 : 0;
  run.items.push_back(it);
  run.circ.push_back(circ);
  run.var.push_back(var);
  KDEHIP_CHECK_RC(run.alloc(prefix));
  unsigned char *h = run.host(), *d = run.dev();
  std::memcpy(h, a->means + N * D, sizeof(double) * N * D);
  std::memcpy(h + o_w, a->weights + N, sizeof(double) * N);
  if (!self) {
    std::memcpy(h + o_q, b->means + M * D, sizeof(double) * M * D);
    std::memcpy(h + o_qw, b->weights + M, sizeof(double) * M);
  }
  KsumItem &ri = run.items[0];
  ri.src = reinterpret_cast<const double *>(d);
  ri.w = reinterpret_cast<const double *>(d + o_w);
  ri.qry = self ? ri.src : reinterpret_cast<const double *>(d + o_q);
  ri.qw = self ? ri.w : reinterpret_cast<const double *>(d + o_qw);
  if (!var) {
    std::memcpy(h + o_va, a->bandwidth + N * D, sizeof(double) * D);
    std::memcpy(h + o_vb, b->bandwidth + M * D, sizeof(double) * D);
    ri.va = reinterpret_cast<const double *>(d + o_va);
    ri.vb = reinterpret_cast<const double *>(d + o_vb);
  }
  ri.out = run.result(0);
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  *out = *run.host_result(0);
  return KDEHIP_OK;
}
