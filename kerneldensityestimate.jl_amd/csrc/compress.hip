// compress.hip -- a density cut to M of its own points by kernel herding (include/kdehip.h section 5t; no reference
// counterpart).  With c_i, alpha_i the leaves and leaf weights of p, o(i) the original index of leaf i, v the kernel variances
// (the caller's, or twice p's leaf variances) and a(s, j) the exponent of pair_sweep.hpp between leaf j as the query and
// leaf s as the source (nhib[k] = -0.5 / v_k), the kernel mean is z_j = sum_i alpha_i exp(a(i, j)) and step t = 0 .. M-1 picks
// the not-yet-chosen leaf with the largest (z_j - r_j * (1 / (t + 1)), -o(j)), records it, and adds exp(a(pick, j)) to every r_j.
//   compress_z_kernel<D>       one launch per distinct (D, circular, route): the sweep of eval_partial_kernel with the
//                              density's own leaves as queries: scratch [ngroups][N];
//   compress_z_finish_kernel   one thread per leaf: the groups in group order -> z; r = 0, nothing taken;
//   compress_self_kernel       one workgroup per item: sum_j alpha_j z_j, thread t over j = t, t + 256, .. in order, then the
//                              fixed 256-wide tree of 5b;
//   compress_one_kernel<D>     route A, N <= KDEHIP_COMPRESS_ONE_BLOCK_MAX: ONE workgroup of 1024 threads per item runs all M
//                              steps; a lane keeps its (at most 2) leaves, their z and r in registers; two barriers a step;
//   compress_step_kernel<D>    route B, any N: launch t = 0 .. M of 256-thread blocks, one leaf per thread.  Every block
//                              reduces the blocks' candidates of step t - 1 to the pick, the thread that owns the pick
//                              records it, every thread adds the pick's kernel column to its r and the block writes its
//                              candidate of step t to the other of two buffers.
// An item of a batch may also ask for its density: the picks of all such items are gathered by the run itself into one block,
// come down in one copy and go through the host builder (resident_from_host_points, pack_device.hip).
// The pick is the maximum of a total order (score, then original index, then leaf) and every r_j grows in step order, so
// neither depends on how the leaves are dealt to lanes, wavefronts or blocks: the two routes, the host entry, the resident
// entry and any batch give the same bits.  No atomics, no grid-wide barrier, no cooperative launch, no spinning on memory.
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

constexpr int kOneThreads = 1024;                                            // route A: the workgroup
constexpr int kOnePoints = KDEHIP_COMPRESS_ONE_BLOCK_MAX / kOneThreads;      // ... and the leaves a lane keeps
constexpr int kStepThreads = 256;                                            // route B: leaves per block
constexpr int kWave = 64;
static_assert(KDEHIP_COMPRESS_ONE_BLOCK_MAX % kOneThreads == 0 && kOnePoints >= 1 && kOnePoints <= 8, "route A keeps whole leaves per lane");

// A candidate of the argmax: the score, the original index (0-based) and the leaf.
struct Cand {
  double score;
  int32_t o, j;
};
static_assert(sizeof(Cand) == 16, "Cand layout");

__device__ __forceinline__ Cand no_cand() { return {-INFINITY, INT32_MAX, INT32_MAX}; }
// the total order: the larger score, then the lower original index (then the lower leaf: a caller's permutation may repeat)
__device__ __forceinline__ bool cand_before(const Cand &a, const Cand &b) {
  return a.score > b.score || (a.score == b.score && (a.o < b.o || (a.o == b.o && a.j < b.j)));
}
// the best candidate of the wavefront, in every lane
__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    Cand d;
    d.score = __shfl_xor(c.score, off, kWave);
    d.o = __shfl_xor(c.o, off, kWave);
    d.j = __shfl_xor(c.j, off, kWave);
    if (cand_before(d, c)) c = d;
  }
  return c;
}
// ... of the block's W wavefronts: lane 0 of each has written sCand[wave] and a barrier has passed; in every thread
template <int W>
__device__ __forceinline__ Cand block_best(const Cand *sCand) {
  Cand c = sCand[0];
#pragma unroll
  for (int w = 1; w < W; ++w) {
    const Cand d = sCand[w];
    if (cand_before(d, c)) c = d;
  }
  return c;
}

// One density.  The head has the leaves as sources AND queries (N == Nq).
struct CompressItem : PairHead {
  const double *var;     // [D] the caller's kernel variances, or null: twice bw
  const double *bw;      // [D] the first leaf's variances (not read when var is set)
  const int64_t *perm;   // [N] leaf -> original point (1-based)
  double *partial;       // [ngroups][N] the z pass's scratch
  double *z, *r;         // [N]
  uint8_t *taken;        // [N] route B: 1 once the leaf is chosen
  Cand *cand;            // [2][nb] route B: the blocks' candidates, even and odd steps
  int64_t *idx;          // [M] out: original index (1-based) of pick t
  double *zpick, *rpick; // [M] out, or null
  double *points;        // [M][D] out (D x M column-major), or null
  double *self_sum;      // [1] out
  int32_t ngroups, D, M, nb, stepwise, pad_;
};

__device__ __forceinline__ double kernel_var(const CompressItem &it, int k) { return it.var ? it.var[k] : 2.0 * it.bw[k]; }

template <int D>
__device__ __forceinline__ void load_nhib(const CompressItem &it, double (&nhib)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) nhib[k] = -0.5 / kernel_var(it, k);
}

// exp(a(s, j)): leaf j (x) as the query, the pick (s) as the source -- the expression and fma order of pair_sweep
template <int D, bool CIRC>
__device__ __forceinline__ double kernel_column(const double (&x)[D], const double (&s)[D], const double (&nhib)[D], unsigned circ,
                                                const double *sExpTab) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double d = x[k] - s[k];
    if constexpr (CIRC) {
      if ((circ >> k) & 1u) d = circ_wrap(d);
    }
    acc = fma(d * d, nhib[k], acc);
  }
  return exp_nonpos(acc, sExpTab);
}

// score_j = z_j - r_j * inv, inv = 1 / (t + 1): a product and a difference, each rounded (no fused multiply-add)
__device__ __forceinline__ double herd_score(double z, double r, double inv) {
  const double m = r * inv;
  return z - m;
}

// what the thread that owns pick t writes
__device__ __forceinline__ void record_pick(const CompressItem &it, int t, int j, double z, double r) {
  it.idx[t] = it.perm[j];
  if (it.zpick) it.zpick[t] = z;
  if (it.rpick) it.rpick[t] = r;
  if (it.points)
    for (int k = 0; k < it.D; ++k) it.points[static_cast<int64_t>(t) * it.D + k] = it.src[static_cast<int64_t>(j) * it.D + k];
}

// partial[g][j] = sum over the source chunks c of group g, in chunk order, of sum_{i in chunk c} alpha_i exp(a(i, j)): the
// sweep and the sum of eval_partial_kernel (evaluate.hip) with the caller's nhib and no leave-one-out.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void compress_z_kernel(const CompressItem *__restrict__ items,
                                                                  const int32_t *__restrict__ first, int n,
                                                                  const uint32_t *__restrict__ masks) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const ItemBlock ib = item_block(first, n);
  const CompressItem it = items[ib.item];
  const unsigned circ = circ_mask<CIRC>(masks, ib.item);
  const PairPlace at = pair_place(it, ib.k);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  double nhib[D];
  load_nhib<D>(it, nhib);
  double total = 0.0;
  pair_sweep<D, CIRC>(it, at, circ, nhib, sSrc, [&](auto &&each) {
    double sum = 0.0;
    each([&](int64_t, double w, double a) { sum += w * exp_nonpos(a, sExpTab); });
    total += sum;
  });
  if (at.q < it.Nq) it.partial[at.grp * it.Nq + at.q] = total;
}

// grid (leaf blocks of the largest item, items): z_j = the groups in group order; r_j = 0; leaf j not taken
__global__ __launch_bounds__(kEvalThreads) void compress_z_finish_kernel(const CompressItem *__restrict__ items) {
  const CompressItem it = items[blockIdx.y];
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kEvalThreads + threadIdx.x;
  if (j >= it.N) return;
  double s = 0.0;
  for (int g = 0; g < it.ngroups; ++g) s += it.partial[static_cast<int64_t>(g) * it.N + j];
  it.z[j] = s;
  it.r[j] = 0.0;
  it.taken[j] = 0;
}

// one workgroup per item: self_sum = sum_j alpha_j z_j
__global__ __launch_bounds__(kEvalThreads) void compress_self_kernel(const CompressItem *__restrict__ items) {
  __shared__ double red[kEvalThreads];
  const CompressItem it = items[blockIdx.x];
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < it.N; j += kEvalThreads) {
    const double term = it.w[j] * it.z[j];
    s += term;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  const double total = block_tree_sum<kEvalThreads>(red);
  if (threadIdx.x == 0) *it.self_sum = total;
}

// Route A.  Block b runs item b of the launch's items (one D, Euclidean or circular, N <= KDEHIP_COMPRESS_ONE_BLOCK_MAX).
// Lane l keeps leaves l, l + 1024, .. (kOnePoints of them at most).  A step: every lane's best live leaf -> the wavefront's
// (shuffles) -> sCand[wave]; barrier; every thread takes the best of the 16; the owner records the pick and puts its
// coordinates into sPick; barrier; every lane adds the pick's kernel column to its r.  Two barriers a step in every
// wavefront, whatever it holds (the owner's branch has none).
template <int D, bool CIRC>
__global__ __launch_bounds__(kOneThreads) void compress_one_kernel(const CompressItem *__restrict__ items,
                                                                   const uint32_t *__restrict__ masks) {
  __shared__ Cand sCand[kOneThreads / kWave];
  __shared__ double sPick[D];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const CompressItem it = items[blockIdx.x];
  const unsigned circ = circ_mask<CIRC>(masks, static_cast<int>(blockIdx.x));
  const int N = static_cast<int>(it.N), M = it.M;
  const int tid = static_cast<int>(threadIdx.x);
  const int np = (N + kOneThreads - 1) / kOneThreads;  // block-uniform: the rows of leaves in use
  double nhib[D];
  load_nhib<D>(it, nhib);
  double x[kOnePoints][D], z[kOnePoints], r[kOnePoints];
  int32_t o[kOnePoints];
  unsigned live = 0u;  // bit p: leaf p * 1024 + tid exists and is not chosen yet
#pragma unroll
  for (int p = 0; p < kOnePoints; ++p) {
    const int j = p * kOneThreads + tid;
    const bool have = j < N;
#pragma unroll
    for (int k = 0; k < D; ++k) x[p][k] = have ? it.src[static_cast<int64_t>(j) * D + k] : 0.0;
    z[p] = have ? it.z[j] : 0.0;
    r[p] = 0.0;
    o[p] = have ? static_cast<int32_t>(it.perm[j] - 1) : INT32_MAX;
    if (have) live |= 1u << p;
  }
  __syncthreads();  // the table
  for (int t = 0; t < M; ++t) {
    const double inv = 1.0 / static_cast<double>(t + 1);
    Cand best = no_cand();
#pragma unroll
    for (int p = 0; p < kOnePoints; ++p) {
      if (p < np && ((live >> p) & 1u)) {
        const Cand c{herd_score(z[p], r[p], inv), o[p], p * kOneThreads + tid};
        if (cand_before(c, best)) best = c;
      }
    }
    best = wave_best(best);
    if ((tid & (kWave - 1)) == 0) sCand[tid / kWave] = best;
    __syncthreads();
    const Cand pick = block_best<kOneThreads / kWave>(sCand);
    if ((pick.j & (kOneThreads - 1)) == tid) {
#pragma unroll
      for (int p = 0; p < kOnePoints; ++p) {
        if (p == pick.j / kOneThreads) {
          record_pick(it, t, pick.j, z[p], r[p]);
          live &= ~(1u << p);
#pragma unroll
          for (int k = 0; k < D; ++k) sPick[k] = x[p][k];
        }
      }
    }
    __syncthreads();
    double s[D];
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] = sPick[k];
#pragma unroll
    for (int p = 0; p < kOnePoints; ++p) {
      if (p < np) r[p] += kernel_column<D, CIRC>(x[p], s, nhib, circ, sExpTab);
    }
  }
}

// Route B, launch t = 0 .. M of one item: nb blocks, thread -> leaf j = block * 256 + thread.
//   t > 0: the blocks' candidates of step t - 1 (cand[(t - 1) & 1]) -> the pick, the same in every block; the thread that owns
//          it records it and marks its leaf; t == M ends here; every thread adds the pick's kernel column to its r;
//   t < M: the block's best not-taken leaf by the score of step t -> cand[t & 1][block].
// A launch reads one of the two buffers and writes the other; launches on one stream run in order.
template <int D, bool CIRC>
__global__ __launch_bounds__(kStepThreads) void compress_step_kernel(const CompressItem *__restrict__ item,
                                                                    const uint32_t *__restrict__ mask, int t) {
  constexpr int kWaves = kStepThreads / kWave;
  __shared__ Cand sCand[kWaves];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const CompressItem it = *item;
  const unsigned circ = circ_mask<CIRC>(mask, 0);
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kStepThreads + tid;
  const bool have = j < it.N;
  double rj = 0.0;
  bool gone = false;
  if (t > 0) {
    const Cand *prev = it.cand + static_cast<int64_t>((t - 1) & 1) * it.nb;
    Cand best = no_cand();
    for (int b = tid; b < it.nb; b += kStepThreads) {
      const Cand c = prev[b];
      if (cand_before(c, best)) best = c;
    }
    best = wave_best(best);
    if ((tid & (kWave - 1)) == 0) sCand[tid / kWave] = best;
    __syncthreads();
    const Cand pick = block_best<kWaves>(sCand);
    __syncthreads();  // (sCand is written again below)
    if (pick.j >= it.N) return;  // (uniform; never with M <= N: a leaf is left at every step)
    if (have) {
      rj = it.r[j];
      gone = it.taken[j] != 0;
      if (j == pick.j) {
        record_pick(it, t - 1, pick.j, it.z[j], rj);
        it.taken[j] = 1;
        gone = true;
      }
    }
    if (t == it.M) return;  // (uniform) the last launch only records
    if (have) {
      double x[D], s[D], nhib[D];
      load_nhib<D>(it, nhib);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        x[k] = it.src[j * D + k];
        s[k] = it.src[static_cast<int64_t>(pick.j) * D + k];
      }
      rj += kernel_column<D, CIRC>(x, s, nhib, circ, sExpTab);
      it.r[j] = rj;
    }
  }
  const double inv = 1.0 / static_cast<double>(t + 1);
  Cand mine = no_cand();
  if (have && !gone) mine = Cand{herd_score(it.z[j], rj, inv), static_cast<int32_t>(it.perm[j] - 1), static_cast<int32_t>(j)};
  mine = wave_best(mine);
  if ((tid & (kWave - 1)) == 0) sCand[tid / kWave] = mine;
  __syncthreads();
  if (tid == 0) it.cand[static_cast<int64_t>(t & 1) * it.nb + blockIdx.x] = block_best<kWaves>(sCand);
}

// The run of one call (pair_sweep.hpp PairRun).  The block: [caller's data | descriptors | first[], masks | the explicit
// variances | results | per item: self_sum, z, r, taken, candidates, the z pass's scratch].
// Protocol: add() every item -> alloc(prefix bytes, result doubles) -> point the items at their data and outputs ->
// enqueue(stream) -> wait().
class CompressRun : public PairRun<CompressItem> {
 public:
  void add(const CompressItem &it, uint32_t mask, const double *var) {
    items.push_back(it);
    circ.push_back(mask);
    var_.push_back(var);
  }
  int alloc(size_t prefix, size_t nresults) {
    const size_t n = items.size();
    int64_t blocks = 0;
    for (CompressItem &it : items) {
      blocks += split(it);
      it.nb = static_cast<int32_t>((it.N + kStepThreads - 1) / kStepThreads);
    }
    if (blocks > INT32_MAX || n > 65535) return set_error(KDEHIP_ERR_UNSUPPORTED, "compress: too large for one launch");
    Carve c;
    const size_t o_var = carve_head(c, prefix, 1, sizeof(double) * KDEHIP_MAX_DIMS * n, nresults);
    struct Off { size_t self, z, r, taken, cand, partial; };
    std::vector<Off> off(n);
    for (size_t k = 0; k < n; ++k) {
      const CompressItem &it = items[k];
      const size_t N = static_cast<size_t>(it.N);
      off[k].self = c.take(sizeof(double));
      off[k].z = c.take(sizeof(double) * N);
      off[k].r = c.take(sizeof(double) * N);
      off[k].taken = c.take(N);
      off[k].cand = c.take(sizeof(Cand) * 2 * it.nb);
      off[k].partial = c.take(sizeof(double) * N * it.ngroups);
    }
    KDEHIP_CHECK(alloc_block(c));
    for (size_t k = 0; k < n; ++k) {
      CompressItem &it = items[k];
      it.self_sum = reinterpret_cast<double *>(dev() + off[k].self);
      it.z = reinterpret_cast<double *>(dev() + off[k].z);
      it.r = reinterpret_cast<double *>(dev() + off[k].r);
      it.taken = dev() + off[k].taken;
      it.cand = reinterpret_cast<Cand *>(dev() + off[k].cand);
      it.partial = reinterpret_cast<double *>(dev() + off[k].partial);
      if (!var_[k]) continue;
      std::memcpy(host() + o_var + sizeof(double) * KDEHIP_MAX_DIMS * k, var_[k], sizeof(double) * it.D);
      it.var = reinterpret_cast<const double *>(dev() + o_var) + KDEHIP_MAX_DIMS * k;
    }
    return KDEHIP_OK;
  }
  // Descriptors sorted by (D, circular, route), one upload; the z pass (one launch per run of equal key, the finish and the
  // self sums in one launch each), then per run: ONE route-A launch for its items, or M + 1 launches for each item of route B.
  int enqueue(hipStream_t st) {
    prepare([&](size_t k) { return 4 * items[k].D + (circ[k] ? 2 : 0) + (items[k].stepwise ? 1 : 0); });
    KDEHIP_CHECK(send(st));
    const size_t n = items.size();
    int64_t maxN = 1;
    for (const CompressItem &it : items) maxN = std::max(maxN, it.N);
    KDEHIP_CHECK_RC(for_each_run([&](const CompressItem &it, const CompressItem *d_it, const int32_t *d_f, int cnt, int blocks,
                                     const uint32_t *d_m) -> int {
      KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
        constexpr int kD = decltype(dim)::value;
        launch_pair<CompressItem>(compress_z_kernel<kD, false>, compress_z_kernel<kD, true>, blocks, st, d_it, d_f, cnt, d_m);
      }));
      KDEHIP_CHECK(hipGetLastError());
      return KDEHIP_OK;
    }));
    hipLaunchKernelGGL(compress_z_finish_kernel, dim3(static_cast<unsigned>((maxN + kEvalThreads - 1) / kEvalThreads), static_cast<unsigned>(n)),
                       dim3(kEvalThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(compress_self_kernel, dim3(static_cast<unsigned>(n)), dim3(kEvalThreads), 0, st, d_items());
    KDEHIP_CHECK(hipGetLastError());
    return for_each_run([&](const CompressItem &it, const CompressItem *d_it, const int32_t *, int cnt, int, const uint32_t *d_m) -> int {
      const size_t a = static_cast<size_t>(d_it - d_items());
      if (!it.stepwise) {
        KDEHIP_CHECK_RC(dispatch_dims(it.D, [&](auto dim) {
          constexpr int kD = decltype(dim)::value;
          const auto kernel = d_m ? compress_one_kernel<kD, true> : compress_one_kernel<kD, false>;
          hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(cnt)), dim3(kOneThreads), 0, st, d_it, d_m);
        }));
        KDEHIP_CHECK(hipGetLastError());
        return KDEHIP_OK;
      }
      for (int e = 0; e < cnt; ++e) {
        const CompressItem &ie = items[a + e];
        for (int t = 0; t <= ie.M; ++t) {
          KDEHIP_CHECK_RC(dispatch_dims(ie.D, [&](auto dim) {
            constexpr int kD = decltype(dim)::value;
            const auto kernel = d_m ? compress_step_kernel<kD, true> : compress_step_kernel<kD, false>;
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(ie.nb)), dim3(kStepThreads), 0, st, d_it + e,
                               d_m ? d_m + e : nullptr, t);
          }));
          KDEHIP_CHECK(hipGetLastError());
        }
      }
      return KDEHIP_OK;
    });
  }

 private:
  std::vector<const double *> var_;  // per item: the caller's D variances (host), or null
};

// ---- arguments ------------------------------------------------------------------------------------------------------------

constexpr char kWords[] = "compress: ";
const char kNeedVariances[] = "compress: per-point bandwidths need explicit variances (twice the leaf variance is one vector)";
static_assert(sizeof(kdehip_compress_item) == 96, "kdehip_compress_item layout (_lib.CCompressItem mirrors it)");

// M, var and flags of a density of N points in D dimensions; none touches a device
int check_numbers(int64_t N, int64_t D, int64_t M, const double *var, uint32_t flags) {
  if (N > INT32_MAX) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "the density has 2^31 points or more");
  if (M < 1 || M > N) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "M must lie in 1..N");
  if (flags & ~static_cast<uint32_t>(KDEHIP_COMPRESS_STEPWISE)) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "unknown flag bits");
  for (int64_t k = 0; var && k < D; ++k)
    if (!(std::isfinite(var[k]) && var[k] > 0.0)) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "every variance must be finite and > 0");
  return KDEHIP_OK;
}

int check_resident(const kdehip_device_density *p, int64_t M, const double *var, uint32_t flags) {
  KDEHIP_CHECK_RC(check_resident_density(p, false));
  KDEHIP_CHECK_RC(check_numbers(p->N, p->D, M, var, flags));
  if (!var && !leaves_share_bandwidth(p)) return set_error(KDEHIP_ERR_UNSUPPORTED, kNeedVariances);
  return KDEHIP_OK;
}

bool stepwise(int64_t N, uint32_t flags) { return (flags & KDEHIP_COMPRESS_STEPWISE) || N > KDEHIP_COMPRESS_ONE_BLOCK_MAX; }

CompressItem resident_item(const kdehip_device_density *p, int64_t M, uint32_t flags) {
  const LeafRows l = leaf_rows(p);
  CompressItem it{};
  it.src = it.qry = l.src; it.w = l.w; it.bw = l.bw; it.perm = l.perm;
  it.N = it.Nq = p->N; it.D = p->D; it.M = static_cast<int32_t>(M); it.stepwise = stepwise(p->N, flags) ? 1 : 0;
  return it;
}

struct CompressOut { int64_t *d_idx; double *d_points, *d_zpick, *d_rpick, *d_self_sum; };

// the resident items of one call: every check has passed and the device is current
int run_resident(int n, const kdehip_device_density *const *p, const int64_t *M, const double *const *var, const uint32_t *flags,
                 const uint32_t *masks, const CompressOut *out) {
  CompressRun run;
  for (int i = 0; i < n; ++i) run.add(resident_item(p[i], M[i], flags[i]), masks[i], var[i]);
  KDEHIP_CHECK_RC(run.alloc(0, 0));
  for (int i = 0; i < n; ++i) {
    CompressItem &it = run.items[i];
    it.idx = out[i].d_idx; it.points = out[i].d_points; it.zpick = out[i].d_zpick; it.rpick = out[i].d_rpick;
    if (out[i].d_self_sum) it.self_sum = out[i].d_self_sum;
  }
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  return run.wait();
}

}  // namespace

extern "C" int kdehip_compress(const kdehip_density *p, int64_t M, const double *var, int flags_, int64_t *idx, double *zpick,
                               double *rpick, double *self_sum, int device, const uint8_t *manifold) {
  // every check that needs no device comes first
  if (!p || !idx) return set_error(KDEHIP_ERR_ARG, "null argument");
  const uint32_t flags = static_cast<uint32_t>(flags_);
  KDEHIP_CHECK_RC(check_host_density(p));
  const int D = static_cast<int>(p->ndim);
  const int64_t N = p->npts;
  KDEHIP_CHECK_RC(check_numbers(N, D, M, var, flags));
  uint32_t circ = 0;
  if (manifold_arg(manifold, D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  if (!var) KDEHIP_CHECK_RC(check_one_bandwidth(p, kNeedVariances));
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  CompressRun run;  // caller data: [means | weights | bw | the leaf row of the permutation], results: [idx | zpick | rpick | self_sum]
  CompressItem it{};
  it.N = it.Nq = N; it.D = D; it.M = static_cast<int32_t>(M); it.stepwise = stepwise(N, flags) ? 1 : 0;
  run.add(it, circ, var);
  const size_t o_perm = align256(host_density_bytes(p)), prefix = o_perm + sizeof(int64_t) * N;
  const size_t m = static_cast<size_t>(M);
  KDEHIP_CHECK_RC(run.alloc(prefix, 3 * m + 1));
  CompressItem &ri = run.items[0];
  ri.bw = pack_host_density(run, ri, p);
  ri.qry = ri.src;
  std::memcpy(run.host() + o_perm, p->permutation + N, sizeof(int64_t) * N);
  ri.perm = reinterpret_cast<const int64_t *>(run.dev() + o_perm);
  ri.idx = reinterpret_cast<int64_t *>(run.result(0));
  ri.zpick = run.result(m); ri.rpick = run.result(2 * m); ri.self_sum = run.result(3 * m);
  KDEHIP_CHECK_RC(run.enqueue(hipStreamPerThread));
  KDEHIP_CHECK_RC(run.wait());
  std::memcpy(idx, run.host_result(0), sizeof(int64_t) * m);
  if (zpick) std::memcpy(zpick, run.host_result(m), sizeof(double) * m);
  if (rpick) std::memcpy(rpick, run.host_result(2 * m), sizeof(double) * m);
  if (self_sum) *self_sum = *run.host_result(3 * m);
  return KDEHIP_OK;
}

extern "C" int kdehip_compress_device(const kdehip_device_density *p, int64_t M, const double *var, int flags_, int64_t *d_idx,
                                      double *d_points, double *d_zpick, double *d_rpick, double *d_self_sum,
                                      const uint8_t *manifold) {
  if (!p || !d_idx) return set_error(KDEHIP_ERR_ARG, "null argument");
  const uint32_t flags = static_cast<uint32_t>(flags_);
  KDEHIP_CHECK_RC(check_resident(p, M, var, flags));
  uint32_t circ = 0;
  if (manifold_arg(manifold, p->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(p->device));
  const CompressOut out{d_idx, d_points, d_zpick, d_rpick, d_self_sum};
  return run_resident(1, &p, &M, &var, &flags, &circ, &out);
}

// The items of a batch: the run, then for the items that ask for a density (out) the route of
// kdehip_density_marginal_device -- their picks gathered on the device by the run itself ([points (D M) | the first leaf's
// variances (D)] per item in ONE block), ONE copy down, the host builder with ks and weights 1 / M, the blocks back up.
extern "C" int kdehip_compress_device_batch(int n, const kdehip_compress_item *items) {
  KDEHIP_CHECK_RC(check_batch_list(n, items, "compress batch: "));
  for (int i = 0; i < n; ++i)
    if (items[i].out) *items[i].out = nullptr;
  if (n == 0) return KDEHIP_OK;
  size_t gather = 0, most = 0;  // doubles
  for (int i = 0; i < n; ++i) {
    const kdehip_compress_item &b = items[i];
    if (!b.p || (!b.d_idx && !b.out)) return set_error(KDEHIP_ERR_ARG, "null argument");
    KDEHIP_CHECK_RC(check_resident(b.p, b.M, b.var, b.flags));
    KDEHIP_CHECK_RC(check_same_device(b.p, items[0].p, "compress batch: "));
    KDEHIP_CHECK_RC(check_circular_mask(b.circular_mask, b.p->D, "compress batch: "));
    if (!b.out) continue;
    const int D = b.p->D;
    const uint8_t *tm = b.tree_manifold;
    KDEHIP_CHECK_RC(manifold_arg_or_null(tm, D, nullptr, kTreeManifold));
    for (int k = 0; b.ks && k < D; ++k)
      if (!(std::isfinite(b.ks[k]) && b.ks[k] > 0.0)) return set_error(KDEHIP_ERR_ARG, std::string(kWords) + "every ks entry must be finite and > 0");
    if (!b.ks && !leaves_share_bandwidth(b.p)) return set_error(KDEHIP_ERR_UNSUPPORTED, kOneBandwidth);
    gather += static_cast<size_t>(b.M) * (D + 1) + D;
    most = std::max(most, static_cast<size_t>(b.M));
  }
  const int device = items[0].p->device;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  const hipStream_t cs = hipStreamPerThread;
  CallBlock gathered;
  if (gather) {
    KDEHIP_CHECK(gathered.alloc(sizeof(double) * gather, sizeof(double) * gather));
    gathered.touch(cs);
  }
  double *d_blk = reinterpret_cast<double *>(gathered.dev()), *blk = reinterpret_cast<double *>(gathered.host());
  std::vector<const kdehip_device_density *> p(n);
  std::vector<int64_t> M(n);
  std::vector<const double *> var(n);
  std::vector<uint32_t> flags(n), masks(n);
  std::vector<CompressOut> out(n);
  std::vector<size_t> at(n, 0);  // an item's place in the gathered block: [points | idx (when the caller wants none) | variances]
  size_t o = 0;
  for (int i = 0; i < n; ++i) {
    const kdehip_compress_item &b = items[i];
    p[i] = b.p; M[i] = b.M; var[i] = b.var; flags[i] = b.flags; masks[i] = b.circular_mask;
    out[i] = CompressOut{b.d_idx, b.d_points, b.d_zpick, b.d_rpick, b.d_self_sum};
    if (!b.out) continue;
    const size_t m = static_cast<size_t>(b.M), D = static_cast<size_t>(b.p->D);
    at[i] = o;
    out[i].d_points = d_blk + o;
    if (!b.d_idx) out[i].d_idx = reinterpret_cast<int64_t *>(d_blk + o + m * D);
    o += m * (D + 1) + D;
  }
  KDEHIP_CHECK_RC(run_resident(n, p.data(), M.data(), var.data(), flags.data(), masks.data(), out.data()));
  if (!gather) return KDEHIP_OK;
  for (int i = 0; i < n; ++i) {
    const kdehip_compress_item &b = items[i];
    if (!b.out) continue;
    const size_t m = static_cast<size_t>(b.M), D = static_cast<size_t>(b.p->D);
    KDEHIP_CHECK(hipMemcpyAsync(d_blk + at[i] + m * (D + 1), leaf_rows(b.p).bw, sizeof(double) * D, hipMemcpyDeviceToDevice, cs));
    if (b.d_points) KDEHIP_CHECK(hipMemcpyAsync(b.d_points, d_blk + at[i], sizeof(double) * m * D, hipMemcpyDeviceToDevice, cs));
  }
  KDEHIP_CHECK(gathered.download(0, sizeof(double) * gather, cs));
  KDEHIP_CHECK(gathered.wait());
  std::vector<double> w;
  try {
    w.resize(most);
  } catch (const std::exception &) {
    return set_error(KDEHIP_ERR_ALLOC, "out of host memory");
  }
  int rc = KDEHIP_OK;
  for (int i = 0; i < n && rc == KDEHIP_OK; ++i) {
    const kdehip_compress_item &b = items[i];
    if (!b.out) continue;
    const size_t m = static_cast<size_t>(b.M);
    const int D = b.p->D;
    const double *bw = blk + at[i] + m * (D + 1);
    double sd[KDEHIP_MAX_DIMS];
    for (int k = 0; k < D; ++k) sd[k] = b.ks ? b.ks[k] : std::sqrt(bw[k]);
    std::fill(w.begin(), w.begin() + m, 1.0 / static_cast<double>(b.M));
    const uint8_t *tm = b.tree_manifold;
    (void)manifold_arg_or_null(tm, D, nullptr, kTreeManifold);  // (checked above: all zeros -> the Euclidean builder)
    rc = resident_from_host_points(b.out, device, D, b.M, blk + at[i], sd, w.data(), tm, cs);
  }
  if (rc != KDEHIP_OK)  // one bad item fails the whole call: no handle is returned
    for (int i = 0; i < n; ++i)
      if (items[i].out && *items[i].out) {
        kdehip_density_free(*items[i].out);
        *items[i].out = nullptr;
      }
  return rc;
}

// The compressed density as a resident handle: a batch of one item that asks for nothing else.
extern "C" int kdehip_density_compress_device(kdehip_device_density **out, const kdehip_device_density *p, int64_t M,
                                              const double *var, const double *ks, const uint8_t *manifold,
                                              const uint8_t *tree_manifold) {
  if (!out) return set_error(KDEHIP_ERR_ARG, "null out pointer");
  *out = nullptr;
  if (!p) return set_error(KDEHIP_ERR_ARG, "null argument");
  uint32_t circ = 0;
  if (manifold_arg(manifold, p->D, &circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  kdehip_compress_item it{};
  it.p = p; it.var = var; it.M = M; it.circular_mask = circ;
  it.out = out; it.ks = ks; it.tree_manifold = tree_manifold;
  return kdehip_compress_device_batch(1, &it);
}
