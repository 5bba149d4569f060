// knn.hip -- k nearest neighbours on the ball tree's leaf order, gfx950 (include/kdehip.h section 5n).
//
// The skeleton of evaltol.hip with another per-lane state: the leaves are in tree order, so every kEvalChunk-leaf chunk is
// a compact box; a plan pass flags the (256-query block, chunk) tiles that can hold one of a query's k nearest leaves, and a
// sweep walks the flagged chunks only.  Three passes, fp64, no atomics, no read-back between them:
//   knn_box_kernel<D>                per chunk: the box of its leaves (chunk_box_kernel of evaltol.hip without the weights);
//   knn_plan_kernel<D, CIRC, KCAP>   one lane per query: the nearest chunk c*, its k best leaves (r_q = the k-th smallest
//                                    distance within it), and one flag per (query block, chunk): some live lane has
//                                    dmin2(q, c) <= r_q;
//   knn_sweep_kernel<D, CIRC, KCAP>  one block per query block: the flagged chunks through a two-buffer LDS ring, every lane
//                                    keeping its k best (d2, original index) in registers, sorted, starting from the
//                                    plan's list of c* -- so the threshold is r_q from the first chunk on, and a chunk
//                                    walk that approaches the query (tree order) does not insert at every step.
// The distance is the sweep's own chain, fma(d * d, s_k, acc) with s_k > 0: monotone in |d| and correctly rounded, so the
// nearest corner of a box bounds the COMPUTED distance of every leaf inside it and nothing that is skipped could have
// entered a list.  The result is the brute-force one, bit for bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "call_block.hpp"
#include "circ_wrap.hpp"
#include "device_density.hpp"
#include "entry_helpers.hpp"
#include "kdehip_internal.hpp"
#include "knn.hpp"
#include "manifold_arg.hpp"
#include "pair_sweep.hpp"
#include "phase_timer.hpp"

using namespace kdehip;

namespace {

constexpr int kWave = 64;                         // lanes per wavefront (gfx950)
constexpr int kBlockWaves = kEvalThreads / kWave;
constexpr int kBoxTile = 128;                     // chunk boxes per LDS tile of the plan pass: two flag words

struct KnnParams {
  const double *src;
  const int64_t *src_index;
  const double *qry;
  const int64_t *qry_index;
  double *boxes;     // [nchunks][2 D]: lo[D], hi[D]
  uint64_t *flags;   // [qblocks][nwords]: bit c % 64 of word c / 64 = the tile (query block, chunk c) is visited
  int32_t *counts;   // [qblocks] visited tiles of the query block
  double *seed_d2;   // [k][Nq] the plan's list of every query (its k best within c*), rank-major: what the sweep starts from
  int32_t *seed_id;  // [k][Nq]
  int32_t *cstar;    // [Nq] the chunk that list was taken from (-1: none), which the sweep leaves alone for that query
  int64_t *stats;
  double *d2_out;
  int64_t *idx_out;
  int64_t N, Nq, nchunks, qblocks, nwords;
  double scale[KDEHIP_MAX_DIMS];
  int32_t k, loo;
  uint32_t circ;
};

// The k best candidates of one lane by the key (d2, original index), ascending, in registers: every index below is a
// compile-time constant once the loops are unrolled.  A list of capacity KCAP serves any k <= KCAP: its first KCAP - k
// entries are (-Inf, -1), which no candidate (d2 >= 0) displaces, so the LAST entry is the k-th best candidate so far.
template <int KCAP>
struct KnnList {
  double d[KCAP];
  int32_t id[KCAP];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
      const bool dead = j < KCAP - k;
      d[j] = dead ? -INFINITY : INFINITY;
      id[j] = dead ? -1 : INT32_MAX;
    }
  }
  __device__ __forceinline__ double last() const { return d[KCAP - 1]; }
  // rank r (0 = best) sits in entry KCAP - k + r: the k ranks to and from [k][stride] arrays at column q
  __device__ __forceinline__ void store_ranks(int k, double *sd, int32_t *si, int64_t stride, int64_t q) const {
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
      const int r = j - (KCAP - k);
      if (r >= 0) { sd[r * stride + q] = d[j]; si[r * stride + q] = id[j]; }
    }
  }
  __device__ __forceinline__ void load_ranks(int k, const double *sd, const int32_t *si, int64_t stride, int64_t q) {
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
      const int r = j - (KCAP - k);
      if (r >= 0) { d[j] = sd[r * stride + q]; id[j] = si[r * stride + q]; }
    }
  }
  __device__ __forceinline__ bool beats_last(double nd, int32_t ni) const {
    return nd < d[KCAP - 1] || (nd == d[KCAP - 1] && ni < id[KCAP - 1]);
  }
  // (nd, ni) beats the last entry: it takes its place and moves up by compare-exchanges
  __device__ __forceinline__ void insert(double nd, int32_t ni) {
    d[KCAP - 1] = nd;
    id[KCAP - 1] = ni;
#pragma unroll
    for (int j = KCAP - 1; j > 0; --j) {
      const bool up = d[j] < d[j - 1] || (d[j] == d[j - 1] && id[j] < id[j - 1]);
      const double dl = up ? d[j] : d[j - 1], dh = up ? d[j - 1] : d[j];
      const int32_t il = up ? id[j] : id[j - 1], ih = up ? id[j - 1] : id[j];
      d[j - 1] = dl; d[j] = dh;
      id[j - 1] = il; id[j] = ih;
    }
  }
};

// One block per chunk, one thread per leaf: the leaves go to LDS, then thread j < D takes lo and hi of dimension j over the
// chunk's leaves in leaf order.
template <int D>
__global__ __launch_bounds__(kEvalChunk) void knn_box_kernel(KnnParams p) {
  __shared__ double s[kEvalChunk * D];
  const int64_t c = blockIdx.x, i0 = c * kEvalChunk;
  const int cnt = static_cast<int>((p.N - i0 < kEvalChunk) ? (p.N - i0) : kEvalChunk);
  const int t = threadIdx.x;
  if (t < cnt) {
#pragma unroll
    for (int j = 0; j < D; ++j) s[t * D + j] = p.src[(i0 + t) * D + j];
  }
  __syncthreads();
  if (t < D) {
    double lo = s[t], hi = s[t];
    for (int i = 1; i < cnt; ++i) {
      const double v = s[i * D + t];
      lo = (v < lo) ? v : lo;
      hi = (v > hi) ? v : hi;
    }
    p.boxes[c * (2 * D) + t] = lo;
    p.boxes[c * (2 * D) + D + t] = hi;
  }
}

// d2 of (x, the nearest corner of the box): the distance's chain on dmin_j = max(0, lo_j - x_j, x_j - hi_j), 0 in a
// circular dimension
template <int D, bool CIRC>
__device__ __forceinline__ double box_dmin2(const double (&x)[D], const double *__restrict__ box, unsigned circ,
                                            const double (&sc)[D]) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double dmin = fmax(0.0, fmax(box[j] - x[j], x[j] - box[D + j]));
    if constexpr (CIRC) {
      if ((circ >> j) & 1u) dmin = 0.0;
    }
    acc = fma(dmin * dmin, sc[j], acc);
  }
  return acc;
}

// d2 of (x, the leaf at s)
template <int D, bool CIRC>
__device__ __forceinline__ double leaf_d2(const double (&x)[D], const double *__restrict__ s, unsigned circ,
                                          const double (&sc)[D]) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double d = x[j] - s[j];
    if constexpr (CIRC) {
      if ((circ >> j) & 1u) d = circ_wrap(d);
    }
    acc = fma(d * d, sc[j], acc);
  }
  return acc;
}

// The `cnt` leaves at src ([cnt][D]; their original indices at idx) offered to the lane's list, in leaf order; leaf `skip` of
// them (or none: -1) is left out.  kScanBatch distances are formed before any is compared: the loads of a batch are in flight
// together, where a loop that may branch into an insertion after every leaf would wait for each one's latency in turn.  The
// slots past the last leaf re-read it and offer (+Inf, INT32_MAX), which beats no entry.
constexpr int kScanBatch = 8;
template <int D, bool CIRC, int KCAP, typename Index>
__device__ __forceinline__ void scan_leaves(KnnList<KCAP> &list, const double (&x)[D], const double (&sc)[D], unsigned circ,
                                            const double *__restrict__ src, const Index *__restrict__ idx, int cnt, int skip) {
  for (int i = 0; i < cnt; i += kScanBatch) {
    double dd[kScanBatch];
    int32_t ii[kScanBatch];
#pragma unroll
    for (int u = 0; u < kScanBatch; ++u) {
      const bool out = i + u >= cnt || i + u == skip;
      const int iu = (i + u < cnt) ? i + u : cnt - 1;
      const double d2 = leaf_d2<D, CIRC>(x, src + iu * D, circ, sc);
      const int32_t id = static_cast<int32_t>(idx[iu]);
      dd[u] = out ? INFINITY : d2;
      ii[u] = out ? INT32_MAX : id;
    }
    // the slots that beat the list as it stands, lowest first; ONE insertion site (a slot is picked by a chain of selects
    // over static indices), and a slot is asked again once earlier ones have tightened the list
    unsigned cand = 0;
#pragma unroll
    for (int u = 0; u < kScanBatch; ++u) cand |= list.beats_last(dd[u], ii[u]) ? 1u << u : 0u;
    while (cand) {
      const int pick = __builtin_ctz(cand);
      cand &= cand - 1;
      double nd = dd[0];
      int32_t ni = ii[0];
#pragma unroll
      for (int u = 1; u < kScanBatch; ++u) {
        nd = (pick == u) ? dd[u] : nd;
        ni = (pick == u) ? ii[u] : ni;
      }
      if (list.beats_last(nd, ni)) list.insert(nd, ni);
    }
  }
}

// the lane's query: its coordinates (0 beyond Nq) and whether it is live -- q < Nq and every coordinate finite
template <int D>
__device__ __forceinline__ bool load_query(const KnnParams &p, int64_t q, double (&x)[D], double (&sc)[D]) {
  bool live = q < p.Nq;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    x[j] = (q < p.Nq) ? p.qry[q * D + j] : 0.0;
    live = live && (fabs(x[j]) < INFINITY);  // (false for a NaN)
    sc[j] = p.scale[j];
  }
  return live;
}

// The plan of one query block (block b of the grid): section 5n steps 2-5.
template <int D, bool CIRC, int KCAP>
__global__ __launch_bounds__(kEvalThreads) void knn_plan_kernel(KnnParams p) {
  constexpr int kBox = 2 * D;
  __shared__ double sBox[kBoxTile * kBox];
  __shared__ int sNeed[kBlockWaves][kBoxTile];
  __shared__ int sCnt[2];
  const int64_t qb = blockIdx.x, q = qb * kEvalThreads + threadIdx.x;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const unsigned circ = CIRC ? p.circ : 0u;
  double x[D], sc[D];
  const bool live = load_query<D>(p, q, x, sc);
  auto stage = [&](int64_t c0, int cnt) {
    for (int t = threadIdx.x; t < cnt * kBox; t += kEvalThreads) sBox[t] = p.boxes[c0 * kBox + t];
  };
  // leave-one-out: the query's own chunk does not count when it holds no other leaf (the 1-leaf last chunk)
  const int64_t alone = (p.loo && q == p.N - 1 && (p.N - 1) % kEvalChunk == 0) ? q / kEvalChunk : -1;

  // pass one: the nearest chunk (smallest dmin2, the lowest such c)
  double best = INFINITY;
  int64_t cstar = -1;
  for (int64_t c0 = 0; c0 < p.nchunks; c0 += kBoxTile) {
    const int cnt = static_cast<int>((p.nchunks - c0 < kBoxTile) ? (p.nchunks - c0) : kBoxTile);
    __syncthreads();  // the tile before this one has been read
    stage(c0, cnt);
    __syncthreads();
    for (int ci = 0; ci < cnt; ++ci) {
      const double dm = box_dmin2<D, CIRC>(x, sBox + ci * kBox, circ, sc);
      if (c0 + ci != alone && (cstar < 0 || dm < best)) { best = dm; cstar = c0 + ci; }
    }
  }
  // r_q: the k-th smallest distance among the eligible leaves of c*, +Inf if there are fewer than k
  double rq = INFINITY;
  KnnList<KCAP> list;
  list.init(p.k);
  if (live && cstar >= 0) {
    const int64_t i0 = cstar * kEvalChunk;
    const int cnt = static_cast<int>((p.N - i0 < kEvalChunk) ? (p.N - i0) : kEvalChunk);
    const int own = (p.loo && q >= i0 && q < i0 + cnt) ? static_cast<int>(q - i0) : -1;
    scan_leaves<D, CIRC>(list, x, sc, circ, p.src + i0 * D, p.src_index + i0, cnt, own);
    rq = list.last();
  }
  if (q < p.Nq) {  // the sweep starts from this list and leaves c* alone
    list.store_ranks(p.k, p.seed_d2, p.seed_id, p.Nq, q);
    p.cstar[q] = (live && cstar >= 0) ? static_cast<int32_t>(cstar) : -1;
  }

  // pass two: the flags.  Per chunk a ballot per wavefront, the four wavefronts OR-ed through LDS, 64 flags to a word.
  int visited = 0;  // (lane 0 of wavefronts 0 and 1: their words)
  for (int64_t c0 = 0; c0 < p.nchunks; c0 += kBoxTile) {
    const int cnt = static_cast<int>((p.nchunks - c0 < kBoxTile) ? (p.nchunks - c0) : kBoxTile);
    __syncthreads();  // the tile before this one, and its sNeed, have been read
    stage(c0, cnt);
    __syncthreads();
    for (int ci = 0; ci < cnt; ++ci) {
      const double dm = box_dmin2<D, CIRC>(x, sBox + ci * kBox, circ, sc);
      const bool need = live && dm <= rq;  // (non-strict: a tie may win on index)
      const unsigned long long votes = __ballot(need);
      if (lane == 0) sNeed[wave][ci] = votes != 0ull;
    }
    __syncthreads();
    int f = 0;
    if (static_cast<int>(threadIdx.x) < cnt) {
#pragma unroll
      for (int v = 0; v < kBlockWaves; ++v) f |= sNeed[v][threadIdx.x];
    }
    const unsigned long long word = __ballot(f != 0);  // wavefront v < 2: the chunks c0 + 64 v .. c0 + 64 v + 63
    const int64_t wi = c0 / kWave + wave;
    if (lane == 0 && wave < kBoxTile / kWave && wi < p.nwords) {
      p.flags[qb * p.nwords + wi] = word;
      visited += __popcll(word);
    }
  }
  if (lane == 0 && wave < 2) sCnt[wave] = visited;
  __syncthreads();
  if (threadIdx.x == 0) p.counts[qb] = sCnt[0] + sCnt[1];
}

// one thread: the query blocks' counts in block order
__global__ void knn_stats_kernel(KnnParams p) {
  int64_t visited = 0;
  for (int64_t b = 0; b < p.qblocks; ++b) visited += p.counts[b];
  p.stats[0] = visited;
  p.stats[1] = p.qblocks * p.nchunks;
}

// One block per query block: its flagged chunks in chunk order, the two-buffer ring prefetching the next flagged chunk as
// eval_tol_partial_kernel does (the flags of the block's row are block-uniform words: no vote and no further barrier in the
// loop).  A staged chunk carries its leaves' original indices and its box beside the coordinates.  A lane leaves a staged chunk alone
// when the chunk's nearest corner lies beyond its current k-th candidate.
template <int D, bool CIRC, int KCAP>
__global__ __launch_bounds__(kEvalThreads) void knn_sweep_kernel(KnnParams p) {
  __shared__ double sSrc[2][kEvalChunk * D];
  __shared__ int32_t sIdx[2][kEvalChunk];
  __shared__ double sBox[2][2 * D];
  const int64_t qb = blockIdx.x, q = qb * kEvalThreads + threadIdx.x;
  const unsigned circ = CIRC ? p.circ : 0u;
  const uint64_t *__restrict__ row = p.flags + qb * p.nwords;
  const int64_t c_end = p.nchunks, N = p.N;
  // the first flagged chunk at or after c, or c_end: a word at a time (a block walks ALL the chunks here, mostly unflagged
  // ones; the bits past the last chunk are 0)
  auto next = [&](int64_t c) {
    while (c < c_end) {
      const uint64_t w = row[c >> 6] >> (c & 63);
      if (w) return c + __builtin_ctzll(w);
      c = (c | 63) + 1;
    }
    return c_end;
  };
  double x[D], sc[D];
  const bool live = load_query<D>(p, q, x, sc);
  // A chunk on its way to LDS: this thread's share of its coordinates, indices and box.  fetch() issues the loads, put()
  // stores them -- with the scan of the chunk before in between, so one block per CU does not wait for global memory at
  // every chunk.
  constexpr int kPer = (kEvalChunk * D + kEvalThreads - 1) / kEvalThreads;
  struct Fetch { double v[kPer]; double box; int32_t id; };
  const int tid = threadIdx.x;
  auto fetch = [&](int64_t c, Fetch &f) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int t = tid + u * kEvalThreads;
      f.v[u] = (t < cnt * D) ? p.src[i0 * D + t] : 0.0;
    }
    f.id = (tid < cnt) ? static_cast<int32_t>(p.src_index[i0 + tid]) : 0;
    f.box = (tid < 2 * D) ? p.boxes[c * (2 * D) + tid] : 0.0;
  };
  auto put = [&](const Fetch &f, int buf) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int t = tid + u * kEvalThreads;
      if (t < kEvalChunk * D) sSrc[buf][t] = f.v[u];
    }
    if (tid < kEvalChunk) sIdx[buf][tid] = f.id;
    if (tid < 2 * D) sBox[buf][tid] = f.box;
  };
  KnnList<KCAP> list;  // the plan's list of the nearest chunk: the threshold is r_q from the first chunk on
  list.init(p.k);
  int64_t mine = -1;
  if (q < p.Nq) {
    list.load_ranks(p.k, p.seed_d2, p.seed_id, p.Nq, q);
    mine = p.cstar[q];
  }
  Fetch f;
  int64_t c = next(0);
  if (c < c_end) {
    fetch(c, f);
    put(f, 0);
  }
  int buf = 0;
  while (c < c_end) {
    __syncthreads();  // chunk c is staged; the other buffer is free again
    const int64_t cn = next(c + 1);
    if (cn < c_end) fetch(cn, f);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    const double dm = box_dmin2<D, CIRC>(x, sBox[buf], circ, sc);
    if (live && c != mine && dm <= list.last()) {
      const int own = (p.loo && q >= i0 && q < i0 + cnt) ? static_cast<int>(q - i0) : -1;
      scan_leaves<D, CIRC>(list, x, sc, circ, sSrc[buf], sIdx[buf], cnt, own);
    }
    if (cn < c_end) put(f, buf ^ 1);
    c = cn;
    buf ^= 1;
  }
  if (q < p.Nq) {
    const int64_t col = p.qry_index ? p.qry_index[q] - 1 : q;
    double *od = p.d2_out + col * p.k;
    int64_t *oi = p.idx_out + col * p.k;
    const int skip = KCAP - p.k;
#pragma unroll
    for (int j = 0; j < KCAP; ++j) {
      if (j >= skip) {
        od[j - skip] = live ? list.d[j] : __builtin_nan("");
        oi[j - skip] = live ? static_cast<int64_t>(list.id[j]) : 0;
      }
    }
  }
}

struct KnnSizes { int64_t nchunks, qblocks, nwords; size_t o_flags, o_counts, o_seed_d2, o_seed_id, o_cstar, bytes; };
inline size_t pad8(size_t x) { return (x + 7) & ~size_t(7); }
KnnSizes knn_sizes(int64_t N, int64_t Nq, int D, int k) {
  KnnSizes s;
  s.nchunks = (N + kEvalChunk - 1) / kEvalChunk;
  s.qblocks = (Nq + kEvalThreads - 1) / kEvalThreads;
  s.nwords = (s.nchunks + kWave - 1) / kWave;
  s.o_flags = sizeof(double) * static_cast<size_t>(s.nchunks) * (2 * D);
  s.o_counts = s.o_flags + sizeof(uint64_t) * static_cast<size_t>(s.qblocks) * s.nwords;
  s.o_seed_d2 = s.o_counts + pad8(sizeof(int32_t) * static_cast<size_t>(s.qblocks));
  s.o_seed_id = s.o_seed_d2 + sizeof(double) * static_cast<size_t>(Nq) * k;
  s.o_cstar = s.o_seed_id + pad8(sizeof(int32_t) * static_cast<size_t>(Nq) * k);
  s.bytes = s.o_cstar + pad8(sizeof(int32_t) * static_cast<size_t>(Nq));
  return s;
}

// the plan and the sweep of one capacity; `mark`: the event between them, if any
template <int D, int KCAP, typename Mark>
void launch_plan_sweep(const KnnParams &p, unsigned qblocks, hipStream_t st, Mark &&mark) {
  if (p.circ) hipLaunchKernelGGL((knn_plan_kernel<D, true, KCAP>), dim3(qblocks), dim3(kEvalThreads), 0, st, p);
  else hipLaunchKernelGGL((knn_plan_kernel<D, false, KCAP>), dim3(qblocks), dim3(kEvalThreads), 0, st, p);
  mark(2);
  if (p.circ) hipLaunchKernelGGL((knn_sweep_kernel<D, true, KCAP>), dim3(qblocks), dim3(kEvalThreads), 0, st, p);
  else hipLaunchKernelGGL((knn_sweep_kernel<D, false, KCAP>), dim3(qblocks), dim3(kEvalThreads), 0, st, p);
}

}  // namespace

size_t kdehip::knn_scratch_bytes(int64_t N, int64_t Nq, int D, int k) { return knn_sizes(N, Nq, D, k).bytes; }

int kdehip::enqueue_knn_passes(const KnnPass &t, hipStream_t st, hipEvent_t *marks) {
  const KnnSizes s = knn_sizes(t.N, t.Nq, t.D, t.k);
  if (t.Nq < 1 || t.N < 1) return KDEHIP_OK;
  // (the lists hold original indices in 32 bits)
  if (t.N >= INT32_MAX || s.qblocks > INT32_MAX) return set_error(KDEHIP_ERR_UNSUPPORTED, "knn: search too large for one launch");
  KnnParams p{};
  p.src = t.src; p.src_index = t.src_index; p.qry = t.qry; p.qry_index = t.qry_index;
  p.boxes = reinterpret_cast<double *>(t.scratch);
  p.flags = reinterpret_cast<uint64_t *>(t.scratch + s.o_flags);
  p.counts = reinterpret_cast<int32_t *>(t.scratch + s.o_counts);
  p.seed_d2 = reinterpret_cast<double *>(t.scratch + s.o_seed_d2);
  p.seed_id = reinterpret_cast<int32_t *>(t.scratch + s.o_seed_id);
  p.cstar = reinterpret_cast<int32_t *>(t.scratch + s.o_cstar);
  p.stats = t.stats;
  p.d2_out = t.d2_out; p.idx_out = t.idx_out;
  p.N = t.N; p.Nq = t.Nq; p.nchunks = s.nchunks; p.qblocks = s.qblocks; p.nwords = s.nwords;
  for (int j = 0; j < KDEHIP_MAX_DIMS; ++j) p.scale[j] = t.scale[j];
  p.k = t.k; p.loo = t.loo;
  p.circ = t.circ;
  const unsigned nchunks = static_cast<unsigned>(s.nchunks), qblocks = static_cast<unsigned>(s.qblocks);
  auto mark = [&](int k) { if (marks) (void)hipEventRecord(marks[k], st); };
  KDEHIP_CHECK_RC(dispatch_dims(t.D, [&](auto dim) {
    constexpr int kD = decltype(dim)::value;
    mark(0);
    hipLaunchKernelGGL(knn_box_kernel<kD>, dim3(nchunks), dim3(kEvalChunk), 0, st, p);
    mark(1);
    // the smallest instantiated capacity >= k
    if (t.k <= 1) launch_plan_sweep<kD, 1>(p, qblocks, st, mark);
    else if (t.k <= 8) launch_plan_sweep<kD, 8>(p, qblocks, st, mark);
    else launch_plan_sweep<kD, KDEHIP_KNN_MAX_K>(p, qblocks, st, mark);
    mark(3);
  }));
  if (t.stats) hipLaunchKernelGGL(knn_stats_kernel, dim3(1), dim3(1), 0, st, p);
  KDEHIP_CHECK(hipGetLastError());
  return KDEHIP_OK;
}

namespace {

// what both entries check of k, scale and manifold before any device is touched; fills the pass's k, scale and circ
int read_knn_args(int D, int64_t N, int k, bool loo, const double *scale, const uint8_t *manifold, KnnPass *t) {
  if (D < 1 || D > KDEHIP_MAX_DIMS) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
  if (k < 1 || k > KDEHIP_KNN_MAX_K) return set_error(KDEHIP_ERR_ARG, "knn: k must lie in 1..KDEHIP_KNN_MAX_K");
  if (k > (loo ? N - 1 : N)) return set_error(KDEHIP_ERR_ARG, "knn: k exceeds the density's points (less one for leave-one-out)");
  for (int j = 0; j < KDEHIP_MAX_DIMS; ++j) t->scale[j] = 1.0;
  for (int j = 0; scale && j < D; ++j) {
    if (!(scale[j] > 0.0 && scale[j] < INFINITY)) return set_error(KDEHIP_ERR_ARG, "knn: every scale must be finite and > 0");
    t->scale[j] = scale[j];
  }
  if (manifold_arg(manifold, D, &t->circ) != KDEHIP_OK) return KDEHIP_ERR_ARG;
  t->D = D; t->N = N; t->k = k; t->loo = loo ? 1 : 0;
  return KDEHIP_OK;
}

}  // namespace

extern "C" int kdehip_knn(const kdehip_density *bd, const double *pos, int64_t Nq, int k, int leave_one_out, const double *scale,
                          double *d2_out, int64_t *idx_out, int64_t *stats, int device, const uint8_t *manifold) {
  if (!bd || !d2_out || !idx_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  const int64_t N = bd->npts;
  KnnPass t{};
  KDEHIP_CHECK_RC(read_knn_args(static_cast<int>(bd->ndim > KDEHIP_MAX_DIMS ? KDEHIP_MAX_DIMS + 1 : bd->ndim), N, k,
                                leave_one_out != 0, scale, manifold, &t));
  const int D = t.D;
  if (N < 1 || !bd->means || !bd->permutation) return set_error(KDEHIP_ERR_ARG, "malformed density");
  if (leave_one_out) Nq = N;
  else if (!pos || Nq < 0) return set_error(KDEHIP_ERR_ARG, "pos must hold Nq >= 0 points");
  if (stats) stats[0] = stats[1] = 0;
  if (Nq == 0) return KDEHIP_OK;
  for (int64_t i = 0; i < N; ++i)  // (the sweep writes through it)
    if (bd->permutation[N + i] < 1 || bd->permutation[N + i] > N) return set_error(KDEHIP_ERR_ARG, "malformed density");
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(device));
  hipStream_t st = hipStreamPerThread;  // the calling thread's own stream, like every blocking entry point (kdehip.h)
  // ONE device block [leaf centres | leaf indices | queries || d2 | idx | stats || scratch] and a pinned image of it up to
  // the scratch: what precedes the results goes up in one copy, the results come back in one.
  Carve c;
  const size_t o_src = c.take(sizeof(double) * N * D);
  const size_t o_idx = c.take(sizeof(int64_t) * N);
  const size_t o_qry = c.take(leave_one_out ? 0 : sizeof(double) * Nq * D);
  const size_t o_res = c.mark();
  const size_t res_bytes = (sizeof(double) + sizeof(int64_t)) * static_cast<size_t>(Nq) * k + sizeof(int64_t) * 2;
  c.take(res_bytes);
  const size_t o_scratch = c.mark();
  c.take(knn_scratch_bytes(N, Nq, D, k));
  CallBlock blk;
  KDEHIP_CHECK(blk.alloc(c.mark(), o_scratch));
  unsigned char *h = blk.host(), *d = blk.dev();
  std::memcpy(h + o_src, bd->means + N * D, sizeof(double) * N * D);  // (leaf centres == the points, leaf order)
  std::memcpy(h + o_idx, bd->permutation + N, sizeof(int64_t) * N);
  if (!leave_one_out) std::memcpy(h + o_qry, pos, sizeof(double) * Nq * D);
  t.src = reinterpret_cast<const double *>(d + o_src);
  t.src_index = reinterpret_cast<const int64_t *>(d + o_idx);
  t.qry = leave_one_out ? t.src : reinterpret_cast<const double *>(d + o_qry);
  t.qry_index = leave_one_out ? t.src_index : nullptr;  // leave-one-out: output in original point order
  t.Nq = Nq;
  t.d2_out = reinterpret_cast<double *>(d + o_res);
  t.idx_out = reinterpret_cast<int64_t *>(t.d2_out + Nq * k);
  t.stats = t.idx_out + Nq * k;
  t.scratch = d + o_scratch;
  KDEHIP_CHECK(blk.upload(o_res, st));
  PassMarks marks(kPhaseKnnBox, true);  // kdehip_profile_phase_read 6..8
  KDEHIP_CHECK_RC(enqueue_knn_passes(t, st, marks.events()));
  KDEHIP_CHECK(blk.download(o_res, res_bytes, st));
  KDEHIP_CHECK(blk.wait());
  marks.collect();
  std::memcpy(d2_out, h + o_res, sizeof(double) * Nq * k);
  std::memcpy(idx_out, h + o_res + sizeof(double) * Nq * k, sizeof(int64_t) * Nq * k);
  if (stats) std::memcpy(stats, h + o_res + (sizeof(double) + sizeof(int64_t)) * Nq * k, sizeof(int64_t) * 2);
  return KDEHIP_OK;
}

extern "C" int kdehip_knn_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, int k, const double *scale,
                                    double *d_d2_out, int64_t *d_idx_out, int64_t *d_stats, void *stream,
                                    const uint8_t *manifold) {
  if (!bd || !at || !d_d2_out || !d_idx_out) return set_error(KDEHIP_ERR_ARG, "null argument");
  KnnPass t{};
  KDEHIP_CHECK_RC(read_knn_args(bd->D, bd->N, k, at == bd, scale, manifold, &t));
  if (at->D != bd->D) return set_error(KDEHIP_ERR_DIM_MISMATCH, "knn -- dimensions of two BallTreeDensities must match");
  if (at->device != bd->device) return set_error(KDEHIP_ERR_ARG, "densities on different devices");
  const int64_t N = bd->N, Nq = at->N;
  const int D = bd->D;
  if (Nq < 1) return KDEHIP_OK;
  DeviceGuard guard;
  KDEHIP_CHECK_RC(guard.enter(bd->device));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  CaptureScope scope(st);  // (a captured call's block is kept until kdehip_clear_cache: section 5h)
  CallBlock blk;
  KDEHIP_CHECK(blk.alloc(knn_scratch_bytes(N, Nq, D, k)));
  t.src = bd->means + N * D;
  t.src_index = bd->perm + N;
  t.qry = at->means + Nq * D;
  t.qry_index = at->perm + Nq;
  t.Nq = Nq;
  t.d2_out = d_d2_out; t.idx_out = d_idx_out; t.stats = d_stats;
  t.scratch = blk.dev();
  blk.touch(st);
  KDEHIP_CHECK_RC(enqueue_knn_passes(t, st));
  if (scope.capturing()) return blk.keep(bd->device);
  reap_deferred(bd->device);
  return blk.defer(bd->device);
}
