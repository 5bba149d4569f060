// evaltol.hip -- evaluation within a tolerance on gfx950 (include/kdehip.h section 5m).
//
// The counterpart of the reference's setForceEvalDirect!(false) (src/DualTree01.jl:248-299: stop descending a pair of balls
// once their boxes show it cannot move the result by errTol), on the layout the direct sweep already has: the leaves are in
// tree order, so every kEvalChunk-leaf chunk the sweep stages is a compact ball of the tree.  Three passes, fp64, no atomics,
// no read-back between them:
//   chunk_box_kernel<D>             per chunk: the box of its leaves and the sum of their weights, in leaf order;
//   tol_plan_kernel<D, CIRC>        one lane per query: a lower bound L_q of the query's unnormalised sum (the boxes' far
//                                   corners, and the nearest chunk summed exactly), tau_q from it, and one flag per (query
//                                   block, chunk): some live lane of the block needs the chunk;
//   eval_tol_partial_kernel<D, CIRC> the direct sweep of pair_sweep.hpp restricted to the block's flagged chunks: the same
//                                   grid, group split, chunk order and arithmetic per pair, so with every flag up it writes
//                                   the direct kernel's bits.
// Only non-negative terms are left out: the result is a truncation from below, never above the direct value.
#include <hip/hip_runtime.h>

#include <cmath>

#include "circ_wrap.hpp"
#include "entry_helpers.hpp"
#include "evaltol.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"
#include "pair_sweep.hpp"

using namespace kdehip;

namespace {

constexpr int kWave = 64;                         // lanes per wavefront (gfx950)
constexpr int kBlockWaves = kEvalThreads / kWave;
constexpr int kBoxTile = 128;                     // chunk boxes per LDS tile of the plan pass: two flag words
constexpr double kLogTauMargin = 0x1p-20;         // log tau_q is lowered by this much (section 5m "rounding")
constexpr double kCircFar = 3.141592653589793 * (1.0 + 0x1p-20);  // dmax of a circular dimension: pi and the wrap's rounding

// what the kernels read: the sweep's head first (pair_place), then the rest of TolPass with the scratch carved
struct TolParams : PairHead {
  const double *bw;
  double *partial;
  double *boxes;     // [nchunks][2 D + 1]: lo[D], hi[D], W
  uint64_t *flags;   // [qblocks][nwords]: bit c % 64 of word c / 64 = the tile (query block, chunk c) is visited
  int32_t *counts;   // [qblocks] visited tiles of the query block
  int64_t *stats;
  int64_t nchunks, qblocks, nwords;
  double norm0, rel_tol, abs_tol;
  int32_t loo;
  uint32_t circ;
};

// One block per chunk, one thread per leaf: the leaves go to LDS, then thread k < D takes lo and hi of dimension k and
// thread D the weight sum, each over the chunk's leaves in leaf order.
template <int D>
__global__ __launch_bounds__(kEvalChunk) void chunk_box_kernel(TolParams p) {
  __shared__ double s[kEvalChunk * (D + 1)];
  const int64_t c = blockIdx.x, i0 = c * kEvalChunk;
  const int cnt = static_cast<int>((p.N - i0 < kEvalChunk) ? (p.N - i0) : kEvalChunk);
  const int t = threadIdx.x;
  if (t < cnt) {
#pragma unroll
    for (int k = 0; k < D; ++k) s[t * (D + 1) + k] = p.src[(i0 + t) * D + k];
    s[t * (D + 1) + D] = p.w[i0 + t];
  }
  __syncthreads();
  double *box = p.boxes + c * (2 * D + 1);
  if (t < D) {
    double lo = s[t], hi = s[t];
    for (int i = 1; i < cnt; ++i) {
      const double v = s[i * (D + 1) + t];
      lo = (v < lo) ? v : lo;
      hi = (v > hi) ? v : hi;
    }
    box[t] = lo;
    box[D + t] = hi;
  } else if (t == D) {
    double W = 0.0;
    for (int i = 0; i < cnt; ++i) W += s[i * (D + 1) + D];
    box[2 * D] = W;
  }
}

// a_min and a_max of (x, box): the sweep's own chain -- fma(d * d, nhib[k], acc), k ascending -- on the nearest and the
// farthest difference.  Every operation of the chain is monotone and correctly rounded, so for a leaf i of the box the
// exponent the sweep computes lies between the two VALUES computed here, not only between the exact ones.
template <int D, bool CIRC>
__device__ __forceinline__ void box_bounds(const double (&x)[D], const double *__restrict__ box, unsigned circ,
                                           const double (&nhib)[D], double &amin, double &amax) {
  amin = 0.0;
  amax = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double below = box[k] - x[k], above = x[k] - box[D + k];  // lo - x, x - hi
    double dmin = fmax(0.0, fmax(below, above));
    double dmax = fmax(fabs(below), fabs(above));
    if constexpr (CIRC) {
      if ((circ >> k) & 1u) { dmin = 0.0; dmax = kCircFar; }
    }
    amin = fma(dmin * dmin, nhib[k], amin);
    amax = fma(dmax * dmax, nhib[k], amax);
  }
}

// The plan of one query block (block b of the grid): see the head of the file and section 5m steps 2-4.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void tol_plan_kernel(TolParams p) {
  constexpr int kBox = 2 * D + 1;
  __shared__ double sBox[kBoxTile * kBox];
  __shared__ double sExpTab[32];
  __shared__ int sNeed[kBlockWaves][kBoxTile];
  __shared__ int sCnt[2];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const int64_t qb = blockIdx.x, q = qb * kEvalThreads + threadIdx.x;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const unsigned circ = CIRC ? p.circ : 0u;
  double x[D], nhib[D];
  bool live = q < p.Nq;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[k] = (q < p.Nq) ? p.qry[q * D + k] : 0.0;
    live = live && (x[k] == x[k]);
    nhib[k] = -0.5 / p.bw[k];
  }
  auto stage = [&](int64_t c0, int cnt) {
    for (int t = threadIdx.x; t < cnt * kBox; t += kEvalThreads) sBox[t] = p.boxes[c0 * kBox + t];
  };
  const int64_t own = p.loo ? q / kEvalChunk : -1;  // leave-one-out: the chunk of the query's own leaf

  // pass one: the nearest chunk (largest a_min, the lowest such c) and the first bound, sum_c W_c exp(a_max) without the
  // own chunk
  double best = -INFINITY, far_sum = 0.0;
  int64_t cstar = 0;
  for (int64_t c0 = 0; c0 < p.nchunks; c0 += kBoxTile) {
    const int cnt = static_cast<int>((p.nchunks - c0 < kBoxTile) ? (p.nchunks - c0) : kBoxTile);
    __syncthreads();  // the tile before this one has been read
    stage(c0, cnt);
    __syncthreads();
    for (int ci = 0; ci < cnt; ++ci) {
      double amin, amax;
      box_bounds<D, CIRC>(x, sBox + ci * kBox, circ, nhib, amin, amax);
      if (amin > best) { best = amin; cstar = c0 + ci; }
      if (c0 + ci != own) far_sum += sBox[ci * kBox + 2 * D] * exp_nonpos(amax, sExpTab);
    }
  }
  // the second bound: the nearest chunk summed exactly, as the sweep sums it (without the own leaf)
  double near_sum = 0.0;
  if (live) {
    const int64_t i0 = cstar * kEvalChunk;
    const int cnt = static_cast<int>((p.N - i0 < kEvalChunk) ? (p.N - i0) : kEvalChunk);
    for (int i = 0; i < cnt; ++i) {
      const double *s = p.src + (i0 + i) * D;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double d = x[k] - s[k];
        if constexpr (CIRC) {
          if ((circ >> k) & 1u) d = circ_wrap(d);
        }
        acc = fma(d * d, nhib[k], acc);
      }
      double v = p.w[i0 + i] * exp_nonpos(acc, sExpTab);
      if (p.loo && i0 + i == q) v = 0.0;
      near_sum += v;
    }
  }
  const double norm = gauss_norm(p.norm0, D, [&](int k) { return p.bw[k]; });
  const double tau = fmax(p.rel_tol * fmax(far_sum, near_sum), p.abs_tol * norm);
  const bool all = !(tau > 0.0);  // tau_q == 0: every chunk is needed
  const double log_tau = all ? -INFINITY : log(tau) - kLogTauMargin;

  // pass two: the flags.  Per chunk a ballot per wavefront, the four wavefronts OR-ed through LDS, 64 flags to a word.
  int visited = 0;  // (lane 0 of wavefronts 0 and 1: their words)
  for (int64_t c0 = 0; c0 < p.nchunks; c0 += kBoxTile) {
    const int cnt = static_cast<int>((p.nchunks - c0 < kBoxTile) ? (p.nchunks - c0) : kBoxTile);
    __syncthreads();  // the tile before this one, and its sNeed, have been read
    stage(c0, cnt);
    __syncthreads();
    for (int ci = 0; ci < cnt; ++ci) {
      double amin, amax;
      box_bounds<D, CIRC>(x, sBox + ci * kBox, circ, nhib, amin, amax);
      const bool need = live && (all || amin > log_tau);
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
__global__ void tol_stats_kernel(TolParams p) {
  int64_t visited = 0;
  for (int64_t b = 0; b < p.qblocks; ++b) visited += p.counts[b];
  p.stats[0] = visited;
  p.stats[1] = p.qblocks * p.nchunks;
}

// partial[g][q] = the sum over the FLAGGED chunks c of group g, in chunk order, of the chunk's sum as eval_partial_kernel
// forms it (evaluate.hip): the same place in the item (pair_place), the same staging and pair arithmetic as pair_sweep, with
// the two-buffer ring prefetching the next flagged chunk.  The flags of the block's row are block-uniform words read with
// uniform loads: no vote and no further barrier in the loop.  A group with no flagged chunk writes 0.
template <int D, bool CIRC>
__global__ __launch_bounds__(kEvalThreads) void eval_tol_partial_kernel(TolParams p) {
  __shared__ double sSrc[2][kEvalChunk * (D + 1)];
  __shared__ double sExpTab[32];
  if (threadIdx.x < 32) sExpTab[threadIdx.x] = kExp2Tab[threadIdx.x];
  const int64_t kb = blockIdx.x;
  const PairPlace at = pair_place(p, kb);
  if (at.c_begin >= at.c_end) return;  // block-uniform
  const unsigned circ = CIRC ? p.circ : 0u;
  const uint64_t *__restrict__ row = p.flags + (kb % p.qblocks) * p.nwords;
  const int64_t c_end = at.c_end;
  auto next = [&](int64_t c) {  // the first flagged chunk at or after c, or c_end
    while (c < c_end && !((row[c >> 6] >> (c & 63)) & 1ull)) ++c;
    return c;
  };
  const double *const src = p.src, *const w = p.w;
  const int64_t N = p.N;
  double x[D], nhib[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[k] = (at.q < p.Nq) ? p.qry[at.q * D + k] : 0.0;
    nhib[k] = -0.5 / p.bw[k];
  }
  auto stage = [&](int64_t c, int buf) {
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
    for (int t = threadIdx.x; t < cnt * (D + 1); t += kEvalThreads) {
      const int i = t / (D + 1), f = t % (D + 1);
      sSrc[buf][t] = (f < D) ? src[(i0 + i) * D + f] : w[i0 + i];
    }
  };
  double total = 0.0;
  int64_t c = next(at.c_begin);
  if (c < c_end) stage(c, 0);
  int buf = 0;
  while (c < c_end) {
    __syncthreads();  // chunk c is staged; the other buffer is free again
    const int64_t cn = next(c + 1);
    if (cn < c_end) stage(cn, buf ^ 1);
    const int64_t i0 = c * kEvalChunk;
    const int cnt = static_cast<int>((N - i0 < kEvalChunk) ? (N - i0) : kEvalChunk);
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
      double v = s[D] * exp_nonpos(acc, sExpTab);
      if (p.loo && i0 + i == at.q) v = 0.0;
      sum += v;
    }
    total += sum;
    c = cn;
    buf ^= 1;
  }
  if (at.q < p.Nq) p.partial[at.grp * p.Nq + at.q] = total;
}

struct TolSizes { int64_t nchunks, qblocks, nwords; size_t o_flags, o_counts, bytes; };
TolSizes tol_sizes(int64_t N, int64_t Nq, int D) {
  TolSizes s;
  s.nchunks = (N + kEvalChunk - 1) / kEvalChunk;
  s.qblocks = (Nq + kEvalThreads - 1) / kEvalThreads;
  s.nwords = (s.nchunks + kWave - 1) / kWave;
  s.o_flags = sizeof(double) * static_cast<size_t>(s.nchunks) * (2 * D + 1);
  s.o_counts = s.o_flags + sizeof(uint64_t) * static_cast<size_t>(s.qblocks) * s.nwords;
  s.bytes = s.o_counts + ((sizeof(int32_t) * static_cast<size_t>(s.qblocks) + 7) & ~size_t(7));
  return s;
}

}  // namespace

size_t kdehip::tol_scratch_bytes(int64_t N, int64_t Nq, int D) { return tol_sizes(N, Nq, D).bytes; }

int kdehip::enqueue_tol_passes(const TolPass &t, hipStream_t st, hipEvent_t *marks) {
  const TolSizes s = tol_sizes(t.N, t.Nq, t.D);
  if (t.Nq < 1 || t.N < 1) return KDEHIP_OK;
  if (s.nchunks > INT32_MAX || s.qblocks * t.ngroups > INT32_MAX)
    return set_error(KDEHIP_ERR_UNSUPPORTED, "evaluation too large for one launch");
  TolParams p{};
  p.src = t.src; p.w = t.w; p.qry = t.qry;
  p.N = t.N; p.Nq = t.Nq; p.chunks_per_group = t.chunks_per_group;
  p.bw = t.bw;
  p.partial = t.partial;
  p.boxes = reinterpret_cast<double *>(t.scratch);
  p.flags = reinterpret_cast<uint64_t *>(t.scratch + s.o_flags);
  p.counts = reinterpret_cast<int32_t *>(t.scratch + s.o_counts);
  p.stats = t.stats;
  p.nchunks = s.nchunks; p.qblocks = s.qblocks; p.nwords = s.nwords;
  p.norm0 = t.norm0; p.rel_tol = t.rel_tol; p.abs_tol = t.abs_tol;
  p.loo = t.loo;
  p.circ = t.circ;
  const unsigned nchunks = static_cast<unsigned>(s.nchunks), qblocks = static_cast<unsigned>(s.qblocks);
  const unsigned sweep = static_cast<unsigned>(s.qblocks * t.ngroups);
  auto mark = [&](int k) { if (marks) (void)hipEventRecord(marks[k], st); };
  KDEHIP_CHECK_RC(dispatch_dims(t.D, [&](auto dim) {
    constexpr int kD = decltype(dim)::value;
    mark(0);
    hipLaunchKernelGGL(chunk_box_kernel<kD>, dim3(nchunks), dim3(kEvalChunk), 0, st, p);
    mark(1);
    if (t.circ) hipLaunchKernelGGL((tol_plan_kernel<kD, true>), dim3(qblocks), dim3(kEvalThreads), 0, st, p);
    else hipLaunchKernelGGL((tol_plan_kernel<kD, false>), dim3(qblocks), dim3(kEvalThreads), 0, st, p);
    mark(2);
    if (t.circ) hipLaunchKernelGGL((eval_tol_partial_kernel<kD, true>), dim3(sweep), dim3(kEvalThreads), 0, st, p);
    else hipLaunchKernelGGL((eval_tol_partial_kernel<kD, false>), dim3(sweep), dim3(kEvalThreads), 0, st, p);
    mark(3);
  }));
  if (t.stats) hipLaunchKernelGGL(tol_stats_kernel, dim3(1), dim3(1), 0, st, p);
  KDEHIP_CHECK(hipGetLastError());
  return KDEHIP_OK;
}
