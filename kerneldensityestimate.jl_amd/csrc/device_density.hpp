// device_density.hpp -- densities that live in HBM (pack_device.hip) and what the packers share.
#pragma once

#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "kdehip_internal.hpp"

namespace kdehip {

// The frontiers of ONE density for levels 0..L (levelDown!, reference src/MSGibbs01.jl:500-523): data independent,
// so they are expanded once -- per product by the host packer, per density for densities kept on the device.
struct Frontiers {
  std::vector<int32_t> ids;      // node ids (1-based), level l at [off[l], off[l+1])
  std::vector<uint8_t> fresh;    // per id: 1 where the node enters the frontier (a leaf stays as its own child: 0 from then on)
  std::vector<int64_t> off;      // L + 2 entries
  std::vector<uint8_t> uniform;  // L + 1: every node of the frontier has the bandwidth vector of its first node
  std::vector<double> uratio;    // L + 1, uniform frontiers: max over nodes and dimensions of |mean_d| / sqrt(2 bandwidth_d)
                                 // (what the shared-bandwidth evaluator's rounding error grows with: pack_layout_shapes)
  bool bad = false;              // look = true: a mean beyond 1e100, a non-positive / non-finite variance or weight was seen
  double lo[KDEHIP_MAX_DIMS], hi[KDEHIP_MAX_DIMS];  // look = true: range of the variances per dimension
  int64_t nodes = 0;             // sum_{l >= 1} n_l
};
// `look`: also examine every node once (the conditions of the fast arithmetic form, pack_levels.cpp).
int expand_frontiers(const kdehip_density &t, int D, int L, bool look, Frontiers &out);
// The same in two steps: the ids depend on the child arrays only, the flags (shared bandwidth per level, ranges, finiteness)
// on the values -- kde!(points) of a device matrix expands the ids while the GPU still searches the bandwidth.
int expand_frontier_ids(const kdehip_density &t, int D, int L, Frontiers &out);
void examine_frontiers(const kdehip_density &t, int D, int L, bool look, Frontiers &out);

// The shape of one tile: all pack_layout needs once the frontiers are known.
struct TileShape {
  int64_t n;
  bool uniform;
  double uratio;  // Frontiers.uratio of a uniform frontier
};
// Phases 2-4 of pack_layout (tile geometry, staging modes, conditional tables) from the shapes [M][L+1] alone.
int pack_layout_shapes(int M, int D, int L, const TileShape *shapes, const uint8_t *mask, int precision, bool fast,
                       PackedProduct &out);
// whether D variances in [lo, 2*hi] keep the product/rsqrt arithmetic inside the range of the precision
bool variances_in_range(const double *bw_lo, const double *bw_hi, int D, int precision);

// One tile of a plan image as the gather kernel of pack_device.hip sees it (what pack_layout_shapes decided): where its
// frontier's nodes come from (the density's arrays in HBM) and where header, rows and permutation row go.  Absolute
// pointers: one launch fills the tiles of any number of products (kdehip_prod_philox_batch).
struct FillJob {
  const double *means, *bandwidth, *weights;
  const int64_t *perm;
  const int32_t *front;  // the frontier's node ids (1-based)
  void *hdr;             // T*: the tile header
  int32_t *perm_out;     // the tile's permutation row
  int32_t n, B, F, uniform, D, pad_;
};
static_assert(sizeof(FillJob) == 80, "FillJob layout");
int launch_fill_tiles(int precision, const FillJob *d_jobs, int ntiles, int maxB, void *stream);
// The fp32 screen tiles of an fp64 plan (kdehip_internal.hpp "fp32 screening") from its fp64 tiles, one workgroup per
// (density, level); enqueue only.
int launch_screen_build(const PlanDev &plan, void *stream);

// kdehip_density_set_bandwidth (balltree.cpp) that also reports what the packers' examination of the nodes would find
struct NodeStats { bool bad; double lo[KDEHIP_MAX_DIMS], hi[KDEHIP_MAX_DIMS]; };
// (`order`: the internal nodes, every node AFTER its descendants when read back to front -- children_first_order -- when the
// caller has worked it out already; it depends on the child arrays only)
int set_bandwidth_examined(int64_t D, int64_t N, const double *ks, int64_t nks, const double *weights, const int64_t *left_child,
                           const int64_t *right_child, const double *means, double *bandwidth, double *bandwidthMin,
                           double *bandwidthMax, NodeStats *st, const std::vector<int64_t> *order = nullptr);
int children_first_order(int64_t N, const int64_t *left_child, const int64_t *right_child, std::vector<int64_t> &order);

}  // namespace kdehip

namespace kdehip {
// The densities a batched call builds (kdehip_mul_device_batch) live in ONE device block and ONE pinned mirror -- one
// allocation, two uploads for the whole batch instead of three small transfers per density --, released when the last of
// them is freed.
struct SharedBlock {
  std::atomic<int> refs{0};
  void *d_blob = nullptr;
  size_t blob_bytes = 0;
  void *mirror = nullptr;
  size_t mirror_bytes = 0;
};

// What a refit (include/kdehip.h section 5r, refit.hip) needs of a density's topology, made from the child arrays by the
// first refit of a handle and shared by that density and every refit of it: ONE device block
// [node ids | left child | right child] (int32 each) of the internal nodes, sorted by height -- a node of height h has
// its children at heights below h, the leaves at height 0.
struct RefitTable {
  int device = 0;
  void *d_tab = nullptr;
  size_t bytes = 0;
  int64_t nI = 0;             // internal nodes (N - 1; 1 for a single-point density)
  std::vector<int64_t> hoff;  // height h = 1 .. H: the nodes [hoff[h - 1], hoff[h])
  ~RefitTable();              // (refit.hip: the block goes back to the cache)
};
}  // namespace kdehip

// A BallTreeDensity resident on one device (include/kdehip.h "densities in HBM").
struct kdehip_device_density {
  int device = 0;
  int64_t N = 0;
  int D = 0;
  int Lown = 0;               // levels of its own tree: floor(log(N)/log 2 + 1); deeper frontiers repeat the last one (all leaves)
  kdehip::Frontiers fr;       // sizes, offsets and flags (the ids themselves live on the device: `front`)
  void *d_blob = nullptr;     // the one device allocation; the pointers below point into it
  size_t blob_bytes = 0;
  const double *means = nullptr, *bandwidth = nullptr, *weights = nullptr;
  const int64_t *perm = nullptr;
  const int32_t *front = nullptr;
  // A density the library built itself (kdehip_density_from_device_points) keeps the reference's twelve arrays as a
  // host mirror for kdehip_density_download, in ONE pinned block from the library's cache (a fresh 1 MB heap block per
  // density is an mmap of its own: 250 page faults to fill it and -- in a process with a live HIP runtime, whose driver
  // hooks every unmap -- a munmap of ~2 ms to drop it: the "host tree alone 2.1 ms" of profiles/r04p): the head of the
  // block IS the image of the device block ([means | bandwidth | weights | permutation | frontier ids], uploaded
  // straight from here), the other eight arrays follow
  bool built = false;
  void *mirror = nullptr;
  size_t mirror_bytes = 0;
  struct Mirror {
    double *centers = nullptr, *ranges = nullptr, *means = nullptr, *bandwidth = nullptr, *bwmin = nullptr, *bwmax = nullptr,
           *weights = nullptr;
    int64_t *left = nullptr, *right = nullptr, *lowest = nullptr, *highest = nullptr, *perm = nullptr;
  } m;
  double bw[KDEHIP_MAX_DIMS] = {};  // its LOOCV bandwidth (standard deviations)
  kdehip::SharedBlock *shared = nullptr;  // set: d_blob / mirror above are null, the arrays live in the batch's blocks
  // The table sample.hip draws from, built by the first sample call (include/kdehip.h section 2f): ONE device block of its
  // own -- also for a density in a shared batch block -- [C (fp64, original order) | inverse permutation (int32: original
  // index -> leaf) | status].  `cdf_ready` is published (release) once the build has completed on the device.
  std::mutex cdf_mu;
  std::atomic<bool> cdf_ready{false};
  int cdf_rc = 0;         // KDEHIP_OK, or KDEHIP_ERR_ARG for weights / a permutation the table cannot be built from
  void *d_cdf = nullptr;
  size_t cdf_bytes = 0;
  // Refits (section 5r): a density the caller uploaded keeps its child arrays (slots 1..N as int32: [left | right]) -- a
  // built one has them in its mirror --, and the table made from them by the first refit.
  std::vector<int32_t> kids;
  mutable std::mutex refit_mu;
  mutable std::shared_ptr<kdehip::RefitTable> refit;
};

namespace kdehip {
// (evaluate.hip) whether every leaf of a resident density has its first leaf's variances: the one bandwidth vector the
// direct evaluation reads
bool leaves_share_bandwidth(const kdehip_device_density *h);
// kdehip_prod_philox_device with everything -- preparation and sampling -- on ONE stream (product.hip): what a blocking
// caller that waits for the product anyway uses (kdehip_mul_device).
int prod_philox_device_blocking_stream(int Ndens, kdehip_device_density *const *trees, int64_t Np, int Niter, uint64_t seed,
                                       int64_t sample_offset, int addEntropy, const uint8_t *partialDimMask, int precision,
                                       double *d_points, int64_t *d_indices, void *stream, const uint8_t *manifold = nullptr);
// (pack_device.hip) a resident density from HOST data by the host builder -- pts D x N column-major, ks D standard deviations,
// N weights, tree_manifold or NULL --, uploaded on `stream` of `device`, which is current: the tail of the marginal, the
// conditional and the compressed density
int resident_from_host_points(kdehip_device_density **out, int device, int D, int64_t N, const double *pts, const double *ks,
                              const double *weights, const uint8_t *tree_manifold, hipStream_t stream);
// kdehip_prod_philox_batch with a manifold per item (product.hip; manifolds or any of its entries may be NULL)
int prod_philox_batch_manifold(int nprod, const kdehip_batch_item *items, const uint8_t *const *manifolds, int precision,
                               void *stream);
}  // namespace kdehip
