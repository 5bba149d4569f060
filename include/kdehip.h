/*
 * kdehip.h -- C ABI of libkdehip.so: the MI355X (gfx950) implementation of the multiscale-Gibbs
 * KDE product hot path of JuliaRobotics/KernelDensityEstimate.jl.
 *
 * The reference is pure Julia and has no FFI layer; the seam this library replaces is the Julia
 * method `gibbs1` (reference src/MSGibbs01.jl:527-629), called only from `prodAppxMSGibbsS`
 * (src/MSGibbs01.jl:645-703).  A Julia caller binds these entry points with `ccall`
 * (see INTEGRATION.md); the Python mirror in kerneldensityestimate.jl_amd/ binds them with ctypes.
 *
 * Conventions: plain pointers and sizes only.  All matrices are column-major as in Julia
 * (points: ndims x Np, indices: Ndens x Np).  Node ids inside a density are the reference's
 * 1-based ids with NO_CHILD = -1 (src/BallTree01.jl:5).  Every function returning `int` returns
 * KDEHIP_OK (0) or a negative error code; kdehip_last_error() gives the message (thread-local).
 * The library never keeps a caller's host pointer after a call returns.
 * There is no CPU fallback: without a usable HIP device every compute entry point fails with
 * KDEHIP_ERR_NO_DEVICE.
 */
#ifndef KDEHIP_H
#define KDEHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDEHIP_VERSION 600 /* 0.6.0 */

enum {
  KDEHIP_OK = 0,
  KDEHIP_ERR_ARG = -1,         /* invalid argument (message says which)                            */
  KDEHIP_ERR_DIM_MISMATCH = -2,/* "kdes must have same dimension"  (src/MSGibbs01.jl:720-722)     */
  KDEHIP_ERR_RAND_SHORT = -3,  /* randU / randN shorter than the run consumes (Julia BoundsError) */
  KDEHIP_ERR_NO_DEVICE = -4,   /* no HIP device / HIP runtime failure at init                      */
  KDEHIP_ERR_HIP = -5,         /* a HIP call failed                                                */
  KDEHIP_ERR_ALLOC = -6,
  KDEHIP_ERR_UNSUPPORTED = -7  /* e.g. ndims or Ndens above the compiled limits                    */
};

#define KDEHIP_MAX_DIMS 8    /* kernels are instantiated for ndims = 1..8                          */
#define KDEHIP_MAX_DENS 16   /* densities per product                                              */

/* The six flat arrays of a BallTreeDensity that gibbs1 reads through its accessors
 * (reference src/BallTreeDensity01.jl:11-24,86-93; src/BallTree01.jl:10-28,78-94).
 * Lengths: means/bandwidth = ndim*2*npts (node i, dim k at (i-1)*ndim + k-1; bandwidth holds
 * VARIANCES, src/KDE01.jl:45); the others = 2*npts. */
typedef struct kdehip_density {
  int64_t npts;               /* bt.num_points */
  int64_t ndim;               /* bt.dims       */
  const double *means;
  const double *bandwidth;
  const double *weights;      /* bt.weights      */
  const int64_t *left_child;  /* bt.left_child   */
  const int64_t *right_child; /* bt.right_child  */
  const int64_t *permutation; /* bt.permutation  */
} kdehip_density;

/* ---- library ---------------------------------------------------------------------------------- */
int kdehip_version(void);
const char *kdehip_last_error(void);
int kdehip_device_count(void); /* 0 when no device is usable */
/* The library keeps freed device / pinned-host blocks (up to 1 GiB per device) for the next call instead of
 * returning them to the driver: a one-shot product would otherwise spend most of its time in hipMalloc/hipFree.
 * This hands everything back (no reference counterpart: Julia's GC owns the reference's scratch). */
void kdehip_clear_cache(void);

/* ---- (1) drop-in for gibbs1 (reference src/MSGibbs01.jl:527-537) ------------------------------
 * Host buffers in, host buffers out, blocking.  The blocking entry points of this header are thread-safe and enqueue
 * their work on the calling thread's own stream (hipStreamPerThread): calls of concurrent host threads overlap on the
 * device instead of queueing behind each other on the null stream.  Arguments in the reference's order:
 *   Ndens, trees, Np, Niter, pts (out, ndims*Np), ind (out, Ndens*Np, = permutation+1, :615),
 *   randU (nU values), randN (nN values), then the keywords addEntropy, ndims, partialDimMask
 *   (Ndens*ndims bytes, density-major, 1 = active; NULL = all active).  `device` = HIP ordinal.
 * RNG consumption is the reference's: 0-based sample s, select call c reads randU[s*K + c - 1],
 * normal q*ndims+d of sample s is randN[s*R + q*ndims + d] (K, R from kdehip_product_info).
 * Only the Euclidean manifold operators (the reference defaults addop=+, diffop=-, getEuclidMu,
 * getEuclidLambda) exist behind this ABI. */
int kdehip_gibbs1(int Ndens, const kdehip_density *trees, int64_t Np, int Niter, double *pts,
                  int64_t *ind, const double *randU, int64_t nU, const double *randN, int64_t nN,
                  int addEntropy, int ndims, const uint8_t *partialDimMask, int device);

/* gibbs1 called with glbs.recordChoosen = true (reference src/MSGibbs01.jl:29-31, :109-112, :426, :575-583):
 * additionally returns the label trace labels[(s*Ndens + j)*nlevels + (l-1)] = bt.permutation[ind_j] as it
 * stands after the last sampleIndex of level l = 1..nlevels (what labelsChoosen[s+1][j+1][l] ends up holding;
 * with Niter = 0 the reference records nothing and the buffer is left as it was).  nlevels =
 * floor(log(max_j Npts_j)/log 2 + 1) (:568).  labels == NULL makes this kdehip_gibbs1. */
int kdehip_gibbs1_trace(int Ndens, const kdehip_density *trees, int64_t Np, int Niter, double *pts,
                        int64_t *ind, const double *randU, int64_t nU, const double *randN, int64_t nN,
                        int addEntropy, int ndims, const uint8_t *partialDimMask, int device,
                        int32_t *labels);

/* The same on `ngpus` GPUs of one node (devices device .. device+ngpus-1), one process: the chains are split into
 * contiguous ranges (sample s of the call depends only on the densities and on its own slices randU[s*K ..],
 * randN[s*R ..], so the result is identical for every ngpus), each device gets the packed densities and its slice
 * of the streams, and returns its slice of pts / ind (/ labels, as kdehip_gibbs1_trace; may be NULL) to the host.
 * ngpus = 1 is kdehip_gibbs1_trace. */
int kdehip_gibbs1_multi(int Ndens, const kdehip_density *trees, int64_t Np, int Niter, double *pts,
                        int64_t *ind, const double *randU, int64_t nU, const double *randN, int64_t nN,
                        int addEntropy, int ndims, const uint8_t *partialDimMask, int device, int ngpus,
                        int32_t *labels);

/* ---- manifolds: the operator tuples addop / diffop / getMu / getLambda as an ENUM ------------------------------------
 * The reference takes its on-manifold operators as per-dimension Julia FUNCTIONS (src/MSGibbs01.jl:650-653, broadcast at
 * :672-675) and applies them at three hook points: diffop inside every kernel evaluation (:290), getLambda / getMu in the
 * Gaussian product (:183-184, applied :210-213), addop where a sample is composed with its noise (:456).  Functions
 * cannot cross a C ABI, and the reference itself defines only the Euclidean set (its callers bring the others): this
 * entry takes, per dimension, KDEHIP_MANIFOLD_EUCLIDEAN (the reference's defaults) or KDEHIP_MANIFOLD_CIRCULAR with THIS
 * library's stated semantic -- nothing in the reference pins it:
 *     wrap(t)        = t - 2 pi floor((t + pi) / (2 pi))            in [-pi, pi)
 *     diffop(a, b)   = wrap(a - b)         addop(a, b) = wrap(a + b)         getLambda(lambdas) = sum(lambdas)
 *     getMu(mus, lambdas, scale) = addop(ref, scale * sum_j lambdas_j diffop(mus_j, ref)),  ref = mus of the first j with
 *                      lambdas_j > 0   (the information-weighted mean in the tangent space at ref; the Euclidean formula
 *                      whenever no difference wraps)
 * The densities are the caller's arrays as built (the reference's tree construction has hooks of its own,
 * src/BallTree01.jl:315: kdehip_make_density_tree, section 4, for callers who build here).  Runs the general sampler's generic arithmetic (the
 * reference's divide + log accumulation); caller streams in the reference's order, as kdehip_gibbs1_trace.  manifold == NULL
 * = all Euclidean = kdehip_gibbs1_trace.  oracle/kde_oracle.c okde_gibbs1_manifold is the same enum on the CPU; the Julia
 * shim maps NOTHING to it automatically (a caller's circular functions need not be these). */
#define KDEHIP_MANIFOLD_EUCLIDEAN 0
#define KDEHIP_MANIFOLD_CIRCULAR 1
int kdehip_gibbs1_manifold(int Ndens, const kdehip_density *trees, int64_t Np, int Niter, double *pts, int64_t *ind,
                           const double *randU, int64_t nU, const double *randN, int64_t nN, int addEntropy, int ndims,
                           const uint8_t *partialDimMask, const uint8_t *manifold /* ndims bytes or NULL */, int device,
                           int32_t *labels /* optional */);

/* prodAppxMSGibbsS when the caller passes no randU / randN (reference src/MSGibbs01.jl:645-703; its
 * `rand(...)` / `randn(...)` defaults, :661-662, are replaced by the on-device Philox4x32-10 stream keyed by
 * (seed, sample index, draw index): kdehip_philox_fill_* reproduce the numbers).  One-shot: pack, upload, run,
 * copy back.  precision 64 or 32; ngpus and labels as in kdehip_gibbs1_multi. */
int kdehip_prod_philox(int Ndens, const kdehip_density *trees, int64_t Np, int Niter, double *pts, int64_t *ind,
                       uint64_t seed, int addEntropy, int ndims, const uint8_t *partialDimMask, int precision,
                       int device, int ngpus, int32_t *labels);

/* ---- (2) resident product plan ----------------------------------------------------------------
 * The densities are re-laid-out once (per-level tiles, "pack_levels") and kept in HBM so repeated
 * products -- and bench.py's timed region -- start with inputs resident on the device.  The first run
 * of a plan additionally fills its conditional tables (tens of microseconds) and synchronises its
 * stream once; later runs only enqueue work.  A plan may be used from several threads/streams. */
typedef struct kdehip_product kdehip_product;

typedef struct kdehip_product_info_t {
  int32_t ndens, ndims, nlevels;     /* nlevels = floor(log(max Npts)/log 2 + 1), :568            */
  int32_t precision;                 /* 64 or 32                                                   */
  int64_t nodes_per_sweep;           /* sum_j sum_{l=1..L} n_{j,l}: kernel evals of one sweep      */
  int64_t bytes_per_eval;            /* (2*ndims+1)*sizeof(T)                           */
  int64_t packed_bytes;              /* device bytes held by the plan                              */
  int32_t fast_math_path;            /* 1: product/rsqrt forms; 0: the reference's divide+log form  */
  int32_t device;
} kdehip_product_info_t;

/* precision: 64 (reference arithmetic) or 32.  mask as in kdehip_gibbs1. */
int kdehip_product_create(kdehip_product **out, int Ndens, const kdehip_density *trees, int ndims,
                          const uint8_t *partialDimMask, int precision, int device);
/* The same on a manifold (`manifold`: ndims bytes of KDEHIP_MANIFOLD_EUCLIDEAN / KDEHIP_MANIFOLD_CIRCULAR or NULL, the
 * operators of "manifolds" above): a resident plan whose runs apply the circular operators.  The plan chooses its arithmetic
 * as kdehip_prod_philox_device_manifold (2c) does: the sampler's circular fast mode when the node values qualify for the fast
 * forms, the generic arithmetic of kdehip_gibbs1_manifold otherwise; no conditional tables and no fp32 screens in either.
 * CONTRACT: kdehip_product_sample_philox(seed, sample_offset) on such a plan returns, bit for bit, what
 * kdehip_prod_philox_device_manifold returns for the same densities, mask, manifold, seed and offset.  Every entry that takes
 * a plan works on a circular one: kdehip_product_sample_streams (caller streams, d_labels), kdehip_product_info
 * (fast_math_path as it is), kdehip_product_kernel_name ("gibbs_product_kernel"), kdehip_product_screen_stats (0 levels),
 * kdehip_product_set_variant, kdehip_product_launch_geometry, kdehip_product_fallback_count.
 *   - manifold == NULL or all zeros IS kdehip_product_create, bit for bit (it forwards here with NULL);
 *   - a manifold byte above 1 is KDEHIP_ERR_ARG, ndims above KDEHIP_MAX_DIMS KDEHIP_ERR_UNSUPPORTED, a circular dimension with
 *     precision 32 KDEHIP_ERR_UNSUPPORTED -- all checked before any device is touched. */
int kdehip_product_create_manifold(kdehip_product **out, int Ndens, const kdehip_density *trees, int ndims,
                                   const uint8_t *partialDimMask, const uint8_t *manifold /* ndims bytes or NULL */,
                                   int precision, int device);
/* kdehip_prod_philox on a manifold: the one-shot form of such a plan (pack, upload, run with sample offset 0, copy back), on
 * one or several GPUs -- bit for bit the plan's result, so the same for every ngpus (chains in contiguous ranges, Philox
 * keyed by the global sample index).  Unlike kdehip_gibbs1_manifold it runs the circular fast mode where the plan would: its
 * labels are that entry's on the host twin of the Philox streams, its points agree to rounding (1e-12).  manifold == NULL or
 * all zeros IS kdehip_prod_philox; errors as above. */
int kdehip_prod_philox_manifold(int Ndens, const kdehip_density *trees, int64_t Np, int Niter, double *pts, int64_t *ind,
                                uint64_t seed, int addEntropy, int ndims, const uint8_t *partialDimMask,
                                const uint8_t *manifold /* ndims bytes or NULL */, int precision, int device, int ngpus,
                                int32_t *labels);
/* (waits for the device first if runs were enqueued through the device-pointer entry points below) */
void kdehip_product_destroy(kdehip_product *plan);
int kdehip_product_info(const kdehip_product *plan, kdehip_product_info_t *info);
/* Per-sample RNG consumption for a given Niter: K uniforms (first M slots never read), R normals. */
int64_t kdehip_product_randu_per_sample(const kdehip_product *plan, int Niter);
int64_t kdehip_product_randn_per_sample(const kdehip_product *plan);

/* Run Np chains.  All pointers are DEVICE pointers on the plan's device; `stream` is a hipStream_t
 * (NULL = default stream); the call only enqueues work.  d_points: double[ndims*Np];
 * d_indices: int64[Ndens*Np]; d_labels: optional int32[Np*Ndens*nlevels] (permutation of the label
 * kept at the end of every level, the recordChoosen trace of src/MSGibbs01.jl:109-112) or NULL. */
int kdehip_product_sample_streams(kdehip_product *plan, int64_t Np, int Niter,
                                  const double *d_randU, int64_t nU, const double *d_randN,
                                  int64_t nN, int addEntropy, double *d_points, int64_t *d_indices,
                                  int32_t *d_labels, void *stream);
/* Same, random numbers from the on-device Philox4x32-10 stream keyed by (seed, global sample
 * index = sample_offset + s, draw index): results do not depend on how samples are split over
 * calls or GPUs. */
int kdehip_product_sample_philox(kdehip_product *plan, int64_t Np, int Niter, uint64_t seed,
                                 int64_t sample_offset, int addEntropy, double *d_points,
                                 int64_t *d_indices, int32_t *d_labels, void *stream);
/* Host-buffer convenience wrapper around the Philox run (allocates, runs, copies back, blocking). */
int kdehip_product_sample_philox_host(kdehip_product *plan, int64_t Np, int Niter, uint64_t seed,
                                      int64_t sample_offset, int addEntropy, double *points,
                                      int64_t *indices, int32_t *labels);
/* Diagnostic: how many label draws of this plan's runs so far took the reference's underflow branch
 * (`pT < 1e-99` -> uniform draw over the frontier, src/MSGibbs01.jl:311-315).  Waits for the device.
 * Negative = error code. */
int64_t kdehip_product_fallback_count(kdehip_product *plan);
/* Diagnostic: fp32 screening of the deep levels (fp64 plans of 2..4 or 8 densities with every dimension active): on a
 * level whose fp64 tiles are streamed or chunked through LDS, the plan also holds the level's tiles in fp32 -- resident in
 * LDS together, streamed one per step, or in chunks, whichever fits; up to 128 entries per lane --; a draw step evaluates
 * the frontier in packed fp32 with a rigorous bound on the error of its cumulative
 * sums and keeps the fp32 decision only when the uniform draw is farther than that bound from every boundary it could
 * cross -- otherwise the step is repeated in fp64.  Labels and points are those of the fp64 arithmetic bit for bit
 * (csrc/screen_device.hpp).  levels: how many levels of the plan are screened; steps / repeats: label draws
 * taken on screened levels so far, and how many of them were repeated in fp64.  Waits for the device.  Any pointer may be
 * NULL. */
int kdehip_product_screen_stats(kdehip_product *plan, int32_t *levels, int64_t *steps, int64_t *repeats);
/* Scheduling knob for experiments/benchmarks; results never depend on it.  0 = library default,
 * 1 = read every tile from global memory (no LDS staging), 4 = no conditional tables, 5 = no fp32 screening,
 * 2 / 8 / 16 = 4 / 8 / 16 chains per workgroup (one wavefront per chain).  Default: chosen from the number of chains. */
int kdehip_product_set_variant(kdehip_product *plan, int variant);
/* Diagnostic: the launch geometry a run of Np chains of this plan gets under its current variant -- wavefronts per
 * workgroup and wavefronts per chain (always 1 since round 5: a chain is one wavefront). */
int kdehip_product_launch_geometry(const kdehip_product *plan, int64_t Np, int32_t *waves_per_workgroup,
                                   int32_t *waves_per_chain);
/* Diagnostic: the sampling kernel a run of Np chains of this plan launches under its current variant --
 * "gibbs_lean_kernel" (chain state in registers: products of 2..4 densities, fp64 products of 8, every dimension
 * active) or "gibbs_product_kernel" (any density count, masks, the reference's divide + log arithmetic).  A static
 * string. */
const char *kdehip_product_kernel_name(const kdehip_product *plan, int64_t Np);

/* ---- (2b) resident plans on several GPUs of one node (one process) --------------------------------
 * One plan per device (the packed densities are replicated), chains in contiguous ranges, Philox counters keyed by
 * the GLOBAL sample index (results identical for every number of devices), and ONE all-gather of [pGM | indices]
 * fused into the sampling kernel: its epilogue stores every final point and label straight into the arrays of ALL
 * devices (peer-mapped pointers, the stores travel over xGMI; no copy engine, no extra launch).  After the call's
 * work has run, EVERY device holds the complete d_points[g] (double[ndims*Np]) and d_indices[g] (int64[Ndens*Np]);
 * these are device pointers on device first_device+g, streams[g] (hipStream_t, or streams == NULL for the null
 * streams) is where device g's work is enqueued.  The call only enqueues.  Ordering, both ways: device g's kernel
 * starts only after the work already queued on EVERY streams[h] is over (it overwrites their arrays: consumers of
 * the previous product on those streams are safe), and each stream continues only once the slices of all other
 * devices have arrived.  Topologies without peer access fall back to hipMemcpyPeerAsync, one copy per array and
 * destination (kdehip_product_multi_transfers_per_product tells: 0 = fused).
 * VISIBILITY of the peer-written slices: the stores are plain global stores of the producing kernel; they are complete
 * and visible to device h when work on streams[h] that was enqueued AFTER this call starts (the call makes streams[h]
 * wait for every device's `done` event, and a kernel that starts behind that wait begins with a system-scope acquire
 * of its caches).  A consumer that is ALREADY RUNNING on device h while the product is sampled -- a persistent kernel
 * polling the arrays -- has no such acquire and may read stale lines from its L2: consume the result from work
 * enqueued behind the call.
 * ALLOCATION of d_points[h] / d_indices[h]: plain hipMalloc memory is peer-mapped by hipDeviceEnablePeerAccess (done at
 * create).  Arrays from a stream-ordered pool (hipMallocAsync) or from virtual-memory mappings are reachable from a
 * peer only if the pool / mapping grants that device access (hipMemPoolSetAccess / hipMemSetAccess); the call looks at
 * every destination once per product and takes the copy path for anything it cannot show reachable
 * (KDEHIP_PEER_STORES=0 forces the copy path, =1 skips the look-up).  The verdicts are remembered per plan, keyed by the
 * array's ADDRESS and the writing device: an array that is freed and re-allocated at the same address from another kind
 * of allocator keeps its old verdict until kdehip_clear_cache() is called (which forgets all of them) -- a caller that
 * switches allocators under a live plan calls it, or sets KDEHIP_PEER_STORES. */
typedef struct kdehip_product_multi kdehip_product_multi;
int kdehip_product_multi_create(kdehip_product_multi **out, int Ndens, const kdehip_density *trees, int ndims,
                                const uint8_t *partialDimMask, int precision, int first_device, int ngpus);
/* The same on a manifold: the circular plan of kdehip_product_create_manifold replicated per device (same mode selection,
 * same errors, all checked before any device is touched).  The fused peer-store epilogue applies unchanged -- the circular
 * mode is an arithmetic mode of the same kernel --, and the result is the single plan's for every ngpus.  manifold == NULL
 * or all zeros IS the entry above. */
int kdehip_product_multi_create_manifold(kdehip_product_multi **out, int Ndens, const kdehip_density *trees, int ndims,
                                         const uint8_t *partialDimMask, const uint8_t *manifold /* ndims bytes or NULL */,
                                         int precision, int first_device, int ngpus);
void kdehip_product_multi_destroy(kdehip_product_multi *mp);
int kdehip_product_multi_ngpus(const kdehip_product_multi *mp);
kdehip_product *kdehip_product_multi_plan(kdehip_product_multi *mp, int g); /* the plan on device g (owned by mp) */
int kdehip_product_multi_sample_philox(kdehip_product_multi *mp, int64_t Np, int Niter, uint64_t seed,
                                       int64_t sample_offset, int addEntropy, double *const *d_points,
                                       int64_t *const *d_indices, void *const *streams);
/* copy-engine transfers each device issues per product: 0 when the all-gather is fused into the kernel */
int kdehip_product_multi_transfers_per_product(const kdehip_product_multi *mp);

/* ---- (2c) densities that live in HBM, and products of them ------------------------------------------------
 * The reference hands gibbs1 host arrays (src/MSGibbs01.jl:527-537) and sections (1) and (2) do the same.  A caller
 * whose densities stay on the device between products -- the inputs of the next product are the outputs of the
 * previous ones -- uploads each BallTreeDensity ONCE (its means, bandwidth, weights, permutation and the frontier of
 * every level, expanded from its child arrays at upload; src/BallTreeDensity01.jl:11-24, src/MSGibbs01.jl:500-523)
 * and then runs prodAppxMSGibbsS (src/MSGibbs01.jl:645-703) on handles: the per-product re-layout into tiles is a
 * gather kernel on the GPU, only a few KB of descriptors cross PCIe, nothing comes back.  Same results as
 * kdehip_prod_philox, bit for bit (same layout, same kernels, same Philox stream). */
typedef struct kdehip_device_density kdehip_device_density;
int kdehip_density_upload(kdehip_device_density **out, const kdehip_density *host, int device);
void kdehip_density_free(kdehip_device_density *d); /* waits for the device first */
int64_t kdehip_density_npts(const kdehip_device_density *d);
int kdehip_density_ndim(const kdehip_device_density *d);
/* prodAppxMSGibbsS on device-resident densities, enqueue only: pack (GPU) + conditional tables + sampling.  The sampling
 * -- everything that touches the outputs -- runs on `stream` (hipStream_t, NULL = default stream); the preparation of
 * the product (descriptor upload, tile gather, tables: it reads only the immutable densities and writes only the
 * plan's own block) runs on a stream of the library's, and `stream` waits for it: of products enqueued back to back,
 * number k+1 is prepared while number k samples.  (Because of that second stream a call cannot be recorded by a stream
 * capture on `stream`; graphs are made of the runs of a resident plan, kdehip_product_sample_*.)  d_points (double[ndims*Np]), d_indices (int64[Ndens*Np]) and the optional
 * d_labels (as kdehip_product_sample_philox) are device pointers on the densities' device.  Random numbers: the
 * device Philox stream keyed by (seed, sample_offset + s, draw).  The plan built for the call is released by a later
 * call (or kdehip_clear_cache) once its work has run; at most 8 such calls are in flight per device and stream (a
 * caller beyond that waits for the oldest call of ITS OWN stream, never for another stream's work).  Devices 0..63. */
int kdehip_prod_philox_device(int Ndens, kdehip_device_density *const *trees, int64_t Np, int Niter, uint64_t seed,
                              int64_t sample_offset, int addEntropy, const uint8_t *partialDimMask, int precision,
                              double *d_points, int64_t *d_indices, int32_t *d_labels, void *stream);
/* The same on a manifold (`manifold`: ndims bytes of KDEHIP_MANIFOLD_EUCLIDEAN / KDEHIP_MANIFOLD_CIRCULAR or NULL, the
 * operators of "manifolds" above, as kdehip_gibbs1_manifold takes them): resident inputs, device outputs, device Philox -- the
 * tiles are re-laid-out on the GPU, no random numbers and no tiles cross PCIe.  A density set whose node values qualify for
 * the fast arithmetic (finite, variances in range) runs the sampler's circular fast mode -- fast reciprocals, the
 * product/rsqrt normalisation, the uniform-bandwidth and per-node fast evaluators with wrap() on the differences of the
 * circular dimensions, the tangent-space getMu, wrap() where a sample is composed with its noise; no conditional tables and
 * no fp32 screens --, any other set the generic arithmetic of kdehip_gibbs1_manifold.  Labels are those of that entry on the
 * host twin of the Philox streams, points agree to rounding (1e-12).  manifold == NULL or all zeros IS the entry above, bit
 * for bit.  A manifold byte above 1 is KDEHIP_ERR_ARG, more than KDEHIP_MAX_DIMS dimensions KDEHIP_ERR_UNSUPPORTED, a
 * circular dimension with precision 32 KDEHIP_ERR_UNSUPPORTED. */
int kdehip_prod_philox_device_manifold(int Ndens, kdehip_device_density *const *trees, int64_t Np, int Niter, uint64_t seed,
                                       int64_t sample_offset, int addEntropy, const uint8_t *partialDimMask,
                                       const uint8_t *manifold, int precision, double *d_points, int64_t *d_indices,
                                       int32_t *d_labels, void *stream);

/* The same with host output buffers (pts: ndims*Np, ind: Ndens*Np), blocking: for hosts that keep no device arrays of
 * their own -- a Julia caller without AMDGPU.jl uploads its densities once and then pays neither the host re-layout
 * nor the upload of the tiles per product (sample offset 0). */
int kdehip_prod_philox_resident(int Ndens, kdehip_device_density *const *trees, int64_t Np, int Niter, uint64_t seed,
                                int addEntropy, const uint8_t *partialDimMask, int precision, double *pts, int64_t *ind);
/* ... on a manifold: kdehip_prod_philox_device_manifold (sample offset 0) with host output buffers, bit for bit. */
int kdehip_prod_philox_resident_manifold(int Ndens, kdehip_device_density *const *trees, int64_t Np, int Niter, uint64_t seed,
                                         int addEntropy, const uint8_t *partialDimMask, const uint8_t *manifold,
                                         int precision, double *pts, int64_t *ind);

/* ---- (2d) the resident chain: products feed products without leaving HBM -----------------------------------
 * The reference's `*` is `pGM, = prodAppxMSGibbsS(...); kde!(pGM)` (src/MSGibbs01.jl:707-726), and in a belief-propagation
 * sweep its result is an input of the next products.  kdehip_prod_philox_device leaves pGM in HBM; these entries turn it
 * into the next product's input there.
 *
 * kdehip_density_from_device_points = `kde!(points)` (src/KDE01.jl:3-27) on a D x N column-major matrix that lives on
 * `device` (d_points; `stream` = the hipStream_t that produced it, waited for): the LOOCV bandwidth search reads the device
 * matrix as it is, the ball tree (src/BallTree01.jl:415-434) is built by the library's pooled host builder from ONE 8*D*N
 * byte copy that comes down while the search runs, and the density's block goes straight back up.  Blocking; the result
 * is bit for bit the density kdehip_make_density_auto builds from the same points.  bw_out (D standard deviations) and
 * nevals are optional.  N >= 2. */
int kdehip_density_from_device_points(kdehip_device_density **out, const double *d_points, int64_t D, int64_t N,
                                      int device, void *stream, double *bw_out, int32_t *nevals);
/* The same with a per-dimension manifold for the bandwidth search (section 5d: only the leave-one-out likelihoods of the
 * search wrap; the tree is the Euclidean builder's).  manifold == NULL or all zeros is the entry above, bit for bit; bw_out
 * and nevals are bit for bit kdehip_auto_bandwidth_manifold's for the same points. */
int kdehip_density_from_device_points_manifold(kdehip_device_density **out, const double *d_points, int64_t D, int64_t N,
                                               int device, void *stream, double *bw_out, int32_t *nevals,
                                               const uint8_t *manifold /* D bytes or NULL */);
/* `*(trees; addEntropy)` (src/MSGibbs01.jl:707-726) on handles: Np = round(mean Npts), Niter = 5, device Philox keyed by
 * `seed`, then kde!(pGM) -- the product matrix never leaves the device; one density with addEntropy = 0 is the reference's
 * shortcut (:713-716: kde! of its own points).  Blocking, on the calling thread's stream.  Same numbers as
 * kdehip_prod_philox(seed) followed by kdehip_make_density_auto on the host. */
int kdehip_mul_device(kdehip_device_density **out, int Ndens, kdehip_device_density *const *trees, uint64_t seed,
                      int addEntropy, double *bw_out, int32_t *nevals);
/* `*` on a manifold: kdehip_prod_philox_device_manifold (Niter = 5, Np = round(mean Npts), sample offset 0), then
 * kdehip_density_from_device_points_manifold on the product matrix with the same manifold -- bit for bit those two calls; the
 * result stays resident.  One density with addEntropy = 0 is the shortcut, its kde! with the manifold.  manifold == NULL or
 * all zeros IS kdehip_mul_device.  Manifold errors as kdehip_prod_philox_device_manifold. */
int kdehip_mul_device_manifold(kdehip_device_density **out, int Ndens, kdehip_device_density *const *trees, uint64_t seed,
                               int addEntropy, double *bw_out, int32_t *nevals, const uint8_t *manifold /* ndims bytes or NULL */);
/* `*` for MANY products in one call -- the reference's serving shape: a belief-propagation sweep calls `*`
 * (src/MSGibbs01.jl:707-726) dozens of times on densities of 100-300 points (test/runtests.jl:189-201), and one at a time
 * each is a blocking call of >= 10 dependent small launches.  Here every product is sampled by the batched sampler
 * (kdehip_prod_philox_batch), the LOOCV bandwidth searches (src/KDE01.jl:3-27, src/CrossValidation.jl:44-120) of all
 * outputs of one size advance in the SAME launches, the ball trees (src/BallTree01.jl:415-434) are built by the pooled
 * host builder under the searches from ONE copy of all matrices, and the nprod resulting densities share one device block.
 * out[i] (nprod handles, each freed with kdehip_density_free; the shared block goes with the last of them) is bit for
 * bit the density kdehip_mul_device(items[i]) returns: same product (Philox keyed by items[i].seed), same bandwidth
 * search evaluations, same tree.  bw_out (optional): nprod rows of KDEHIP_MAX_DIMS doubles, row i = the D bandwidths of
 * result i; nevals (optional): nprod counts.  An item with one density and addEntropy = 0 is the reference's shortcut
 * (:713-716); results of fewer than 2 or more than 2048 points are built by a call of their own inside this one.
 * All densities on one device.  Blocking, on the calling thread's stream.  On an error no handle is returned. */
typedef struct kdehip_mul_item {
  int32_t Ndens;
  int32_t addEntropy;
  kdehip_device_density *const *trees; /* Ndens handles */
  uint64_t seed;
} kdehip_mul_item;
int kdehip_mul_device_batch(int nprod, const kdehip_mul_item *items, kdehip_device_density **out, double *bw_out,
                            int32_t *nevals);
/* The same with a manifold per item: manifolds == NULL, or nprod rows of KDEHIP_MAX_DIMS bytes (as bw_out has nprod rows of
 * KDEHIP_MAX_DIMS doubles), row i holding the manifold of item i in its first ndims bytes.  Items without a
 * circular dimension take the batched sampler as above; circular items are sampled by kdehip_prod_philox_batch_manifold
 * (2e: one launch per dimension count for those in the circular fast mode), and the bandwidth searches of the circular items of one (ndims, size,
 * manifold) advance in shared launches with their likelihoods wrapped.  out[i] is bit for bit what
 * kdehip_mul_device_manifold(items[i], row i) returns; manifolds == NULL IS the entry above. */
int kdehip_mul_device_batch_manifold(int nprod, const kdehip_mul_item *items, const uint8_t *manifolds,
                                     kdehip_device_density **out, double *bw_out, int32_t *nevals);
/* The three entries above with the operators of tree construction (section 4, "tree construction on a manifold"): the
 * named entry plus a trailing tree_manifold (ndims bytes or NULL) that the host builder of the result's tree takes
 * (kdehip_make_density_tree); `manifold` keeps its meaning (the sampler and the bandwidth search).  The reference's
 * kde!(points, addop, diffop) is the call with both set to the same value.  tree_manifold == NULL or all zeros IS the
 * _manifold entry, bit for bit; a byte above 1 is KDEHIP_ERR_ARG before any device is touched.  kdehip_mul_device_tree covers
 * the one-density shortcut.  The batch takes tree_manifolds as it takes manifolds (NULL, or nprod rows of KDEHIP_MAX_DIMS
 * bytes): out[i] is bit for bit what kdehip_mul_device_tree(items[i], row i of manifolds, row i of tree_manifolds) returns,
 * and items with and without a circular tree may be mixed. */
int kdehip_density_from_device_points_tree(kdehip_device_density **out, const double *d_points, int64_t D, int64_t N,
                                           int device, void *stream, double *bw_out, int32_t *nevals,
                                           const uint8_t *manifold /* D bytes or NULL */,
                                           const uint8_t *tree_manifold /* D bytes or NULL */);
int kdehip_mul_device_tree(kdehip_device_density **out, int Ndens, kdehip_device_density *const *trees, uint64_t seed,
                           int addEntropy, double *bw_out, int32_t *nevals, const uint8_t *manifold,
                           const uint8_t *tree_manifold);
int kdehip_mul_device_batch_tree(int nprod, const kdehip_mul_item *items, const uint8_t *manifolds,
                                 const uint8_t *tree_manifolds, kdehip_device_density **out, double *bw_out, int32_t *nevals);
/* The reference's arrays of a density the library built (the entries above), shaped as in kdehip_make_density; any
 * pointer may be NULL; bw_out: its D LOOCV bandwidths (standard deviations).  A density that came from
 * kdehip_density_upload has no such mirror (KDEHIP_ERR_UNSUPPORTED): its arrays are the caller's. */
int kdehip_density_download(const kdehip_device_density *d, double *centers, double *ranges, double *weights,
                            int64_t *left_child, int64_t *right_child, int64_t *lowest_leaf, int64_t *highest_leaf,
                            int64_t *permutation, double *means, double *bandwidth, double *bandwidthMin,
                            double *bandwidthMax, double *bw_out);

/* ---- (2e) many products in one call ----------------------------------------------------------------------------
 * The serving pattern of a belief-propagation host: dozens of independent 100-300-chain products per sweep, each of which
 * fills a fraction of the device and is latency bound.  One call lays all of them out in one device block (one descriptor
 * upload, one gather launch for every tile) and samples each (dimension count, density count) group of fp64 products of
 * 2..4 densities with every dimension active in ONE launch -- workgroups indexed by (product, chain block), each fetching
 * its product's plan through the scalar cache.  Every product's result is bit for bit that of kdehip_prod_philox_device
 * with the same arguments.  Products outside that domain (fp32, masks, 1 or more than 4 densities) are enqueued one by one
 * inside the same call.  Enqueue only, everything on `stream`; all densities on one device. */
typedef struct kdehip_batch_item {
  int32_t Ndens;
  int32_t Niter;
  kdehip_device_density *const *trees;  /* Ndens handles */
  int64_t Np;
  uint64_t seed;
  int64_t sample_offset;
  int32_t addEntropy;
  int32_t reserved_;
  const uint8_t *partialDimMask;        /* Ndens*ndims bytes or NULL */
  double *d_points;                     /* device, double[ndims*Np]  */
  int64_t *d_indices;                   /* device, int64[Ndens*Np]   */
  int32_t *d_labels;                    /* device, optional          */
} kdehip_batch_item;
int kdehip_prod_philox_batch(int nprod, const kdehip_batch_item *items, int precision, void *stream);
/* The same with a manifold per item: manifolds == NULL, or nprod rows of KDEHIP_MAX_DIMS bytes (the shape
 * kdehip_mul_device_batch_manifold takes), row i holding the manifold of item i in its first ndims bytes and zeros behind
 * them.  Euclidean items ride exactly as above.  Circular fp64 items whose plans reach the sampler's circular fast mode ride
 * ONE launch per dimension count -- any density count, masked ones included: a batched instantiation of the general kernel,
 * 8 chains per workgroup --; circular items on the generic arithmetic are enqueued one by one inside the call.  Every item's
 * result is bit for bit that of kdehip_prod_philox_device_manifold with the same arguments.  manifolds == NULL or all zeros
 * IS the entry above.  A row byte above 1, or a circular byte at or beyond the item's ndims, is KDEHIP_ERR_ARG; a circular
 * item with precision 32, or more than KDEHIP_MAX_DIMS dimensions, KDEHIP_ERR_UNSUPPORTED -- before any device is touched.
 * kdehip_mul_device_batch_manifold and _tree (2d) sample their circular items through this path.
 * Environment, read once per process: KDEHIP_BATCH_CIRC=0 enqueues the circular items one by one instead (the route before
 * the batched instantiation existed; the same bits -- a switch for timing one route against the other). */
int kdehip_prod_philox_batch_manifold(int nprod, const kdehip_batch_item *items, const uint8_t *manifolds, int precision,
                                      void *stream);
/* Diagnostic: of the calling thread's last kdehip_prod_philox_batch / _manifold call that reached its launches, how many
 * batched sampling launches it made (one per group) and how many items it enqueued one by one.  Either pointer may be NULL.
 * (kdehip_mul_device_batch* call the batch on the calling thread too.) */
void kdehip_prod_philox_batch_launches(int32_t *batched, int32_t *singles);

/* ---- (2f) drawing from a density: sample, rand, resample ---------------------------------------------------------
 * `sample(p, Npts)` (reference src/KDE01.jl:164-183):  w = the leaf weights in ORIGINAL point order (getWeights);
 * C = cumsum(w), a sequential left-to-right fp64 sum, then C = C ./ C[end]; the label of a uniform u is the first i with
 * C[i] > u (strict: a zero-weight point is never drawn); the point is x = P[:, i] + sqrt(V[:, i]) .* n with P the leaf means
 * (the centers getPoints reads, in every density kde! builds) and V the leaf variances (`bandwidth`), in original order --
 * the multiply and the add are separate roundings (no fused multiply-add), sqrt and the divide are correctly rounded.
 * ind = the 1-based original index of the drawn point (the reference's convention, = the product's permutation+1).
 * Random numbers: sample s of a call has the global index g = sample_offset + s and draws u = the uniform and n[d] = the
 * normal d < D that kdehip_philox_fill_uniform(seed, g, 1, K = 1) / kdehip_philox_fill_normal(seed, g, 1, R = D) return
 * (philox.hpp: philox_uniform(seed, g, 1), philox_normal(seed, g, d)) -- the reference's rand / randn are replaced by the
 * Philox stream, so every result is reproducible on the host, and a call with sample_offset continues an earlier one.
 * (The device's log / sin / cos may differ from the host libm in the last bits of a normal; labels never depend on them.)
 * Output order: draw order, pts D x Npts column-major (as the product's).  The reference sorts its uniforms and returns
 * the samples grouped by ascending label; the distribution is the same.
 * Given labels (`sample(p, Npts, ind)`, src/KDE01.jl:185-189): ind_in holds Npts 1-based labels and the call consumes only
 * the normals.  The host entry refuses an out-of-range label (KDEHIP_ERR_ARG); the device entries never read out of
 * bounds: an out-of-range label gives a NaN point and ind = 0.
 * Arguments: Npts = 0 does nothing; Npts < 0, weights that are negative or not finite, or whose total is not positive
 * (and finite) are KDEHIP_ERR_ARG; D above KDEHIP_MAX_DIMS is KDEHIP_ERR_UNSUPPORTED.  The host entry checks all of this
 * before it touches a device.
 * Device handles: the first sample call on a handle builds its table (C in original order and the inverse permutation, one
 * wavefront per density, about N dependent fp64 adds) on the calling thread's stream and blocks until it is complete --
 * that call validates the weights and can return KDEHIP_ERR_ARG.  Later calls only enqueue: the table is complete in
 * memory before any call can use it, from any thread or stream.  Concurrent first calls on one handle build it once.
 * kdehip_density_free releases the table (also for the handles of a kdehip_mul_device_batch block). */

/* Host density, host buffers, blocking, on hipStreamPerThread.  ind_in: NULL = draw the labels. */
int kdehip_sample(const kdehip_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset, const int64_t *ind_in,
                  double *pts, int64_t *ind, int device);
/* A resident density; device pointers (d_ind_in may be NULL); enqueue only on `stream` (hipStream_t, NULL = the null
 * stream) once the handle's table exists (the first call builds it, see above). */
int kdehip_sample_device(kdehip_device_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset,
                         const int64_t *d_ind_in, double *d_pts, int64_t *d_ind, void *stream);
/* Many draws in one call: items of any densities (mixed D and N) on one device.  One table-build launch for the handles
 * that have no table yet (blocking, as above), then one draw launch per distinct D on `stream`.  Every item's result is bit
 * for bit that of kdehip_sample_device with the same arguments. */
typedef struct kdehip_sample_item {
  kdehip_device_density *density;
  int64_t Npts;
  uint64_t seed;
  int64_t sample_offset;
  const int64_t *d_ind_in;  /* device, Npts 1-based labels, or NULL = draw */
  double *d_pts;            /* device, double[D*Npts] */
  int64_t *d_ind;           /* device, int64[Npts]    */
} kdehip_sample_item;
int kdehip_sample_device_batch(int n, const kdehip_sample_item *items, void *stream);
/* `resample(p, Np, :lcv)` (src/BallTreeDensity01.jl:312-334): sample(p, Np) into a pooled device buffer, then
 * kdehip_density_from_device_points -- the result is bit for bit kdehip_make_density_auto on the same points.  Np <= 0 means
 * Npts(p) (the reference's default calls an undefined getNpts; Npts(p) is its evident intent).  Needs Np >= 2.  Blocking, on
 * the calling thread's stream; bw_out (D standard deviations) and nevals are optional. */
int kdehip_resample_device(kdehip_device_density **out, kdehip_device_density *p, int64_t Np, uint64_t seed, double *bw_out,
                           int32_t *nevals);

/* ---- diagnostics (not part of the drop-in surface; bench.py and the tests use them) -----------------------------
 * While enabled, every kdehip_prod_philox_device call brackets its sampling launch with a pair of timing events on the
 * caller's stream; kdehip_profile_sampler_read waits for the device's calls in flight and returns the sum of those
 * durations and their count for the calls that were enqueued on `stream` since the switch was last set (which also resets
 * the sums).  The switch is process-wide; the sums are kept per device and caller stream, so concurrent callers on
 * streams of their own do not mix.  The blocking one-shot entries (kdehip_gibbs1*, kdehip_prod_philox) are bracketed too; they
 * run on the calling thread's stream, which kdehip_profile_sampler_read knows as hipStreamPerThread ((hipStream_t)2). */
void kdehip_profile_sampler(int enable);
int kdehip_profile_sampler_read(int device, void *stream, double *total_ms, int64_t *launches);
/* With the switch on, kdehip_product_multi_sample_philox brackets every device's sampling launch too; this returns, for
 * the LAST product of `mp` (waiting for it), kernel_ms[g] = the duration of device g's launch and done_ms[g] = the host
 * time at which g's slice had arrived on every device, relative to the first device to get there (both arrays: ngpus
 * entries): a straggling device or link shows up as skew, a slow kernel as duration. */
int kdehip_product_multi_timing(kdehip_product_multi *mp, double *kernel_ms, double *done_ms);

/* The callers either side of the product (section 5, 2d) are blocking entries on the calling thread's own stream: their
 * device work cannot be bracketed from outside.  With kdehip_profile_sampler(1), the LOOCV bandwidth search (which = 0:
 * preparation + every round of a search, per batch of rounds), kdehip_evaluate (which = 1: the partial and finish
 * kernels) and the GPU tree builder (which = 2: kdehip_make_densities_device's kernel) bracket their launches with a pair
 * of timing events; this returns the sum of those durations and the number of bracketed phases since the last read, and
 * resets both (process-wide sums).  bench.py --frow reports them as kernel time.  kdehip_evaluate_tol (section 5m) adds, in
 * the same way, its three passes one by one: which = 3 the chunk boxes, 4 the plan, 5 the sweep over the flagged chunks
 * (which = 1 is then the whole call: the three passes and the finish kernel).  kdehip_knn (section 5n) likewise: which = 6 the
 * chunk boxes, 7 the plan, 8 the sweep.  A refit (section 5r): which = 9, its passes from the copy to the examination. */
int kdehip_profile_phase_read(int which, double *total_ms, int64_t *count);
/* The fp32 screen of the deep levels (csrc/screen_device.hpp) certifies its decisions with an error bound whose premise is
 * that the hardware's v_rcp_f32, v_rsq_f32 and v_exp_f32 are within 1 ulp (a relative error of at most 2 u, u = 2^-24).
 * This entry MEASURES that on `device`: over the `count` fp32 bit patterns from `first_bits` on it returns the largest
 * error of instruction `which` against fp64 formed on the device -- 0: v_rcp_f32, 1: v_rsq_f32, 2: v_exp_f32 (2^x), each
 * relative, in units of u; 3: |v_exp_f32(x) - 2^x| in units of 2^-126 (for x < -126, where the bound only needs "off by
 * less than the smallest normal").  worst_bits / worst_result_bits (optional): the input with the largest error and the
 * hardware's result for it.  tests/test_gpu_ulp.py sweeps the screen's whole input ranges with it.  Blocking. */
int kdehip_selftest_fp32(int which, uint32_t first_bits, uint64_t count, int device, double *max_err,
                         uint32_t *worst_bits, uint32_t *worst_result_bits);
/* The fp64 exponentials every density kernel calls once per pair (csrc/fastexp.hpp), MEASURED on `device` against a
 * double-double reference (csrc/expdd.hpp, relative error <= 2^-80).  which = 0: exp_nonpos (32-entry table), 1:
 * exp256_nonpos (256-entry table); each is evaluated through its _begin / _end halves and through the one-call form, with
 * the table staged in LDS as the kernels stage it, and *form_mismatches (optional) counts the inputs at which the two forms
 * differ in any bit.  The inputs are generated on the device: input i (first <= i < first + count) of `family` is
 *   0 dense       upper word 0xBE100000 + i / 16 (-2^-30 .. -708), lower word 0, 0xFFFFFFFF or mix(i) (i % 16 = 0, 1, else)
 *   1 half-way    the double nearest -(n + 1/2) c, c = ln2/32 (which 0) or ln2/256 (which 1), n = i / 129, moved by
 *                 i % 129 - 64 places in the order of the doubles: where the reduction's rounding flips
 *   2 whole       the same about -(n + 1) c, n = i / 129: where the reduced argument cancels
 *   3 range       2^26 + 1 arguments spread over [-745.2, -708.3] (results below the smallest normal number)
 *   4 range       2^24 + 1 arguments spread over [-1000.0 (which 1) or -800.0 (which 0), -745.2] (results that round to 0)
 *   5 near zero   biased exponent 993 - i / 8 (2^-30 down to the subnormals), 8 mantissas each, negative
 *   6 raw         the bit pattern `first + i` itself (single inputs, neighbourhoods, non-finite values)
 * (the exact maps are kdehip::exp64_input, csrc/selftest.hip, repeated in tests/test_gpu_exp64.py).  One error unit for
 * all: |got - ref| / ulp(ref), ulp(ref) = 2^(e-52) for 2^e <= ref < 2^(e+1), floored at 2^-1074 (below the normal range it
 * counts spacings of the subnormal grid); an argument below -770 has ref = 0; a NaN on either side counts as 2^60.
 * Returns the largest error, the 64 bits of its input and of the device's result (the lowest such i on a tie).  count <=
 * 2^40.  Blocking. */
int kdehip_selftest_exp64(int which, int family, uint64_t first, uint64_t count, int device, double *max_err,
                          uint64_t *worst_bits, uint64_t *worst_result_bits, uint64_t *form_mismatches);

/* ---- (3) host twin of the device RNG ----------------------------------------------------------
 * Fills the arrays a caller would pass as randU / randN so that a streams-run (or the Julia
 * reference, via its randU=/randN= keywords, src/MSGibbs01.jl:661-662) consumes exactly the
 * numbers the Philox run draws.  out_u has nsamples*K, out_n has nsamples*R entries. */
void kdehip_philox_fill_uniform(uint64_t seed, int64_t sample_begin, int64_t nsamples, int64_t K,
                                double *out_u);
void kdehip_philox_fill_normal(uint64_t seed, int64_t sample_begin, int64_t nsamples, int64_t R,
                               double *out_n);

/* ---- (4) density construction (host; reference kde!(points, ks, weights), src/KDE01.jl:34-57 ->
 * makeBallTreeDensity, src/BallTreeDensity01.jl:192-231 -> buildTree!, src/BallTree01.jl:415-434).
 * A Julia caller keeps using its own kde!; this entry serves hosts without the reference.
 * points: D x N column-major; ks: nks = 1 or D standard deviations (squared inside);
 * weights_in: N or NULL (= ones).  Outputs are caller-allocated: centers, ranges, means,
 * bandwidth: D*2N; weights and the five index arrays: 2N; bandwidthMin/Max: D*N.
 * Thread-safe.  From 512 points up the top levels hand their left subtree to a process-wide pool of at most 15
 * worker threads (started on first use, asleep in between, never joined; csrc/host_pool.hpp): the arrays do not
 * depend on the number of threads, and a process that fork()ed away from the workers builds serially. */
int kdehip_make_density(int64_t D, int64_t N, const double *points, const double *ks, int64_t nks,
                        const double *weights_in, double *centers, double *ranges, double *weights,
                        int64_t *left_child, int64_t *right_child, int64_t *lowest_leaf,
                        int64_t *highest_leaf, int64_t *permutation, double *means,
                        double *bandwidth, double *bandwidthMin, double *bandwidthMax);

/* Tree construction on a manifold: kde!(points, ks, weights, addop, diffop) (src/KDE01.jl:34-57 -> makeBallTreeDensity ->
 * buildTree! -> buildBall!).  tree_manifold: D bytes of KDEHIP_MANIFOLD_EUCLIDEAN / KDEHIP_MANIFOLD_CIRCULAR or NULL.  In a
 * circular dimension addop(a, b) = wrap(a + b) and diffop(a, b) = wrap(a - b) ("manifolds" above; csrc/circ_wrap.hpp, the one
 * expression host and device share) replace + / - at exactly the reference's hook points; nothing is added, clamped or repaired:
 *   most_spread_coord (src/BallTree01.jl:142-173)   mean = addop(mean, w c); variance += diffop(c, mean)^2.  The sums stay
 *                        sequential, the last leaf of the range is left out, w = 1 / (high - low), the comparison a strict >.
 *   select! (:223-242)   the test c_i - c_pivot < 0 becomes diffop(c_i, c_pivot) < 0.  Pivot choice, the single forward scan,
 *                        the final swap and the m <= pos / m >= pos updates are unchanged.  The wrapped comparison is not a
 *                        total order; every pass still fixes its pivot and shrinks the range, so the loop ends, and the
 *                        result is whatever the reference's scan produces.
 *   getMiniMaxi / calcStatsBall! (:249-336)   a = addop(c_L, r_L), b = addop(c_R, r_R), maxi = a > b ? a : b;
 *                        c = diffop(c_L, r_L), c2 = diffop(c_R, r_R), mini = c < c2 ? c : c2; halfspan = diffop(maxi, mini) / 2
 *                        (stored in ranges); center = addop(mini, halfspan).  Half-spans can come out NEGATIVE on data spread
 *                        round the circle; they are stored as computed.
 * What stays Euclidean, as in the reference: calcStatsDensity! (src/BallTreeDensity01.jl:156-185: node weights, the
 * moment-matched means / bandwidth, bandwidthMin / Max -- the reference passes its operators down to calcStatsBall! only),
 * the child numbering and lowest / highest_leaf, and the leaf values (points are stored as given, any representative, no
 * wrapping of inputs).
 *   - wrap(t) == t for -pi <= t < pi: a circular build on data in which no hooked expression leaves that interval returns the
 *     Euclidean build's bits.  Any data inside [-1, 1] qualifies (means and differences stay below 2, box edges inside
 *     [-1, 1], spans at most 2).
 *   - tree_manifold == NULL or all zeros IS kdehip_make_density, bit for bit (it forwards here with NULL).
 *   - a byte above 1 is KDEHIP_ERR_ARG, checked before any array is written.
 * `manifold` (sections 2c, 2d, 5d: the sampler, evaluation, the bandwidth search) and `tree_manifold` (the builders) are
 * separate arguments: the _manifold entries keep building Euclidean trees. */
int kdehip_make_density_tree(int64_t D, int64_t N, const double *points, const double *ks, int64_t nks,
                             const double *weights_in, double *centers, double *ranges, double *weights,
                             int64_t *left_child, int64_t *right_child, int64_t *lowest_leaf,
                             int64_t *highest_leaf, int64_t *permutation, double *means,
                             double *bandwidth, double *bandwidthMin, double *bandwidthMax,
                             const uint8_t *tree_manifold /* D bytes or NULL */);

/* A density whose points each have a bandwidth of their own (multibandwidth = 1; the `else` branch of makeBallTreeDensity,
 * src/BallTreeDensity01.jl:216-225, which kde! never takes).  ks: D*N standard deviations, column-major (ks[i*D + k] is
 * point i's in dimension k), in the ORIGINAL point order of `points`; squared inside.  There is no nks.
 *   - The tree, the boxes, the weights and the means are exactly kdehip_make_density_tree's: they do not depend on ks.
 *   - bandwidthMin / bandwidthMax are D*2N here, rows by node like `bandwidth`.  The leaf rows of all three are ks^2 through
 *     the permutation; an internal row of `bandwidth` is the moment match of calcStatsDensity! (:180-185), of Min / Max the
 *     smaller / larger of its children's rows by the reference's strict comparisons (:164-177).
 *   - A ks entry that is not finite and > 0 is KDEHIP_ERR_ARG, checked before any array is written.
 *   - With all N columns of ks equal, `bandwidth` is bit for bit kdehip_make_density_tree's with that column.
 * What reads such a density: section 5o (evaluation, log-likelihoods), the sampler (non-uniform tiles), kdehip_sample (the
 * drawn leaf's own variance), kdehip_kernel_sum with explicit variances, kdehip_knn, kdehip_density_upload.  Every other
 * entry keeps refusing it with KDEHIP_ERR_UNSUPPORTED. */
int kdehip_make_density_varbw(int64_t D, int64_t N, const double *points, const double *ks /* D*N */,
                              const double *weights_in, double *centers, double *ranges, double *weights,
                              int64_t *left_child, int64_t *right_child, int64_t *lowest_leaf,
                              int64_t *highest_leaf, int64_t *permutation, double *means,
                              double *bandwidth, double *bandwidthMin /* D*2N */, double *bandwidthMax /* D*2N */,
                              const uint8_t *tree_manifold /* D bytes or NULL */);

/* The bandwidth-dependent half of the construction on an existing tree: topology, bounding boxes, weights and means
 * do not depend on ks, only `bandwidth` (leaves ks^2, internal nodes by moment matching,
 * src/BallTreeDensity01.jl:141-187) and bandwidthMin/Max do.  Lets kde!(points) build its tree while the GPU searches
 * the LOOCV bandwidth; the result is bit-identical to kdehip_make_density called with this ks. */
int kdehip_density_set_bandwidth(int64_t D, int64_t N, const double *ks, int64_t nks, const double *weights,
                                 const int64_t *left_child, const int64_t *right_child, const double *means,
                                 double *bandwidth, double *bandwidthMin, double *bandwidthMax);

/* The same construction on the GPU, for a batch of `nb` densities of one dimension count (one workgroup per
 * density, level-synchronous; csrc/treebuild.hip): bit-identical arrays -- same node numbering, leaf order and
 * statistics as kdehip_make_density and the reference.  Every pointer argument is an array of nb pointers to
 * caller-allocated host arrays shaped as in kdehip_make_density (ks[j]: nks values; weights_in may be NULL, or hold
 * NULL entries, for unit weights).  Densities the device builder cannot hold in LDS are refused with
 * KDEHIP_ERR_UNSUPPORTED (kdehip_make_density_device_supported tells beforehand; callers then use
 * kdehip_make_density). */
int kdehip_make_density_device_supported(int64_t D, int64_t N);
int kdehip_make_densities_device(int nb, int64_t D, const int64_t *Ns, const double *const *points,
                                 const double *const *ks, int64_t nks, const double *const *weights_in,
                                 double *const *centers, double *const *ranges, double *const *weights,
                                 int64_t *const *left_child, int64_t *const *right_child,
                                 int64_t *const *lowest_leaf, int64_t *const *highest_leaf,
                                 int64_t *const *permutation, double *const *means, double *const *bandwidth,
                                 double *const *bandwidthMin, double *const *bandwidthMax, int device);
/* The same with the operators of kdehip_make_density_tree: ONE tree_manifold of D bytes (or NULL) for the whole batch;
 * bit-identical to kdehip_make_density_tree per member.  An all-Euclidean batch runs the kernel of the entry above (which
 * forwards here with NULL); a byte above 1 is KDEHIP_ERR_ARG before any device is touched.
 * kdehip_make_density_device_supported is unchanged. */
int kdehip_make_densities_device_tree(int nb, int64_t D, const int64_t *Ns, const double *const *points,
                                      const double *const *ks, int64_t nks, const double *const *weights_in,
                                      double *const *centers, double *const *ranges, double *const *weights,
                                      int64_t *const *left_child, int64_t *const *right_child,
                                      int64_t *const *lowest_leaf, int64_t *const *highest_leaf,
                                      int64_t *const *permutation, double *const *means, double *const *bandwidth,
                                      double *const *bandwidthMin, double *const *bandwidthMax, int device,
                                      const uint8_t *tree_manifold /* D bytes or NULL */);

/* ---- (5) direct evaluation and automatic bandwidth (the callers either side of the product) ----
 * kdehip_evaluate: `evaluateDualTree(bd, pos)` / `bd(pos)` with the reference's default
 * FORCE_EVAL_DIRECT = true (src/DualTree01.jl:130-162, 303-346, 370-446): p_out[q] = density of `bd` at
 * column q of pos (D x Nq, column-major).  leave_one_out != 0 is the `bd == locations` case
 * (`makeDualTree(bd, errTol)`, :361-368): pos is ignored, the density is evaluated at its own points
 * without the self term and divided by (1 - w_q) (:335); p_out has npts entries in the ORIGINAL point
 * order.  Host buffers, blocking. */
int kdehip_evaluate(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out,
                    double *p_out, int device);
/* kdehip_auto_bandwidth: the bandwidth `kde!(points)` selects (src/KDE01.jl:3-27): per dimension,
 * `ksize` of the 1-D marginal = golden-section search (tol 1e-2) over the leave-one-out
 * log-likelihood (src/CrossValidation.jl:15-120).  points: D x N column-major; bw_out: D standard
 * deviations; nevals (optional): number of likelihood evaluations -- the reference's count: for the smaller marginals
 * the search evaluates the two possible successors of the point in flight in the same launch (csrc/loocv.hip
 * loo_round_spec_kernel); the ones golden does not ask for are neither booked nor counted. */
int kdehip_auto_bandwidth(int64_t D, int64_t N, const double *points, double *bw_out, int32_t *nevals,
                          int device);
/* `kde!(points)` in one call (src/KDE01.jl:3-27: LOOCV bandwidth per dimension, then kde!(points, bwds)): the host tree
 * builder runs on the library's worker threads WHILE the GPU searches the bandwidth -- topology, bounding boxes,
 * weights and means do not depend on it -- and the variances are filled in afterwards.  Arrays as
 * kdehip_make_density (unit weights), bw_out and nevals as kdehip_auto_bandwidth; bit-identical to the two calls one
 * after the other.  N >= 2. */
int kdehip_make_density_auto(int64_t D, int64_t N, const double *points, double *bw_out, int32_t *nevals, int device,
                             double *centers, double *ranges, double *weights, int64_t *left_child, int64_t *right_child,
                             int64_t *lowest_leaf, int64_t *highest_leaf, int64_t *permutation, double *means,
                             double *bandwidth, double *bandwidthMin, double *bandwidthMax);

/* ---- (5b) evalAvgLogL, and evaluation of resident densities ----------------------------------------------------
 * `evalAvgLogL(bd, at)` (src/DualTree01.jl:450-470): L = evaluateDualTree(bd, at) -- bd at at's points, by the direct sum
 * of kdehip_evaluate -- and W = at's weights; if some L_q == 0 has W_q != 0 the result is -Inf (whatever else is NaN),
 * otherwise sum_q W_q log L_q with the L_q == 0 terms counted as 0.  at's points are its leaf means (the centers getPoints
 * reads in every density kde! builds).  leave_one_out is the reference's `bd == at` (an identity test, :333): the self term
 * is skipped and L_q is divided by (1 - w_q) (:335); it needs at == bd (KDEHIP_ERR_ARG otherwise).  at == bd without the
 * flag is the reference's evalAvgLogL(bd, deepcopy(bd)).
 * The other functions of the reference are compositions of this one (leave_one_out = 1 exactly where the arguments are
 * the same object):
 *   entropy(bd)   = -evalAvgLogL(bd, bd)                         (:505-508)
 *   kld(p, q)     = evalAvgLogL(p, p) - evalAvgLogL(q, p)        (:477-503, method = :direct; kld(p, p) is not 0)
 *   minkld(p, q)  = min(|kld(p, q)|, |kld(q, p)|)                (:510)
 * Arguments: ndims must match (KDEHIP_ERR_DIM_MISMATCH); D above KDEHIP_MAX_DIMS, or an evaluated density whose leaves do
 * not share one bandwidth vector, is KDEHIP_ERR_UNSUPPORTED (as kdehip_evaluate; `at` contributes only points and weights).
 * Every entry checks all of its arguments before it touches a device.
 * Arithmetic: every L_q is bit for bit what kdehip_evaluate returns for that point (same kernels' arithmetic, same split of
 * the sum, which depends on the pair's (N, Nq) alone); W_q log L_q is summed in at's leaf order, in blocks of 256 by a fixed
 * tree, the blocks in order.  The result is the same bits from the host entry, a single device call and any batch, run
 * after run. */
int kdehip_eval_avg_logl(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out, int device);
/* Host densities (at may be NULL when leave_one_out is set), one pinned upload, blocking, on hipStreamPerThread. */
typedef struct kdehip_logl_item {
  const kdehip_device_density *bd;
  const kdehip_device_density *at;
  int32_t leave_one_out;
  int32_t reserved_;
} kdehip_logl_item;
/* Resident densities, all on one device: d_out[i] (device, n doubles) = evalAvgLogL(items[i].bd, items[i].at).  One
 * partial-sum launch per distinct D, one finish launch and one reduction launch for all items.  Enqueue only, on `stream`
 * (hipStream_t, NULL = the null stream). */
int kdehip_eval_avg_logl_device_batch(int n, const kdehip_logl_item *items, double *d_out, void *stream);
/* The same for one pair, blocking on the calling thread's stream; the result to host memory. */
int kdehip_eval_avg_logl_device(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                double *out);
/* `evaluateDualTree(bd, pos)` on a resident density, enqueue only on `stream`: d_pos = D x Nq column-major device points,
 * d_out = Nq device doubles in query order.  leave_one_out != 0: d_pos and Nq are ignored, bd is evaluated at its own
 * points as kdehip_evaluate does, d_out holds npts values in the original point order. */
int kdehip_evaluate_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int leave_one_out, double *d_out,
                           void *stream);
/* bd at at's points (leave-one-out when at == bd), d_out = npts(at) device doubles in at's ORIGINAL point order (through
 * its permutation, as getPoints orders them); enqueue only on `stream`. */
int kdehip_evaluate_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out, void *stream);

/* ---- (5d) circular dimensions in evaluation, log-likelihoods and the bandwidth search ------------------------------------
 * The entries of sections 5, 5b and 2d with a trailing per-dimension `manifold` (KDEHIP_MANIFOLD_EUCLIDEAN /
 * KDEHIP_MANIFOLD_CIRCULAR, ndims bytes or NULL, as kdehip_gibbs1_manifold takes it), at the places where the reference
 * threads `diffop` (evalDirect -> maxDistKer! -> distGauss!, src/DualTree01.jl:14-47, 130-162; evalAvgLogL / entropy / kld /
 * minkld, :450-510, as compositions; kde!(points, addop, diffop) -> ksize -> golden -> nLOO_LL -> entropy,
 * src/KDE01.jl:3-27, src/CrossValidation.jl:15-120) and nowhere deeper.  Semantic, with wrap() of "manifolds" above:
 *   - in a circular dimension k every difference x_qk - c_ik becomes wrap(x_qk - c_ik) before it is squared -- the ONE fp64
 *     expression (csrc/circ_wrap.hpp) the sampler, oracle/kde_oracle.c and tests/pymodel.py wrapRad share, divide included,
 *     same constants.  Nothing else changes: the same -1/(2 bw_k), the same exponential, the same Gaussian normalisation
 *     (a circular density keeps the Gaussian constant, :325-335), the same division by 1 - w_q for leave-one-out.
 *   - inputs need not lie in [-pi, pi): the wrap is applied to the difference, any representative works.
 *   - manifold == NULL or all zeros IS the existing entry, bit for bit (the existing entries forward here with NULL).
 *   - wrap(t) == t exactly whenever -pi <= t < pi, so a circular call on data in which no pair difference leaves that
 *     interval returns the Euclidean call's bits: the split of every sum stays a function of (N, Nq) alone (section 5b).
 *   - a manifold byte other than 0 or 1 is KDEHIP_ERR_ARG, checked before any device is touched.
 * Bandwidth search: only the leave-one-out likelihoods wrap.  The marginal's sort, neighborMinMax and with it the search
 * bracket are the Euclidean ones, as in the reference (marginal(p, [i]) and the kde! inside ksize build their 1-D trees with
 * the default operators), and kdehip_make_density_auto_manifold / kdehip_density_from_device_points_manifold build the
 * tree with the Euclidean builder.  The tree's own operators are a separate argument, tree_manifold (section 4, "tree
 * construction on a manifold"): kdehip_make_density_auto_tree below takes both, and the reference's kde!(points, addop, diffop)
 * is the call with both set to the same value; its search is untouched by tree_manifold.
 * Products: besides kdehip_gibbs1_manifold (host trees, caller streams, the generic arithmetic), the resident entries take a
 * manifold -- kdehip_prod_philox_device_manifold, kdehip_prod_philox_resident_manifold (2c), kdehip_mul_device_manifold,
 * kdehip_mul_device_batch_manifold (2d) -- and run the sampler's circular fast mode; their _tree forms (2d) add the
 * builder's operators.  Drawing, resampling, marginals and the summaries take theirs in section 5e.  Still Euclidean only:
 * the Python mirror's `a * b`; kdehip_density_set_bandwidth needs no manifold (topology and means do not depend on the
 * bandwidth, and the moment matching is Euclidean in the reference). */
int kdehip_evaluate_manifold(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, double *p_out,
                             int device, const uint8_t *manifold);
int kdehip_evaluate_device_manifold(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int leave_one_out,
                                    double *d_out, void *stream, const uint8_t *manifold);
int kdehip_evaluate_device_at_manifold(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out,
                                       void *stream, const uint8_t *manifold);
int kdehip_eval_avg_logl_manifold(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out,
                                  int device, const uint8_t *manifold);
int kdehip_eval_avg_logl_device_manifold(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                         double *out, const uint8_t *manifold);
/* The batch takes a manifold per item, as a mask (bit d = dimension d circular; a bit at or above the item's ndims is
 * KDEHIP_ERR_ARG).  kdehip_logl_item's reserved_ word was never checked, so it keeps having no meaning:
 * kdehip_eval_avg_logl_device_batch forwards here with mask 0.  Euclidean and circular items of any D may be mixed; each
 * result is bit for bit the single call's. */
typedef struct kdehip_logl_manifold_item {
  const kdehip_device_density *bd;
  const kdehip_device_density *at;
  int32_t leave_one_out;
  uint32_t circular_mask;
} kdehip_logl_manifold_item;
int kdehip_eval_avg_logl_device_batch_manifold(int n, const kdehip_logl_manifold_item *items, double *d_out, void *stream);
int kdehip_auto_bandwidth_manifold(int64_t D, int64_t N, const double *points, double *bw_out, int32_t *nevals, int device,
                                   const uint8_t *manifold);
int kdehip_make_density_auto_manifold(int64_t D, int64_t N, const double *points, double *bw_out, int32_t *nevals, int device,
                                      double *centers, double *ranges, double *weights, int64_t *left_child,
                                      int64_t *right_child, int64_t *lowest_leaf, int64_t *highest_leaf, int64_t *permutation,
                                      double *means, double *bandwidth, double *bandwidthMin, double *bandwidthMax,
                                      const uint8_t *manifold);
/* kde!(points, addop, diffop) (src/KDE01.jl:3-27): `manifold` for the bandwidth search as above, `tree_manifold` for the
 * builder of the final tree (:24; kdehip_make_density_tree).  tree_manifold == NULL or all zeros IS the entry above. */
int kdehip_make_density_auto_tree(int64_t D, int64_t N, const double *points, double *bw_out, int32_t *nevals, int device,
                                  double *centers, double *ranges, double *weights, int64_t *left_child,
                                  int64_t *right_child, int64_t *lowest_leaf, int64_t *highest_leaf, int64_t *permutation,
                                  double *means, double *bandwidth, double *bandwidthMin, double *bandwidthMax,
                                  const uint8_t *manifold, const uint8_t *tree_manifold);

/* ---- (5c) summaries: marginal, getKDERange, getKDEMax, getKDEMean, getKDEfit, intersIntgAppxIS -------------------------
 * The calls a belief-propagation host makes after a solve (src/KDE01.jl:143-153, src/DualTree01.jl:512-618), on densities
 * that live in HBM (and, for getKDEMax / intersIntgAppxIS, on host densities uploaded for the call).  A density's points are
 * its leaf means (as in 5b); "original order" is getPoints order, through the permutation.  dims are 1-based here (0-based in
 * the Python mirror).  Only the Euclidean operators exist HERE: the reference's addop / diffop arguments of these functions
 * are not part of THESE entries, which forward to the _manifold forms of section 5e with NULL; evaluation, log-likelihoods
 * and the bandwidth search take a manifold in section 5d.
 *   marginal(p, dims)  = kde!(getPoints(p)[dims, :], getBW(p, [1])[dims], getWeights(p)): size(bandwidth, 2) > 2N is false
 *                        for the flat arrays, so the bandwidth is that of ORIGINAL point 1; getBW returns sqrt(variance) and
 *                        kde! squares it again, so the marginal's variance is fl(sqrt(v))^2, not v.  The weights are
 *                        normalised again as kdehip_make_density normalises them.  Repeated and reordered dims are allowed.
 *   getKDERange(p, extend) = per dimension lo = min, hi = max over the points, dr = extend * (hi - lo), (lo - dr, hi + dr):
 *                        D x 2 column-major (the reference's rangeV; range[d] = lo, range[D + d] = hi).  Exact.
 *   grid(lo, hi, Ngrid) = x_k = lo + k h for k < Ngrid - 1, h = (hi - lo) / (Ngrid - 1), x_{Ngrid-1} = hi, every operation
 *                        rounded on its own (no fused multiply-add); Ngrid >= 2.  Julia's range(lo, stop=hi, length=N) forms
 *                        its points in double-double arithmetic: the two may differ in the last bit.
 *   getKDEMax(p, N)    = per dimension i: the 1-D marginal over [i], its range with extend 0.1 (:562 uses the default), that
 *                        marginal evaluated on the grid by the direct sum (FORCE_EVAL_DIRECT), and x_k of the FIRST k with the
 *                        maximum value (findfirst(isequal(maximum(y)), y): a NaN wins).  The grid values are those of the
 *                        marginal density -- weights w_i / S (S = the weights' total, summed in a fixed tree), variance
 *                        fl(sqrt(v_1))^2, norm sqrt(2 pi) sqrt(variance) -- summed over p's leaves in p's tree order, in leaf
 *                        groups that depend on (N, Ngrid) alone, with the evaluator's exp: not bit-equal to kdehip_evaluate on a
 *                        host-built marginal (whose leaf order differs), within about 1e-13 relative of the exact value (the
 *                        tests hold them to 1e-12).
 *   getKDEMean(p)      = Statistics.mean(getPoints(p), dims=2): unweighted; per dimension the sequential left-to-right fp64 sum
 *                        in original order from +0.0 (Julia's sum(A, dims=2) of a column-major matrix loops over the columns),
 *                        then / N (current Statistics: result ./= n; older versions scaled by 1//n, which can differ in the
 *                        last bit).  Bit for bit.
 *   getKDEfit(p)       = fit(MvNormal, getPoints(p)): the mean above and the covariance (1/N) sum_j (x_j - mu)(x_j - mu)^T, each
 *                        entry a sequential sum in original order (BLAS's order is not reproducible: a tolerance).
 *   intersIntgAppxIS(p, q, N) = D = 1 or 2 (others KDEHIP_ERR_UNSUPPORTED, the reference errors); the grid of dimension d is
 *                        grid(getKDERange(p, 0.3)[d]) (= p's marginal range), dx_d = x_1 - x_0; p and q are evaluated on it by
 *                        the kernels of kdehip_evaluate (every value bit for bit what kdehip_evaluate returns there).  1-D:
 *                        0 + (sum_k p_k q_k) dx_1; 2-D: row i is the points (x1_j, x2_i), j = 0..N-1, its sum_j p q in j order,
 *                        and acc += (dx_1 row_i) dx_2 over the rows in order.  The reference's `sum` is pairwise: a tolerance.
 * Every entry checks all of its arguments before it touches a device: NULLs, Ngrid < 2 (KDEHIP_ERR_ARG), Ngrid above 2^24
 * (2^14 for a 2-D intersIntgAppxIS: KDEHIP_ERR_UNSUPPORTED), nsel outside 1..KDEHIP_MAX_DIMS, dims outside 1..D, the
 * dimensions of p and q (KDEHIP_ERR_DIM_MISMATCH), D above KDEHIP_MAX_DIMS (KDEHIP_ERR_UNSUPPORTED). */

/* marginal of a resident density (the dims gathered on the device, one copy down, the host builder with explicit ks and
 * weights, the block back up).  The result keeps the host mirror: kdehip_density_download works on it (bw_out = the
 * marginal's ks).  Blocking, on the calling thread's stream. */
int kdehip_density_marginal_device(kdehip_device_density **out, const kdehip_device_density *p, int nsel,
                                   const int32_t *dims);
/* Summaries of many resident densities (any D and N, one device) in one call, enqueue only on `stream` (hipStream_t, NULL =
 * the null stream): one moments launch (one workgroup per item), then -- for the items that ask for the grid -- one grid
 * launch and one argmax launch for all of them.  The grid is grid(getKDERange(p, extend)[d], Ngrid): getKDEMax is extend =
 * 0.1.  Outputs are device pointers; NULL ones are skipped.  Every item's result is bit for bit what it gets alone. */
typedef struct kdehip_summary_item {
  const kdehip_device_density *density;
  double extend;
  int64_t Ngrid;       /* >= 2 (also when no grid output is asked for) */
  double *d_range;     /* 2D: D x 2 column-major, (lo - dr, hi + dr) per dimension */
  double *d_mean;      /* D */
  double *d_cov;       /* D*D */
  double *d_argmax;    /* D: getKDEMax */
  double *d_values;    /* D*Ngrid: the 1-D marginal over [d] on its grid at [d*Ngrid, (d+1)*Ngrid) */
} kdehip_summary_item;
int kdehip_summary_device_batch(int n, const kdehip_summary_item *items, void *stream);
/* The same for one resident density, host outputs (any may be NULL; values: D*Ngrid), blocking on the calling thread's
 * stream.  extend: one double, or NULL for the reference's default 0.1. */
int kdehip_density_summary(const kdehip_device_density *p, const double *extend, int64_t Ngrid, double *range, double *mean,
                           double *cov, double *argmax, double *values);
/* getKDEMax of a host density (uploaded for the call), out: D values, grid_values: NULL or D*Ngrid as d_values above.
 * Blocking.  The same bits as the resident entries on the same density. */
int kdehip_kde_max(const kdehip_density *p, int64_t Ngrid, double *out, double *grid_values, int device);
/* intersIntgAppxIS of two host densities (uploaded for the call) / of two resident densities on one device; blocking. */
int kdehip_inters_intg_appx_is(const kdehip_density *p, const kdehip_density *q, int64_t Ngrid, double *out, int device);
int kdehip_inters_intg_appx_is_device(const kdehip_device_density *p, const kdehip_device_density *q, int64_t Ngrid,
                                      double *out);

/* ---- (5e) circular dimensions in the summaries, marginal, sample and resample ----------------------------------------------
 * The entries of 5c and 2f with the per-dimension enum of "manifolds" (KDEHIP_MANIFOLD_EUCLIDEAN / KDEHIP_MANIFOLD_CIRCULAR,
 * ndims bytes or NULL).  The reference threads addop / diffop through getKDERange, getKDERangeLinspace, getKDEMax and
 * intersIntgAppxIS (src/DualTree01.jl:512-618) and leaves getKDEMean / getKDEfit with a "TODO: update for on-manifold"; as with
 * the sampler's circular mode the semantic here is this library's own, on the convention of 5d: wrap() (csrc/circ_wrap.hpp) to
 * [-pi, pi), tangent space at a reference angle.  For a circular dimension k of a density with points x_j in original order
 * the reference angle is a0 = x_1k (ORIGINAL point 1) and the tangent offsets are t_j = wrap(x_jk - a0).  pi and 2 pi are
 * circ_wrap's constants; every operation below is rounded on its own.
 *   getKDEMean         mu_k = wrap(a0 + s / N), s = the sequential left-to-right fp64 sum of the t_j in original order from
 *                      +0.0; unweighted, as the reference's mean.  Euclidean dimensions keep the bits of 5c.  Bit for bit.
 *   getKDEfit          the mean above; covariance (1/N) sum_j r_j r_j^T with r_jk = wrap(x_jk - mu_k) in a circular dimension
 *                      and x_jk - mu_k otherwise, each entry a sequential sum in original order, then / N.
 *   getKDERange(extend) lo_t = min_j t_j, hi_t = max_j t_j, dr = extend * (hi_t - lo_t), alo = a0 + lo_t, ahi = a0 + hi_t,
 *                      range = (alo - dr, ahi + dr), left UNWRAPPED so that grid() stays a monotone linspace; if
 *                      (ahi + dr) - (alo - dr) > 2 pi the range is (mid - pi, mid + pi) with mid = 0.5 * (alo + ahi), the
 *                      midpoint of the unextended arc.  This is the arc through the data as seen from point 1, not the
 *                      shortest arc.  Bit for bit.
 *   grid values, getKDEMax  the 1-D marginal over [k] on grid(range) with every difference x - c_i wrapped before it is
 *                      squared; otherwise exactly as 5c: same weights, variance fl(sqrt(v_1))^2, norm (a circular density keeps
 *                      the Gaussian constant), leaf groups and exp.  argmax = wrap(x_k) of the first maximal k; d_values keeps
 *                      its meaning (the values at the unwrapped grid points).
 *   intersIntgAppxIS   D = 1, 2: the grids from p's circular range with extend 0.3, dx_d = x_1 - x_0, p and q evaluated by the
 *                      kernels of kdehip_evaluate_manifold (every value bit for bit what that entry returns there), the sums
 *                      of 5c.
 *   marginal(p, dims)  the tree of the result is built with tree_manifold (nsel bytes: the caller passes the operators of the
 *                      SELECTED dimensions, tree_manifold[dims]) by kdehip_make_density_tree; points, weights and the
 *                      fl(sqrt(v))^2 bandwidth are those of 5c.
 *   sample / rand      the Euclidean draw c + bw z of 2f, then wrap() in the circular dimensions: a circular coordinate is bit
 *                      for bit circ_wrap of the value the Euclidean call returns; labels and Euclidean dimensions keep theirs.
 *   resample           the wrapped draw, then kde!(pts, addop, diffop): kdehip_density_from_device_points_tree with `manifold`
 *                      (the bandwidth search) and `tree_manifold` (the builder), without leaving HBM.
 * Inputs need not lie in [-pi, pi).  fp64 only.  manifold == NULL or all zeros returns the bits of the entries of 5c / 2f
 * (which forward here with NULL); a byte above 1 is KDEHIP_ERR_ARG, checked before any device is touched.  Not here: weighted
 * circular means, a largest-gap range.
 * The batches take the manifold per item as a mask (bit d = dimension d circular; a bit at or above the item's ndims is
 * KDEHIP_ERR_ARG), as kdehip_eval_avg_logl_device_batch_manifold does.  Euclidean and circular items of any D may be mixed:
 * items with a circular bit run the circular instantiation of each kernel, the others the launches of
 * kdehip_summary_device_batch / kdehip_sample_device_batch; every item's result is bit for bit what it gets alone. */
typedef struct kdehip_summary_manifold_item {
  kdehip_summary_item item;
  uint32_t circular_mask;
  uint32_t reserved_;
} kdehip_summary_manifold_item;
int kdehip_summary_device_batch_manifold(int n, const kdehip_summary_manifold_item *items, void *stream);
int kdehip_density_summary_manifold(const kdehip_device_density *p, const double *extend, int64_t Ngrid, double *range,
                                    double *mean, double *cov, double *argmax, double *values,
                                    const uint8_t *manifold /* ndims bytes or NULL */);
int kdehip_kde_max_manifold(const kdehip_density *p, int64_t Ngrid, double *out, double *grid_values, int device,
                            const uint8_t *manifold);
int kdehip_inters_intg_appx_is_manifold(const kdehip_density *p, const kdehip_density *q, int64_t Ngrid, double *out,
                                        int device, const uint8_t *manifold);
int kdehip_inters_intg_appx_is_device_manifold(const kdehip_device_density *p, const kdehip_device_density *q, int64_t Ngrid,
                                               double *out, const uint8_t *manifold);
int kdehip_density_marginal_device_tree(kdehip_device_density **out, const kdehip_device_density *p, int nsel,
                                        const int32_t *dims, const uint8_t *tree_manifold /* nsel bytes or NULL */);
int kdehip_sample_manifold(const kdehip_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset, const int64_t *ind_in,
                           double *pts, int64_t *ind, int device, const uint8_t *manifold);
int kdehip_sample_device_manifold(kdehip_device_density *p, int64_t Npts, uint64_t seed, int64_t sample_offset,
                                  const int64_t *d_ind_in, double *d_pts, int64_t *d_ind, void *stream,
                                  const uint8_t *manifold);
typedef struct kdehip_sample_manifold_item {
  kdehip_sample_item item;
  uint32_t circular_mask;
  uint32_t reserved_;
} kdehip_sample_manifold_item;
int kdehip_sample_device_batch_manifold(int n, const kdehip_sample_manifold_item *items, void *stream);
int kdehip_resample_device_manifold(kdehip_device_density **out, kdehip_device_density *p, int64_t Np, uint64_t seed,
                                    double *bw_out, int32_t *nevals, const uint8_t *manifold /* ndims bytes or NULL */,
                                    const uint8_t *tree_manifold /* ndims bytes or NULL */);

/* ---- (5f) log-domain evaluation: evaluate_log, log-domain evalAvgLogL / entropy / kld / minkld ----------------------------
 * The entries of 5 / 5b / 5d form p(x) = sum_i w_i exp(a_i) / norm in the linear domain, as the reference does: once every
 * a_i is below about -745 (a query some 38 standard deviations from the nearest kernel) p is exactly 0, evalAvgLogL is -Inf
 * and kld is +-Inf or NaN.  Those entries keep that behaviour, bit for bit.  The entries below return log p(x) itself, by
 * log-sum-exp in the evaluation kernel, and the log-likelihoods built on it; they are this library's own, the reference has
 * no counterpart.  Semantic, for a density bd with leaves i, weights w_i and ONE bandwidth vector v_k (section 5), a query x
 * and a per-dimension `manifold` as in 5d (NULL = Euclidean; no Euclidean twins):
 *   a_i     = sum_k d_ik^2 * (-0.5 / v_k), d_ik = x_k - c_ik, through wrap() first in a circular dimension: the expression,
 *             fma order and -0.5 / v_k of the direct kernel
 *   S       = { i : w_i > 0 } (leave-one-out: and i != q).  A leaf of weight zero takes no part in the maximum: a near,
 *             weightless point would otherwise push every real term into underflow
 *   m       = max_{i in S} a_i
 *   log p   = m + log( sum_{i in S} w_i exp(a_i - m) ) - log(norm)   [- log(1 - w_q) for leave-one-out],
 *             norm = (2 pi)^(D/2) * prod_k sqrt(v_k) as in section 5; S empty gives -Inf
 *   evalAvgLogL(bd, at) = sum over { q : W_q != 0 } of W_q * log p(x_q), in the block order and the fixed 256-wide tree of
 *             5b; -Inf only if some such log p is -Inf
 *   entropy, kld, minkld: the compositions of 5b, leave_one_out exactly where the arguments are the same object.
 * The sum is split as in 5b: consecutive 128-leaf chunks in groups that depend on (N, Nq) alone; a group carries (m, s), the
 * carried s rescaled by exp(m_old - m_new) once per chunk, and the groups are combined in group order with M = max m_g,
 * sum_g s_g exp(m_g - M).  So the host entry, a single resident call and any batch return the same bits, run after run.
 * Where nothing underflows log p agrees with log of the direct entry to rounding (1e-12 relative), not bit for bit.
 * Arguments: those of 5 / 5b / 5d, checked before a device is touched -- NULLs (KDEHIP_ERR_ARG), ndims mismatch
 * (KDEHIP_ERR_DIM_MISMATCH), D above KDEHIP_MAX_DIMS or per-point bandwidths (KDEHIP_ERR_UNSUPPORTED), a manifold byte above
 * 1 or a mask bit at or beyond ndims in a batch (KDEHIP_ERR_ARG).  fp64 only. */
/* Host arrays, blocking: logp_out as p_out of kdehip_evaluate (leave_one_out: npts values in the ORIGINAL point order). */
int kdehip_evaluate_log(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, double *logp_out,
                        int device, const uint8_t *manifold);
/* Resident, enqueue only on `stream`: as kdehip_evaluate_device / kdehip_evaluate_device_at (original point order of `at`,
 * leave-one-out when at == bd). */
int kdehip_evaluate_log_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int leave_one_out,
                               double *d_out, void *stream, const uint8_t *manifold);
int kdehip_evaluate_log_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, double *d_out,
                                  void *stream, const uint8_t *manifold);
/* Log-domain evalAvgLogL: host arrays; resident and blocking; resident batch, enqueue only (every item log-domain, Euclidean
 * and circular items of any D mixed, each result bit for bit the single call's). */
int kdehip_eval_avg_logl_log(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, double *out, int device,
                             const uint8_t *manifold);
int kdehip_eval_avg_logl_log_device(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                    double *out, const uint8_t *manifold);
int kdehip_eval_avg_logl_log_device_batch(int n, const kdehip_logl_manifold_item *items, double *d_out, void *stream);

/* ---- (5g) exact overlap measures by kernel sums: intersIntg, ise, mmd ------------------------------------------------------
 * How far apart are two densities?  The log-likelihoods of 5b / 5f are asymmetric, not 0 at p == q and depend on both LOOCV
 * bandwidths; intersIntgAppxIS (5c) is a grid sum in 1-D and 2-D.  For Gaussian-kernel mixtures the quantities have closed
 * forms in any dimension, all of them compositions of ONE primitive, a weighted all-pairs Gaussian sum reduced to a scalar
 * (csrc/ksum.hip; this library's own, the reference has no counterpart):
 *   S(A, B; v) = sum_{j<M} b_j sum_{i<N} a_i exp(-1/2 sum_k diff_k(y_jk, x_ik)^2 / v_k)
 * with A = (x_i, a_i) and B = (y_j, b_j) the leaf points and leaf weights of the densities a and b, v a variance vector and
 * diff_k the plain difference y_jk - x_ik, through wrap() first in a circular dimension (5d).  With normalize != 0 the sum is
 * divided by prod_k sqrt(2 pi v_k): multiplied by 1 / ((2 pi)^(D/2) * prod_k sqrt(v_k)), the product over k ascending.
 *   integral p q      = S(p, q; v_p + v_q), normalised                       (`intersIntg`: exact, any D <= KDEHIP_MAX_DIMS)
 *   integral (p-q)^2  = intersIntg(p,p) - 2 intersIntg(p,q) + intersIntg(q,q)   (`ise`: symmetric, 0 iff p == q)
 *   MMD^2(p, q; h)    = S(p,p;h^2) - 2 S(p,q;h^2) + S(q,q;h^2)                  (`mmd`: biased, kernel exp(-|x-y|^2 / 2h^2))
 * var: D explicit variances (a HOST pointer in every entry, the batch items included), or NULL = the sum of the two
 * densities' leaf variances, a's first leaf's plus b's, added in the kernel.  NULL needs densities whose leaves share one
 * bandwidth vector (KDEHIP_ERR_UNSUPPORTED otherwise, as kdehip_evaluate); with explicit variances only points and weights
 * are read, so per-point bandwidths are fine.
 * The full square is summed: no leave-one-out and no shortcut for a == b, so S(p, p) and S(p, an equal copy of p) are the same
 * bits and ise(p, p) and mmd(p, p, h) are exactly 0.  Cost: one all-pairs pass, as one kdehip_evaluate of a at b's points.
 * Arithmetic: the exponent, its fma order, -0.5 / v_k and the exponential are those of kdehip_evaluate; lane j multiplies its
 * sum over a's leaves by b_j, the 256 lanes of a block are added in a fixed tree, and the blocks in block order.  The split of
 * the sum depends on the pair's (N, M) alone: each result is the same bits from the host entry, a single device call and any
 * batch, run after run.  S(a, b) and S(b, a) are sums in different orders: equal to rounding, not bit for bit.
 * Circular dimensions (5d): circular data in which no pair difference leaves [-pi, pi) gives the Euclidean call's bits; a
 * circular dimension keeps the Gaussian constant when normalised, as evaluation does -- the library's nearest-image
 * semantic, the one kdehip_evaluate_manifold uses (the integral over the circle of two wrapped Gaussians it is not).
 * Errors, all checked before any device is touched: ndims differ -- KDEHIP_ERR_DIM_MISMATCH; D above KDEHIP_MAX_DIMS, or
 * var == NULL with per-point bandwidths on either side -- KDEHIP_ERR_UNSUPPORTED; a variance that is not finite or not > 0, a
 * manifold byte above 1 or a mask bit at or above D, a null density or output, densities on different devices within one
 * batch -- KDEHIP_ERR_ARG. */
typedef struct kdehip_ksum_item {
  const kdehip_device_density *a, *b;
  const double *var;        /* HOST pointer, D variances, each finite and > 0; NULL = a's leaf variances + b's */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
  int32_t normalize;        /* != 0: divide by prod_k sqrt(2 pi v_k) */
} kdehip_ksum_item;
/* Resident densities, all on one device: d_out[i] (device, n doubles) = S of item i.  One partial-sum launch per distinct D
 * (one more for its circular items) and one reduction launch for all items; Euclidean and circular items of any D may be
 * mixed.  The variances are copied during the call.  Enqueue only, on `stream` (hipStream_t, NULL = the null stream). */
int kdehip_kernel_sum_device_batch(int n, const kdehip_ksum_item *items, double *d_out, void *stream);
/* One resident pair, blocking on the calling thread's stream; the result to host memory.  manifold: ndims bytes or NULL. */
int kdehip_kernel_sum_device(const kdehip_device_density *a, const kdehip_device_density *b, const double *var,
                             int normalize, double *out, const uint8_t *manifold);
/* Host densities, one pinned upload, blocking, on hipStreamPerThread. */
int kdehip_kernel_sum(const kdehip_density *a, const kdehip_density *b, const double *var, int normalize,
                      double *out, int device, const uint8_t *manifold);

/* ---- (5h) the gradient of the density and its joint modes by mean shift ---------------------------------------------------
 * Where is a belief, jointly?  getKDEMax (5c) is the reference's answer: the grid argmax of every 1-D marginal, taken
 * independently -- for a multimodal density a point that may belong to no mode; getKDEMean / getKDEfit are moments.  The
 * entries below give the gradient of (log) p and the fixed points of the mean-shift iteration, the joint modes
 * (csrc/modes.hip; this library's own, the reference has no counterpart).  For a density bd with leaves i, weights w_i and
 * ONE bandwidth vector v_k (section 5), a query x and a per-dimension `manifold` as in 5d (NULL = Euclidean):
 *   d_ik    = x_k - c_ik, through wrap() first in a circular dimension
 *   a_i     = sum_k d_ik^2 * (-0.5 / v_k): the expression and fma order of the direct kernel
 *   S       = { i : w_i > 0 }, m = max_{i in S} a_i (the rule of 5f: a weightless leaf neither sets the maximum nor adds)
 *   S_0     = sum_{i in S} w_i exp(a_i - m),  S_k = sum_{i in S} w_i exp(a_i - m) d_ik
 *   log p   = m + log S_0 - log norm,  p = exp(m) S_0 / norm,  norm = (2 pi)^(D/2) prod_k sqrt(v_k) as in section 5
 *   grad log p (x)_k = -S_k / (S_0 v_k),  grad p = p * grad log p
 *   the mean-shift step: x_k <- x_k - S_k / S_0, through wrap() in a circular dimension.
 * S empty: log p = -Inf, p = 0 and the gradient is 0; such a start does not move (0 steps).  The ratio S_k / S_0 is formed
 * from sums scaled by exp(-m), so it is defined wherever some a_i is finite -- far beyond where p underflows.
 * The sum is split as in 5b / 5f: consecutive 128-leaf chunks in groups that depend on (npts, Nq) alone; a group carries
 * (m, s_0, .., s_D), rescaled by exp(m_old - m_new) once per chunk, and the groups are combined in group order with
 * M = max m_g, sum_g s_jg exp(m_g - M).  No atomics.  So the host entry, a resident call and any batch return the same bits,
 * run after run; a start's trajectory depends on the density, the start, tol and that split alone -- not on what else is in
 * the call, nor on how the sweeps are grouped between the host's checks.
 * Mean shift: every start takes steps until max_k |S_k / S_0| / sqrt(v_k) <= tol (the step just taken is the last: the
 * point is frozen and never written again) or until it has taken maxiter steps.  iters[q] = the steps taken, negative when
 * the last of them was still above tol; logp[q] = log p at the returned x[q], from one closing evaluation.  Query blocks
 * (256 starts) whose starts are all frozen cost nothing in later sweeps.
 * Not here: leave-one-out gradients, per-point bandwidths, kernels other than the Gaussian.
 * Errors, all checked before any device is touched: null arguments (val and grad both NULL included), Nq / nstart < 0,
 * start == NULL with nstart != npts, tol negative or not finite, maxiter / niter < 0, a manifold byte above 1 or a mask bit
 * at or above D, densities on different devices within one batch -- KDEHIP_ERR_ARG; D outside 1..KDEHIP_MAX_DIMS or per-point
 * bandwidths -- KDEHIP_ERR_UNSUPPORTED.  Nq == 0, n == 0 and maxiter == 0 are KDEHIP_OK (maxiter == 0: the starts and their
 * log p).  fp64 only. */
/* Host density, blocking: pos as kdehip_evaluate takes it (Nq points, D values each); val [Nq] (log p, or p with
 * log_domain == 0) or NULL; grad [Nq][D] (of log p, or of p with log_domain == 0) or NULL. */
int kdehip_evaluate_grad(const kdehip_density *bd, const double *pos, int64_t Nq, int log_domain, double *val, double *grad,
                         int device, const uint8_t *manifold);
/* Resident density, device arrays, enqueue only on `stream`. */
int kdehip_evaluate_grad_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int log_domain,
                                double *d_val, double *d_grad, const uint8_t *manifold, void *stream);
/* tol is a HOST pointer to ONE value in every entry (this ABI passes integers and pointers only, so that every binding of it
 * can be checked against this header type by type); NULL is KDEHIP_ERR_ARG.
 * Host density, blocking.  start: nstart points, or NULL = the density's own points in their ORIGINAL order (nstart must be
 * npts).  x [nstart][D], logp [nstart], iters [nstart]: host arrays.  The sweeps run in rounds with one read of the number
 * of live starts between them; the round length changes no bit of the result. */
int kdehip_meanshift(const kdehip_density *bd, const double *start, int64_t nstart, const double *tol, int maxiter, double *x,
                     double *logp, int32_t *iters, int device, const uint8_t *manifold);
/* The same for a resident density: d_start a device array or NULL, the results to HOST arrays; blocking. */
int kdehip_meanshift_device(const kdehip_device_density *bd, const double *d_start, int64_t nstart, const double *tol,
                            int maxiter, double *x, double *logp, int32_t *iters, const uint8_t *manifold);
typedef struct kdehip_meanshift_item {
  const kdehip_device_density *bd;
  const double *d_start;    /* device, [nstart][D], or NULL = bd's own points in original order (nstart == npts) */
  int64_t nstart;
  double *d_x;              /* device, [nstart][D]; may be d_start */
  double *d_logp;           /* device, [nstart] */
  int32_t *d_iters;         /* device, [nstart] */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
  uint32_t reserved_;
} kdehip_meanshift_item;
/* Resident densities, all on one device.  Enqueue only on `stream`: exactly niter step sweeps and the closing evaluation,
 * one launch per distinct (D, circular) per sweep for all items together, and no read-back -- so the call can be captured
 * in a HIP graph.  The descriptor and scratch blocks of a captured call (a device and a pinned block, some tens of KB plus
 * (D + 2) * groups * nstart doubles per item) are kept until kdehip_clear_cache, because the graph's nodes use them at every
 * replay: every capture adds a pair, so capture once and replay, and kdehip_clear_cache INVALIDATES every graph captured
 * from this entry -- destroy those graphs first, or do not replay them afterwards.  Every item's results are bit for bit
 * those of kdehip_meanshift_device with maxiter == niter. */
int kdehip_meanshift_device_batch(int n, const kdehip_meanshift_item *items, const double *tol, int niter, void *stream);

/* ---- (5i) conditioning a density on some of its dimensions: weights, moments and draws ------------------------------------
 * What does a joint belief say about these coordinates, given those?  `marginal` (5c) drops dimensions; the entries below
 * fix them (csrc/conditional.hip; this library's own, the reference has no counterpart).  For a density bd of dimension D
 * with leaves i in LEAF ORDER, centres c_i, weights w_i and ONE bandwidth vector v (the rule of section 5):
 *   given_mask  bit d set = dimension d is given.  G = the given dimensions, ascending, ng = |G|; F = the others, ascending,
 *               nf = D - ng.  Required: 1 <= ng <= D - 1 and no bit at or above D, otherwise KDEHIP_ERR_ARG -- in particular
 *               a 1-D density can never be conditioned.
 *   a query     y[q]: ng values in the order of G.  `manifold` as in 5d (NULL = Euclidean).
 * Per query:
 *   d_ik    = y_k - c_ik (k in G), through wrap() first in a circular dimension
 *   a_i     = sum_{k in G, ascending} d_ik^2 * (-0.5 / v_k): the expression and fma order of the direct kernel
 *   S       = { i : w_i > 0 },  m = max_{i in S} a_i,  t_i = w_i exp(a_i - m),  S_0 = sum_{i in S} t_i
 *   logz    = m + log S_0 - log((2 pi)^(ng/2) prod_{k in G} sqrt(v_k))     (= the log of the G-marginal at y)
 *   omega_i = t_i / S_0                                                    (0 outside S)
 *   mean_k  = sum_{i in S} omega_i c_ik                                    (k in F)
 *   var_k   = v_k + sum_{i in S} omega_i (c_ik - mean_k)^2                 (k in F; the diagonal only; never below v_k)
 * Moments: the first and second moments of c_ik - r_k about ONE fixed reference point r inside the data's hull (the root
 * node's mean) are accumulated in one pass beside S_0; mean_k = r_k + S1_k / S_0 and the excess S2_k / S_0 - (S1_k / S_0)^2
 * is clamped at 0.  Consequence: var_k is accurate to an absolute error proportional to R_k^2, R_k the data's range in
 * dimension k -- a conditional far narrower than the data loses relative digits.  When mean or var is asked for while a FREE
 * dimension is circular the call returns KDEHIP_ERR_UNSUPPORTED; circular GIVEN dimensions are fully supported (wrapped
 * differences).
 * The draw (ONE per query): the global index is g = sample_offset + q and the random numbers are those kdehip_sample (2f)
 * uses for index g of an nf-dimensional density, u = kdehip_philox_fill_uniform(seed, g, 1, K = 1) and
 * n[j] = kdehip_philox_fill_normal(seed, g, 1, R = nf)[j].  With C_i = sum_{j <= i, j in S} t_j in leaf order the label is
 * the first i in S with C_i > u * S_0; if rounding leaves none, the last leaf of S.  ind[q] = the 1-based ORIGINAL index of
 * that leaf (through the permutation); pts[q][j] = c_{i,F_j} + sqrt(v_{F_j}) * n[j], the multiply and the add rounded
 * separately as in 2f, wrapped to [-pi, pi) where F_j is circular.
 * The C_i are defined in exact arithmetic.  The implementation forms them in the group split of 5b / 5f / 5h, so a u * S_0
 * within a relative 1e-9 of some C_i may resolve to the neighbouring leaf of S.  Everything else about the label is exact,
 * and host, resident and batched calls return the same bits run after run.
 * S empty: logz = -Inf, mean and var are NaN, ind = 0 and the point is NaN.  No entry reads out of bounds.
 * The sum is split as in 5b / 5f / 5h (128-leaf chunks in groups that depend on (npts, Nq) alone, combined in group order);
 * no atomics; a full call evaluates at most two exp per (query, leaf) pair: one sweep for (m, S_0, moments), one -- only
 * in the (256-query block, group) pairs some query's draw fell into -- for the label.
 * Errors, all checked before any device is touched: null arguments (all outputs NULL included; pts and ind are given
 * together or not at all), Nq < 0, a bad given_mask, a manifold byte above 1 or a circular_mask bit at or above D,
 * densities on different devices within a batch -- KDEHIP_ERR_ARG; D outside 1..KDEHIP_MAX_DIMS, per-point bandwidths, or
 * moments over a circular free dimension -- KDEHIP_ERR_UNSUPPORTED.  Nq == 0 and n == 0 are KDEHIP_OK.  fp64 only.
 * Not here: the full conditional covariance, moments on circular free dimensions, more than one draw per query (use
 * kdehip_density_condition_device / `condition`, then sample), per-point bandwidths, kernels other than the Gaussian. */
/* Host density, host arrays, blocking.  given [Nq][ng]; logz [Nq], mean / var [Nq][nf], pts [Nq][nf] with ind [Nq]: any may
 * be NULL (not all; pts and ind together). */
int kdehip_conditional(const kdehip_density *bd, uint32_t given_mask, const double *given, int64_t Nq, uint64_t seed,
                       int64_t sample_offset, double *logz, double *mean, double *var, double *pts, int64_t *ind, int device,
                       const uint8_t *manifold);
/* Resident density, device arrays, enqueue only on `stream` (hipStream_t, NULL = the null stream). */
int kdehip_conditional_device(const kdehip_device_density *bd, uint32_t given_mask, const double *d_given, int64_t Nq,
                              uint64_t seed, int64_t sample_offset, double *d_logz, double *d_mean, double *d_var,
                              double *d_pts, int64_t *d_ind, const uint8_t *manifold, void *stream);
typedef struct kdehip_conditional_item {
  const kdehip_device_density *bd;
  const double *d_given;    /* device, [Nq][ng] */
  int64_t Nq;
  uint64_t seed;
  int64_t sample_offset;
  double *d_logz;           /* device, [Nq], or NULL */
  double *d_mean;           /* device, [Nq][nf], or NULL */
  double *d_var;            /* device, [Nq][nf], or NULL */
  double *d_pts;            /* device, [Nq][nf], or NULL (then d_ind is NULL too) */
  int64_t *d_ind;           /* device, [Nq] */
  uint32_t given_mask;      /* bit d = dimension d is given */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
} kdehip_conditional_item;
/* Many resident items (mixed D, N, Nq and masks) on one device, enqueue only on `stream`.  Launches per pass are one per
 * distinct (D, circular) for all items together.  Every item's results are bit for bit those of kdehip_conditional_device. */
int kdehip_conditional_device_batch(int n, const kdehip_conditional_item *items, void *stream);
/* The weights themselves: w_out[q][o] = omega of ORIGINAL point o, o = 0..npts-1 (what kde(points[F], ks[F], w) takes);
 * logz [Nq] or NULL.  Host density, blocking. */
int kdehip_condition_weights(const kdehip_density *bd, uint32_t given_mask, const double *given, int64_t Nq, double *w_out,
                             double *logz, int device, const uint8_t *manifold);
/* Resident density, device arrays, enqueue only on `stream`. */
int kdehip_condition_weights_device(const kdehip_device_density *bd, uint32_t given_mask, const double *d_given, int64_t Nq,
                                    double *d_w_out, double *d_logz, const uint8_t *manifold, void *stream);
/* p(x_F | x_G = y) as a resident density, by the route of kdehip_density_marginal_device (5c): F and the weights omega
 * gathered on the device, one copy down, the host builder with ks = the bandwidth of ORIGINAL point 0 in F (marginal's rule)
 * and those weights, the block back up.  Blocking, on the calling thread's stream.  y: a HOST array of ng doubles;
 * tree_manifold: nf bytes (the operators of the result's tree, 5e) or NULL.  logz = -Inf (no leaf in S) or NaN (a NaN in y) is
 * KDEHIP_ERR_ARG. */
int kdehip_density_condition_device(kdehip_device_density **out, const kdehip_device_density *p, uint32_t given_mask,
                                    const double *y, const uint8_t *manifold, const uint8_t *tree_manifold);

/* ---- (5j) non-finite positions from the caller ----------------------------------------------------------------------------
 * For the entries that take an array of positions -- kdehip_evaluate[_manifold] and kdehip_evaluate_log with pos,
 * kdehip_evaluate_grad, kdehip_evaluate_hess (5k), kdehip_meanshift with start, kdehip_conditional, kdehip_condition_weights,
 * kdehip_density_condition_device, and the resident and batched forms of each:
 *   a NaN in any coordinate of a query (for the conditionals: in any given value) makes every floating-point output of THAT
 *   query NaN -- p, log p, every gradient component, logz, mean, var, the whole row of w_out, the drawn point -- with ind = 0;
 *   a mean-shift start with a NaN is returned as given with iters = 0 and logp = NaN, and never counts as live;
 *   kdehip_density_condition_device fails with KDEHIP_ERR_ARG.  No other query's outputs change by a bit.
 *   +-Inf in a coordinate is infinitely far from every leaf: p = 0, log p = logz = -Inf, and everything else as for "S empty"
 *   in 5h / 5i (gradient 0, the start returned with iters = 0, mean / var / the point NaN, ind = 0, the row of w_out all 0).
 * NaN or Inf INSIDE a density (points, weights, bandwidths) is outside this contract. */

/* ---- (5k) the curvature of the density: the Hessian of log p and a covariance for every mode -------------------------------
 * How wide is a mode?  getKDEfit (5c) is ONE moment-matched Gaussian for the whole density -- for a multimodal belief the
 * wrong width in the way getKDEMax is the wrong mode.  The entries below give the Hessian of log p at a query and, where it is
 * negative definite, the covariance of the Gaussian with that curvature (the Laplace approximation of the mode)
 * (csrc/modes.hip; this library's own, the reference has no counterpart).  With d_ik, a_i, S, m, S_0 and S_k exactly as in 5h
 * and t_i = w_i exp(a_i - m):
 *   S_kl  = sum_{i in S} t_i d_ik d_il                                 (k <= l: D (D + 1) / 2 sums)
 *   g_k   = -S_k / (S_0 v_k)                                           (the gradient of log p, as 5h)
 *   H_kl  = S_kl / (S_0 v_k v_l) - delta_kl / v_k - g_k g_l            (the Hessian of log p at x)
 * Equivalently -H = V^-1 - V^-1 C V^-1 with V = diag(v) and C the covariance of the differences d_i under the
 * responsibilities t_i / S_0: C is positive semidefinite, so wherever -H is definite (-H)^-1 - V is positive semidefinite --
 * a mode is never narrower than the kernel.
 * Covariance: cov = (-H)^-1 from a Cholesky factorisation of -H.  If every pivot is finite and > 0, definite = 1; otherwise
 * definite = 0 and all D x D entries of cov are NaN -- the query sits at a saddle, a minimum or in a flat direction, not at a
 * maximum.
 * Layout: hess and cov are [Nq][D][D], the full matrix; both triangles are stored from the one computed value, so the matrices
 * are symmetric bit for bit.  logp is [Nq], grad [Nq][D], definite [Nq] int32.
 * S empty: logp = -Inf, grad = 0, hess = 0, definite = 0, cov = NaN.  A query with a NaN coordinate (5j): NaN in every
 * floating-point output of that query and definite = 0.  In a circular dimension d_ik is wrapped and H is the Hessian of that
 * expression (as the gradient of 5h is its gradient): exact wherever no difference that carries weight sits on the cut.
 * The sum is split as in 5h: consecutive 128-leaf chunks in groups that depend on (npts, Nq) alone; a group carries
 * (m, s_0, s_k, s_kl), rescaled by exp(m_old - m_new) once per chunk; within a chunk t_i, d_ik t_i and (d_ik t_i) d_il are
 * summed from 0 in leaf order (one fma each for s_k and s_kl) and the chunk's sums are then added to the carried ones; the
 * groups are combined in group order with M = max m_g, sum_g s_jg exp(m_g - M).  No atomics.  Then, per query,
 *   g_k = -S_k / (S_0 v_k);  H_kl = fma(-g_k, g_l, S_kl / ((S_0 v_k) v_l) [- 1 / v_k when k == l])            (k <= l)
 *   -H = L L^T column by column: pivot_j = -H_jj - sum_{i<j} L_ji^2 (i ascending, one fma each), L_jj = sqrt(pivot_j),
 *   L_rj = (-H_rj - sum_{i<j} L_ri L_ji) / L_jj;  R = L^-1 by forward substitution;  cov_kl = sum_{r >= l} R_rk R_rl (k <= l).
 * So the host entry, a resident call and any batch return the same bits, run after run.  Bit equality of logp and grad with
 * kdehip_evaluate_grad is NOT promised: it is another kernel.
 * Cancellation: at a mode of data spread sigma under a bandwidth h << sigma, H_kk is the difference of two terms of size
 * 1 / h^2 whose result is about 1 / (sigma^2 + h^2): roughly log10(sigma^2 / h^2) digits are lost.  Harmless in fp64 for any
 * bandwidth the LOOCV search returns; it is why there is no fp32 variant.
 * Only the Hessian of log p crosses the ABI (that of p is p (H + g g^T)).  fp64 only.
 * Errors, all checked before any device is touched: null arguments (every output NULL included), Nq < 0, a manifold byte
 * above 1 or a mask bit at or above D, densities on different devices within one batch -- KDEHIP_ERR_ARG; D outside
 * 1..KDEHIP_MAX_DIMS or per-point bandwidths -- KDEHIP_ERR_UNSUPPORTED.  Nq == 0 and n == 0 are KDEHIP_OK.
 * Not here: leave-one-out curvature, per-point bandwidths, kernels other than the Gaussian, fp32. */
/* Host density, blocking: pos as kdehip_evaluate takes it.  Any output may be NULL, but not all of them. */
int kdehip_evaluate_hess(const kdehip_density *bd, const double *pos, int64_t Nq, double *logp, double *grad, double *hess,
                         double *cov, int32_t *definite, int device, const uint8_t *manifold);
/* Resident density, device arrays, enqueue only on `stream`. */
int kdehip_evaluate_hess_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, double *d_logp, double *d_grad,
                                double *d_hess, double *d_cov, int32_t *d_definite, const uint8_t *manifold, void *stream);
typedef struct kdehip_hess_item {
  const kdehip_device_density *bd;
  const double *d_pos;      /* device, [Nq][D] */
  int64_t Nq;
  double *d_logp;           /* device, [Nq], or NULL */
  double *d_grad;           /* device, [Nq][D], or NULL */
  double *d_hess;           /* device, [Nq][D][D], or NULL */
  double *d_cov;            /* device, [Nq][D][D], or NULL */
  int32_t *d_definite;      /* device, [Nq], or NULL (not all five NULL) */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
  uint32_t reserved_;
} kdehip_hess_item;
/* Resident densities (mixed D, N and Nq), all on one device.  Enqueue only on `stream`: one partial launch per distinct
 * (D, circular) and ONE finish launch for all items together, and no read-back -- so the call can be captured in a HIP graph,
 * under the rules of kdehip_meanshift_device_batch (5h): the blocks of a captured call ((2 + D + D (D + 1) / 2) * groups * Nq
 * doubles of scratch per item) are kept until kdehip_clear_cache, which INVALIDATES every graph captured from this entry.
 * Every item's results are bit for bit those of kdehip_evaluate_hess_device. */
int kdehip_evaluate_hess_device_batch(int n, const kdehip_hess_item *items, void *stream);

/* ---- (5l) the probability mass of a density: box mass, marginal cdf and quantiles ------------------------------------------
 * How much of a belief lies somewhere?  getKDERange (5c) is a support box, not a probability.  For a Gaussian-kernel density
 * with ONE bandwidth vector the mass of an axis-aligned box and the quantiles of a marginal have exact expressions; the entries
 * below evaluate them (csrc/mass.hip; this library's own, the reference has no counterpart).  The density bd has dimension D,
 * leaves i in LEAF ORDER, centres c_i, weights w_i and ONE bandwidth vector v (the rule of section 5: per-point bandwidths
 * are KDEHIP_ERR_UNSUPPORTED, in evaluate's words).
 *   dim_mask    (64 bits wide) bit d set = dimension d is bounded.  B = the bounded dimensions, ascending, nb = |B|.  Required:
 *               1 <= nb <= D and no bit at or above D, otherwise KDEHIP_ERR_ARG.  An unbounded dimension contributes the
 *               factor 1 and is never read.
 *   a query     lo[q], hi[q]: nb values each, in the order of B.  -Inf and +Inf are bounds like any other.
 * Box mass.  For k in B, s_k = 1.0 / sqrt(2 v_k), the root and the division correctly rounded, formed once and not per pair.
 * For a pair (q, i) and k in B, with a = (lo_k - c_ik) * s_k and b = (hi_k - c_ik) * s_k (difference, then product):
 *   f_ik = 0                                  if !(a < b)    (empty or degenerate; also what a NaN gives inside the sweep)
 *        = (erfc(a) - erfc(b)) / 2            if a >= 0      (the box lies right of the centre)
 *        = (erfc(-b) - erfc(-a)) / 2          if b <= 0      (left of it)
 *        = 1 - (erfc(-a) + erfc(b)) / 2       otherwise      (it holds the centre)
 *   mass[q] = sum_i w_i prod_{k in B, ascending} f_ik
 * The three forms keep every difference in the tail where it is relatively accurate (the cdf form Phi(b) - Phi(a) loses all
 * digits beyond 8 bandwidths on the right); they are part of the contract so that a model and the device share the formula.
 * erfc is the device library's; its error, measured against the host libm's erfc over [0, 26], is in DESIGN.md section
 * 24.  A leaf with w_i == 0 adds nothing.  A NaN in any bound of a query makes mass[q] NaN: the finish kernel asks this of the
 * bounds themselves, as 5j words it for positions; no other query changes by a bit.  lo_k >= hi_k in any bounded dimension
 * gives exactly 0.
 * The sum is split as in 5b / 5f / 5h: consecutive 128-leaf chunks in groups that depend on (npts, Nq) alone; within a
 * chunk w_i * (the product, k ascending from f_i,B_0) is summed from 0 in leaf order (a product, then a sum: no fma), the
 * chunk's sum is added to the group's, and the groups are combined in group order.  No atomics.  Host, resident and batched
 * calls return the same bits, run after run.
 * Quantile.  For ONE dimension k (0-based `dim`) the marginal cdf and pdf are
 *   F_k(x) = (sum_i w_i erfc(-t_i)) / 2,   f_k(x) = (sum_i w_i exp(-t_i^2)) * (s_k / sqrt(pi)),   t_i = (x - c_ik) * s_k
 * (F_k is the box mass with B = {k}, lo = -Inf, hi = x), and for a level alpha[q] in (0, 1) x[q] solves F_k(x) = alpha[q] by
 * a bracketed Newton iteration on the device:
 *   bracket     [xl, xh] = [cmin - 39 sigma_k, cmax + 39 sigma_k], sigma_k = sqrt(v_k), cmin and cmax over the leaves with
 *               w_i > 0: erfc(39 / sqrt 2) underflows, so F_k is exactly 0 at xl and exactly (sum_i w_i erfc(-t_i)) / 2 with
 *               every erfc equal to 2 -- the total weight -- at xh.
 *   iterate     the first x is 0.5 * (xl + xh).  After each evaluation r = F_k(x) - alpha: r < 0 moves xl to x, otherwise xh
 *               moves to x.  The next x is the Newton point x - r / f_k(x) if f_k(x) > 0, the point lies strictly inside
 *               (xl, xh) AND (the rtsafe rule) |2 r / f_k(x)| <= |the step before last|; otherwise it is xl + 0.5 * (xh - xl).
 *               "The step before last" is the distance moved two iterates ago, a bisection counting as half its bracket; for
 *               the first two decisions it is the width of the start bracket.  So a Newton step that no longer halves the
 *               step before last forces a bisection.
 *   stop        when |r| <= tol (converged = 1) or after max_iter evaluations (converged = 0).  tol (a HOST pointer to one
 *               double, as kdehip_meanshift takes its tol; NULL means the default) is absolute in F: *tol must be finite and
 *               >= 1e-14, and 0 means the default 1e-12; max_iter must be >= 1, and 0 means the default 100; anything else
 *               is KDEHIP_ERR_ARG.
 *   outputs     x [Nq]; optional (NULL to skip) resid [Nq] = F_k(x) - alpha at the returned x, iters [Nq] int32 = the number
 *               of evaluations, converged [Nq] int32.
 *   An alpha outside (0, 1) or NaN gives x = resid = NaN, iters = 0, converged = 0 for that level only; so does a density
 *   none of whose leaves has w_i > 0.
 * Order of the sums: lane t of the 256 adds its leaves i = t, t + 256, ... in that order (w_i * erfc(-t_i), w_i * exp(-t_i^2)),
 * the 256 partial sums are combined in a fixed halving tree.  Host, resident and batched calls therefore return the same bits.
 * `manifold` as in 5d.  A bounded dimension, or the quantile's dimension, that is circular is KDEHIP_ERR_UNSUPPORTED (the mass
 * of an arc needs the wrapped kernel); circular dimensions that are not bounded are fine: they contribute the factor 1.
 * The _device and _device_batch entries are enqueue-only: they do not synchronise the host, and a capture of ONE stream into a
 * HIP graph can hold them, under the rules of kdehip_meanshift_device_batch (5h): the blocks of a captured call are kept until
 * kdehip_clear_cache, which INVALIDATES every graph captured from these entries.
 * Errors, all checked before any device is touched: null arguments, Nq < 0, a bad dim_mask or dim, a manifold byte above 1 or
 * a circular_mask bit at or above D, a bad tol or max_iter, densities on different devices within one batch --
 * KDEHIP_ERR_ARG; D outside 1..KDEHIP_MAX_DIMS, per-point bandwidths, a circular bounded dimension or a circular quantile
 * dimension -- KDEHIP_ERR_UNSUPPORTED.  Nq == 0 and n == 0 are KDEHIP_OK.  fp64 only.
 * Not here: circular bounded dimensions, rotated boxes, joint multi-dimensional quantile regions, per-point bandwidths. */
/* Host density, host arrays, blocking.  lo, hi [Nq][nb]; mass [Nq]. */
int kdehip_box_mass(const kdehip_density *bd, uint64_t dim_mask, const double *lo, const double *hi, int64_t Nq, double *mass,
                    int device, const uint8_t *manifold);
/* Resident density, device arrays, enqueue only on `stream` (hipStream_t, NULL = the null stream). */
int kdehip_box_mass_device(const kdehip_device_density *bd, uint64_t dim_mask, const double *d_lo, const double *d_hi, int64_t Nq,
                           double *d_mass, const uint8_t *manifold, void *stream);
typedef struct kdehip_box_mass_item {
  const kdehip_device_density *bd;
  const double *d_lo;       /* device, [Nq][nb] */
  const double *d_hi;       /* device, [Nq][nb] */
  int64_t Nq;
  double *d_mass;           /* device, [Nq] */
  uint64_t dim_mask;        /* bit d = dimension d is bounded */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
  uint32_t reserved_;
} kdehip_box_mass_item;
/* Many resident items (mixed D, N, Nq and masks) on one device, enqueue only on `stream`: one sweep launch per distinct nb
 * and ONE finish launch for all items together.  Every item's results are bit for bit those of kdehip_box_mass_device. */
int kdehip_box_mass_device_batch(int n, const kdehip_box_mass_item *items, void *stream);
/* Host density, host arrays, blocking.  alpha [Nq]; x [Nq]; resid, iters, converged [Nq] or NULL. */
int kdehip_quantile(const kdehip_density *bd, int dim, const double *alpha, int64_t Nq, const double *tol, int max_iter, double *x,
                    double *resid, int32_t *iters, int32_t *converged, int device, const uint8_t *manifold);
/* Resident density, device arrays, enqueue only on `stream`. */
int kdehip_quantile_device(const kdehip_device_density *bd, int dim, const double *d_alpha, int64_t Nq, const double *tol,
                           int max_iter, double *d_x, double *d_resid, int32_t *d_iters, int32_t *d_converged, const uint8_t *manifold,
                           void *stream);
typedef struct kdehip_quantile_item {
  const kdehip_device_density *bd;
  const double *d_alpha;    /* device, [Nq] */
  int64_t Nq;
  double *d_x;              /* device, [Nq] */
  double *d_resid;          /* device, [Nq], or NULL */
  int32_t *d_iters;         /* device, [Nq], or NULL */
  int32_t *d_converged;     /* device, [Nq], or NULL */
  int32_t dim;              /* the marginal's dimension, 0-based */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
} kdehip_quantile_item;
/* Many resident items (mixed D, N, Nq and dimensions) on one device, enqueue only on `stream`: ONE launch for all levels of
 * all items.  Every item's results are bit for bit those of kdehip_quantile_device with the same tol and max_iter. */
int kdehip_quantile_device_batch(int n, const kdehip_quantile_item *items, const double *tol, int max_iter, void *stream);

/* ---- (5m) evaluation within a tolerance: the all-pairs sum pruned on the ball tree ------------------------------------------
 * The reference's other evaluation mode, setForceEvalDirect!(false): a pair of balls is left alone once their boxes show it
 * can no longer move the result by errTol (src/DualTree01.jl:248-299).  Here the balls are the sweep's own: the leaves are in
 * LEAF ORDER, so every chunk of 128 consecutive leaves is a compact ball of the tree, and a query block is 256 consecutive
 * queries in the order the entry processes them.  With p what kdehip_evaluate (section 5) defines, every query q gets
 *   p(q) * (1 - rel_tol) - abs_tol  <=  p_hat(q)  <=  p(q)                                     (up to rounding, below)
 * -- a truncation: only non-negative terms are left out, p_hat is never above p; it is not the reference's midpoint of two
 * bounds.  The density has dimension D, N leaves i with centres c_i and weights w_i, ONE bandwidth vector v, and
 * nh_k = -0.5 / v_k (one correctly rounded division), as in section 5.  The rule (csrc/evaltol.hip):
 *  1. Chunk boxes.  For chunk c (the leaves 128 c .. min(128 c + 127, N - 1)): lo_c[k], hi_c[k] = the least and the largest
 *     c_ik over its leaves, W_c = the sum of its weights from 0 in leaf order.
 *  2. Bounds of a pair (q, c), by the sweep's own chain -- acc = fma(d * d, nh_k, acc), from 0, k ascending:
 *       a_min(q, c) with d = dmin_k = max(0, lo_c[k] - x_qk, x_qk - hi_c[k]),
 *       a_max(q, c) with d = dmax_k = max(|lo_c[k] - x_qk|, |x_qk - hi_c[k]|);
 *     in a circular dimension the box is not used: dmin_k = 0 and dmax_k = pi (1 + 2^-20) (pi as fp64 rounds it; the factor
 *     covers the rounding of the wrap).  Every leaf i of c has a_max <= a_i <= a_min, for the COMPUTED values: each
 *     operation of the chain is monotone in |d| and correctly rounded, so no margin is needed on a_min.
 *  3. A lower bound L_q of the unnormalised sum, the larger of
 *       sum over c, ascending, of W_c * exp(a_max(q, c)), and
 *       the exact partial sum of the chunk with the largest a_min(q, c) (ties: the lowest c), as the sweep forms it:
 *       sum over its leaves in leaf order of w_i exp(a_i).
 *     For leave-one-out the query is leaf q of the density: the first bound then leaves out the whole chunk q / 128 (the
 *     weight W_c - w_q of its other leaves cannot be formed without cancellation), the second the term i == q alone.
 *  4. tau_q = max(rel_tol * L_q, abs_tol * norm), norm the Gaussian constant of section 5.  Chunk c is NEEDED by q iff
 *     tau_q == 0 or a_min(q, c) > log(tau_q) - 2^-20.  The 2^-20 is the rounding margin: it lowers tau_q by one part in a
 *     million, a thousand times more than the errors it has to cover (the exponential's and the logarithm's few ulp, the
 *     N / 128 + 128 additions behind L_q, and sum_i w_i = 1 only to N ulp).  A tile (query block, chunk) is VISITED iff some
 *     live query of the block needs the chunk; live = q < Nq and no NaN coordinate.
 *  5. The result: the direct sweep of section 5 restricted to the visited tiles -- the same groups of consecutive chunks
 *     (a function of (N, Nq) alone), the same chunk order within a group, the same arithmetic per pair; a group with no
 *     visited chunk contributes 0 -- and then the same finish: the groups in group order, / norm, / (1 - w_q) for
 *     leave-one-out, NaN for a query with a NaN coordinate, output through the permutation.
 * Why it holds: a skipped term has a_i <= a_min <= log tau_q - 2^-20, so what q loses is at most tau_q sum_c W_c <= tau_q,
 * and rel_tol * L_q <= rel_tol * (the unnormalised p).  "Up to rounding": p_hat and p are two fp64 sums of the kept terms in
 * the same order, so they differ from the exact bound by what any two such sums may differ, some N ulp.
 * Consequences: rel_tol == abs_tol == 0 visits every tile and returns kdehip_evaluate's bits; the result depends on the
 * density, the queries IN THEIR PROCESSING ORDER (which queries share a block) and the two tolerances alone, so it is the
 * same run after run and between the two entries.  No atomics.
 *   rel_tol, abs_tol   HOST pointers to one double each, as kdehip_quantile takes its tol.  NULL rel_tol = 1e-3 (the
 *                      reference's default errTol), NULL abs_tol = 0.  Required: 0 <= rel_tol < 1, 0 <= abs_tol < Inf;
 *                      anything else, NaN included, is KDEHIP_ERR_ARG.
 *   stats              int64[2] or NULL: the tiles visited, and the tiles in all = ceil(Nq / 256) * ceil(N / 128).
 * Errors, all checked before any device is touched: the tolerances and those of kdehip_evaluate / kdehip_evaluate_device_at
 * with their codes (per-point bandwidths and D above KDEHIP_MAX_DIMS are KDEHIP_ERR_UNSUPPORTED).  fp64 only.
 * Not here: batches of many small items (two chunks leave nothing to prune), tolerance forms of the log-domain entries, of
 * the log-likelihoods, the gradients and the kernel sums, per-point bandwidths. */
/* Host density, host arrays, blocking.  The queries are processed in the given order; leave_one_out processes the density's
 * leaves in leaf order and returns the values in original point order, as kdehip_evaluate does. */
int kdehip_evaluate_tol(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, const double *rel_tol,
                        const double *abs_tol, double *p_out, int64_t *stats, int device, const uint8_t *manifold);
/* Resident densities: at's leaves in leaf order are the queries, d_out [at's npts] in at's original point order; at == bd is
 * leave-one-out.  d_stats: DEVICE int64[2] or NULL.  Enqueue only on `stream`: no read-back between the passes, so a capture
 * of ONE stream into a HIP graph can hold the call, under the rules of kdehip_meanshift_device_batch (5h): the blocks of a
 * captured call are kept until kdehip_clear_cache, which INVALIDATES every graph captured from this entry.  Bit for bit
 * kdehip_evaluate_tol of the same densities' host arrays. */
int kdehip_evaluate_device_at_tol(const kdehip_device_density *bd, const kdehip_device_density *at, const double *rel_tol,
                                  const double *abs_tol, double *d_out, int64_t *d_stats, void *stream, const uint8_t *manifold);

/* ---- (5n) nearest neighbours on the ball tree: the k leaves nearest to a query ----------------------------------------------
 * The ball tree's own question, which the reference no longer asks (the toolbox it rewrites had knn; only neighborMinMax,
 * src/CrossValidation.jl:100-108, is left of it).  The skeleton is 5m's: the leaves are in LEAF ORDER, every chunk of 128
 * consecutive leaves is a compact box, a query block is 256 consecutive queries in the order the entry processes them.  Unlike
 * 5m the answer is EXACT: what brute force over all N leaves returns, bit for bit.
 * Distance.  d2(q, i) = acc after acc = fma(d_k * d_k, s_k, acc), from 0, k ascending, with d_k = x_qk - c_ik, wrapped to
 *   [-pi, pi) in a circular dimension as in 5d.  s_k > 0 is a per-dimension scale; scale == NULL is s_k = 1, the squared
 *   Euclidean distance.  The chain is monotone in |d_k| and correctly rounded, so the nearest-corner value of a chunk box,
 *       dmin2(q, c): the same chain on dmin_k = max(0, lo_c[k] - x_qk, x_qk - hi_c[k]), dmin_k = 0 in a circular dimension,
 *   is <= the COMPUTED d2(q, i) of every leaf i of c: no rounding margin.
 * Result for a query q: the k leaves with the smallest key (d2, original point index), in ascending order of that key -- ties
 *   in d2 go to the lower original index, so the answer depends neither on the tree nor on the processing order.
 *   d2_out [Nq][k] doubles and idx_out [Nq][k] int64 (k fastest: a (k, Nq) column-major matrix), idx 1-BASED original indices,
 *   the convention of kdehip_sample's labels.  A query with a non-finite coordinate gets NaN distances and index 0.
 * Leave-one-out: the queries are the density's own leaves, and leaf q is excluded BY INDEX, not by distance -- a duplicate of
 *   the point stays a neighbour at distance 0.
 * Limits: 1 <= k <= KDEHIP_KNN_MAX_K; k <= N (N - 1 for leave-one-out); D <= KDEHIP_MAX_DIMS; N < 2^31 - 1; fp64 only.  The
 *   bandwidths are not read: per-point bandwidths are fine (as kdehip_kernel_sum with explicit variances).
 * The plan (csrc/knn.hip), part of the contract so that `stats` is reproducible:
 *  1. Chunk boxes lo_c, hi_c as in 5m step 1.
 *  2. Per query, c* = the chunk with the smallest dmin2(q, c), ties to the lowest c.  For a leave-one-out query whose own chunk
 *     holds no other leaf, that chunk does not count.
 *  3. r_q = the k-th smallest d2 among the eligible leaves of c* (all of them; without leaf q for leave-one-out), computed
 *     exactly; +Inf if c* has fewer than k eligible leaves.
 *  4. Chunk c is NEEDED by q iff dmin2(q, c) <= r_q (non-strict: a tie may win on index).
 *  5. A tile (query block, chunk) is VISITED iff some live query of the block needs the chunk; live = q < Nq and every
 *     coordinate finite.
 *  6. stats: int64[2] or NULL -- the tiles visited, and the tiles in all = ceil(Nq / 256) * ceil(N / 128), as in 5m.
 * The sweep visits the flagged tiles only; a lane may also leave a staged chunk alone that its own current k-th candidate
 * already excludes.  Whatever is skipped holds no leaf that could enter the list (d2 >= dmin2 > the k-th key's d2), so the
 * result is the exact one.  No atomics.
 * Errors, all checked before any device is touched: KDEHIP_ERR_ARG for NULL outputs, Nq < 0, k out of range, a scale that is
 * not finite and > 0, a manifold byte above 1; KDEHIP_ERR_UNSUPPORTED for D above KDEHIP_MAX_DIMS; KDEHIP_ERR_DIM_MISMATCH for
 * `at` of another dimension.  Nq == 0 is KDEHIP_OK.
 * Not here: batches of many small items, radius queries, k > KDEHIP_KNN_MAX_K, fp32. */
#define KDEHIP_KNN_MAX_K 32
/* Host density, host arrays, blocking.  The queries are processed in the given order; leave_one_out (pos, Nq unread) processes
 * the density's leaves in leaf order and returns the columns in original point order, as kdehip_evaluate does.  scale: NULL or
 * D doubles. */
int kdehip_knn(const kdehip_density *bd, const double *pos, int64_t Nq, int k, int leave_one_out, const double *scale,
               double *d2_out, int64_t *idx_out, int64_t *stats, int device, const uint8_t *manifold);
/* Resident densities: at's leaves in leaf order are the queries, the columns of d_d2_out / d_idx_out (DEVICE, [at's npts][k])
 * in at's original point order; at == bd is leave-one-out.  scale: HOST pointer or NULL.  d_stats: DEVICE int64[2] or NULL.
 * Enqueue only on `stream` and capturable under the rules of kdehip_evaluate_device_at_tol.  Bit for bit kdehip_knn of the
 * same densities' host arrays. */
int kdehip_knn_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, int k, const double *scale,
                         double *d_d2_out, int64_t *d_idx_out, int64_t *d_stats, void *stream, const uint8_t *manifold);

/* ---- (5o) densities with per-point bandwidths: evaluation and log-likelihoods ------------------------------------------------
 * The sample-point adaptive estimator: every source i has variances v_ik of its own (kdehip_make_density_varbw, section 4),
 *     p(x) = (2 pi)^(-D/2) sum_i w_i / prod_k sqrt(v_ik) exp(a_i),   a_i = sum_k diff_k(x_k, c_ik)^2 nh_ik,  nh_ik = -0.5 / v_ik
 * (k ascending, one fma per dimension; diff_k the plain difference, through wrap() in a circular dimension, 5d).  The entries
 * of 5, 5b and 5f read ONE bandwidth vector and keep refusing such densities; these read a variance per source and accept
 * ANY density, one with a single vector included -- its values agree with 5 / 5f to rounding, not bit for bit, because the
 * normaliser is folded into every term here and applied once after the sum there.
 * The plan (csrc/varbw.hip, csrc/pair_sweep.hpp pair_sweep_var):
 *  1. A prepass over the N leaves, in leaf order, into the call's block: nh_ik; c_i = w_i / prod_k sqrt(v_ik) (k ascending,
 *     correctly rounded roots); for log_domain != 0 instead lc_i = log w_i - 1/2 sum_k log v_ik, -Inf for w_i == 0.
 *  2. The sweep keeps the mapping of 5: one lane per query, 256 queries per block, groups of 128-leaf chunks through a
 *     two-buffer LDS ring, the split a function of (N, Nq) alone.  It stages 2D + 1 values per source: [c_i. | nh_i. | c_i].
 *     Direct step: sum c_i exp(a_i), the self term dropped for leave-one-out.  Log step: t_i = a_i + lc_i, m = max t_i over
 *     S = { w_i > 0, i != q if leave-one-out }, s = sum exp(t_i - m), rescaled once per chunk (5f).  The maximum is over
 *     t_i, not a_i: the normalisers differ per source.
 *  3. The finish sums the group partials in group order (no atomics): p = sum / (2 pi)^(D/2) [/ (1 - w_q)], or
 *     log p = M + log S - (D/2) log 2pi [- log(1 - w_q)], -Inf for S empty.  A query with a NaN coordinate gets NaN (5j).
 *     A log-likelihood is sum_q W_q log p_q under the rules of 5b (direct) or 5f (log_domain): src/DualTree01.jl:456-466.
 * The host entry, a resident call and a second run give the same bits.
 * Errors, all checked before any device is touched: KDEHIP_ERR_ARG for NULL arguments, leave_one_out with at != bd, a manifold
 * byte above 1; KDEHIP_ERR_UNSUPPORTED for D outside 1..KDEHIP_MAX_DIMS; KDEHIP_ERR_DIM_MISMATCH for `at` of another
 * dimension.  The variances themselves are not examined: a non-positive one gives what the arithmetic gives.
 * Not here: evaluation within a tolerance (5m), gradients, Hessians and modes (5h, 5k), conditionals (5i), box masses and
 * quantiles (5l), kdehip_kernel_sum with var == NULL, the bandwidth metric of kdehip_knn, resident marginal / condition of
 * such densities, a batched entry, a D + 2 staging for variances that are one vector times a per-point scale, fp32. */
/* Host density, host arrays, blocking; one pinned upload, as kdehip_evaluate.  leave_one_out: pos and Nq are unread, the values
 * come back in original point order. */
int kdehip_evaluate_varbw(const kdehip_density *bd, const double *pos, int64_t Nq, int leave_one_out, int log_domain,
                          double *p_out, int device, const uint8_t *manifold);
/* evalAvgLogL (5b; log_domain: 5f) of bd at at's points; at == NULL with leave_one_out means bd.  Blocking. */
int kdehip_eval_avg_logl_varbw(const kdehip_density *bd, const kdehip_density *at, int leave_one_out, int log_domain,
                               double *out, int device, const uint8_t *manifold);
/* Resident densities, enqueue only on `stream`: d_out (DEVICE) gets at's npts values in at's original point order.
 * leave_one_out needs at == bd; at == bd without it keeps the self terms.  A capture of ONE stream into a HIP graph can hold
 * these three calls under the rules of kdehip_evaluate_device_at_tol (5m): the blocks of a captured call are kept until
 * kdehip_clear_cache. */
int kdehip_evaluate_varbw_device_at(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                    int log_domain, double *d_out, void *stream, const uint8_t *manifold);
/* ... at Nq positions in HBM (d_pos: [Nq][D]), values in query order */
int kdehip_evaluate_varbw_device(const kdehip_device_density *bd, const double *d_pos, int64_t Nq, int log_domain,
                                 double *d_out, void *stream, const uint8_t *manifold);
/* ... the log-likelihood into ONE double in HBM */
int kdehip_eval_avg_logl_varbw_device(const kdehip_device_density *bd, const kdehip_device_density *at, int leave_one_out,
                                      int log_domain, double *d_out, void *stream, const uint8_t *manifold);
/* 1 if every leaf of the resident density has its first leaf's variances (what the entries of 5 / 5b / 5f ask), else 0;
 * 0 with KDEHIP_ERR_ARG in kdehip_last_error for NULL. */
int kdehip_density_uniform_bandwidth(const kdehip_device_density *density);

/* ---- (5p) the exact product of two densities: labels, draws and log Z -------------------------------------------------------
 * The samplers of sections 1-3 approximate a product after Niter sweeps.  For TWO densities the product has a closed form
 * (csrc/prodexact.hip; this library's own: the reference has no counterpart, the toolbox it descends from had productExact).
 * For p of dimension D with leaves i in LEAF ORDER, centres a_i, weights alpha_i and ONE bandwidth vector u (variances, the
 * rule of section 5), and q with b_j, beta_j and v, of the same D in 1..KDEHIP_MAX_DIMS: p q is a mixture of N1 N2 Gaussians
 * that share the variance u_k v_k / s_k, s_k = u_k + v_k; component (i, j) has the mean a_ik + (b_jk - a_ik) u_k / s_k and a
 * weight proportional to alpha_i beta_j N(a_i - b_j; 0, s).  Euclidean, fp64 only.  With S_p = { i : alpha_i > 0 } and
 * S_q = { j : beta_j > 0 }:
 *   e_ij  = sum_k (a_ik - b_jk)^2 * (-0.5 / s_k), k ascending, one fma per dimension: the direct kernel's expression (5)
 *   m_i   = max_{j in S_q} e_ij,  T_i = sum_{j in S_q} beta_j exp(e_ij - m_i),  L_i = log alpha_i + m_i + log T_i   (the log
 *           domain of 5f; L_i = -Inf outside S_p)
 *   M     = max_{i in S_p} L_i,  R_i = exp(L_i - M),  R = sum_{i in S_p} R_i
 *   logz  = M + log R - log((2 pi)^(D/2) prod_k sqrt(s_k))
 *           (= log int p q; finite where the integral itself, 5g, underflows to 0)
 * The draw: draw t of Np has the global index g = sample_offset + t and the random numbers
 *   u = kdehip_philox_fill_uniform(seed, g, 1, K = 2),  n = kdehip_philox_fill_normal(seed, g, 1, R = D).
 * i is the first leaf of S_p whose cumulative sum of R (leaf order) exceeds u[0] * R; j is the first leaf of S_q whose
 * cumulative sum of beta_j exp(e_ij - m_i) exceeds u[1] * T_i; in either search, if rounding leaves none, the last leaf of the set.
 *   ind[t]    = (the 1-based ORIGINAL index of i in p, the 1-based ORIGINAL index of j in q)          (int64 [Np][2])
 *   pts[t][k] = fma(b_jk - a_ik, u_k / s_k, a_ik) + sqrt(u_k v_k / s_k) * n[k]                       (double [Np][D])
 * -- the divide, the product u_k v_k, its divide by s_k and the root each correctly rounded, the last multiply and add rounded
 * separately as in 2f.
 * Numerics and determinism: the cumulative sums are defined in exact arithmetic.  The implementation forms the sums over j in
 * the group split of 5b / 5i (128-leaf chunks of q in groups that depend on (N2, N1) alone, combined in group order) and the
 * scan of R_i in 256 contiguous segments of ceil(N1 / 256) leaves (each summed left to right, the segment totals summed left to
 * right), so a threshold within a relative 1e-9 of a boundary may resolve to the neighbouring leaf of the set.  Everything
 * else about a label is exact -- a leaf outside S_p or S_q is never drawn --, and the host entry, a resident call and an item
 * of any batch return the same bits run after run.  No atomics.
 * S_p or S_q empty: logz = -Inf, ind = (0, 0) and the point is NaN.  No entry reads out of bounds.
 * Cost: one exp per (i, j) pair for the rows; at most one exp per (draw, j) pair for the labels -- only the group of q's
 * chunks a draw's second threshold fell into is swept again, and a (256-draw block, group) pair that no draw chose is not
 * swept at all.
 * Errors, all checked before any device is touched: null arguments (all outputs NULL included; pts and ind are given together
 * or not at all), Np < 0, densities on different devices -- KDEHIP_ERR_ARG; D differs between p and q --
 * KDEHIP_ERR_DIM_MISMATCH; D outside 1..KDEHIP_MAX_DIMS or per-point bandwidths -- KDEHIP_ERR_UNSUPPORTED.  Np == 0 and
 * n == 0 are KDEHIP_OK (with Np == 0 a logz that was asked for is still written).
 * Not here: circular dimensions, partialDimMask, more than two densities in one sweep (fold: product_components, then a
 * density of the mixture), fp32. */
/* Host densities, host arrays, blocking.  pts [Np][D] with ind [Np][2], logz [1]: pts and ind together; not all NULL. */
int kdehip_prod_exact(const kdehip_density *p, const kdehip_density *q, int64_t Np, uint64_t seed, int64_t sample_offset,
                      double *pts, int64_t *ind, double *logz, int device);
/* Resident densities, device arrays, enqueue only on `stream` (hipStream_t, NULL = the null stream), no read-back.  A capture
 * of ONE stream into a HIP graph can hold the call under the rules of kdehip_evaluate_device_at_tol (5m): the blocks of a
 * captured call are kept until kdehip_clear_cache. */
int kdehip_prod_exact_device(const kdehip_device_density *p, const kdehip_device_density *q, int64_t Np, uint64_t seed,
                             int64_t sample_offset, double *d_pts, int64_t *d_ind, double *d_logz, void *stream);
typedef struct kdehip_prod_exact_item {
  const kdehip_device_density *p;
  const kdehip_device_density *q;
  int64_t Np;
  uint64_t seed;
  int64_t sample_offset;
  double *d_pts;            /* device, [Np][D], or NULL (then d_ind is NULL too) */
  int64_t *d_ind;           /* device, [Np][2] */
  double *d_logz;           /* device, [1], or NULL */
} kdehip_prod_exact_item;
/* Many resident items (mixed D, N1, N2 and Np) on one device, enqueue only on `stream`.  Launches per pass are one per
 * distinct D for all items together.  Every item's results are bit for bit those of kdehip_prod_exact_device. */
int kdehip_prod_exact_device_batch(int n, const kdehip_prod_exact_item *items, void *stream);
/* The mixture itself, in ORIGINAL point order and row-major: component c = i N2 + j (i, j 0-based original indices) has
 * means[c][k] = the mean above (without the noise) and weights[c] = exp((log alpha_i + log beta_j + e_ij) - (M + log R)), 0
 * outside S_p x S_q (and everywhere when either set is empty); var[k] = u_k v_k / s_k.  means [N1 N2][D], weights [N1 N2],
 * var [D]: none may be NULL.  N1 N2 > 2^20 is KDEHIP_ERR_UNSUPPORTED; the other refusals are those above.  Host densities,
 * blocking. */
int kdehip_product_components(const kdehip_density *p, const kdehip_density *q, double *means, double *weights, double *var,
                              int device);
/* Resident densities, device arrays, enqueue only on `stream`. */
int kdehip_product_components_device(const kdehip_device_density *p, const kdehip_device_density *q, double *d_means,
                                     double *d_weights, double *d_var, void *stream);

/* ---- (5q) joint bandwidth selection: the leave-one-out likelihood over all dimensions ---------------------------------------
 * kde!(points) (section 5, kdehip_auto_bandwidth) searches the leave-one-out likelihood of every 1-D marginal on its own; for
 * D > 1 that undersmooths (the best 1-D bandwidth shrinks like N^(-1/5), the best joint one like N^(-1/(D+4))).  The entries
 * below maximise the JOINT leave-one-out likelihood over the whole bandwidth vector by a fixed-point iteration
 * (csrc/bwjoint.hip; this library's own, the reference has no counterpart).  For a density bd with leaves c_i in LEAF ORDER,
 * weights w_i, a per-dimension `manifold` as in 5d (NULL = Euclidean) and a current variance vector v:
 *   d_ijk = c_ik - c_jk, through wrap() first in a circular dimension
 *   a_ij  = sum_k d_ijk^2 * (-0.5 / v_k): the expression and fma order of the direct kernel
 *   S_i   = { j : w_j > 0, j != i } -- by INDEX: a duplicate of point i is in S_i; the rule of 5f otherwise
 *   m_i   = max_{S_i} a_ij,  S0_i = sum_{S_i} w_j exp(a_ij - m_i),  T_ik = sum_{S_i} w_j exp(a_ij - m_i) d_ijk^2
 *   Q     = { i : w_i > 0, S_i not empty },  W = sum_{i in Q} w_i
 *   L(v)  = the leave-one-out average log-likelihood exactly as kdehip_eval_avg_logl_log(bd, bd, 1) defines it (5f):
 *           sum over { i : w_i > 0 } of w_i (m_i + log S0_i - log norm(v) - log(1 - w_i)), -Inf if some such S_i is empty
 *   v_new_k = ( sum_{i in Q} w_i T_ik / S0_i ) / W
 * This is EM for a mixture with fixed centres and one shared diagonal covariance: T_ik / S0_i is the responsibility-weighted
 * mean squared difference of point i (the 1 - w_i of leave-one-out cancels in it), so L(v_new) >= L(v) at every step.
 * The iteration starts from v_0 = start_k^2 (start: D standard deviations; NULL = bd's own bandwidth, its first leaf's
 * variances) and stops after the step with max_k |log(v_new_k / v_k)| / 2 <= tol -- a tolerance in log standard deviation --
 * or after maxiter steps.  Results: bw_out = sqrt(v), D standard deviations; iters = the steps taken, negative when the last
 * of them was still above tol (as kdehip_meanshift reports); logl = L at the returned bandwidth, from one closing sweep;
 * trace (optional, maxiter + 1 doubles): trace[t] = L(v_t) for t = 0 .. |iters|, the rest is not written -- every sweep yields
 * the L of the iterate it read, so the trace costs nothing extra.
 * Degenerate data -- a v_new_k that is 0 or not finite: a dimension in which all points coincide, or fewer than two leaves of
 * positive weight --: nothing is updated, the iteration freezes at the last valid iterate (iters keeps its value) and
 * status = 1; with too few weighted leaves that iterate is the start itself, logl = -Inf and iters = 0.  status = 0 otherwise.
 * Convergence is linear: two starts end within a few tol of each other, not at the same bits.  The contract is the trajectory
 * from a given start, not "the optimum".
 * Arithmetic and determinism: each step is one all-pairs sweep split as in 5b / 5f / 5h (128-leaf chunks in groups that depend
 * on npts alone; a group carries (m, s_0, t_1..t_D), rescaled by exp(m_old - m_new) once per chunk; the groups combined in
 * group order), the leaves' terms summed in the fixed 256-wide tree of 5b and the blocks in block order.  No atomics.  The
 * sweeps of all items of a call share their launches (one per distinct (D, circular)), and a finished item is never written
 * again: an item's result depends on the density, the start, tol and maxiter alone.  The host entry, the resident entry and
 * any batch give the same bits, run after run, however the sweeps are grouped between the host's reads of the items' states.
 * All three entries are BLOCKING and none takes a stream: the result is D doubles that the caller needs on the host to build
 * the density, and the sweeps run in rounds with one read of the items' states between them.  tol is a HOST pointer to ONE
 * value, as in 5h.
 * Errors, all checked before any device is touched: a null bd, tol, bw_out, logl, iters or status, tol negative or not finite,
 * maxiter < 0, npts < 2, a start entry not finite or <= 0, a manifold byte above 1 or a mask bit at or above D, batch items on
 * different devices -- KDEHIP_ERR_ARG; D outside 1..KDEHIP_MAX_DIMS or per-point bandwidths (in kdehip_evaluate's words) --
 * KDEHIP_ERR_UNSUPPORTED.  n == 0 is KDEHIP_OK; maxiter == 0 is KDEHIP_OK and returns the start with its logl.  fp64 only.
 * Not here: per-point bandwidths, full covariance, applying the result to a resident density without leaving HBM, and an
 * enqueue-only form on a caller's stream. */
/* Host density, host results, blocking. */
int kdehip_bandwidth_joint(const kdehip_density *bd, const double *start /* D sds, or NULL = bd's own bandwidth */,
                           const double *tol, int maxiter, double *bw_out /* D sds */, double *logl, int32_t *iters,
                           int32_t *status, double *trace /* [maxiter + 1] or NULL */, int device, const uint8_t *manifold);
/* Resident density, HOST results (start is a host pointer too), blocking. */
int kdehip_bandwidth_joint_device(const kdehip_device_density *bd, const double *start, const double *tol, int maxiter,
                                  double *bw_out, double *logl, int32_t *iters, int32_t *status, double *trace,
                                  const uint8_t *manifold);
typedef struct kdehip_bwjoint_item {
  const kdehip_device_density *bd;
  const double *start;      /* HOST pointer, D standard deviations, or NULL = bd's own bandwidth */
  double *bw_out;           /* host, [D] */
  double *logl;             /* host, [1] */
  int32_t *iters;           /* host, [1] */
  int32_t *status;          /* host, [1] */
  uint32_t circular_mask;   /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
  uint32_t reserved_;
} kdehip_bwjoint_item;
/* Many resident densities (mixed D and npts) on one device, host results, blocking: the serving shape.  The items share the
 * three launches of a sweep, and every item's results are bit for bit those of kdehip_bandwidth_joint_device. */
int kdehip_bandwidth_joint_device_batch(int n, const kdehip_bwjoint_item *items, const double *tol, int maxiter);

/* ---- (5r) reweighting and moving a density without re-forming its tree ------------------------------------------------------
 * changeWeights!(bd, newWeights) and movePoints!(bd, delta) (reference src/BallTreeDensity01.jl:278-309): every leaf takes a
 * new weight, or moves by an offset of its own, and the statistics of the internal nodes are recomputed from their children,
 * bottom-up ("just fix up the statistics"); the tree itself -- child arrays, leaf ranges, permutation -- stays.  The topology
 * of the reference's builder does not read the weights (most_spread_coord, src/BallTree01.jl:148), so a reweighted density IS
 * the density kde!(getPoints(bd), bw, newWeights) would build for weights that kde! does not rescale; after a move the result
 * is a VALID BUT LOOSER tree than a rebuild's, as in the reference: every node still bounds and summarises its leaves, so the
 * sampler, evaluation within a tolerance (5m) and the neighbour search (5n) stay correct and prune less after large moves.
 *
 * The formula of one internal node from its children a and b -- calcStatsBall! (src/BallTree01.jl:282-336) and
 * calcStatsDensity! (src/BallTreeDensity01.jl:141-187), as kdehip_make_density computes them, no fused multiply-add anywhere:
 *   top = max(c_a + r_a, c_b + r_b), bottom = min(c_a - r_a, c_b - r_b), r = (top - bottom) / 2, c = bottom + r
 *     (every + and - of this line through wrap() in a dimension tree_manifold marks circular)
 *   w = w_a + w_b;  wt = w_a + w_b + eps;  u_a = w_a / wt, u_b = w_b / wt
 *   m = u_a m_a + u_b m_b;  v = u_a (v_a + m_a^2) + u_b (v_b + m_b^2) - m^2
 *   per-point bandwidths: bandwidthMax = max of the children's, bandwidthMin = min
 *
 * Host entry (CPU only, no device is touched).  The twelve input arrays are those kdehip_make_density (or _varbw) shapes, the
 * twelve outputs have the same sizes and may not alias the inputs.
 *   new_weights  npts doubles indexed by ORIGINAL point (leaf i takes new_weights[permutation - 1]), used AS GIVEN: the
 *                reference does not normalise here.  NULL keeps the weights.
 *   delta        ndims x npts column-major, indexed by ORIGINAL point, added to the leaf's centre and mean -- wrap(x + delta)
 *                in a dimension tree_manifold marks circular (addop).  NULL moves nothing.
 *   tree_manifold  ndims bytes or NULL (section 4).
 *   varbw        0: one bandwidth vector; bandwidthMin / bandwidthMax (npts x ndims) are copied.  Nonzero: the arrays of
 *                kdehip_make_density_varbw; bandwidthMin / bandwidthMax (2 npts x ndims) are recomputed for the internal nodes.
 * Refusals, all before anything is written: a null array or both new_weights and delta NULL -- KDEHIP_ERR_ARG ("null"); a
 * weight that is negative or not finite -- KDEHIP_ERR_ARG ("new_weights"); a delta that is not finite -- KDEHIP_ERR_ARG
 * ("delta"); a tree_manifold byte above 1 -- KDEHIP_ERR_ARG; npts < 1 -- KDEHIP_ERR_ARG; ndims outside 1..KDEHIP_MAX_DIMS --
 * KDEHIP_ERR_UNSUPPORTED ("ndims"); child arrays that are no tree -- KDEHIP_ERR_ARG. */
int kdehip_density_refit(int64_t ndims, int64_t npts, const double *centers, const double *ranges, const double *weights,
                         const int64_t *left_child, const int64_t *right_child, const int64_t *lowest_leaf,
                         const int64_t *highest_leaf, const int64_t *permutation, const double *means, const double *bandwidth,
                         const double *bandwidthMin, const double *bandwidthMax, int varbw, const double *new_weights,
                         const double *delta, const uint8_t *tree_manifold, double *centers_out, double *ranges_out,
                         double *weights_out, int64_t *left_child_out, int64_t *right_child_out, int64_t *lowest_leaf_out,
                         int64_t *highest_leaf_out, int64_t *permutation_out, double *means_out, double *bandwidth_out,
                         double *bandwidthMin_out, double *bandwidthMax_out);

/* Resident entries (csrc/refit.hip).  The result is a NEW handle on p's device; p is not written and stays usable.  Both
 * entries are BLOCKING, like every entry that makes a density, and take no stream: they run on the calling thread's own
 * stream and wait for it, and the caller's device arrays must be complete when the call is made.
 *   kind  KDEHIP_REFIT_KEEP     d_values is NULL; only d_delta is applied (d_delta NULL is then KDEHIP_ERR_ARG).
 *         KDEHIP_REFIT_WEIGHTS  d_values = npts weights, used as given (a negative or non-finite one: KDEHIP_ERR_ARG).
 *         KDEHIP_REFIT_LOGL     d_values = npts log-likelihoods l_i: the Bayes update of the weights,
 *                                 m = max l_i over the leaves with w_i > 0,  S = sum_i w_i exp(l_i - m),
 *                                 w_i' = (w_i exp(l_i - m)) / S   (a leaf with w_i = 0 keeps 0),
 *                                 log_evidence = m + log S,  ess = 1 / sum_i w_i'^2.
 *                               Both sums run over the 128-leaf chunks in LEAF order -- inside a chunk the fixed pairwise
 *                               tree over its 128 terms (strides 64, 32, .., 1), then the chunks in chunk order -- with no
 *                               atomics: a batch, a single call and every repeat give the same bits.  exp is the device
 *                               library's.  S that is 0 or not finite, an l_i that is NaN or +Inf, or no leaf of positive
 *                               weight: KDEHIP_ERR_ARG and *out = NULL, as kdehip_density_condition_device treats logz = -Inf.
 *   leaf_order  0: d_values and d_delta are indexed by ORIGINAL point (the reference's convention, and the order in which
 *               kdehip_evaluate_log_device_at(likelihood, p) returns its values); 1: by leaf position -- the order of
 *               kdehip_evaluate_log_device when its queries are the density's own leaf rows.
 *   d_delta     ndims x npts column-major device array or NULL; must be finite (else KDEHIP_ERR_ARG, *out = NULL).
 *   tree_manifold  ndims bytes or NULL: the operators of the box formula and of the move.
 *   log_evidence, ess  optional HOST doubles, written for KDEHIP_REFIT_LOGL only.
 * The internal nodes are recomputed by the formula above, one node per lane, height by height (a height = one launch while it
 * is wide, the top of the tree in one workgroup): bit for bit what kdehip_density_refit gives on the same arrays.  The child
 * pairs and the height lists are derived from the child arrays once per handle and kept on it (an uploaded density keeps a
 * copy of its child arrays for that).  What the sampler's packers know about a density's values -- one shared bandwidth per
 * level, the range of the variances, finiteness -- is recomputed for the new values and equals what kdehip_density_upload of
 * the same arrays finds.  If p was built by the library, the result keeps the twelve arrays for kdehip_density_download:
 * centres, ranges, means, variances and weights are fetched AT THE REFIT, in the call's one readback; a result of an uploaded
 * p has no such arrays, as p has none.  Per-point bandwidths are supported (bandwidthMin / bandwidthMax of a built source are
 * its leaves' one vector and are copied).
 * Refusals before any device work: null out or p, an unknown kind, d_values NULL (non-NULL) where kind needs (forbids) it,
 * nothing to do, a tree_manifold byte above 1 -- KDEHIP_ERR_ARG; batch items on different devices -- KDEHIP_ERR_ARG.
 * Not here: an enqueue-only (graph-capturable) refit, a refit in place, re-forming the tree after large moves. */
#define KDEHIP_REFIT_KEEP 0
#define KDEHIP_REFIT_WEIGHTS 1
#define KDEHIP_REFIT_LOGL 2
int kdehip_density_refit_device(kdehip_device_density **out, const kdehip_device_density *p, const double *d_values, int kind,
                                int leaf_order, const double *d_delta, const uint8_t *tree_manifold, double *log_evidence,
                                double *ess);
typedef struct kdehip_refit_item {
  const kdehip_device_density *p;
  const double *d_values;       /* device, [npts], or NULL (KDEHIP_REFIT_KEEP) */
  const double *d_delta;        /* device, [ndims x npts], or NULL */
  double *log_evidence;         /* host, [1], or NULL */
  double *ess;                  /* host, [1], or NULL */
  int32_t kind;
  int32_t leaf_order;
  uint32_t circular_mask;       /* bit d = dimension d circular in the tree's operators; a bit at or above ndims is KDEHIP_ERR_ARG */
  uint32_t reserved_;
} kdehip_refit_item;
/* Many densities (mixed in npts, ndims, kind and order) on one device: the items share their launches (the count does not
 * depend on n while the heights are narrow) and ONE readback; every result is bit for bit the single call's.  One bad item
 * fails the whole call: every out[i] is NULL and no handle is created. */
int kdehip_density_refit_device_batch(int n, const kdehip_refit_item *items, kdehip_device_density **out);

/* ---- (5s) entropic optimal transport between two densities: Sinkhorn's iteration and the barycentric map ---------------------
 * kld, ise, mmd and intersIntg compare two densities point by point; none of them sees how FAR apart their mass lies, and none
 * says how to move one onto the other.  The entries below solve the entropic optimal transport problem between the leaves of
 * two densities (csrc/sinkhorn.hip; this library's own, the reference has no counterpart).
 *   p has leaves x_i (i < N) and weights a_i, q has y_j (j < M) and b_j -- the weights as the densities hold them (kde's
 *     sum to 1); the bandwidths play no part except in the default scale.
 *   scale  a positive D-vector s; NULL = sqrt(v_p + v_q) per dimension, the combination of 5g, from the first leaves'
 *          variances.  A density with per-point bandwidths must be given scale explicitly.
 *   reg    eps > 0, in units of the scaled squared distance.
 *   c_ij = 1/2 sum_k diff_k(x_i, y_j)^2 / s_k^2, diff_k the plain difference, through wrap() in a circular dimension (5d);
 *   A_ij = -c_ij / eps = sum_k diff_k^2 * nhib_k, nhib_k = -1 / (2 eps s_k^2): the expression and fma order of the direct kernel.
 * The potentials are kept divided by eps: phi_i, gamma_j.  With
 *   T_x(gamma)_i = -LSE_{j : b_j > 0} (log b_j + gamma_j + A_ij),   T_y(phi)_j the same with the roles exchanged
 * (log b_j + gamma_j is -Inf for a weightless leaf: it takes no part), a CROSS item (q is not p) starts from phi = gamma = 0,
 * steps = 0 and repeats
 *   1. tau = T_x(gamma), r_i = exp(phi_i - tau_i);
 *   2. err = sum_{a_i > 0} a_i |r_i - 1|: the L1 row-marginal error of the plan at (phi, gamma);
 *   3. mass = sum a_i r_i;
 *   4. if (steps >= 1 and err <= tol) or steps == maxiter: finish with the current (phi, gamma);
 *   5. otherwise phi = tau, gamma = T_y(phi), steps += 1.
 * A SELF item (q is p: the same struct, the same handle) runs the same loop with tau = T_x(phi) over p's own leaves and step 5
 * phi = (phi + tau) / 2, gamma = phi: the symmetric average, which on a symmetric problem converges in tens of steps where
 * the alternating updates take thousands.
 * Results of an item:
 *   value = eps (sum a_i phi_i + sum b_j gamma_j - (mass - 1)): the dual objective, min <pi, c> + eps KL(pi | a x b) at
 *           convergence; transport_cost = <pi, c> of the plan pi_ij = a_i b_j exp(phi_i + gamma_j + A_ij); err, mass;
 *   iters = steps, negated if err > tol (the convention of 5q);
 *   phi (N), gamma (M): in the order of getPoints / getWeights (by ORIGINAL point);
 *   the barycentric map: m_i = sum_j e_ij diff(y_j, x_i) / sum_j e_ij, e_ij = exp(log b_j + gamma_j + A_ij - max_j), from one
 *           more sweep at the finished potentials; it does not depend on phi_i or a_i, so weightless leaves of p move too.
 *           delta = m; map = x + m, through wrap() in a circular dimension.
 * The Sinkhorn divergence S(p, q) = value(p, q) - value(p, p) / 2 - value(q, q) / 2 is three items, one cross and two self,
 * all three at ONE scale (the cross item's: kdehip_sinkhorn_item.scale_p / scale_q).
 * Arithmetic and determinism: a half-step is one all-pairs sweep split as in 5b / 5f / 5q (128-leaf chunks in groups that
 * depend on the two sizes alone; a group carries a running maximum and a sum rescaled once per chunk; the groups combined in
 * group order), the queries' terms summed in the fixed 256-wide tree of 5b and the blocks in block order.  No atomics.  The
 * half-steps of all items of a call share their launches (one per distinct (D, circular)), and a finished item is never
 * written again: an item's result depends on the two densities, scale, reg, tol and maxiter alone.  The host entry, the
 * resident entry and any batch give the same bits, however the iterations are grouped between the host's reads of the
 * items' states.  Circular data in which no difference wraps give the Euclidean bits.
 * All three entries are BLOCKING, take no stream and return host scalars.  reg and tol are HOST pointers to ONE value each, as
 * tol is in 5h and 5q (an item of a batch holds the values themselves).
 * Errors, KDEHIP_ERR_ARG, all checked before any device is touched: a null p, q, reg, tol or scalar result, ndims that differ or lie
 * outside 1..KDEHIP_MAX_DIMS, reg or a scale entry not finite or <= 0, tol negative or NaN, maxiter < 0, a manifold byte above
 * 1 or a mask bit at or above ndims, 2^31 points or more, densities on different devices, per-point bandwidths without a
 * scale, and a host density without a leaf of positive weight.  A RESIDENT density without a leaf of positive weight is
 * found by the first half-step (its weights live on the device): KDEHIP_ERR_ARG then too, the outputs are not meaningful.
 * Not here: eps-annealing, unbalanced transport, barycentres, an enqueue-only form. */
/* Host densities, host results, blocking.  phi [N], gamma [M], delta and map [ndims x N column-major, by original point]: each
 * optional (NULL). */
int kdehip_sinkhorn(const kdehip_density *p, const kdehip_density *q, const double *scale /* D, or NULL */, const double *reg,
                    const double *tol, int maxiter, double *value, double *transport_cost, double *err, double *mass, int32_t *iters, double *phi,
                    double *gamma, double *delta, double *map, int device, const uint8_t *manifold);
/* Resident densities, HOST scalars (scale is a host pointer too), optional DEVICE vectors: d_phi [N], d_gamma [M], d_map
 * [ndims x N column-major] by original point; d_delta [ndims x N column-major] in LEAF order -- ready for
 * kdehip_density_refit_device(.., KDEHIP_REFIT_KEEP, leaf_order = 1, d_delta, ..).  Blocking: the vectors are complete on
 * return, and the caller's own work on p and q must be complete when the call is made. */
int kdehip_sinkhorn_device(const kdehip_device_density *p, const kdehip_device_density *q, const double *scale,
                           const double *reg, const double *tol, int maxiter, double *value, double *transport_cost, double *err, double *mass,
                           int32_t *iters, double *d_phi, double *d_gamma, double *d_delta, double *d_map,
                           const uint8_t *manifold);
typedef struct kdehip_sinkhorn_item {
  const kdehip_device_density *p, *q;   /* q == p selects the self iteration */
  const double *scale;                  /* HOST pointer, D entries, or NULL */
  const kdehip_device_density *scale_p, *scale_q;   /* both NULL, or the two densities whose variances give the default scale
                                                        in the place of p's and q's: the self items of a divergence take the
                                                        cross item's scale.  Not read when scale is given. */
  double reg, tol;
  double *value, *transport_cost, *err, *mass;   /* host, [1] each */
  int32_t *iters;                       /* host, [1] */
  double *d_phi, *d_gamma, *d_delta, *d_map;     /* device or NULL, as kdehip_sinkhorn_device */
  int32_t maxiter;
  uint32_t circular_mask;               /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
} kdehip_sinkhorn_item;
/* Many pairs (mixed D, sizes, cross and self) on one device: the items share the launches of every half-step, and every item's
 * results are bit for bit those of kdehip_sinkhorn_device at the same scale.  One bad item fails the whole call. */
int kdehip_sinkhorn_device_batch(int n, const kdehip_sinkhorn_item *items);

/* ---- (5t) compression: a density cut to M of its own points by kernel herding (csrc/compress.hip) ------------------------
 * The library's own; the reference has no counterpart.  resample and sample go from N points to M at random and repeat
 * points; herding picks, one after another, the points of p that best match p's kernel mean embedding, and the MMD of the
 * equal-weight density on the picks falls like 1/M where random subsets give 1/sqrt(M).
 *   c_i (i < N) are the leaf points of p in tree order, alpha_i their weights as the density holds them, o(i) their original
 *     index (0-based; the permutation's leaf row minus 1).
 *   v_k are the kernel variances: the caller's var (D entries), or with var = NULL twice p's leaf variance -- the quantity
 *     minimised is then, up to the Gaussian constant, the integrated squared error between p and the equal-weight density on
 *     the picks at p's own bandwidth (what `ise` measures).  nh_k = -0.5 / v_k.
 *   Exponent: a(s, j) = sum_k fma(d_k^2, nh_k, acc), k ascending from acc = 0, d_k = c_jk - c_sk, through wrap() in a
 *     circular dimension (5d): the expression and fma order of the direct kernel, leaf j the query and leaf s the source.
 *   Kernel mean: z_j = sum_i alpha_i exp(a(i, j)), by the all-pairs sweep in the summation order of 5b: the 128-leaf chunks of
 *     a group in order, then the groups in ascending order (the split depends on N alone).
 *   Self sum: self_sum = sum_j alpha_j z_j: 256 partial sums, sum t over j = t, t + 256, .. ascending, combined in the fixed
 *     256-wide tree of 5b.
 *   Steps, t = 0 .. M-1, from r_j = 0:
 *     score_j = z_j - r_j * inv_t, inv_t = 1.0 / (double)(t + 1) (a correctly rounded division); the product and the
 *       difference are each rounded: NO fused multiply-add, so that a NumPy model has the same bits;
 *     the pick s_t is the not-yet-chosen j with the largest (score_j, -o(j)): ties go to the lower original index;
 *     idx[t] = o(s_t) + 1, zpick[t] = z_{s_t}, rpick[t] = r_{s_t} as they stand at the pick;
 *     then r_j += exp(a(s_t, j)) for every j.
 *   Points of weight 0 are candidates like any other.  1 <= M <= N.  fp64 only.
 * From the traces a caller forms the whole curve of the squared MMD (without the Gaussian constant) between p and the
 * equal-weight density on the first m picks,
 *   mmd2(m) = self_sum - (2/m) sum_{t<m} zpick[t] + (m + 2 sum_{t<m} rpick[t]) / m^2,
 * and the run is ANYTIME: the first m picks and traces of a run to M are bit for bit the run to m.
 * Two routes with the same bits (the pick is the maximum of a total order and every r_j grows in step order, so nothing
 * depends on how the leaves are dealt to lanes, wavefronts or workgroups; no atomics):
 *   route A, N <= KDEHIP_COMPRESS_ONE_BLOCK_MAX: ONE workgroup runs all M steps in one launch, a lane's leaves in registers;
 *   route B, any N: one plain launch per step (M + 1 in all, enqueued back to back); KDEHIP_COMPRESS_STEPWISE in flags forces it.
 * No grid-wide barrier, no cooperative launch, no spinning on memory.  The z pass is one launch per distinct (D, circular,
 * route) of a call's items, route A one launch per distinct (D, circular) for the items that fit.
 * All four entries are BLOCKING and take no stream; the caller's own work on p must be complete when the call is made.
 * Errors, all checked before any device is touched: KDEHIP_ERR_ARG for a null p, idx or handle, M < 1 or M > N, a var or ks
 * entry not finite or <= 0, unknown flag bits, a manifold byte above 1 or a mask bit at or above ndims, 2^31 points or more,
 * densities of a batch on different devices; KDEHIP_ERR_UNSUPPORTED for ndims outside 1..KDEHIP_MAX_DIMS and for per-point
 * bandwidths without var.
 * Not here: weights other than 1/M, herding towards another target than p's own kernel mean, fp32, an enqueue-only form. */
#define KDEHIP_COMPRESS_ONE_BLOCK_MAX 2048 /* route A: 1024 threads x 2 leaves in registers */
#define KDEHIP_COMPRESS_STEPWISE 1         /* flags: route B whatever N */
/* A host density, host results.  idx [M] (1-based, by ORIGINAL point); zpick, rpick [M] and self_sum [1]: each optional (NULL). */
int kdehip_compress(const kdehip_density *p, int64_t M, const double *var /* D, or NULL */, int flags, int64_t *idx,
                    double *zpick, double *rpick, double *self_sum, int device, const uint8_t *manifold);
/* A resident density; var is a HOST pointer.  DEVICE results: d_idx [M]; d_points [ndims x M column-major, in pick order],
 * d_zpick, d_rpick [M], d_self_sum [1]: each optional (NULL).  Complete on return. */
int kdehip_compress_device(const kdehip_device_density *p, int64_t M, const double *var, int flags, int64_t *d_idx,
                           double *d_points, double *d_zpick, double *d_rpick, double *d_self_sum, const uint8_t *manifold);
typedef struct kdehip_compress_item {
  const kdehip_device_density *p;
  const double *var;                    /* HOST pointer, D entries, or NULL */
  int64_t M;
  int64_t *d_idx;                       /* device, [M] */
  double *d_points, *d_zpick, *d_rpick, *d_self_sum;   /* device or NULL, as kdehip_compress_device */
  uint32_t flags;                       /* KDEHIP_COMPRESS_STEPWISE or 0 */
  uint32_t circular_mask;               /* bit d = dimension d circular; a bit at or above ndims is KDEHIP_ERR_ARG */
  kdehip_device_density **out;          /* HOST pointer or NULL: also the compressed density, as kdehip_density_compress_device
                                           builds it (d_idx may then be NULL) */
  const double *ks;                     /* HOST pointer, D standard deviations, or NULL = p's own; read with out only */
  const uint8_t *tree_manifold;         /* ndims bytes or NULL; read with out only */
} kdehip_compress_item;
/* Many densities (mixed D, N and M, Euclidean and circular, both routes) on one device in one call; every item's results are
 * bit for bit those of kdehip_compress_device, its density that of kdehip_density_compress_device: the picks of all items come
 * down in ONE copy.  One bad item fails the whole call and returns no handle. */
int kdehip_compress_device_batch(int n, const kdehip_compress_item *items);
/* The compressed density as a NEW resident handle, by the route of kdehip_density_marginal_device (5c): the picks gathered on
 * the device in pick order, ONE copy down, the host builder with bandwidth ks (D standard deviations; NULL = p's own, which
 * must then be one vector), weights 1/M and the operators of tree_manifold (5e, or NULL), the block back up:
 * kde!(getPoints(p)[:, idx], ks, fill(1/M, M)).  On an error *out = NULL. */
int kdehip_density_compress_device(kdehip_device_density **out, const kdehip_device_density *p, int64_t M, const double *var,
                                   const double *ks, const uint8_t *manifold, const uint8_t *tree_manifold);

#ifdef __cplusplus
}
#endif
#endif /* KDEHIP_H */
