"""Host-side mirror of the reference's product API over the libkdehip.so C ABI.

Mirrors `prodAppxMSGibbsS` (reference src/MSGibbs01.jl:645-703) and `gibbs1` (:527-629) -- same
argument names and meaning, same return value `(points[ndims, Np], indices[Ndens, Np])`, same error
behaviour (dimension mismatch -> error, short randU/randN -> IndexError like Julia's BoundsError).
All computation happens in the HIP kernels; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib, manifold as _mf
from ._lib import SEED_MASK, addr, f64p, i64p, i32p, optr, ptr, u8p, u64
from .density import BallTreeDensity, Ndim, Npts


# the names manifold.parse / manifold.per_product had while they lived here (tests and scripts import them from this module)
_manifold_array, _batch_manifolds = _mf.parse, _mf.per_product


def _mask_array(partialDimMask, Ndens, ndims):
    if partialDimMask is None:
        return None
    m = np.ascontiguousarray(np.asarray(partialDimMask, dtype=bool).reshape(Ndens, ndims).astype(np.uint8))
    return m


def nlevels(maxNp: int) -> int:
    """floor(Int, log(maxNp)/log(2) + 1) (reference src/MSGibbs01.jl:568, :660)."""
    return int(math.floor(math.log(float(maxNp)) / math.log(2.0) + 1.0))


class ProductPlan:
    """Densities of one product, re-laid-out per level and resident in HBM (kdehip_product_*).

    Keeps inputs on the device across calls: the timed region of bench.py and repeated products on
    the same densities start from HBM-resident data.
    `manifold`: the per-dimension enum of `gibbs1` -- every run of the plan applies the circular operators
    (kdehip_product_create_manifold; precision 64 only), with the numbers of `prodAppxMSGibbsS_device(manifold=)`.
    """

    def __init__(self, trees, partialDimMask=None, precision=64, device=0, ndims=None, manifold=None):
        trees = list(trees)
        self.Ndens = len(trees)
        self.ndims = int(ndims) if ndims is not None else max(Ndim(t) for t in trees)
        self._keep = trees  # arrays must outlive the create call only; kept for introspection
        self.manifold = _mf.parse(manifold, self.ndims, unknown_name=ValueError)   # the uint8 enum array, or None
        arr = (_lib.CDensity * self.Ndens)(*[t._cstruct() for t in trees])
        mask = _mask_array(partialDimMask, self.Ndens, self.ndims)
        h = C.c_void_p()
        _lib.check(_lib.lib.kdehip_product_create_manifold(C.byref(h), self.Ndens, arr, self.ndims,
                                                           optr(mask, u8p), _mf.pointer(self.manifold),
                                                           int(precision), int(device)))
        self._h = h
        info = _lib.CProductInfo()
        _lib.check(_lib.lib.kdehip_product_info(self._h, C.byref(info)))
        self.nlevels = info.nlevels
        self.precision = info.precision
        self.nodes_per_sweep = info.nodes_per_sweep
        self.bytes_per_eval = info.bytes_per_eval
        self.packed_bytes = info.packed_bytes
        self.fast_math_path = bool(info.fast_math_path)
        self.device = info.device

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.kdehip_product_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- work model -------------------------------------------------------------
    def randu_per_sample(self, Niter: int) -> int:
        return int(_lib.lib.kdehip_product_randu_per_sample(self._h, int(Niter)))

    def randn_per_sample(self) -> int:
        return int(_lib.lib.kdehip_product_randn_per_sample(self._h))

    def evals_per_sample(self, Niter: int) -> int:
        """E = (Niter+1) * sum_j sum_l n_{j,l} Gaussian-kernel evaluations per output sample."""
        return (int(Niter) + 1) * int(self.nodes_per_sweep)

    def fallback_count(self) -> int:
        """Label draws of this plan's runs that took the reference's `pT < 1e-99` uniform fallback (:311-315)."""
        n = int(_lib.lib.kdehip_product_fallback_count(self._h))
        if n < 0:
            _lib.check(n)
        return n

    def screen_stats(self) -> dict:
        """fp32 screening (kdehip_product_screen_stats): screened levels, label draws taken on them, draws repeated in fp64."""
        lv, st, rp = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.lib.kdehip_product_screen_stats(self._h, C.byref(lv), C.byref(st), C.byref(rp)))
        return {"levels": int(lv.value), "steps": int(st.value), "repeats": int(rp.value)}

    def set_variant(self, v: int):
        _lib.check(_lib.lib.kdehip_product_set_variant(self._h, int(v)))

    def kernel_name(self, Np: int) -> str:
        """the sampling kernel a run of Np chains launches: "gibbs_lean_kernel" or "gibbs_product_kernel" """
        return _lib.lib.kdehip_product_kernel_name(self._h, int(Np)).decode()

    def launch_geometry(self, Np: int) -> dict:
        """Wavefronts per workgroup a run of Np chains gets under the current variant (`team`: always 1, kept for callers)."""
        w, t = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib.kdehip_product_launch_geometry(self._h, int(Np), C.byref(w), C.byref(t)))
        return {"waves": int(w.value), "team": int(t.value)}

    # ---- device-pointer runs (torch tensors or raw addresses) -----------------------------------
    _addr = staticmethod(addr)   # (kept for the scripts and tests that call it)

    def sample_philox_device(self, Np, Niter, seed, sample_offset, addEntropy, d_points, d_indices,
                             d_labels=None, stream=None):
        _lib.check(_lib.lib.kdehip_product_sample_philox(
            self._h, int(Np), int(Niter), u64(seed), int(sample_offset), int(bool(addEntropy)), addr(d_points),
            addr(d_indices), addr(d_labels), addr(stream)))

    def sample_streams_device(self, Np, Niter, d_randU, nU, d_randN, nN, addEntropy, d_points, d_indices,
                              d_labels=None, stream=None):
        _lib.check(_lib.lib.kdehip_product_sample_streams(
            self._h, int(Np), int(Niter), addr(d_randU), int(nU), addr(d_randN), int(nN),
            int(bool(addEntropy)), addr(d_points), addr(d_indices), addr(d_labels), addr(stream)))

    # ---- host-buffer run -------------------------------------------------------------------------
    def sample(self, Np, Niter=3, seed=0, sample_offset=0, addEntropy=True, want_labels=False):
        """Np chains with the on-device Philox stream; returns (points[D,Np], indices[M,Np][, labels])."""
        D, M, L = self.ndims, self.Ndens, self.nlevels
        pts = np.zeros(D * Np)
        ind = np.ones(M * Np, dtype=np.int64)
        labels = np.zeros(Np * M * L, dtype=np.int32) if want_labels else None
        _lib.check(_lib.lib.kdehip_product_sample_philox_host(
            self._h, int(Np), int(Niter), u64(seed), int(sample_offset), int(bool(addEntropy)), ptr(pts, f64p),
            ptr(ind, i64p), optr(labels, i32p)))
        out = (pts.reshape(Np, D).T.copy(), ind.reshape(Np, M).T.copy())
        if want_labels:
            out = out + (labels.reshape(Np, M, L),)
        return out


class MultiProductPlan:
    """One resident plan per GPU of a node, one process (kdehip_product_multi_*): chains in contiguous ranges, Philox
    counters keyed by the global sample index, one all-gather of [pGM | indices] fused into the sampling kernel (peer
    stores over xGMI), after which every device holds the complete result.  `manifold`: as `ProductPlan`
    (kdehip_product_multi_create_manifold): the circular plan on every device, the same result for every `ngpus`."""

    def __init__(self, trees, partialDimMask=None, precision=64, first_device=0, ngpus=1, ndims=None, manifold=None):
        trees = list(trees)
        self.Ndens = len(trees)
        self.ndims = int(ndims) if ndims is not None else max(Ndim(t) for t in trees)
        self.manifold = _mf.parse(manifold, self.ndims, unknown_name=ValueError)
        arr = (_lib.CDensity * self.Ndens)(*[t._cstruct() for t in trees])
        mask = _mask_array(partialDimMask, self.Ndens, self.ndims)
        h = C.c_void_p()
        _lib.check(_lib.lib.kdehip_product_multi_create_manifold(C.byref(h), self.Ndens, arr, self.ndims,
                                                                 optr(mask, u8p), _mf.pointer(self.manifold),
                                                                 int(precision), int(first_device), int(ngpus)))
        self._h = h
        self.first_device = int(first_device)
        self.ngpus = int(_lib.lib.kdehip_product_multi_ngpus(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.kdehip_product_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def transfers_per_product(self) -> int:
        """copy-engine transfers each device issues per product: 0 = the all-gather is fused into the sampling kernel
        (stores to the peer-mapped arrays of the other devices)"""
        return int(_lib.lib.kdehip_product_multi_transfers_per_product(self._h))

    def timing(self):
        """(kernel_ms[g], done_ms[g]) of the last product, with `kdehip_profile_sampler(1)` on: duration of every device's
        sampling launch, and when its slice had arrived everywhere relative to the first device (kdehip_product_multi_timing)"""
        k, d = np.zeros(self.ngpus), np.zeros(self.ngpus)
        _lib.check(_lib.lib.kdehip_product_multi_timing(self._h, ptr(k, f64p), ptr(d, f64p)))
        return k, d

    def sample_philox_device(self, Np, Niter, seed, sample_offset, addEntropy, d_points, d_indices, streams=None):
        """d_points / d_indices: one device array (torch tensor or address) per GPU, each holding the COMPLETE result
        afterwards (the all-gather is part of the run); enqueue only."""
        G = self.ngpus
        P = (C.c_void_p * G)(*[addr(x) for x in d_points])
        I = (C.c_void_p * G)(*[addr(x) for x in d_indices])
        S = None if streams is None else (C.c_void_p * G)(*[addr(x) for x in streams])
        _lib.check(_lib.lib.kdehip_product_multi_sample_philox(self._h, int(Np), int(Niter),
                                                               u64(seed), int(sample_offset),
                                                               int(bool(addEntropy)), P, I, S))


class DeviceDensity:
    """A BallTreeDensity kept in HBM: uploaded ONCE (kdehip_density_upload), or built there from a product that never left
    the device (`from_device_points`, `mul_device`).  Products of such densities are laid out by the GPU and move nothing
    but a few KB of descriptors over PCIe (`prodAppxMSGibbsS_device`)."""

    def __init__(self, tree: BallTreeDensity = None, device=0, _handle=None):
        if _handle is None:
            h = C.c_void_p()
            cs = tree._cstruct()
            _lib.check(_lib.lib.kdehip_density_upload(C.byref(h), C.byref(cs), int(device)))
        else:
            h = _handle
        self._h = h
        # An uploaded density's arrays stay the caller's (`download` serves built densities only): `modes` reads the bandwidth
        # and the weights for its host-side merge from this object.  It is a reference, not a copy: a caller who changes the
        # host density after the upload makes the merge disagree with what the device iterates on.
        self._host = tree if _handle is None else None
        self.device = int(device)
        self.num_points = int(_lib.lib.kdehip_density_npts(h))
        self.dims = int(_lib.lib.kdehip_density_ndim(h))
        self.bw = None      # LOOCV bandwidth (standard deviations) of a density built on the device
        self.nevals = None  # likelihood evaluations of that search
        # the manifold it was built with (`from_device_points(manifold=)`, a circular `mul_device`), as the uint8 enum array,
        # or None.  A record only: `a * b` stays Euclidean; `resample`, `sample` and the summaries take `manifold="inherit"`
        self.manifold = None
        # the operators its tree was built with (`tree_manifold=`), likewise a record only; an uploaded density keeps its own
        self.tree_manifold = getattr(tree, "tree_manifold", None) if _handle is None else None

    @classmethod
    def _built(cls, handle, device, bw=None, nevals=None, manifold=None, tree_manifold=None):
        """a handle the library has just built, with the records of how: bandwidth, search evaluations, manifolds"""
        out = cls(device=device, _handle=handle)
        out.bw, out.nevals, out.manifold, out.tree_manifold = bw, nevals, manifold, tree_manifold
        return out

    @classmethod
    def from_device_points(cls, d_points, D, N, device=0, stream=None, manifold=None, tree_manifold=None):
        """`kde!(points)` (reference src/KDE01.jl:3-27) of a D x N column-major matrix that lives in HBM (a torch tensor or
        an address; `stream` = the stream that produced it): LOOCV bandwidth search on the device matrix, ball tree from one
        copy that comes down meanwhile, the density's block straight back up (kdehip_density_from_device_points).
        `manifold`: the bandwidth search of a circular dimension wraps its differences (the tree stays Euclidean);
        `tree_manifold`: the tree builder's operators, as `kde(..., tree_manifold=)` (kdehip_density_from_device_points_tree)."""
        h = C.c_void_p()
        bw = np.empty(int(D))
        ne = C.c_int32(0)
        man = _mf.parse(manifold, int(D))
        tman = _mf.parse(tree_manifold, int(D))
        _lib.check(_lib.lib.kdehip_density_from_device_points_tree(
            C.byref(h), addr(d_points), int(D), int(N), int(device), addr(stream), ptr(bw, f64p),
            C.byref(ne), _mf.pointer(man), _mf.pointer(tman)))
        return cls._built(h, device, bw, int(ne.value), man, tman)

    def download(self) -> BallTreeDensity:
        """The reference's arrays of a density that was built on the device (kdehip_density_download)."""
        from .density import _empty_density
        i64p = _lib.i64p
        bd = _empty_density(self.dims, self.num_points)
        bt = bd.bt
        _lib.check(_lib.lib.kdehip_density_download(
            self._h, ptr(bt.centers, f64p), ptr(bt.ranges, f64p), ptr(bt.weights, f64p), ptr(bt.left_child, i64p),
            ptr(bt.right_child, i64p), ptr(bt.lowest_leaf, i64p), ptr(bt.highest_leaf, i64p), ptr(bt.permutation, i64p),
            ptr(bd.means, f64p), ptr(bd.bandwidth, f64p), ptr(bd.bandwidthMin, f64p), ptr(bd.bandwidthMax, f64p), None))
        bd.tree_manifold = self.tree_manifold
        return bd

    def __mul__(self, other):
        """the Euclidean `*`, also for densities that remember a manifold: use `mul_device(..., manifold=)` on the circle"""
        return mul_device([self, other])

    def evaluate(self, pos=None, lvFlag=False, manifold=None, *, _log=False):
        """`evaluateDualTree(bd, pos, lvFlag)` (reference src/DualTree01.jl:370-421, FORCE_EVAL_DIRECT) on the device
        (kdehip_evaluate_device / kdehip_evaluate_device_at): every value is bit for bit what `evaluateDualTree` gives on the
        density's host arrays.  `pos`: a (D, Nq) numpy array -- values in query order, as a numpy array --, a float64 (D, Nq)
        torch tensor on the density's device -- a device tensor, enqueued on the current torch stream --, or a DeviceDensity
        -- values at its points in ITS original order (getPoints order), as a numpy array.  `pos is self` or lvFlag=True:
        leave-one-out at the density's own points, original order.  `manifold`: circular differences in those dimensions
        (include/kdehip.h section 5d).  A density whose leaves do not share one bandwidth vector
        (kdehip_density_uniform_bandwidth) goes to the entries of section 5o."""
        import torch
        dev = torch.device("cuda", self.device)
        man = _mf.parse(manifold, self.dims)
        mp = _mf.pointer(man)
        if lvFlag:
            pos = self
        if pos is None:
            raise TypeError("evaluate: pos is required unless lvFlag=True")
        varbw = bool(self._h) and not _lib.lib.kdehip_density_uniform_bandwidth(self._h)  # per-point bandwidths: section 5o
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            if isinstance(pos, DeviceDensity):
                if pos.dims != self.dims:
                    raise ValueError("bd and pos must have the same dimension")
                out = torch.empty(max(1, pos.num_points), dtype=torch.float64, device=dev)
                if varbw:
                    _lib.check(_lib.lib.kdehip_evaluate_varbw_device_at(self._h, pos._h, 1 if pos is self else 0, int(_log),
                                                                        addr(out), addr(st.cuda_stream), mp))
                else:
                    at_entry = _lib.lib.kdehip_evaluate_log_device_at if _log else _lib.lib.kdehip_evaluate_device_at_manifold
                    _lib.check(at_entry(self._h, pos._h, addr(out), addr(st.cuda_stream), mp))
                st.synchronize()
                return out.cpu().numpy()[:pos.num_points].copy()
            tensor = hasattr(pos, "data_ptr")
            P = pos if tensor else np.asarray(pos, dtype=np.float64)
            if P.ndim == 1:
                P = P.reshape(1, -1)
            if P.shape[0] != self.dims:
                raise ValueError("bd and pos must have the same dimension")
            Nq = int(P.shape[1])
            # column-major D x Nq = the (Nq, D) row-major array
            flat = P.t().contiguous().to(dev, torch.float64) if tensor else torch.from_numpy(np.ascontiguousarray(P.T)).to(dev)
            out = torch.empty(max(1, Nq), dtype=torch.float64, device=dev)
            if varbw:
                _lib.check(_lib.lib.kdehip_evaluate_varbw_device(self._h, addr(flat), Nq, int(_log), addr(out),
                                                                 addr(st.cuda_stream), mp))
            else:
                entry = _lib.lib.kdehip_evaluate_log_device if _log else _lib.lib.kdehip_evaluate_device_manifold
                _lib.check(entry(self._h, addr(flat), Nq, 0, addr(out), addr(st.cuda_stream), mp))
            if tensor:
                return out[:Nq]
            st.synchronize()
            return out.cpu().numpy()[:Nq].copy()

    def evaluate_log(self, pos=None, lvFlag=False, manifold=None):
        """log of `.evaluate(pos, lvFlag, manifold)` by log-sum-exp in the kernel (kdehip_evaluate_log_device /
        kdehip_evaluate_log_device_at, include/kdehip.h section 5f): finite where the density underflows to 0.  The same
        shapes and return kinds as `.evaluate`, the `at` form (pos a DeviceDensity) included."""
        if isinstance(pos, BallTreeDensity):
            raise TypeError("evaluate_log: a DeviceDensity is evaluated at points or at a DeviceDensity")
        return self.evaluate(pos, lvFlag, manifold=manifold, _log=True)

    def __call__(self, pos=None, lvFlag=False, manifold=None):
        return self.evaluate(pos, lvFlag, manifold=manifold)

    def evaluate_tol(self, at=None, rel_tol=1e-3, abs_tol=0.0, manifold=None, return_stats=False):
        """`.evaluate(at)` within a tolerance (kdehip_evaluate_device_at_tol, include/kdehip.h section 5m): this density at
        the points of the DeviceDensity `at`, processed in ITS leaf order, values in its original order as a numpy array;
        `at` None or self: leave-one-out at the density's own points.  p (1 - rel_tol) - abs_tol <= value <= p, bit for bit
        `kdehip.evaluate_tol` of the host arrays.  return_stats=True: also (tiles visited, tiles in all)."""
        import torch
        at = self if at is None else at
        if not isinstance(at, DeviceDensity):
            raise TypeError("evaluate_tol: a DeviceDensity is evaluated within a tolerance at a DeviceDensity")
        if at.dims != self.dims:
            raise ValueError("bd and pos must have the same dimension")
        dev = torch.device("cuda", self.device)
        man = _mf.parse(manifold, self.dims)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            out = torch.empty(max(1, at.num_points), dtype=torch.float64, device=dev)
            stats = torch.zeros(2, dtype=torch.int64, device=dev)
            _lib.check(_lib.lib.kdehip_evaluate_device_at_tol(
                self._h, at._h, C.byref(C.c_double(float(rel_tol))), C.byref(C.c_double(float(abs_tol))), addr(out),
                addr(stats), addr(st.cuda_stream), _mf.pointer(man)))
            st.synchronize()
            vals = out.cpu().numpy()[:at.num_points].copy()
            if return_stats:
                s = stats.cpu().numpy()
                return vals, (int(s[0]), int(s[1]))
            return vals

    def knn(self, at=None, k=1, metric="euclid", manifold=None, squared=False, return_stats=False):
        """The k points of this density nearest to every point of the DeviceDensity `at` (kdehip_knn_device_at, include/kdehip.h
        section 5n): `(dist, idx)`, numpy arrays of shape (k, at's npts) in ITS original point order, `idx` 1-based among this
        density's points; `at` None or self: every point's neighbours among the others, itself left out by index.  Bit for
        bit `kdehip.knn` of the host arrays.  return_stats=True: also (tiles visited, tiles in all)."""
        import torch
        from .knn import _finish, _scale
        at = self if at is None else at
        if not isinstance(at, DeviceDensity):
            raise TypeError("knn: a DeviceDensity is searched from the points of a DeviceDensity")
        if at.dims != self.dims:
            raise ValueError("bd and pos must have the same dimension")
        k = int(k)
        dev = torch.device("cuda", self.device)
        man = _mf.parse(manifold, self.dims)
        sc = _scale(self, metric, self.dims)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            n = max(1, at.num_points * max(k, 1))
            d2 = torch.empty(n, dtype=torch.float64, device=dev)
            idx = torch.empty(n, dtype=torch.int64, device=dev)
            stats = torch.zeros(2, dtype=torch.int64, device=dev)
            _lib.check(_lib.lib.kdehip_knn_device_at(self._h, at._h, k, _lib.optr(sc, f64p), addr(d2), addr(idx), addr(stats),
                                                     addr(st.cuda_stream), _mf.pointer(man)))
            st.synchronize()
            shape = (at.num_points, k)
            return _finish(np.ascontiguousarray(d2.cpu().numpy()[:shape[0] * k].reshape(shape).T),
                           np.ascontiguousarray(idx.cpu().numpy()[:shape[0] * k].reshape(shape).T), stats.cpu().numpy(),
                           squared, return_stats)

    def evaluate_grad(self, pos, *, log=True, manifold=None):
        """(log p, its gradient) -- or (p, its gradient) with log=False -- at the columns of `pos` (kdehip_evaluate_grad_device,
        include/kdehip.h section 5h): `kdehip.evaluate_grad` of this density."""
        from .modes import evaluate_grad
        return evaluate_grad(self, pos, log=log, manifold=manifold)

    def joint_bandwidth(self, start=None, tol=1e-3, maxiter=200, manifold=None, return_info=False):
        """The (D,) standard deviations of the joint leave-one-out iteration from `start` (kdehip_bandwidth_joint_device,
        include/kdehip.h section 5q): `kdehip.joint_bandwidth` of this density."""
        from .bwjoint import joint_bandwidth
        return joint_bandwidth(self, start, tol, maxiter, manifold, return_info)

    def evaluate_hess(self, pos, *, log=True, manifold=None):
        """(log p, its gradient, its Hessian) at the columns of `pos` (kdehip_evaluate_hess_device, include/kdehip.h section
        5k): `kdehip.evaluate_hess` of this density."""
        from .curvature import evaluate_hess
        return evaluate_hess(self, pos, log=log, manifold=manifold)

    def laplace(self, pos, *, manifold=None):
        """(cov, definite) at the columns of `pos`: `kdehip.laplace` of this density."""
        from .curvature import laplace
        return laplace(self, pos, manifold=manifold)

    def fit_modes(self, starts=None, **kw):
        """(means, covs, mass, logp, definite): `kdehip.fit_modes` of this density."""
        from .curvature import fit_modes
        return fit_modes(self, starts, **kw)

    def box_mass(self, lo, hi, dims=None, *, manifold=None):
        """the probability of the boxes [lo, hi] over `dims` (kdehip_box_mass_device, include/kdehip.h section 5l):
        `kdehip.box_mass` of this density."""
        from .mass import box_mass
        return box_mass(self, lo, hi, dims, manifold=manifold)

    def cdf(self, x, dim, *, manifold=None):
        """the marginal cdf of dimension `dim` at `x`: `kdehip.cdf` of this density."""
        from .mass import cdf
        return cdf(self, x, dim, manifold=manifold)

    def quantile(self, alpha, dim, **kw):
        """the `alpha` quantiles of the marginal of dimension `dim` (kdehip_quantile_device): `kdehip.quantile` of this density."""
        from .mass import quantile
        return quantile(self, alpha, dim, **kw)

    def interval(self, dim, level=0.95, **kw):
        """(lo, hi), the central credible interval of dimension `dim`: `kdehip.interval` of this density."""
        from .mass import interval
        return interval(self, dim, level, **kw)

    def sample_device(self, d_pts, d_ind, Npts, *, seed, sample_offset=0, ind=None, stream=None, manifold=None):
        """`sample(p, Npts[, ind])` (reference src/KDE01.jl:164-189) into caller device arrays (torch tensors or addresses):
        d_pts float64[D*Npts] (column-major D x Npts), d_ind int64[Npts] (1-based original indices), `ind` an optional
        device int64[Npts] of given labels.  The first call on the density builds its table and blocks; later calls only
        enqueue on `stream` (kdehip_sample_device).  `manifold` (a sequence or "inherit"): circular coordinates are stored
        wrapped to [-pi, pi) (kdehip_sample_device_manifold)."""
        man = _mf.resolve(self, manifold, self.dims)
        _lib.check(_lib.lib.kdehip_sample_device_manifold(self._h, int(Npts), u64(seed), int(sample_offset), addr(ind),
                                                          addr(d_pts), addr(d_ind), addr(stream), _mf.pointer(man)))

    def prod_exact(self, other, d_pts, d_ind, *, Np, seed, sample_offset=0, d_logz=None, stream=None):
        """Np exact draws of the product self * other (include/kdehip.h section 5p) into caller device arrays (torch tensors
        or addresses): d_pts float64[Np][D] (= column-major D x Np), d_ind int64[Np][2] (1-based original indices in self
        and other), d_logz an optional float64[1] for log int p q; d_pts and d_ind may both be None when d_logz is given.
        Enqueue only on `stream`, no read-back (kdehip_prod_exact_device)."""
        if not isinstance(other, DeviceDensity):
            raise TypeError("both densities must be BallTreeDensity, or both DeviceDensity")
        _lib.check(_lib.lib.kdehip_prod_exact_device(self._h, other._h, int(Np), u64(seed), int(sample_offset), addr(d_pts),
                                                     addr(d_ind), addr(d_logz), addr(stream)))

    def resample(self, Np=None, *, seed=None, manifold=None, tree_manifold=None) -> "DeviceDensity":
        """`resample(p, Np, :lcv)` (reference src/BallTreeDensity01.jl:312-334) without leaving the device: Np samples
        (None = Npts(p)), then `kde!(points)` on the device matrix (kdehip_resample_device).  The default is Euclidean, also
        for a density that remembers a manifold; `manifold` / `tree_manifold` (sequences or "inherit"): the wrapped draw,
        then `from_device_points(manifold=, tree_manifold=)` on it (kdehip_resample_device_manifold) -- the result
        remembers both."""
        man = _mf.resolve(self, manifold, self.dims)
        tman = _mf.resolve(self, tree_manifold, self.dims, attr="tree_manifold")
        if seed is None:
            seed = _lib.random_seed()
        h = C.c_void_p()
        bw = np.empty(self.dims)
        ne = C.c_int32(0)
        _lib.check(_lib.lib.kdehip_resample_device_manifold(C.byref(h), self._h, 0 if Np is None else int(Np), u64(seed),
                                                            ptr(bw, f64p), C.byref(ne), _mf.pointer(man), _mf.pointer(tman)))
        return self._built(h, self.device, bw, int(ne.value), man, tman)

    def changeWeights(self, w) -> "DeviceDensity":
        """`changeWeights!` (reference src/BallTreeDensity01.jl:278-292) as a NEW resident density: weights w (N, original
        point order, used as given; a tensor stays on the device), the same tree, the node statistics recomputed on the GPU
        (kdehip_density_refit_device, include/kdehip.h section 5r)."""
        from .refit import WEIGHTS, refit_device
        return refit_device(self, w, WEIGHTS)[0]

    def movePoints(self, delta) -> "DeviceDensity":
        """`movePoints!` (reference src/BallTreeDensity01.jl:295-309) as a NEW resident density: every point moved by its
        column of delta ((D, N), original order), the same -- now looser -- tree; the tree's recorded operators wrap the sum
        in a circular dimension."""
        from .refit import KEEP, refit_device
        return refit_device(self, None, KEEP, delta)[0]

    def bayes_update(self, logl, leaf_order=False):
        """`w_i <- w_i L(x_i)` without leaving HBM: (DeviceDensity, log_evidence, ess).  logl: N log-likelihoods (by original
        point, or by leaf position with leaf_order=True), or a DeviceDensity likelihood evaluated at this density's points."""
        from .refit import device_bayes_update
        return device_bayes_update(self, logl, leaf_order)

    @classmethod
    def refit_batch(cls, items):
        """many refits in one call (kdehip_density_refit_device_batch): see `refit.refit_batch`"""
        from .refit import refit_batch
        return refit_batch(items)

    # entropic optimal transport onto another resident density (include/kdehip.h section 5s): see transport.py
    def sinkhorn(self, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False):
        """the entropic transport value between this density and q (`q is self`: the symmetric iteration)"""
        from .transport import sinkhorn
        return sinkhorn(self, q, reg, scale, tol, maxiter, manifold, return_info)

    def sinkhorn_divergence(self, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False):
        """value(self, q) - value(self, self) / 2 - value(q, q) / 2 in one batched run; 0.0 when q is self"""
        from .transport import sinkhorn_divergence
        return sinkhorn_divergence(self, q, reg, scale, tol, maxiter, manifold, return_info)

    def transport_map(self, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False):
        """T (D, N), a device tensor: the barycentric image of every point under the plan onto q"""
        from .transport import transport_map
        return transport_map(self, q, reg, scale, tol, maxiter, manifold, return_info)

    def transport_to(self, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False) -> "DeviceDensity":
        """`movePoints` by the barycentric displacement onto q: a new density; nothing leaves HBM"""
        from .transport import transport_to
        return transport_to(self, q, reg, scale, tol, maxiter, manifold, return_info)

    def equalize(self, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False) -> "DeviceDensity":
        """the ensemble transform: the points moved so that equal weights represent this density"""
        from .transport import equalize
        return equalize(self, reg, scale, tol, maxiter, manifold, return_info)

    @staticmethod
    def sinkhorn_batch(pairs, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, vectors=False):
        """many pairs in one call (kdehip_sinkhorn_device_batch): see `transport.sinkhorn_batch`"""
        from .transport import sinkhorn_batch
        return sinkhorn_batch(pairs, reg, scale, tol, maxiter, manifold, vectors)

    # compression by kernel herding (include/kdehip.h section 5t): see compress.py
    def compress(self, M=None, mmd_tol=None, bw=None, ks=None, manifold=None, return_info=False, tree_manifold=None,
                 stepwise=False) -> "DeviceDensity":
        """M of this density's own points, picked by kernel herding, as a new resident density with weights 1 / M and
        bandwidth `ks` (None: unchanged); the points come to the host through the builder's one copy alone"""
        from .compress import _compress
        return _compress(self, M, mmd_tol, bw, ks, manifold, return_info, tree_manifold, stepwise)

    def herding_order(self, M, bw=None, manifold=None, stepwise=False):
        """(idx, info): the first M herding picks (1-based, by original point) and their traces; nothing is built"""
        from .compress import _herding_order
        return _herding_order(self, M, bw, manifold, stepwise)

    @staticmethod
    def compress_batch(densities, M, bw=None, ks=None, manifold=None, return_info=False, tree_manifold=None, stepwise=False):
        """many densities in one call (kdehip_compress_device_batch): a list of new handles; see `compress._compress_batch`"""
        from .compress import _compress_batch
        return _compress_batch(densities, M, bw, ks, manifold, return_info, tree_manifold, stepwise)

    def marginal(self, dims, *, manifold=None, tree_manifold=None) -> "DeviceDensity":
        """`marginal(p, dims)` (reference src/KDE01.jl:143-153), dims 0-based, built on this density's device
        (kdehip_density_marginal_device): the same arrays as the host `marginal` of the same density.  `tree_manifold` (one
        entry per dimension of this density, or "inherit"): the tree is built with tree_manifold[dims]
        (kdehip_density_marginal_device_tree); the result remembers manifold[dims] and tree_manifold[dims]."""
        from .summary import _marginal_device
        return _marginal_device(self, dims, manifold, tree_manifold)

    def condition(self, dims, values, *, manifold=None, tree_manifold=None) -> "DeviceDensity":
        """p(x_F | x_dims = values) as a density over the other dimensions, built on this density's device
        (kdehip_density_condition_device, include/kdehip.h section 5i): the same arrays as the host `condition`."""
        from .conditional import condition
        return condition(self, dims, values, manifold=manifold, tree_manifold=tree_manifold)

    def conditional_weights(self, dims, Y, *, manifold=None):
        """`kdehip.conditional_weights` of this density (kdehip_condition_weights_device)."""
        from .conditional import conditional_weights
        return conditional_weights(self, dims, Y, manifold=manifold)

    def conditional_moments(self, dims, Y, *, manifold=None):
        """`kdehip.conditional_moments` of this density (kdehip_conditional_device)."""
        from .conditional import conditional_moments
        return conditional_moments(self, dims, Y, manifold=manifold)

    def sample_conditional(self, dims, Y, seed=0, sample_offset=0, *, manifold=None):
        """`kdehip.sample_conditional` of this density (kdehip_conditional_device)."""
        from .conditional import sample_conditional
        return sample_conditional(self, dims, Y, seed, sample_offset, manifold=manifold)

    def getKDEMax(self, N=200, *, values=False, manifold=None):
        """`getKDEMax(p; N)` (reference src/DualTree01.jl:558-570) on the device (kdehip_density_summary[_manifold])."""
        from .summary import getKDEMax
        return getKDEMax(self, N, values=values, manifold=manifold)

    def getKDEMean(self, *, manifold=None):
        """`getKDEMean(p)` on the device; `manifold`: the circular mean (include/kdehip.h section 5e)."""
        from .summary import getKDEMean
        return getKDEMean(self, manifold=manifold)

    def getKDEfit(self, *, manifold=None):
        """`getKDEfit(p)` on the device; `manifold`: the circular mean and wrapped residuals (section 5e)."""
        from .summary import getKDEfit
        return getKDEfit(self, manifold=manifold)

    def getKDERange(self, extend=0.1, *, manifold=None):
        """`getKDERange(p; extend)` on the device; `manifold`: the unwrapped arc of a circular dimension (section 5e)."""
        from .summary import getKDERange
        return getKDERange(self, extend, manifold=manifold)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.kdehip_density_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def mul_device(trees, *, addEntropy=True, seed=None, manifold=None, tree_manifold=None) -> DeviceDensity:
    """`*(trees; addEntropy)` (reference src/MSGibbs01.jl:707-726) on `DeviceDensity` handles, result in HBM: product with
    Niter = 5 and Np = round(mean(Npts)), then `kde!(pGM)` -- the sample matrix never leaves the device
    (kdehip_mul_device).  Same numbers as `mul(host trees, seed=seed)`.
    `manifold`: the circular product (`prodAppxMSGibbsS_device(manifold=)`), then `from_device_points(manifold=)` on its
    matrix (kdehip_mul_device_manifold); the result remembers it.  `tree_manifold`: the operators of the result's tree
    build, as `from_device_points(tree_manifold=)` (kdehip_mul_device_tree)."""
    trees = list(trees)
    man = _mf.parse(manifold, trees[0].dims)
    tman = _mf.parse(tree_manifold, trees[0].dims)
    if seed is None:
        seed = _lib.random_seed()
    M = len(trees)
    arr = (C.c_void_p * M)(*[t._h for t in trees])
    h = C.c_void_p()
    bw = np.empty(trees[0].dims)
    ne = C.c_int32(0)
    _lib.check(_lib.lib.kdehip_mul_device_tree(C.byref(h), M, arr, u64(seed),
                                               int(bool(addEntropy)), ptr(bw, f64p), C.byref(ne),
                                               _mf.pointer(man), _mf.pointer(tman)))
    return DeviceDensity._built(h, trees[0].device, bw, int(ne.value), man, tman)


def mul_device_batch(products, *, addEntropy=True, seeds=None, manifold=None, tree_manifold=None):
    """Many `*` in ONE call (kdehip_mul_device_batch): `products` = a list of lists of `DeviceDensity`; returns one
    `DeviceDensity` per product, each bit for bit what `mul_device(products[i], addEntropy=..., seed=seeds[i])` returns --
    batched sampler, the LOOCV searches of all results of one size in shared launches, trees built under them.
    `addEntropy`: one flag or one per product.  `manifold`: one for all products or one per product (None = Euclidean);
    circular products ride the batched launch of the sampler's circular fast mode (`prodAppxMSGibbsS_batch(manifold=)`), their
    searches share launches (kdehip_mul_device_batch_manifold).
    `tree_manifold`: the tree builders' operators, one for all products or one per product like `manifold`
    (kdehip_mul_device_batch_tree); products with and without a circular tree may be mixed."""
    products = [list(p) for p in products]
    n = len(products)
    if n == 0:
        return []
    if seeds is None:
        seeds = [_lib.random_seed() for _ in range(n)]
    flags = [bool(addEntropy)] * n if isinstance(addEntropy, (bool, int, np.bool_)) else [bool(f) for f in addEntropy]
    items = (_lib.CMulItem * n)()
    keep = []
    for k, trees in enumerate(products):
        arr = (C.c_void_p * len(trees))(*[t._h for t in trees])
        keep.append(arr)
        items[k].Ndens, items[k].addEntropy, items[k].trees = len(trees), int(flags[k]), arr
        items[k].seed = int(seeds[k]) & SEED_MASK
    dims = [p[0].dims if p else 0 for p in products]   # (an empty product: the library refuses it)
    mans, tmans = _mf.per_product(manifold, dims), _mf.per_product(tree_manifold, dims)
    marr, tarr = _mf.matrix(mans), _mf.matrix(tmans)   # row k: product k's manifold / the operators of its tree build
    out = (C.c_void_p * n)()
    bw = np.zeros((n, _lib.MAX_DIMS))
    ne = np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib.kdehip_mul_device_batch_tree(n, items, ptr(marr, u8p), ptr(tarr, u8p), out, ptr(bw, f64p),
                                                     ptr(ne, _lib.i32p)))
    res = []
    for k in range(n):
        res.append(DeviceDensity._built(C.c_void_p(out[k]), products[k][0].device, bw[k, :dims[k]].copy(), int(ne[k]),
                                        mans[k], tmans[k]))
    return res


class ProductBatch:
    """The argument block of one `kdehip_prod_philox_batch` call, built once: a host that issues the same set of products
    sweep after sweep (only seeds / sample offsets change) does not pay the Python-side marshalling per call.
    `manifold`: one for all products or one per product (None = Euclidean), by the convention of `mul_device_batch`; a
    product's own "manifold" key takes precedence (kdehip_prod_philox_batch_manifold)."""

    def __init__(self, products, precision=64, manifold=None):
        n = len(products)
        dims = [list(pr["trees"])[0].dims for pr in products]
        self.manifolds = _mf.per_product(manifold, dims, own=[pr.get("manifold") for pr in products])
        # nprod rows of MAX_DIMS bytes, or None (the library's NULL) when every product is Euclidean
        self._marr = _mf.matrix(self.manifolds) if any(m is not None and m.any() for m in self.manifolds) else None
        self._mptr = _mf.pointer(self._marr)
        self.n = n
        self.precision = int(precision)
        self.items = (_lib.CBatchItem * max(1, n))()
        self._keep = []
        for k, pr in enumerate(products):
            trees = list(pr["trees"])
            M = len(trees)
            arr = (C.c_void_p * M)(*[t._h for t in trees])
            mask = _mask_array(pr.get("partialDimMask"), M, trees[0].dims)
            self._keep.append((arr, mask, trees, pr["d_points"], pr["d_indices"], pr.get("d_labels")))
            it = self.items[k]
            it.Ndens, it.Niter = M, int(pr.get("Niter", 3))
            it.trees = arr
            it.Np = int(pr["Np"])
            it.seed = int(pr.get("seed", 0)) & SEED_MASK
            it.sample_offset = int(pr.get("sample_offset", 0))
            it.addEntropy = int(bool(pr.get("addEntropy", True)))
            it.partialDimMask = optr(mask, u8p)
            it.d_points = addr(pr["d_points"])
            it.d_indices = addr(pr["d_indices"])
            it.d_labels = addr(pr.get("d_labels"))

    def enqueue(self, stream=None, sample_offset=None):
        """one library call for all products (enqueue only); `sample_offset` (optional) replaces every product's"""
        if sample_offset is not None:
            for k in range(self.n):
                self.items[k].sample_offset = int(sample_offset)
        _lib.check(_lib.lib.kdehip_prod_philox_batch_manifold(self.n, self.items, self._mptr, self.precision, addr(stream)))


def batch_launches() -> dict:
    """Diagnostic (kdehip_prod_philox_batch_launches): of this thread's last `prodAppxMSGibbsS_batch` / `ProductBatch.enqueue`
    / `mul_device_batch`, the batched sampling launches (one per group) and the products enqueued one by one."""
    b, s = C.c_int32(0), C.c_int32(0)
    _lib.lib.kdehip_prod_philox_batch_launches(C.byref(b), C.byref(s))
    return {"batched": int(b.value), "singles": int(s.value)}


def prodAppxMSGibbsS_batch(products, *, precision=64, stream=None, manifold=None):
    """Many `prodAppxMSGibbsS` calls on `DeviceDensity` inputs in ONE library call (kdehip_prod_philox_batch): one device
    block, one gather launch, and one sampling launch per (dimension count, density count) group of fp64 products of 2..4
    densities.  `products`: dicts with the keywords of `prodAppxMSGibbsS_device` (trees, d_points, d_indices, Np, and
    optionally Niter=3, seed=0, sample_offset=0, addEntropy=True, partialDimMask, d_labels).  Every product gets the
    numbers the single call would give it.  Enqueues on `stream` and returns.
    `manifold`: one for all products or one per product (or a "manifold" key in a product's dict): circular products whose
    densities qualify for the fast forms ride one launch per dimension count, each with the numbers of
    `prodAppxMSGibbsS_device(manifold=)` (kdehip_prod_philox_batch_manifold)."""
    ProductBatch(products, precision, manifold).enqueue(stream)


def prodAppxMSGibbsS_device(trees, d_points, d_indices, *, Np, Niter=3, seed=0, sample_offset=0, addEntropy=True,
                            partialDimMask=None, precision=64, d_labels=None, stream=None, manifold=None):
    """`prodAppxMSGibbsS` (reference src/MSGibbs01.jl:645-703) on densities that live in HBM (`DeviceDensity`), results
    left in HBM: d_points (float64[ndims*Np]) and d_indices (int64[Ndens*Np]) are device arrays (torch tensors or
    addresses).  Enqueues on `stream` and returns; same numbers as `prodAppxMSGibbsS(..., seed=seed)`.
    `manifold`: the per-dimension enum of `gibbs1` -- the circular operators in the sampler, nothing leaves the device
    (kdehip_prod_philox_device_manifold; precision 64 only)."""
    trees = list(trees)
    M = len(trees)
    arr = (C.c_void_p * M)(*[t._h for t in trees])
    ndims = trees[0].dims
    mask = _mask_array(partialDimMask, M, ndims)
    man = _mf.parse(manifold, ndims)
    _lib.check(_lib.lib.kdehip_prod_philox_device_manifold(
        M, arr, int(Np), int(Niter), u64(seed), int(sample_offset), int(bool(addEntropy)),
        optr(mask, u8p), _mf.pointer(man), int(precision),
        addr(d_points), addr(d_indices), addr(d_labels), addr(stream)))


def prodAppxMSGibbsS_resident(trees, *, Np, Niter=3, seed=0, addEntropy=True, partialDimMask=None, precision=64,
                              manifold=None):
    """`prodAppxMSGibbsS` on `DeviceDensity` inputs with host outputs (blocking): returns (points[ndims, Np],
    indices[Ndens, Np]) -- the numbers of `prodAppxMSGibbsS(..., seed=seed)` without the per-call host re-layout and
    upload.  `manifold`: as `prodAppxMSGibbsS_device` (kdehip_prod_philox_resident_manifold)."""
    trees = list(trees)
    M, D = len(trees), trees[0].dims
    arr = (C.c_void_p * M)(*[t._h for t in trees])
    mask = _mask_array(partialDimMask, M, D)
    man = _mf.parse(manifold, D)
    pts = np.empty(D * Np)   # (every element is written by the call)
    ind = np.empty(M * Np, dtype=np.int64)
    _lib.check(_lib.lib.kdehip_prod_philox_resident_manifold(
        M, arr, int(Np), int(Niter), u64(seed), int(bool(addEntropy)),
        optr(mask, u8p), _mf.pointer(man), int(precision), ptr(pts, f64p), ptr(ind, i64p)))
    return pts.reshape(Np, D).T, ind.reshape(Np, M).T


def philox_streams(seed, sample_begin, nsamples, K, R):
    """Host twin of the device RNG: the (randU, randN) arrays a Philox run consumes
    (kdehip_philox_fill_uniform / _normal)."""
    u = np.empty(nsamples * K)
    n = np.empty(nsamples * R)
    s = u64(seed)
    _lib.lib.kdehip_philox_fill_uniform(s, int(sample_begin), int(nsamples), int(K), ptr(u, f64p))
    _lib.lib.kdehip_philox_fill_normal(s, int(sample_begin), int(nsamples), int(R), ptr(n, f64p))
    return u, n


class GbGlb:
    """The part of the reference's `GbGlb` scratch object (src/MSGibbs01.jl:1-33) a caller can see:
    `recordChoosen` and, after a product, `labelsChoosen[sample][density][level]` (all keys 1-based, :29-31) =
    `bt.permutation[ind]` of the kernel the density holds after the last `sampleIndex` of that level (:109-112).
    Everything else of the reference's scratch lives in registers/LDS of the kernel."""

    def __init__(self, recordChoosen=False):
        self.recordChoosen = bool(recordChoosen)
        self.labelsChoosen = {}

    def _fill(self, labels, Niter):
        """labels[Np, Ndens, L] -> the reference's nested dictionaries (:471-472, :575-583)."""
        Np, M, L = labels.shape
        self.labelsChoosen = {s + 1: {j + 1: ({l + 1: int(labels[s, j, l]) for l in range(L)} if Niter > 0 else {})
                                      for j in range(M)} for s in range(Np)}


def makeEmptyGbGlb(recordChoosen=False):
    """`makeEmptyGbGlb(;recordChoosen=false)` (reference src/MSGibbs01.jl:35-61)."""
    return GbGlb(recordChoosen)


def gibbs1(Ndens, trees, Np, Niter, pts, ind, randU, randN, *, addEntropy=True, ndims=None,
           partialDimMask=None, glbs=None, device=0, ngpus=1, manifold=None):
    """`gibbs1` (reference src/MSGibbs01.jl:527-537): fills the caller's `pts` (length ndims*Np,
    column-major) and `ind` (Ndens x Np, column-major) in place; returns None.  With
    `glbs.recordChoosen` the label trace lands in `glbs.labelsChoosen` as in the reference.
    `manifold`: the reference's operator tuples addop / diffop / getMu / getLambda (:650-653) as a per-dimension ENUM --
    'euclid' (the defaults) or 'circular' (wrap to [-pi, pi), tangent-space mean; this library's stated semantic,
    include/kdehip.h "manifolds") -- kdehip_gibbs1_manifold."""
    trees = list(trees)
    if ndims is None:
        ndims = max(Ndim(t) for t in trees)
    pts = np.asarray(pts)
    ind = np.asarray(ind)
    if pts.dtype != np.float64 or ind.dtype != np.int64 or not pts.flags.c_contiguous:
        raise TypeError("pts must be float64 and ind int64 (caller-allocated, filled in place)")
    flat_ind = ind.reshape(-1, order="F") if ind.ndim == 2 else ind
    tmp_ind = np.ones(Ndens * Np, dtype=np.int64)
    randU = np.ascontiguousarray(randU, dtype=np.float64)
    randN = np.ascontiguousarray(randN, dtype=np.float64)
    arr = (_lib.CDensity * Ndens)(*[t._cstruct() for t in trees])
    mask = _mask_array(partialDimMask, Ndens, ndims)
    labels = None
    if glbs is not None and glbs.recordChoosen:
        labels = np.zeros((Np, Ndens, nlevels(max(Npts(t) for t in trees))), dtype=np.int32)
    man = _mf.parse(manifold, ndims)
    if man is not None and int(ngpus) != 1:
        raise ValueError("gibbs1: manifold= runs on one GPU (kdehip_gibbs1_manifold); ngpus must be 1")
    if man is not None:
        _lib.check(_lib.lib.kdehip_gibbs1_manifold(int(Ndens), arr, int(Np), int(Niter), ptr(pts.reshape(-1), f64p),
                                                   ptr(tmp_ind, i64p), ptr(randU, f64p), randU.size, ptr(randN, f64p),
                                                   randN.size, int(bool(addEntropy)), int(ndims),
                                                   optr(mask, u8p), ptr(man, u8p), int(device), optr(labels, i32p)))
    else:
        _lib.check(_lib.lib.kdehip_gibbs1_multi(int(Ndens), arr, int(Np), int(Niter), ptr(pts.reshape(-1), f64p),
                                                ptr(tmp_ind, i64p), ptr(randU, f64p), randU.size, ptr(randN, f64p),
                                                randN.size, int(bool(addEntropy)), int(ndims),
                                                optr(mask, u8p), int(device), int(ngpus), optr(labels, i32p)))
    if labels is not None:
        glbs._fill(labels, Niter)
    if ind.ndim == 2:
        ind[...] = tmp_ind.reshape(Np, Ndens).T
    else:
        flat_ind[...] = tmp_ind
    return None


def prodAppxMSGibbsS(npd0, trees, anFcns=None, anParams=None, *deprecated_niter, Niter=3, addEntropy=True, ndims=None,
                     Ndens=None, Np=None, maxNp=None, Nlevels=None, randU=None, randN=None, partialDimMask=None,
                     addop=None, diffop=None, getMu=None, getLambda=None, glbs=None,
                     seed=None, device=0, precision=64, ngpus=1, manifold=None, fast_circular=False):
    """`prodAppxMSGibbsS` (reference src/MSGibbs01.jl:645-703).

    npd0 only supplies Np = Npts(npd0) (:658); anFcns/anParams are ignored as in the reference
    (:677-678).  With `randU`/`randN` given they are consumed exactly as the reference consumes
    them; otherwise (the reference would call rand/randn) the on-device Philox stream keyed by
    `seed` is used.  Returns (points[ndims, Np], indices[Ndens, Np]).
    Non-Euclidean addop/diffop/getMu/getLambda FUNCTIONS cannot cross the C ABI and are rejected; `manifold=` gives the
    four tuples as a per-dimension enum instead ('euclid' / 'circular': see `gibbs1`).
    `maxNp` / `Nlevels` only size the reference's default random arrays (:659-662; `gibbs1` recomputes the level
    count from the trees, :568) and are accepted and ignored; a fifth positional argument is the deprecated
    positional `Niter` (:632-643).
    The returned matrices are column-major (Fortran-ordered) VIEWS of the flat result buffers, like Julia's: pass them
    through `np.ascontiguousarray` before handing their `.ctypes` pointer to C code that expects row-major data.
    `manifold` without caller streams: on one GPU the host twin of the Philox streams goes through `gibbs1(manifold=)` -- the
    generic arithmetic, byte for byte the explicit-stream call.  With `ngpus > 1`, or with `fast_circular=True` on any number
    of GPUs, the call takes kdehip_prod_philox_manifold instead: device Philox and the sampler's circular fast mode, the
    numbers of `ProductPlan(manifold=).sample(seed)` and the same for every `ngpus`.  The two routes return identical labels;
    their points differ by rounding only (within 1e-12, compared on the circle in the circular dimensions).
    """
    if deprecated_niter:
        if len(deprecated_niter) > 1:
            raise TypeError("prodAppxMSGibbsS takes at most 5 positional arguments")
        import warnings
        warnings.warn("prodApproxMSGibbs has new keyword interface, use (..; Niter::Int=5 ) instead", DeprecationWarning)
        Niter = int(deprecated_niter[0])
    for name, v in (("addop", addop), ("diffop", diffop), ("getMu", getMu), ("getLambda", getLambda)):
        if v is not None:
            raise NotImplementedError(f"{name}: only the Euclidean defaults exist behind the HIP path")
    trees = list(trees)
    if Ndens is None:
        Ndens = len(trees)
    if ndims is None:
        ndims = max(Ndim(t) for t in trees)
    if Np is None:
        Np = Npts(npd0)
    if (randU is None) != (randN is None):
        raise ValueError("give both randU and randN, or neither")
    philox_manifold = manifold is not None and randU is None and (bool(fast_circular) or int(ngpus) != 1)
    if manifold is not None and randU is None and not philox_manifold:
        # the manifold entry consumes caller streams: the host twin of the device stream gives the run the numbers the
        # Philox path would have drawn for `seed`
        if seed is None:
            seed = _lib.random_seed()
        L = nlevels(max(Npts(t) for t in trees[:Ndens]))
        randU, randN = philox_streams(seed, 0, Np, Ndens * (1 + L * (Niter + 1)), ndims * (L + 1))
    if randU is not None:
        points = np.zeros(ndims * Np)
        indices = np.ones((Ndens, Np), dtype=np.int64)
        gibbs1(Ndens, trees, Np, Niter, points, indices, randU, randN, addEntropy=addEntropy, ndims=ndims,
               partialDimMask=partialDimMask, glbs=glbs, device=device, ngpus=ngpus, manifold=manifold)
        return points.reshape(Np, ndims).T.copy(), indices
    if seed is None:
        seed = _lib.random_seed()
    trace = glbs is not None and glbs.recordChoosen
    trees = trees[:Ndens]
    arr = (_lib.CDensity * Ndens)(*[t._cstruct() for t in trees])
    mask = _mask_array(partialDimMask, Ndens, ndims)
    pts = np.empty(ndims * Np)   # (every element is written by the call)
    ind = np.empty(Ndens * Np, dtype=np.int64)
    labels = np.zeros((Np, Ndens, nlevels(max(Npts(t) for t in trees))), dtype=np.int32) if trace else None
    man = _mf.parse(manifold, ndims) if philox_manifold else None
    _lib.check(_lib.lib.kdehip_prod_philox_manifold(int(Ndens), arr, int(Np), int(Niter), ptr(pts, f64p), ptr(ind, i64p),
                                                    u64(seed), int(bool(addEntropy)), int(ndims),
                                                    optr(mask, u8p), _mf.pointer(man), int(precision), int(device),
                                                    int(ngpus), optr(labels, i32p)))
    if trace:
        glbs._fill(labels, Niter)
    # (ndims, Np) and (Ndens, Np) as the reference returns them: column-major matrices -- views of the flat buffers
    return pts.reshape(Np, ndims).T, ind.reshape(Np, Ndens).T


def mul(trees, *, glbs=None, addEntropy=True, seed=None, device=0):
    """`*(trees; glbs, addEntropy)` (reference src/MSGibbs01.jl:707-726): product with Niter=5 and
    Np = round(mean(Npts)), then `kde!(pGM)` with the automatic (LOOCV) bandwidth."""
    from .bandwidth import kde_auto  # LOOCV bandwidth selection lives with the evaluation kernels
    trees = list(trees)
    if len(trees) == 1 and not addEntropy:  # hack fix for #70, :713-716
        from .density import getPoints
        return kde_auto(getPoints(trees[0]).copy(), device=device)
    d = max(Ndim(t) for t in trees)
    for p in trees:
        if Ndim(p) != d:
            raise ValueError("kdes must have same dimension")
    numpts = int(round(float(np.mean([Npts(t) for t in trees]))))
    if seed is None:
        seed = _lib.random_seed()
    pGM, _ = prodAppxMSGibbsS(None, trees, None, None, Niter=5, addEntropy=addEntropy, Np=numpts, glbs=glbs,
                              seed=seed, device=device)
    return kde_auto(pGM, device=device)
