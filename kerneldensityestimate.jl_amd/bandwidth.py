"""Host-side mirror of the callers either side of the product: automatic-bandwidth `kde!(points)`
(reference src/KDE01.jl:3-27) and direct evaluation `evaluateDualTree` / `bd(pos)`
(src/DualTree01.jl:370-446), both running on the GPU through libkdehip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import f64p, ptr
from .density import BallTreeDensity, kde


def _man_ptr(manifold, ndims):
    """(array kept alive, ctypes pointer or None) of a `manifold=` keyword: None, or one 'euclid' / 'circular' / 0 / 1 per
    dimension (include/kdehip.h section 5d)"""
    man = _mf.parse(manifold, ndims)
    return man, _mf.pointer(man)


def auto_bandwidth(points, device=0, return_evals=False, manifold=None):
    """Per-dimension LOOCV bandwidth (standard deviations) that `kde!(points)` selects; `manifold`: the leave-one-out
    likelihoods of a circular dimension's search take wrapped differences (`kde!(points, addop, diffop)`)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts.reshape(1, -1)
    D, N = pts.shape
    flat = np.ascontiguousarray(pts.T).ravel()
    bw = np.zeros(D)
    ne = C.c_int32(0)
    man, mp = _man_ptr(manifold, D)
    _lib.check(_lib.lib.kdehip_auto_bandwidth_manifold(D, N, ptr(flat, f64p), ptr(bw, f64p), C.byref(ne), int(device), mp))
    return (bw, ne.value) if return_evals else bw


def kde_auto(points, device=0, overlap=None, manifold=None, tree_manifold=None) -> BallTreeDensity:
    """`kde!(points)`: LOOCV bandwidth per dimension, then `kde!(points, bwds)` (src/KDE01.jl:24).

    The tree's topology, bounding boxes, weights and means do not depend on the bandwidth: the host builder runs on the
    library's worker threads WHILE the GPU searches the bandwidth, and the variances are filled in afterwards
    (kdehip_make_density_auto) -- bit-identical to building with the final bandwidth.  `overlap=False`: the two steps one
    after the other (what the tests compare with).  `manifold`: the search's; `tree_manifold`: the final tree's operators
    (kdehip_make_density_auto_tree) -- `kde!(points, addop, diffop)` is both set to the same value."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts.reshape(1, -1)
    D, N = pts.shape
    if overlap is None:
        overlap = True
    man, mp = _man_ptr(manifold, D)
    tman, tptr = _man_ptr(tree_manifold, D)
    if N < 2 or not overlap:
        return kde(pts, auto_bandwidth(pts, device=device, manifold=manifold), tree_manifold=tree_manifold)
    from .density import _empty_density
    flat = np.ascontiguousarray(pts.T).ravel()
    bd = _empty_density(D, N)
    bt = bd.bt
    bw = np.empty(D)
    i64p = _lib.i64p
    _lib.check(_lib.lib.kdehip_make_density_auto_tree(
        D, N, ptr(flat, f64p), ptr(bw, f64p), None, int(device), ptr(bt.centers, f64p), ptr(bt.ranges, f64p),
        ptr(bt.weights, f64p), ptr(bt.left_child, i64p), ptr(bt.right_child, i64p), ptr(bt.lowest_leaf, i64p),
        ptr(bt.highest_leaf, i64p), ptr(bt.permutation, i64p), ptr(bd.means, f64p), ptr(bd.bandwidth, f64p),
        ptr(bd.bandwidthMin, f64p), ptr(bd.bandwidthMax, f64p), mp, tptr))
    bd.tree_manifold = tman
    return bd


def evaluate_log(bd, pos=None, lvFlag=False, manifold=None, device=0):
    """log of `evaluateDualTree(bd, pos, lvFlag)` by log-sum-exp in the kernel (kdehip_evaluate_log, include/kdehip.h
    section 5f): finite where the density itself underflows to 0.  Same shapes as `evaluateDualTree`; host densities only
    (a DeviceDensity has `.evaluate_log`)."""
    from .product import DeviceDensity
    if not isinstance(bd, BallTreeDensity) or isinstance(pos, DeviceDensity):
        raise TypeError("evaluate_log: a BallTreeDensity at host points or a BallTreeDensity (a DeviceDensity has "
                        ".evaluate_log)")
    return _evaluate(_lib.lib.kdehip_evaluate_log, bd, pos, lvFlag, device, manifold, log=True)


def evaluateDualTree(bd: BallTreeDensity, pos=None, lvFlag=False, errTol=1e-3, device=0, manifold=None):
    """`evaluateDualTree(bd, pos, lvFlag)` (src/DualTree01.jl:370-421) with FORCE_EVAL_DIRECT = true
    (errTol is then unused, as in the reference).  pos: (D, Nq) matrix, a vector of 1-D positions, or a
    BallTreeDensity whose points are used; lvFlag=True (or pos is bd) evaluates leave-one-out at bd's
    own points and returns the values in the original point order.
    After `setForceEvalDirect(False)` the call is `evaluate_tol(bd, pos, rel_tol=errTol, lvFlag=lvFlag)`: the sum pruned on
    the ball tree, within the relative tolerance errTol from below (include/kdehip.h section 5m).
    A density with per-point bandwidths (`kde_varbw`, multibandwidth == 1) goes to kdehip_evaluate_varbw (section 5o), here
    and in `evaluate_log`; `evaluate_tol` keeps refusing it."""
    from . import evaltol
    if not evaltol.getForceEvalDirect():
        return evaltol.evaluate_tol(bd, pos, rel_tol=errTol, lvFlag=lvFlag, device=device, manifold=manifold)
    return _evaluate(_lib.lib.kdehip_evaluate_manifold, bd, pos, lvFlag, device, manifold)


def _evaluate(entry, bd, pos, lvFlag, device, manifold, log=False):
    if bd.multibandwidth == 1:  # per-point bandwidths: the entry of section 5o, which takes the domain as an argument
        def entry(cd, pos, Nq, loo, out, device, mp, _log=int(log)):
            return _lib.lib.kdehip_evaluate_varbw(cd, pos, Nq, loo, _log, out, device, mp)
    cd = bd._cstruct()
    man, mp = _man_ptr(manifold, bd.bt.dims)  # (manifold: circular differences in those dimensions, kdehip.h section 5d)
    if lvFlag or pos is bd:
        out = np.zeros(bd.bt.num_points)
        _lib.check(entry(C.byref(cd), None, 0, 1, ptr(out, f64p), int(device), mp))
        return out
    if isinstance(pos, BallTreeDensity):
        from .density import getPoints
        pos = getPoints(pos)
    pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim == 1:
        pos = pos.reshape(1, -1)
    if pos.shape[0] != bd.bt.dims:
        raise ValueError("bd and pos must have the same dimension")
    flat = np.ascontiguousarray(pos.T).ravel()
    out = np.zeros(pos.shape[1])
    _lib.check(entry(C.byref(cd), ptr(flat, f64p), pos.shape[1], 0, ptr(out, f64p), int(device), mp))
    return out
