"""Evaluation within a tolerance: `evaluate_tol` over kdehip_evaluate_tol / kdehip_evaluate_device_at_tol (include/kdehip.h
section 5m; kernels in csrc/evaltol.hip), and the reference's switch `setForceEvalDirect!` (src/KernelDensityEstimate.jl:54).

The all-pairs sum of `evaluateDualTree` pruned on the ball tree: a 128-leaf chunk of the density is skipped for a block of 256
queries once its bounding box shows that none of them can gain more than the tolerance from it.  Every value satisfies

    p * (1 - rel_tol) - abs_tol  <=  p_hat  <=  p        (p = what evaluateDualTree returns),

a truncation from below.  Which queries share a block matters to what is skipped (never to the bound), so the queries are
processed in the leaf order of a tree over them (`order="tree"`, the default: neighbours in space share a block), or as given.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import f64p, ptr
from .density import BallTreeDensity, getPoints, kde

_force_eval_direct = True


def setForceEvalDirect(flag=False):
    """`setForceEvalDirect!(flag)`: with False, `evaluateDualTree(bd, pos, lvFlag, errTol)` and `bd(pos, lvFlag, errTol)`
    evaluate within the relative tolerance `errTol` (`evaluate_tol(rel_tol=errTol)`); with True -- the default, and the
    reference's -- they sum every pair and ignore `errTol`."""
    global _force_eval_direct
    _force_eval_direct = bool(flag)


def getForceEvalDirect() -> bool:
    return _force_eval_direct


def _tolerances(rel_tol, abs_tol):
    return C.byref(C.c_double(float(rel_tol))), C.byref(C.c_double(float(abs_tol)))


def _leaf_rows(t):
    """a host density's points in leaf order, (N, D) row-major, and the 0-based original position of each"""
    N, D = t.bt.num_points, t.bt.dims
    return np.ascontiguousarray(t.bt.centers[N * D:].reshape(N, D)), t.bt.permutation[N:] - 1


def evaluate_tol(bd, pos=None, rel_tol=1e-3, abs_tol=0.0, lvFlag=False, order="tree", device=0, manifold=None,
                 return_stats=False):
    """`evaluateDualTree(bd, pos, lvFlag)` within a tolerance (kdehip_evaluate_tol): values in the caller's order, and with
    return_stats=True also (tiles visited, tiles in all) of the (256-query block x 128-leaf chunk) tiles.

    pos: a (D, Nq) matrix, a vector of 1-D positions or a BallTreeDensity; lvFlag=True (or pos is bd) is leave-one-out at
    bd's own points, processed in bd's leaf order.  order="tree": the queries are processed in the leaf order of a ball tree
    over them -- `kde(pos, [1.0])`, as the reference builds one (src/DualTree01.jl:386); a BallTreeDensity contributes its
    own; order="given": the columns as they are.  rel_tol = abs_tol = 0 returns evaluateDualTree's bits.  A DeviceDensity
    `bd` goes to its `.evaluate_tol`."""
    from .product import DeviceDensity
    if isinstance(bd, DeviceDensity):
        return bd.evaluate_tol(None if lvFlag else pos, rel_tol=rel_tol, abs_tol=abs_tol, manifold=manifold,
                               return_stats=return_stats)
    if not isinstance(bd, BallTreeDensity):
        raise TypeError("evaluate_tol: a BallTreeDensity or a DeviceDensity")
    if order not in ("tree", "given"):
        raise ValueError('evaluate_tol: order is "tree" or "given"')
    cd = bd._cstruct()
    man = _mf.parse(manifold, bd.bt.dims)
    mp = _mf.pointer(man)
    rt, at = _tolerances(rel_tol, abs_tol)
    stats = np.zeros(2, dtype=np.int64)
    sp = ptr(stats, _lib.i64p)
    if lvFlag or pos is bd:
        out = np.zeros(bd.bt.num_points)
        _lib.check(_lib.lib.kdehip_evaluate_tol(C.byref(cd), None, 0, 1, rt, at, ptr(out, f64p), sp, int(device), mp))
        return (out, (int(stats[0]), int(stats[1]))) if return_stats else out
    where = None  # the original position of each processed query, or None: as given
    if isinstance(pos, BallTreeDensity):
        if pos.bt.dims != bd.bt.dims:
            raise ValueError("bd and pos must have the same dimension")
        if order == "tree":
            rows, where = _leaf_rows(pos)
        else:
            rows = np.ascontiguousarray(getPoints(pos).T)
    else:
        P = np.asarray(pos, dtype=np.float64)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        if P.shape[0] != bd.bt.dims:
            raise ValueError("bd and pos must have the same dimension")
        if order == "tree" and P.shape[1] > 1 and np.all(np.isfinite(P)):
            rows, where = _leaf_rows(kde(P, [1.0]))
        else:  # (a tree cannot place a NaN or an infinite point: such queries keep the given order)
            rows = np.ascontiguousarray(P.T)
    Nq = rows.shape[0]
    vals = np.zeros(Nq)
    _lib.check(_lib.lib.kdehip_evaluate_tol(C.byref(cd), ptr(rows, f64p), Nq, 0, rt, at, ptr(vals, f64p), sp, int(device), mp))
    if where is None:
        out = vals
    else:
        out = np.zeros(Nq)
        out[where] = vals
    return (out, (int(stats[0]), int(stats[1]))) if return_stats else out
