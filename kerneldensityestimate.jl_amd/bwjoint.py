"""Joint bandwidth selection: `joint_bandwidth`, `kde_joint` and `joint_bandwidth_device_batch`, over
kdehip_bandwidth_joint[_device] / kdehip_bandwidth_joint_device_batch (include/kdehip.h section 5q; kernels in
csrc/bwjoint.hip).  The library's own: the reference's `kde!(points)` searches the leave-one-out likelihood of every 1-D
marginal on its own, which undersmooths a D-dimensional density.

For a density with leaves c_i, weights w_i and variances v, with d_ijk = c_ik - c_jk (wrapped in a circular dimension),
a_ij = -1/2 sum_k d_ijk^2 / v_k and the sums over S_i = { j : w_j > 0, j != i },

    S0_i = sum_j w_j e^{a_ij},  T_ik = sum_j w_j e^{a_ij} d_ijk^2,  v_k <- sum_i w_i T_ik / S0_i / sum_i w_i

-- a fixed-point step that never lowers the joint leave-one-out log-likelihood L(v); it is iterated from a start until a step
changes no log standard deviation by more than `tol`, or for `maxiter` steps.  The density is a BallTreeDensity (host arrays,
run on `device`) or a DeviceDensity (on its own device); `manifold=` as the other entries take it, "inherit" included.  All
forms block and return host values: the bandwidth is what the caller builds the next density from.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .density import kde
from .loglik import _dims
from .modes import _iteration, _kind


def _start(start, D):
    """None, or D standard deviations as a float64 array (their values are the library's check)"""
    if start is None:
        return None
    s = np.ascontiguousarray(np.asarray(start, dtype=np.float64).ravel())
    if s.size != D:
        raise ValueError("start needs one standard deviation per dimension")
    return s


def joint_bandwidth(p, start=None, tol=1e-3, maxiter=200, manifold=None, return_info=False, device=0):
    """The (D,) standard deviations that the joint leave-one-out iteration reaches from `start` (D standard deviations; None:
    the density's own bandwidth).  With return_info also a dict: `logl`, the leave-one-out average log-likelihood at the
    returned bandwidth (`evalAvgLogL(p', p', log_domain=True)` of the density rebuilt with it); `iters`, the steps taken,
    negative when the last was still above tol; `status`, 1 when degenerate data froze the iteration (a dimension in which
    all points coincide, fewer than two points of positive weight), else 0; `trace`, L at every iterate, start included."""
    kind, D = _kind(p), _dims(p)
    tol, maxiter = _iteration(tol, maxiter)
    man = _mf.resolve(p, manifold, D)
    s = _start(start, D)
    bw, logl, trace = np.zeros(D), C.c_double(0.0), np.full(maxiter + 1, np.nan)
    iters, status = C.c_int32(0), C.c_int32(0)
    if kind == "host":
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_bandwidth_joint(C.byref(cd), _lib.optr(s, _lib.f64p), C.byref(C.c_double(tol)), maxiter,
                                                   _lib.ptr(bw, _lib.f64p), C.byref(logl), C.byref(iters), C.byref(status),
                                                   _lib.ptr(trace, _lib.f64p), int(device), _mf.pointer(man)))
    else:
        _lib.check(_lib.lib.kdehip_bandwidth_joint_device(p._h, _lib.optr(s, _lib.f64p), C.byref(C.c_double(tol)), maxiter,
                                                          _lib.ptr(bw, _lib.f64p), C.byref(logl), C.byref(iters),
                                                          C.byref(status), _lib.ptr(trace, _lib.f64p), _mf.pointer(man)))
    if not return_info:
        return bw
    return bw, dict(logl=logl.value, iters=iters.value, status=status.value, trace=trace[:abs(iters.value) + 1].copy())


def kde_joint(points, weights=None, start=None, tol=1e-3, maxiter=200, manifold=None, tree_manifold=None, device=0):
    """`kde(points, bw, weights)` with the joint leave-one-out bandwidth.  start=None starts from `kde(points)`'s bandwidth,
    the per-marginal LOOCV search: the result is then never worse than `kde!(points)` in leave-one-out likelihood (with
    weights, in the weighted one).  `manifold`: the search's and the iteration's; `tree_manifold`: the tree builder's."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts.reshape(1, -1)
    D = pts.shape[0]
    tol, maxiter = _iteration(tol, maxiter)
    man = _mf.parse(manifold, D)
    if start is None:
        from .bandwidth import auto_bandwidth
        s = auto_bandwidth(pts, device=device, manifold=man)
    else:
        s = _start(start, D)
    p0 = kde(pts, s, weights, tree_manifold=tree_manifold)
    bw = joint_bandwidth(p0, None, tol, maxiter, man, device=device)
    return kde(pts, bw, weights, tree_manifold=tree_manifold)


def joint_bandwidth_device_batch(items, tol=1e-3, maxiter=200):
    """The joint bandwidths of many DeviceDensity items in ONE call (kdehip_bandwidth_joint_device_batch): `items` = dicts
    with `density` and optionally `start` (D standard deviations) and `manifold`.  The items' sweeps share their launches.
    Returns one (bandwidth (D,), dict(logl, iters, status)) per item, each bit for bit
    `density.joint_bandwidth(start, tol, maxiter, manifold, return_info=True)` without the trace."""
    from .product import DeviceDensity
    tol, maxiter = _iteration(tol, maxiter)
    items = list(items)
    n = len(items)
    arr = (_lib.CBwJointItem * max(1, n))()
    keep = []
    for k, it in enumerate(items):
        d = it["density"]
        if not isinstance(d, DeviceDensity):
            raise TypeError("joint_bandwidth_device_batch: items of DeviceDensity")
        s = _start(it.get("start"), d.dims)
        bw, logl, ints = np.zeros(d.dims), np.zeros(1), np.zeros(2, dtype=np.int32)
        keep.append((s, bw, logl, ints))
        arr[k].bd, arr[k].start = d._h, _lib.optr(s, _lib.f64p)
        arr[k].bw_out, arr[k].logl = _lib.ptr(bw, _lib.f64p), _lib.ptr(logl, _lib.f64p)
        arr[k].iters = C.cast(C.c_void_p(ints.ctypes.data), _lib.i32p)
        arr[k].status = C.cast(C.c_void_p(ints.ctypes.data + 4), _lib.i32p)
        arr[k].circular_mask = _mf.mask(_mf.resolve(d, it.get("manifold"), d.dims))
    _lib.check(_lib.lib.kdehip_bandwidth_joint_device_batch(n, arr, C.byref(C.c_double(tol)), maxiter))
    return [(bw, dict(logl=float(logl[0]), iters=int(ints[0]), status=int(ints[1]))) for _, bw, logl, ints in keep]
