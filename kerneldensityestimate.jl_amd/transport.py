"""Entropic optimal transport between two densities: `sinkhorn`, `sinkhorn_divergence`, `transport_map`, `transport_to`,
`equalize` and `sinkhorn_batch`, over kdehip_sinkhorn[_device] / kdehip_sinkhorn_device_batch (include/kdehip.h section 5s;
kernels in csrc/sinkhorn.hip).  The library's own: the reference has no counterpart.

With x_i, a_i the points and weights of p, y_j, b_j those of q, a scale vector s (default sqrt(v_p + v_q), the bandwidths
combined as `intersIntg` combines them) and eps = reg, the cost is c_ij = 1/2 sum_k diff_k(x_i, y_j)^2 / s_k^2 and the
iteration runs in the log domain on potentials divided by eps; `p.sinkhorn(p)` (the same object) runs the symmetric
iteration of a density against itself.  The surface is methods: the five on `BallTreeDensity` (host arrays, run on `device`)
and on `DeviceDensity` (nothing but a few scalars leaves HBM), and `DeviceDensity.sinkhorn_batch` for many pairs in one call;
the functions below are what they call.  `manifold=` as the other entries take it, "inherit" included (read from p).

What `return_info=True` adds is a dict: `value`, `transport_cost`, `err`, `mass`, `iters` (negative when the last step was
still above tol), `phi` (N), `gamma` (M), `map` (D, N) in the order of getPoints, and the displacement -- `delta` (D, N) in
the order of getPoints for host densities, `delta_leaf` (D, N) in LEAF order for resident ones (what
`kdehip_density_refit_device(..., leaf_order=1)` takes).  Host densities give NumPy arrays, resident ones device tensors."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import addr, f64p, i32p, optr, ptr
from .loglik import _dims
from .modes import _kind


def _numbers(reg, tol, maxiter):
    reg, tol, maxiter = float(reg), float(tol), int(maxiter)
    if not (np.isfinite(reg) and reg > 0.0):
        raise ValueError("reg must be finite and > 0")
    if not tol >= 0.0:
        raise ValueError("tol must be >= 0")
    if maxiter < 0:
        raise ValueError("maxiter must be >= 0")
    return reg, tol, maxiter


def _scale(scale, D):
    """None, or D positive entries as a float64 array (their values are the library's check)"""
    if scale is None:
        return None
    s = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).ravel())
    if s.size != D:
        raise ValueError("scale needs one entry per dimension")
    return s


def _pair(p, q):
    kind = _kind(p)
    if _kind(q) != kind:
        raise TypeError("both densities must be BallTreeDensity, or both DeviceDensity")
    D = _dims(p)
    if _dims(q) != D:
        raise ValueError("the two densities must have the same dimension")
    return kind, D


def _npts(p, kind):
    return int(p.bt.num_points) if kind == "host" else int(p.num_points)


def _same(p, q):
    """q is p: the same object, or two wrappers of one handle"""
    if q is p:
        return True
    hp, hq = getattr(p, "_h", None), getattr(q, "_h", None)
    return hp is not None and hq is not None and hp.value is not None and hp.value == hq.value


def _scalars():
    return np.zeros(4), np.zeros(1, dtype=np.int32)


def _info(vals, iters, **vectors):
    out = dict(value=float(vals[0]), transport_cost=float(vals[1]), err=float(vals[2]), mass=float(vals[3]), iters=int(iters[0]))
    out.update(vectors)
    return out


def _at(vals, k):
    return C.cast(vals[k:].ctypes.data, f64p)


def _run_host(p, q, reg, scale, tol, maxiter, man, device, vectors):
    D, N, M = _dims(p), _npts(p, "host"), _npts(q, "host")
    vals, iters = _scalars()
    phi = gamma = delta = tmap = None
    if vectors:
        phi, gamma, delta, tmap = np.zeros(N), np.zeros(M), np.zeros((N, D)), np.zeros((N, D))
    cp = p._cstruct()
    cq = cp if q is p else q._cstruct()
    _lib.check(_lib.lib.kdehip_sinkhorn(C.byref(cp), C.byref(cq), optr(scale, f64p), C.byref(C.c_double(reg)), C.byref(C.c_double(tol)), maxiter, _at(vals, 0), _at(vals, 1),
                                        _at(vals, 2), _at(vals, 3), ptr(iters, i32p), optr(phi, f64p), optr(gamma, f64p),
                                        optr(delta, f64p), optr(tmap, f64p), int(device), _mf.pointer(man)))
    if not vectors:
        return _info(vals, iters)
    return _info(vals, iters, phi=phi, gamma=gamma, delta=np.ascontiguousarray(delta.T), map=np.ascontiguousarray(tmap.T))


def _device_vectors(p, q, dev):
    import torch
    D, N, M = p.dims, p.num_points, q.num_points
    kw = dict(dtype=torch.float64, device=dev)
    return torch.empty(N, **kw), torch.empty(M, **kw), torch.empty((N, D), **kw), torch.empty((N, D), **kw)


def _vector_info(vals, iters, vec):
    phi, gamma, delta, tmap = vec
    return _info(vals, iters, phi=phi, gamma=gamma, delta_leaf=delta.t(), map=tmap.t())


def _run_device(p, q, reg, scale, tol, maxiter, man, vectors):
    import torch
    if p.device != q.device:
        raise ValueError("the two densities are on different devices")
    dev = torch.device("cuda", p.device)
    vals, iters = _scalars()
    with torch.cuda.device(dev):
        vec = _device_vectors(p, q, dev) if vectors else (None,) * 4
        torch.cuda.current_stream(dev).synchronize()  # (the entry is blocking and runs on the library's own stream)
        _lib.check(_lib.lib.kdehip_sinkhorn_device(p._h, p._h if _same(p, q) else q._h, optr(scale, f64p), C.byref(C.c_double(reg)), C.byref(C.c_double(tol)),
                                                   maxiter, _at(vals, 0), _at(vals, 1), _at(vals, 2), _at(vals, 3), ptr(iters, i32p),
                                                   *(addr(v) for v in vec), _mf.pointer(man)))
    return _vector_info(vals, iters, vec) if vectors else _info(vals, iters)


def _run(p, q, reg, scale, tol, maxiter, manifold, device, vectors):
    kind, D = _pair(p, q)
    reg, tol, maxiter = _numbers(reg, tol, maxiter)
    man = _mf.resolve(p, manifold, D)
    s = _scale(scale, D)
    if kind == "host":
        return _run_host(p, q, reg, s, tol, maxiter, man, device, vectors)
    return _run_device(p, q, reg, s, tol, maxiter, man, vectors)


def sinkhorn(p, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False, device=0):
    """The entropic transport value between p and q: eps (sum a phi + sum b gamma - (mass - 1)), the dual objective, equal to
    min <pi, c> + eps KL(pi | a x b) at convergence.  `q is p` runs the symmetric iteration of p against itself."""
    info = _run(p, q, reg, scale, tol, maxiter, manifold, device, bool(return_info))
    return (info["value"], info) if return_info else info["value"]


def sinkhorn_batch(pairs, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, vectors=False):
    """Many pairs of DeviceDensity in ONE call (kdehip_sinkhorn_device_batch).  `pairs`: (p, q) tuples, or dicts with `p`, `q`
    and optionally `reg`, `scale`, `tol`, `maxiter`, `manifold` of their own, or `scale_from=(p', q')`: the default scale of
    that pair in the place of the item's own (the self items of a divergence).  The items share the launches of every half-step.
    Returns one info dict per pair, each bit for bit `p.sinkhorn(q, ..., return_info=True)[1]` (the vectors with vectors=True)."""
    import torch
    from .product import DeviceDensity
    items = [dict(p=it[0], q=it[1]) if isinstance(it, (tuple, list)) else dict(it) for it in pairs]
    n = len(items)
    arr = (_lib.CSinkhornItem * max(1, n))()
    keep = []
    for k, it in enumerate(items):
        p, q = it["p"], it["q"]
        if not (isinstance(p, DeviceDensity) and isinstance(q, DeviceDensity)):
            raise TypeError("sinkhorn_batch: pairs of DeviceDensity")
        _pair(p, q)
        r, t, mi = _numbers(it.get("reg", reg), it.get("tol", tol), it.get("maxiter", maxiter))
        s = _scale(it.get("scale", scale), p.dims)
        vals, iters = _scalars()
        keep.append([s, vals, iters, None, p, q])
        arr[k].p, arr[k].q, arr[k].scale = p._h, p._h if _same(p, q) else q._h, optr(s, f64p)
        arr[k].reg, arr[k].tol, arr[k].maxiter = r, t, mi
        arr[k].value, arr[k].transport_cost, arr[k].err, arr[k].mass = (_at(vals, j) for j in range(4))
        arr[k].iters = ptr(iters, i32p)
        arr[k].circular_mask = _mf.mask(_mf.resolve(p, it.get("manifold", manifold), p.dims))
        if s is None and it.get("scale_from") is not None:
            sp, sq = it["scale_from"]
            _pair(sp, p), _pair(sq, p)
            arr[k].scale_p, arr[k].scale_q = sp._h, sq._h
    if n == 0:
        return []
    if len({it["p"].device for it in items} | {it["q"].device for it in items}) != 1:
        raise ValueError("sinkhorn_batch: the densities are on different devices")
    dev = torch.device("cuda", items[0]["p"].device)
    with torch.cuda.device(dev):
        if vectors:
            for k, kp in enumerate(keep):
                kp[3] = _device_vectors(kp[4], kp[5], dev)
                arr[k].d_phi, arr[k].d_gamma, arr[k].d_delta, arr[k].d_map = (v.data_ptr() for v in kp[3])
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(_lib.lib.kdehip_sinkhorn_device_batch(n, arr))
    return [_vector_info(vals, iters, vec) if vectors else _info(vals, iters) for _, vals, iters, vec, _, _ in keep]


_ZERO = dict(value=0.0, cross=0.0, self_p=0.0, self_q=0.0, iters=(0, 0, 0), err=(0.0, 0.0, 0.0))


def sinkhorn_divergence(p, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False, device=0):
    """S(p, q) = value(p, q) - value(p, p) / 2 - value(q, q) / 2: three items -- one cross, two self -- in one run.  S(p, p)
    with `q is p` is 0.0 by definition, without a launch.  Host densities are uploaded for the call."""
    kind, D = _pair(p, q)
    reg, tol, maxiter = _numbers(reg, tol, maxiter)
    man = _mf.resolve(p, manifold, D)
    s = _scale(scale, D)
    if _same(p, q):
        return (0.0, dict(_ZERO)) if return_info else 0.0
    if kind == "host":
        from .product import DeviceDensity
        with DeviceDensity(p, device) as dp, DeviceDensity(q, device) as dq:
            return sinkhorn_divergence(dp, dq, reg, s, tol, maxiter, man, return_info)
    one = (p, q)  # all three items at ONE scale: the cross item's
    pq, pp, qq = sinkhorn_batch([dict(p=p, q=q), dict(p=p, q=p, scale_from=one), dict(p=q, q=q, scale_from=one)], reg, s, tol,
                                maxiter, man)
    S = pq["value"] - 0.5 * pp["value"] - 0.5 * qq["value"]
    if not return_info:
        return S
    return S, dict(value=S, cross=pq["value"], self_p=pp["value"], self_q=qq["value"],
                   iters=(pq["iters"], pp["iters"], qq["iters"]), err=(pq["err"], pp["err"], qq["err"]))


def transport_map(p, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False, device=0):
    """T (D, N), column i = x_i + m_i: the barycentric image of p's point i under the plan onto q, wrapped to [-pi, pi) in a
    circular dimension; in the order of getPoints.  A device tensor for a DeviceDensity."""
    info = _run(p, q, reg, scale, tol, maxiter, manifold, device, True)
    return (info["map"], info) if return_info else info["map"]


def _moved(p, info, weights=None):
    """p with every point moved by its displacement (and, with weights, reweighted): ONE refit, the same tree"""
    if "delta" in info:
        from .refit import refit_host
        return refit_host(p, new_weights=weights, delta=info["delta"])
    from .refit import KEEP, WEIGHTS, refit_device
    if weights is None:
        return refit_device(p, None, KEEP, info["delta_leaf"], leaf_order=True)[0]
    return refit_device(p, weights, WEIGHTS, info["delta_leaf"], leaf_order=True)[0]  # (equal weights: any order)


def transport_to(p, q, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False, device=0):
    """`p.movePoints(delta)`, delta the barycentric displacement onto q: a NEW density with p's weights and tree.  On a
    DeviceDensity nothing leaves HBM (the displacement goes to the refit in leaf order).  The move itself wraps by the
    operators p's tree was built with (`tree_manifold`), as `movePoints` does."""
    info = _run(p, q, reg, scale, tol, maxiter, manifold, device, True)
    out = _moved(p, info)
    return (out, info) if return_info else out


def equalize(p, reg=1.0, scale=None, tol=1e-6, maxiter=1000, manifold=None, return_info=False, device=0):
    """The ensemble transform of particle filtering, the deterministic cure of uneven weights: p's points with weights 1 / N
    are transported onto p as it is, and the moved points are returned with equal weights (changeWeights and movePoints in
    one refit; the same tree).  The mean of the result is p's weighted mean up to the row-marginal error of the plan."""
    kind = _kind(p)
    N = _npts(p, kind)
    w = np.full(N, 1.0 / N)
    u = p.changeWeights(w)
    try:
        info = _run(u, p, reg, scale, tol, maxiter, manifold, device, True)
    finally:
        if kind == "device":
            u.close()
    out = _moved(p, info, w)
    return (out, info) if return_info else out
