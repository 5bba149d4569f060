"""The gradient of a density and its joint modes by mean shift: `evaluate_grad`, `meanshift`, `meanshift_device_batch`,
`modes` and `getKDEMode`, over kdehip_evaluate_grad[_device] / kdehip_meanshift[_device] / kdehip_meanshift_device_batch
(include/kdehip.h section 5h; kernels in csrc/modes.hip).  The library's own: the reference has `getKDEMax`, the grid argmax
of every 1-D marginal taken on its own.

For a query x and a Gaussian-kernel density with one bandwidth vector v, with d_ik = x_k - c_ik (wrapped in a circular
dimension) and a_i = -1/2 sum_k d_ik^2 / v_k,

    S_0 = sum_i w_i e^{a_i},  S_k = sum_i w_i e^{a_i} d_ik,  grad log p (x)_k = -S_k / (S_0 v_k),  x_k <- x_k - S_k / S_0

-- the last is the mean-shift step, whose fixed points are the modes.  The density is a BallTreeDensity (host arrays, run on
`device`) or a DeviceDensity (on its own device); `manifold=` as the other entries take it, "inherit" included.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .density import BallTreeDensity, getWeights
from .loglik import _dims


def _kind(p):
    from .product import DeviceDensity
    if isinstance(p, BallTreeDensity):
        return "host"
    if isinstance(p, DeviceDensity):
        return "device"
    raise TypeError("both densities must be BallTreeDensity, or both DeviceDensity")


def _host_points(pos, D, what):
    """a (D, Nq) host array (a vector is 1-D positions) as the ABI's Nq rows of D; a device tensor is not a host argument"""
    if hasattr(pos, "data_ptr"):
        raise TypeError(f"{what}: a BallTreeDensity takes host points (a DeviceDensity takes device tensors too)")
    P = np.asarray(pos, dtype=np.float64)
    if P.ndim == 1:
        P = P.reshape(1, -1)
    if P.ndim != 2 or P.shape[0] != D:
        raise ValueError("bd and pos must have the same dimension")
    return np.ascontiguousarray(P.T)


def _device_points(pos, D, dev, what):
    """likewise as a float64 tensor of Nq rows of D on `dev` (a host array is uploaded)"""
    import torch
    if hasattr(pos, "data_ptr"):
        P = pos.reshape(1, -1) if pos.dim() == 1 else pos
        if P.dim() != 2 or P.shape[0] != D:
            raise ValueError("bd and pos must have the same dimension")
        return P.t().contiguous().to(dev, torch.float64)
    return torch.from_numpy(_host_points(pos, D, what)).to(dev)


def evaluate_grad(p, pos, *, log=True, device=0, manifold=None):
    """(val (Nq,), grad (D, Nq)) at the columns of `pos` (D, Nq): log p and its gradient, or with log=False p and its
    gradient (section 5h).  log p and the gradient of log p stay finite and exact where p itself underflows to 0.  A
    DeviceDensity takes host points or a device tensor; the results are numpy arrays."""
    kind, D = _kind(p), _dims(p)
    man = _mf.resolve(p, manifold, D)
    if kind == "host":
        flat = _host_points(pos, D, "evaluate_grad")
        Nq = flat.shape[0]
        val, grad = np.zeros(Nq), np.zeros((Nq, D))
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_evaluate_grad(C.byref(cd), _lib.ptr(flat, _lib.f64p), Nq, int(bool(log)),
                                                 _lib.ptr(val, _lib.f64p), _lib.ptr(grad, _lib.f64p), int(device),
                                                 _mf.pointer(man)))
        return val, np.ascontiguousarray(grad.T)
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        flat = _device_points(pos, D, dev, "evaluate_grad")
        Nq = int(flat.shape[0])
        val = torch.zeros(max(1, Nq), dtype=torch.float64, device=dev)
        grad = torch.zeros((max(1, Nq), D), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib.kdehip_evaluate_grad_device(p._h, _lib.addr(flat), Nq, int(bool(log)), _lib.addr(val),
                                                        _lib.addr(grad), _mf.pointer(man), _lib.addr(st.cuda_stream)))
        st.synchronize()
        return val.cpu().numpy()[:Nq].copy(), np.ascontiguousarray(grad.cpu().numpy()[:Nq].T)


def _iteration(tol, maxiter):
    tol, maxiter = float(tol), int(maxiter)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0")
    if maxiter < 0:
        raise ValueError("maxiter must be >= 0")
    return tol, maxiter


def meanshift(p, starts=None, *, tol=1e-9, maxiter=500, device=0, manifold=None):
    """(x (D, K), logp (K,), iters (K,)): every column of `starts` (D, K) -- None: the density's own points, in getPoints
    order -- moved by mean-shift steps until a step is at most `tol` bandwidths long in every dimension, or for `maxiter`
    steps.  iters = the steps taken, negative where the last of them was still above tol; logp = log p at x.  A start with a
    NaN coordinate stays where it is: iters = 0 and logp = NaN."""
    kind, D = _kind(p), _dims(p)
    tol, maxiter = _iteration(tol, maxiter)
    man = _mf.resolve(p, manifold, D)
    N = p.bt.num_points if kind == "host" else p.num_points
    if kind == "host":
        flat = None if starts is None else _host_points(starts, D, "meanshift")
        K = N if flat is None else flat.shape[0]
        x, logp, iters = np.zeros((K, D)), np.zeros(K), np.zeros(K, dtype=np.int32)
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_meanshift(C.byref(cd), _lib.optr(flat, _lib.f64p), K, C.byref(C.c_double(tol)), maxiter, _lib.ptr(x, _lib.f64p),
                                             _lib.ptr(logp, _lib.f64p), _lib.ptr(iters, _lib.i32p), int(device),
                                             _mf.pointer(man)))
    else:
        import torch
        dev = torch.device("cuda", p.device)
        with torch.cuda.device(dev):
            flat = None if starts is None else _device_points(starts, D, dev, "meanshift")
            K = N if flat is None else int(flat.shape[0])
            x, logp, iters = np.zeros((K, D)), np.zeros(K), np.zeros(K, dtype=np.int32)
            if flat is not None:
                torch.cuda.current_stream(dev).synchronize()  # (the call runs on the calling thread's own stream)
            _lib.check(_lib.lib.kdehip_meanshift_device(p._h, _lib.addr(flat), K, C.byref(C.c_double(tol)), maxiter, _lib.ptr(x, _lib.f64p),
                                                        _lib.ptr(logp, _lib.f64p), _lib.ptr(iters, _lib.i32p),
                                                        _mf.pointer(man)))
    return np.ascontiguousarray(x.T), logp, iters


def meanshift_device_batch(items, tol, niter, stream=None):
    """Mean shift of many DeviceDensity items in ONE call (kdehip_meanshift_device_batch): `items` = dicts with `density`,
    `x` (float64 device tensor of K rows of D: the results), `logp` (float64, K), `iters` (int32, K) and optionally `starts`
    (a device tensor of K rows of D, may be `x` itself; None = the density's own points, K = its size) and `manifold`.
    Exactly `niter` sweeps and the closing evaluation are enqueued on `stream`, with no read-back: the call can be captured
    in a graph.  Every item's results are bit for bit `meanshift(density, starts, tol=tol, maxiter=niter)`, transposed."""
    from .product import DeviceDensity
    tol, niter = _iteration(tol, niter)
    items = list(items)
    n = len(items)
    arr = (_lib.CMeanshiftItem * max(1, n))()
    for k, it in enumerate(items):
        d = it["density"]
        if not isinstance(d, DeviceDensity):
            raise TypeError("meanshift_device_batch: items of DeviceDensity")
        x, starts = it["x"], it.get("starts")
        K = int(x.shape[0])
        if x.dim() != 2 or int(x.shape[1]) != d.dims or (starts is not None and tuple(starts.shape) != tuple(x.shape)):
            raise ValueError("meanshift_device_batch: x and starts are K rows of D")
        if int(it["logp"].numel()) < K or int(it["iters"].numel()) < K:
            raise ValueError("meanshift_device_batch: logp and iters hold K entries")
        arr[k].bd, arr[k].d_start, arr[k].nstart = d._h, _lib.addr(starts), K
        arr[k].d_x, arr[k].d_logp, arr[k].d_iters = _lib.addr(x), _lib.addr(it["logp"]), _lib.addr(it["iters"])
        arr[k].circular_mask = _mf.mask(_mf.resolve(d, it.get("manifold"), d.dims))
    _lib.check(_lib.lib.kdehip_meanshift_device_batch(n, arr, C.byref(C.c_double(tol)), niter, _lib.addr(stream)))


def _host_arrays(p, kind):
    """the density as host arrays: itself, the arrays an uploaded DeviceDensity came from, or a built one's download"""
    if kind == "host":
        return p
    return p._host if getattr(p, "_host", None) is not None else p.download()


def _bandwidth_sd(h):
    """a host density's one bandwidth vector as standard deviations"""
    N, D = h.bt.num_points, h.bt.dims
    return np.sqrt(h.bandwidth[N * D:(N + 1) * D])


def merge_modes(x, logp, iters, sd, merge, man=None):
    """The greedy merge of converged points: in descending logp (ties by index) a point joins the first kept mode within
    `merge` in max_k |diff_k| / sd_k (the difference wrapped where circular), else it founds one.  Returns (indices of the
    founders, labels (K,)); an unconverged point (iters < 0) and a point whose logp is NaN (a start with a NaN coordinate)
    are labelled -1."""
    K = x.shape[1]
    labels = np.full(K, -1, dtype=np.int64)
    order = sorted((k for k in range(K) if iters[k] >= 0 and logp[k] == logp[k]), key=lambda k: (-logp[k], k))
    kept = []
    circ = None if man is None else np.asarray(man, dtype=bool)
    for k in order:
        for j, f in enumerate(kept):
            d = x[:, k] - x[:, f]
            if circ is not None:
                d = np.where(circ, d - 2.0 * np.pi * np.floor((d + np.pi) / (2.0 * np.pi)), d)
            if np.max(np.abs(d) / sd) <= merge:
                labels[k] = j
                break
        else:
            labels[k] = len(kept)
            kept.append(k)
    return kept, labels


def modes(p, starts=None, *, tol=1e-9, maxiter=500, merge=1e-3, device=0, manifold=None):
    """(modes (D, n), logp (n,), mass (n,), labels (K,)): `meanshift` from `starts` (None: the density's own points), the
    converged points merged greedily on the host -- in descending logp, ties by index, a point joins the first kept mode
    within `merge` bandwidths (max_k |diff_k| / sqrt(v_k), wrapped where circular), else it founds a new one.  The modes
    come in descending logp.  mass = the summed weights of the starts labelled to each mode when the starts are the
    density's own points, and the share of the starts (counts / K) otherwise.  Unconverged starts are labelled -1 and belong
    to no mode, and so are starts with a NaN coordinate.  For a DeviceDensity the merge reads the bandwidth and the weights
    from the host density it was uploaded from (or from its download if it was built on the device): do not change that host
    density after the upload."""
    kind, D = _kind(p), _dims(p)
    man = _mf.resolve(p, manifold, D)
    x, logp, iters = meanshift(p, starts, tol=tol, maxiter=maxiter, device=device, manifold=man)
    h = _host_arrays(p, kind)
    kept, labels = merge_modes(x, logp, iters, _bandwidth_sd(h), float(merge), man)
    K = x.shape[1]
    if starts is None:
        w = getWeights(h)
    else:
        w = np.full(K, 1.0 / K) if K else np.zeros(0)
    mass = np.array([float(np.sum(w[labels == j])) for j in range(len(kept))])
    return np.ascontiguousarray(x[:, kept]), logp[kept], mass, labels


def getKDEMode(p, **kw):
    """The joint mode of the density: the highest of `modes(p, **kw)`, a point of the D-dimensional space at which the
    density itself has a local maximum.  `getKDEMax` is the reference's summary -- the grid argmax of every 1-D marginal,
    each dimension on its own: for a multimodal density its coordinates may come from different modes, and the point may lie
    where the density is low.  Use this one when the point has to be a mode."""
    return modes(p, **kw)[0][:, 0]
