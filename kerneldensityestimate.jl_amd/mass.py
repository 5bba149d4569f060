"""The probability mass of a density: `box_mass`, `cdf`, `quantile`, `median`, `interval`, `grid_mass` and the batches
`box_mass_device_batch` / `quantile_device_batch`, over kdehip_box_mass[_device][_batch] and kdehip_quantile[_device][_batch]
(include/kdehip.h section 5l; kernels in csrc/mass.hip).  The library's own: the reference's only range summary is
`getKDERange`, a support box rather than a probability.

For a Gaussian-kernel density with one bandwidth vector v, bounded dimensions B and a box [lo, hi],

    mass = sum_i w_i prod_{k in B} ( Phi((hi_k - c_ik) / sqrt(v_k)) - Phi((lo_k - c_ik) / sqrt(v_k)) ),

each factor written with erfc in the tail where the difference is accurate; the marginal cdf of dimension k is the mass of
(-Inf, x] in B = {k}, and a quantile is the root of cdf(x) = alpha, found on the device by a bracketed Newton iteration.
`dims` are 0-based, distinct and in any order; the rows of `lo` and `hi` follow `dims` as given.  The density is a
BallTreeDensity (host arrays, run on `device`) or a DeviceDensity (on its own device); `manifold=` as the other entries take
it, "inherit" included: a circular dimension cannot be bounded, an unbounded one is fine.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .loglik import _dims
from .modes import _kind


def _bounded(dims, D):
    """(the order that sorts the dims, the mask); None = every dimension"""
    if dims is None:
        dl = list(range(D))
    else:
        dl = [dims] if np.isscalar(dims) else list(dims)
    for d in dl:
        if int(d) != d or not 0 <= int(d) < D:
            raise ValueError(f"box_mass: dims must be integers in 0..{D - 1}")
    dl = [int(d) for d in dl]
    if len(set(dl)) != len(dl):
        raise ValueError("box_mass: dims must be distinct")
    if not dl:
        raise ValueError("box_mass: at least one dimension is bounded")
    return np.argsort(dl), sum(1 << d for d in dl)


def _bounds(lo, hi, nb, order):
    """`lo`, `hi` (nb, Nq) -- a vector is ONE box of nb values, or Nq boxes when nb == 1; either may be a scalar -- as two
    arrays of Nq rows in ascending order of the bounded dimensions"""
    out = []
    for a in (lo, hi):
        if hasattr(a, "data_ptr"):
            a = a.detach().cpu().numpy()
        A = np.asarray(a, dtype=np.float64)
        if A.ndim == 1:
            A = A.reshape(1, -1) if nb == 1 else A.reshape(-1, 1)
        out.append(A)
    lo, hi = out
    if lo.ndim == 0 and hi.ndim == 0:
        lo, hi = lo.reshape(1, 1), hi.reshape(1, 1)
    try:
        lo, hi = np.broadcast_arrays(lo, hi)
    except ValueError:
        raise ValueError("box_mass: lo and hi hold one value per bounded dimension and box") from None
    if lo.ndim != 2 or lo.shape[0] != nb:
        raise ValueError("box_mass: lo and hi hold one value per bounded dimension and box")
    return np.ascontiguousarray(lo[order, :].T), np.ascontiguousarray(hi[order, :].T)


def box_mass(p, lo, hi, dims=None, *, device=0, manifold=None):
    """mass (Nq,): the probability that x_dims lies in [lo[:, q], hi[:, q]] under `p`, the other dimensions free
    (kdehip_box_mass, section 5l).  `lo`, `hi` are (nb, Nq), rows in the order of `dims` (None: all dimensions); +-Inf are
    bounds like any other, lo >= hi in a dimension gives exactly 0, a NaN bound gives NaN for that box only."""
    kind, D = _kind(p), _dims(p)
    order, mask = _bounded(dims, D)
    man = _mf.resolve(p, manifold, D)
    L, H = _bounds(lo, hi, len(order), order)
    Nq = L.shape[0]
    if kind == "host":
        out = np.zeros(Nq)
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_box_mass(C.byref(cd), mask, _lib.ptr(L, _lib.f64p), _lib.ptr(H, _lib.f64p), Nq,
                                            _lib.ptr(out, _lib.f64p), int(device), _mf.pointer(man)))
        return out
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        d_lo, d_hi = torch.from_numpy(L).to(dev), torch.from_numpy(H).to(dev)
        out = torch.zeros(max(1, Nq), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib.kdehip_box_mass_device(p._h, mask, _lib.addr(d_lo), _lib.addr(d_hi), Nq, _lib.addr(out),
                                                   _mf.pointer(man), _lib.addr(st.cuda_stream)))
        st.synchronize()
        return out.cpu().numpy()[:Nq].copy()


def _one_dim(dim, D, what):
    if np.ndim(dim) != 0 or int(dim) != dim or not 0 <= int(dim) < D:
        raise ValueError(f"{what}: dim is one integer in 0..{D - 1}")
    return int(dim)


def cdf(p, x, dim, *, device=0, manifold=None):
    """F (Nq,): the marginal cdf of dimension `dim` at the values `x` -- `box_mass` with lo = -Inf in that one dimension."""
    _kind(p)
    dim = _one_dim(dim, _dims(p), "cdf")
    x = np.asarray(x.detach().cpu().numpy() if hasattr(x, "data_ptr") else x, dtype=np.float64).reshape(1, -1)
    return box_mass(p, np.full_like(x, -np.inf), x, [dim], device=device, manifold=manifold)


def _iteration(tol, max_iter):
    tol, max_iter = float(tol), int(max_iter)
    if not (tol == 0.0 or (np.isfinite(tol) and tol >= 1e-14)):
        raise ValueError("quantile: tol must be finite and >= 1e-14 (0: the default 1e-12)")
    if max_iter < 0:
        raise ValueError("quantile: max_iter must be >= 1 (0: the default 100)")
    return tol, max_iter


def quantile(p, alpha, dim, *, tol=1e-12, max_iter=100, full=False, device=0, manifold=None):
    """x, of alpha's shape: the `alpha` quantiles of the marginal of dimension `dim`, cdf(x) = alpha to `tol` (absolute in
    the cdf), by a bracketed Newton iteration on the device (kdehip_quantile, section 5l).  full=True returns
    (x, resid, iters, converged): resid = cdf(x) - alpha at the returned x, iters the number of cdf evaluations, converged
    False where `max_iter` evaluations did not reach `tol`.  An alpha outside (0, 1) or NaN gives NaN for that level only."""
    kind, D = _kind(p), _dims(p)
    dim = _one_dim(dim, D, "quantile")
    tol, max_iter = _iteration(tol, max_iter)
    man = _mf.resolve(p, manifold, D)
    if hasattr(alpha, "data_ptr"):
        alpha = alpha.detach().cpu().numpy()
    A = np.asarray(alpha, dtype=np.float64)
    shape = A.shape
    a = np.ascontiguousarray(A.reshape(-1))
    Nq = a.shape[0]
    if kind == "host":
        x, resid = np.zeros(Nq), np.zeros(Nq)
        iters, conv = np.zeros(Nq, dtype=np.int32), np.zeros(Nq, dtype=np.int32)
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_quantile(C.byref(cd), dim, _lib.ptr(a, _lib.f64p), Nq, C.byref(C.c_double(tol)), max_iter,
                                            _lib.ptr(x, _lib.f64p),
                                            _lib.optr(resid if full else None, _lib.f64p),
                                            _lib.optr(iters if full else None, _lib.i32p),
                                            _lib.optr(conv if full else None, _lib.i32p), int(device), _mf.pointer(man)))
    else:
        import torch
        dev = torch.device("cuda", p.device)
        with torch.cuda.device(dev):
            d_a = torch.from_numpy(a).to(dev)
            n = max(1, Nq)
            d_x = torch.zeros(n, dtype=torch.float64, device=dev)
            d_r = torch.zeros(n, dtype=torch.float64, device=dev) if full else None
            d_i = torch.zeros(n, dtype=torch.int32, device=dev) if full else None
            d_c = torch.zeros(n, dtype=torch.int32, device=dev) if full else None
            st = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib.kdehip_quantile_device(p._h, dim, _lib.addr(d_a), Nq, C.byref(C.c_double(tol)), max_iter,
                                                       _lib.addr(d_x),
                                                       _lib.addr(d_r), _lib.addr(d_i), _lib.addr(d_c), _mf.pointer(man),
                                                       _lib.addr(st.cuda_stream)))
            st.synchronize()
            x = d_x.cpu().numpy()[:Nq].copy()
            if full:
                resid, iters, conv = (t.cpu().numpy()[:Nq].copy() for t in (d_r, d_i, d_c))
    if not full:
        return x.reshape(shape)[()]
    return x.reshape(shape)[()], resid.reshape(shape)[()], iters.reshape(shape)[()], (conv != 0).reshape(shape)[()]


def median(p, dim, **kw):
    """the median of the marginal of dimension `dim`: `quantile(p, 0.5, dim)`"""
    return quantile(p, 0.5, dim, **kw)


def interval(p, dim, level=0.95, **kw):
    """(lo, hi): the central credible interval of the marginal of dimension `dim` that holds `level` of the mass -- the
    quantiles at (1 - level) / 2 and (1 + level) / 2"""
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("interval: level lies in (0, 1)")
    x = quantile(p, [(1.0 - level) / 2.0, (1.0 + level) / 2.0], dim, **kw)
    return float(x[0]), float(x[1])


def grid_mass(p, edges, dims=None, *, device=0, manifold=None):
    """The mass of every cell of the product grid of the per-dimension edge arrays `edges` (one ascending 1-D array of at
    least two edges per entry of `dims`, None: all dimensions), as ONE `box_mass` call: an array of shape
    (len(edges[0]) - 1, len(edges[1]) - 1, ...) -- a belief as an occupancy grid.  With -Inf and +Inf as the outer edges
    the cells partition the space and sum to the total weight."""
    _kind(p)
    D = _dims(p)
    nb = D if dims is None else (1 if np.isscalar(dims) else len(list(dims)))
    E = [np.asarray(e, dtype=np.float64).reshape(-1) for e in edges]
    if len(E) != nb or any(e.shape[0] < 2 for e in E):
        raise ValueError("grid_mass: one array of at least two edges per bounded dimension")
    shape = tuple(e.shape[0] - 1 for e in E)
    lo = np.stack([g.reshape(-1) for g in np.meshgrid(*[e[:-1] for e in E], indexing="ij")])
    hi = np.stack([g.reshape(-1) for g in np.meshgrid(*[e[1:] for e in E], indexing="ij")])
    return box_mass(p, lo, hi, dims, device=device, manifold=manifold).reshape(shape)


def _device_tensor(t, what, name, dtype):
    """the kernels read and write 8-byte (iters, converged: 4-byte) values at consecutive addresses of device memory"""
    if not getattr(t, "is_cuda", False) or str(t.dtype) != "torch." + dtype or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} device tensor")


def box_mass_device_batch(items, stream=None):
    """The box masses of many DeviceDensity items in ONE call (kdehip_box_mass_device_batch): `items` = dicts with `density`,
    `dims` (None or absent: all dimensions), `lo` and `hi` (float64 device tensors of Nq rows of nb values, the columns in
    ASCENDING order of the bounded dimensions) and `mass` (float64, Nq), optionally `manifold`.  Enqueue only on `stream`, no
    read-back: the call can be captured in a graph.  Every item's results are bit for bit the single call's."""
    from .product import DeviceDensity
    what = "box_mass_device_batch"
    items = list(items)
    n = len(items)
    arr = (_lib.CBoxMassItem * max(1, n))()
    for k, it in enumerate(items):
        d = it["density"]
        if not isinstance(d, DeviceDensity):
            raise TypeError(f"{what}: items of DeviceDensity")
        order, mask = _bounded(it.get("dims"), d.dims)
        lo, hi, mass = it["lo"], it["hi"], it["mass"]
        for name, t in (("lo", lo), ("hi", hi), ("mass", mass)):
            _device_tensor(t, what, name, "float64")
        if lo.dim() != 2 or int(lo.shape[1]) != len(order) or tuple(hi.shape) != tuple(lo.shape):
            raise ValueError(f"{what}: lo and hi are Nq rows of nb values")
        Nq = int(lo.shape[0])
        if int(mass.numel()) < Nq:
            raise ValueError(f"{what}: mass holds Nq values")
        a = arr[k]
        a.bd, a.d_lo, a.d_hi, a.Nq, a.d_mass = d._h, _lib.addr(lo), _lib.addr(hi), Nq, _lib.addr(mass)
        a.dim_mask = mask
        a.circular_mask = _mf.mask(_mf.resolve(d, it.get("manifold"), d.dims))
    _lib.check(_lib.lib.kdehip_box_mass_device_batch(n, arr, _lib.addr(stream)))


def quantile_device_batch(items, *, tol=1e-12, max_iter=100, stream=None):
    """The quantiles of many DeviceDensity items in ONE launch (kdehip_quantile_device_batch): `items` = dicts with `density`,
    `dim`, `alpha` (float64 device tensor, Nq) and `x` (float64, Nq), optionally `resid` (float64, Nq), `iters` and
    `converged` (int32, Nq) and `manifold`; `tol` and `max_iter` are the batch's.  Enqueue only on `stream`, no read-back.
    Every item's results are bit for bit the single call's."""
    from .product import DeviceDensity
    what = "quantile_device_batch"
    tol, max_iter = _iteration(tol, max_iter)
    items = list(items)
    n = len(items)
    arr = (_lib.CQuantileItem * max(1, n))()
    for k, it in enumerate(items):
        d = it["density"]
        if not isinstance(d, DeviceDensity):
            raise TypeError(f"{what}: items of DeviceDensity")
        dim = _one_dim(it["dim"], d.dims, what)
        alpha = it["alpha"]
        _device_tensor(alpha, what, "alpha", "float64")
        Nq = int(alpha.numel())
        outs = {name: it.get(name) for name in ("x", "resid", "iters", "converged")}
        if outs["x"] is None:
            raise ValueError(f"{what}: an item has no x")
        for name, t in outs.items():
            if t is not None:
                _device_tensor(t, what, name, "float64" if name in ("x", "resid") else "int32")
                if int(t.numel()) < Nq:
                    raise ValueError(f"{what}: {name} holds Nq values")
        a = arr[k]
        a.bd, a.d_alpha, a.Nq, a.d_x = d._h, _lib.addr(alpha), Nq, _lib.addr(outs["x"])
        a.d_resid, a.d_iters, a.d_converged = (_lib.addr(outs[x]) for x in ("resid", "iters", "converged"))
        a.dim = dim
        a.circular_mask = _mf.mask(_mf.resolve(d, it.get("manifold"), d.dims))
    _lib.check(_lib.lib.kdehip_quantile_device_batch(n, arr, C.byref(C.c_double(tol)), max_iter, _lib.addr(stream)))
