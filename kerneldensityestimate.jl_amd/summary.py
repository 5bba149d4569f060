"""Summaries of a density: `marginal`, `getKDERange`, `getKDERangeLinspace`, `getKDEMax`, `getKDEMean`, `getKDEfit` and
`intersIntgAppxIS` (reference src/KDE01.jl:143-153, src/DualTree01.jl:512-618), over kdehip_density_marginal_device,
kdehip_summary_device_batch, kdehip_density_summary, kdehip_kde_max and kdehip_inters_intg_appx_is[_device]
(include/kdehip.h section 5c; kernels in csrc/summary.hip).

A density's points are its leaf means in original (getPoints) order; `dims` are 0-based.  A BallTreeDensity gets its
range, mean and fit from numpy -- the sequential sums through np.cumsum, never np.sum, which is pairwise -- and its
getKDEMax / intersIntgAppxIS from the C entries (the density is uploaded for the call).  A DeviceDensity gets everything
on its device.  Arguments that mix the two kinds are a TypeError.  Only the Euclidean operators exist (no addop / diffop).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import f64p, i32p, ptr
from .density import BallTreeDensity, getBW, getWeights, kde


def _is_device(p):
    from .product import DeviceDensity
    if isinstance(p, DeviceDensity):
        return True
    if isinstance(p, BallTreeDensity):
        return False
    raise TypeError("expected a BallTreeDensity or a DeviceDensity")


def _same_kind(ps):
    kinds = {_is_device(p) for p in ps}
    if len(kinds) > 1:
        raise TypeError("densities must all be BallTreeDensity, or all DeviceDensity")
    return kinds.pop()


def _ndim(p):
    return p.dims if _is_device(p) else p.bt.dims


def _leaf_points(p):
    """getPoints(p) from the leaf means: (D, N), original order."""
    N, D = p.bt.num_points, p.bt.dims
    out = np.empty((D, N))
    out[:, p.bt.permutation[N:] - 1] = p.means[N * D:].reshape(N, D).T
    return out


def _dims_list(dims, D):
    dims = [dims] if np.isscalar(dims) else list(dims)
    if not 1 <= len(dims) <= _lib.MAX_DIMS:
        raise ValueError(f"marginal: between 1 and {_lib.MAX_DIMS} dims")
    out = []
    for d in dims:
        if int(d) != d or not 0 <= int(d) < D:
            raise ValueError(f"marginal: dims must be integers in 0..{D - 1}")
        out.append(int(d))
    return out


def grid(lo, hi, N):
    """The summaries' grid: x_k = lo + k h, h = (hi - lo) / (N - 1), x_{N-1} = hi, every operation rounded on its own.
    (Julia's range(lo, stop=hi, length=N) forms its points in double-double: the two may differ in the last bit.)"""
    N = int(N)
    if N < 2:
        raise ValueError("the grid needs N >= 2 points")
    lo, hi = np.float64(lo), np.float64(hi)
    h = (hi - lo) / np.float64(N - 1)
    x = lo + np.arange(N, dtype=np.float64) * h
    x[-1] = hi
    return x


def _summary(p, *, extend=0.1, N=200, range_=False, mean=False, cov=False, argmax=False, values=False):
    """kdehip_density_summary of a DeviceDensity: the asked-for outputs as numpy arrays."""
    D = p.dims
    ext = C.c_double(float(extend))
    out = {}
    bufs = {}
    for name, want, shape in (("range", range_, (2, D)), ("mean", mean, (D,)), ("cov", cov, (D, D)),
                              ("argmax", argmax, (D,)), ("values", values, (D, int(N)))):
        bufs[name] = np.zeros(shape) if want else None
    _lib.check(_lib.lib.kdehip_density_summary(
        p._h, C.byref(ext), int(N), *[None if bufs[k] is None else ptr(bufs[k], f64p)
                                      for k in ("range", "mean", "cov", "argmax", "values")]))
    for k, v in bufs.items():
        if v is not None:
            out[k] = v.T.copy() if k == "range" else v  # range: D x 2 column-major
    return out


def marginal(p, dims):
    """`marginal(p, dims)` (src/KDE01.jl:143-153) = kde(getPoints(p)[dims], getBW(p)[dims, 0], getWeights(p)): the bandwidth
    of ORIGINAL point 0, whose variance comes back as fl(sqrt(v))**2; repeated and reordered dims allowed.  A BallTreeDensity
    gives a BallTreeDensity (host builder), a DeviceDensity a DeviceDensity (kdehip_density_marginal_device)."""
    if _is_device(p):
        return p.marginal(dims)
    dims = _dims_list(dims, p.bt.dims)
    return kde(_leaf_points(p)[dims, :], getBW(p)[dims, 0], getWeights(p))


def getKDERange(p, extend=0.1):
    """`getKDERange(p; extend)` (src/DualTree01.jl:512-540): (D, 2), per dimension (lo - dr, hi + dr) with lo / hi the
    min / max over the points and dr = extend * (hi - lo).  A list of densities: the element-wise union (:542-553)."""
    if isinstance(p, (list, tuple)):
        if not p:
            raise ValueError("getKDERange: no densities")
        _same_kind(p)
        if len({_ndim(x) for x in p}) > 1:
            raise ValueError("getKDERange: densities of different dimensions")
        out = getKDERange(p[0], extend)
        for x in p[1:]:
            r = getKDERange(x, extend)
            out[:, 0] = np.where(out[:, 0] < r[:, 0], out[:, 0], r[:, 0])
            out[:, 1] = np.where(out[:, 1] > r[:, 1], out[:, 1], r[:, 1])
        return out
    if _is_device(p):
        return _summary(p, extend=extend, range_=True)["range"]
    pts = _leaf_points(p)
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    dr = np.float64(extend) * (hi - lo)
    return np.stack([lo - dr, hi + dr], axis=1)


def getKDERangeLinspace(p, extend=0.1, N=200):
    """`getKDERangeLinspace(p; extend, N)` (src/DualTree01.jl:552-556): the grid over getKDERange(p, extend).  1-D densities
    only: for D > 1 the reference's (v[1], v[2]) would be (lo_1, lo_2)."""
    if _ndim(p) != 1:
        raise ValueError("getKDERangeLinspace: 1-D densities only")
    v = getKDERange(p, extend)
    return grid(v[0, 0], v[0, 1], N)


def getKDEMax(p, N=200, *, values=False, device=0):
    """`getKDEMax(p; N)` (src/DualTree01.jl:558-570): per dimension, the grid point of the FIRST maximum of the 1-D marginal
    on the N-point grid over its range with extend 0.1.  values=True also returns the (D, N) grid values."""
    N = int(N)
    if _is_device(p):
        r = _summary(p, N=N, argmax=True, values=values)
        return (r["argmax"], r["values"]) if values else r["argmax"]
    D = p.bt.dims
    m = np.zeros(D)
    vals = np.zeros((D, max(N, 0))) if values else None
    _lib.check(_lib.lib.kdehip_kde_max(C.byref(p._cstruct()), N, ptr(m, f64p), None if vals is None else ptr(vals, f64p),
                                       int(device)))
    return (m, vals) if values else m


def getKDEMean(p):
    """`getKDEMean(p)` (src/DualTree01.jl:572-575) = mean(getPoints(p), dims=2): unweighted, per dimension the sequential
    sum in original order from +0.0, then / N."""
    if _is_device(p):
        return _summary(p, mean=True)["mean"]
    pts = _leaf_points(p)
    s = np.cumsum(np.concatenate([np.zeros((pts.shape[0], 1)), pts], axis=1), axis=1)[:, -1]
    return s / np.float64(pts.shape[1])


def getKDEfit(p):
    """`getKDEfit(p)` (src/DualTree01.jl:576-578) = fit(MvNormal, getPoints(p)): (mu, Sigma) with mu = getKDEMean(p) and
    Sigma = (1/N) sum (x - mu)(x - mu)^T."""
    if _is_device(p):
        r = _summary(p, mean=True, cov=True)
        return r["mean"], r["cov"]
    mu = getKDEMean(p)
    X = _leaf_points(p) - mu[:, None]
    return mu, (X @ X.T) / np.float64(X.shape[1])


def intersIntgAppxIS(p, q, N=201, *, device=0):
    """`intersIntgAppxIS(p, q; N)` (src/DualTree01.jl:581-618), 1-D and 2-D: p and q evaluated by the direct sum on the
    grid over p's marginal ranges with extend 0.3, sum of p q times the cell size (rows in order in 2-D)."""
    dev = _same_kind([p, q])
    out = C.c_double(0.0)
    if dev:
        _lib.check(_lib.lib.kdehip_inters_intg_appx_is_device(p._h, q._h, int(N), C.byref(out)))
    else:
        _lib.check(_lib.lib.kdehip_inters_intg_appx_is(C.byref(p._cstruct()), C.byref(q._cstruct()), int(N), C.byref(out),
                                                       int(device)))
    return float(out.value)


def summary_device_batch(items, stream=None):
    """Summaries of many DeviceDensity in ONE call (kdehip_summary_device_batch): `items` = dicts with `density` and
    optionally `extend` (0.1), `Ngrid` (200) and the device outputs (torch tensors or addresses, float64) `range` (2D,
    D x 2 column-major), `mean` (D), `cov` (D*D), `argmax` (D), `values` (D*Ngrid).  Enqueues on `stream` and returns."""
    from .product import DeviceDensity, ProductPlan
    items = list(items)
    n = len(items)
    arr = (_lib.CSummaryItem * max(1, n))()
    for k, it in enumerate(items):
        if not isinstance(it["density"], DeviceDensity):
            raise TypeError("summary_device_batch: items of DeviceDensity")
        a = arr[k]
        a.density = it["density"]._h
        a.extend = float(it.get("extend", 0.1))
        a.Ngrid = int(it.get("Ngrid", 200))
        a.d_range, a.d_mean, a.d_cov = (ProductPlan._addr(it.get(x)) for x in ("range", "mean", "cov"))
        a.d_argmax, a.d_values = ProductPlan._addr(it.get("argmax")), ProductPlan._addr(it.get("values"))
    _lib.check(_lib.lib.kdehip_summary_device_batch(n, arr, ProductPlan._addr(stream)))


def _marginal_device(p, dims):
    """kdehip_density_marginal_device (DeviceDensity.marginal)."""
    from .product import DeviceDensity
    dl = _dims_list(dims, p.dims)
    d = np.array([x + 1 for x in dl], dtype=np.int32)
    h = C.c_void_p()
    _lib.check(_lib.lib.kdehip_density_marginal_device(C.byref(h), p._h, len(dl), ptr(d, i32p)))
    return DeviceDensity(device=p.device, _handle=h)
