"""Summaries of a density: `marginal`, `getKDERange`, `getKDERangeLinspace`, `getKDEMax`, `getKDEMean`, `getKDEfit` and
`intersIntgAppxIS` (reference src/KDE01.jl:143-153, src/DualTree01.jl:512-618), over kdehip_density_marginal_device,
kdehip_summary_device_batch, kdehip_density_summary, kdehip_kde_max and kdehip_inters_intg_appx_is[_device]
(include/kdehip.h section 5c; kernels in csrc/summary.hip).

A density's points are its leaf means in original (getPoints) order; `dims` are 0-based.  A BallTreeDensity gets its
range, mean and fit from numpy -- the sequential sums through np.cumsum, never np.sum, which is pairwise -- and its
getKDEMax / intersIntgAppxIS from the C entries (the density is uploaded for the call).  A DeviceDensity gets everything
on its device.  Arguments that mix the two kinds are a TypeError.

`manifold=` (None, a per-dimension sequence of 'euclid' / 'circular' or 0 / 1, or "inherit" = the density's recorded
`.manifold`) gives the reference's addop / diffop of these functions as the enum of include/kdehip.h: section 5e states what
each summary means on the circle (tangent offsets wrap(x - a0) at original point 1's angle).  None and all-Euclidean return
today's bits.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import addr, f64p, i32p, optr, ptr
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


_PI, _TWO_PI = np.float64(np.pi), np.float64(2.0 * np.pi)   # circ_wrap's constants (csrc/circ_wrap.hpp)


def _wrap(t):
    """wrap() to [-pi, pi): the one expression of csrc/circ_wrap.hpp, every operation rounded on its own"""
    t = np.asarray(t, dtype=np.float64)
    return t - _TWO_PI * np.floor((t + _PI) / _TWO_PI)


def _manifold(p, manifold, attr="manifold"):
    """the `manifold=` / `tree_manifold=` of a call on the density p (manifold.resolve)"""
    return _mf.resolve(p, manifold, _ndim(p), attr)


def _seqsum(x):
    """the sequential left-to-right sum of each row from +0.0 (np.sum is pairwise)"""
    return np.cumsum(np.concatenate([np.zeros((x.shape[0], 1)), x], axis=1), axis=1)[:, -1]


def _circ_offsets(pts, man):
    """(a0, t): per dimension the reference angle (original point 0; 0.0 in a Euclidean dimension) and the tangent offsets
    wrap(x - a0) (x itself in a Euclidean dimension)"""
    circ = man.astype(bool)
    a0 = np.where(circ, pts[:, 0], 0.0)
    t = pts.copy()
    t[circ] = _wrap(pts[circ] - a0[circ, None])
    return a0, t


def _circ_mean(pts, man):
    a0, t = _circ_offsets(pts, man)
    mu = _seqsum(t) / np.float64(pts.shape[1])
    circ = man.astype(bool)
    mu[circ] = _wrap(a0[circ] + mu[circ])
    return mu


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


def _summary(p, *, extend=0.1, N=200, range_=False, mean=False, cov=False, argmax=False, values=False, man=None):
    """kdehip_density_summary[_manifold] of a DeviceDensity: the asked-for outputs as numpy arrays."""
    D = p.dims
    ext = C.c_double(float(extend))
    out = {}
    bufs = {}
    for name, want, shape in (("range", range_, (2, D)), ("mean", mean, (D,)), ("cov", cov, (D, D)),
                              ("argmax", argmax, (D,)), ("values", values, (D, int(N)))):
        bufs[name] = np.zeros(shape) if want else None
    args = [optr(bufs[k], f64p) for k in ("range", "mean", "cov", "argmax", "values")]
    _lib.check(_lib.lib.kdehip_density_summary_manifold(p._h, C.byref(ext), int(N), *args, _mf.pointer(man)))
    for k, v in bufs.items():
        if v is not None:
            out[k] = v.T.copy() if k == "range" else v  # range: D x 2 column-major
    return out


def marginal(p, dims, *, manifold=None, tree_manifold=None):
    """`marginal(p, dims)` (src/KDE01.jl:143-153) = kde(getPoints(p)[dims], getBW(p)[dims, 0], getWeights(p)): the bandwidth
    of ORIGINAL point 0, whose variance comes back as fl(sqrt(v))**2; repeated and reordered dims allowed.  A BallTreeDensity
    gives a BallTreeDensity (host builder), a DeviceDensity a DeviceDensity (kdehip_density_marginal_device[_tree]).
    `tree_manifold` (one entry per dimension of p, or "inherit"): the result's tree is built with tree_manifold[dims];
    `manifold` (likewise) is only recorded: the result remembers manifold[dims] and tree_manifold[dims]."""
    if _is_device(p):
        return p.marginal(dims, manifold=manifold, tree_manifold=tree_manifold)
    dl = _dims_list(dims, p.bt.dims)
    tman = _mf.select(_manifold(p, tree_manifold, attr="tree_manifold"), dl)
    _manifold(p, manifold)   # (validated; a BallTreeDensity has no manifold record)
    if p.multibandwidth == 1:  # per-point bandwidths: every point keeps its own, the selected rows
        from .varbw import kde_varbw
        return kde_varbw(_leaf_points(p)[dl, :], getBW(p)[dl, :], getWeights(p), tree_manifold=tman)
    return kde(_leaf_points(p)[dl, :], getBW(p)[dl, 0], getWeights(p), tree_manifold=tman)


def _circ_range(pts, man, extend):
    """section 5e: per circular dimension the arc (a0 + lo_t - dr, a0 + hi_t + dr), unwrapped, at most one turn"""
    a0, t = _circ_offsets(pts, man)
    lo, hi = t.min(axis=1), t.max(axis=1)
    dr = np.float64(extend) * (hi - lo)
    alo, ahi = a0 + lo, a0 + hi    # (only read in the circular dimensions)
    rlo, rhi = alo - dr, ahi + dr
    circ = man.astype(bool)
    rlo = np.where(circ, rlo, lo - dr)
    rhi = np.where(circ, rhi, hi + dr)
    with np.errstate(invalid="ignore"):
        turn = circ & (rhi - rlo > _TWO_PI)
    mid = np.float64(0.5) * (alo + ahi)
    return np.stack([np.where(turn, mid - _PI, rlo), np.where(turn, mid + _PI, rhi)], axis=1)


def getKDERange(p, extend=0.1, *, manifold=None):
    """`getKDERange(p; extend)` (src/DualTree01.jl:512-540): (D, 2), per dimension (lo - dr, hi + dr) with lo / hi the
    min / max over the points and dr = extend * (hi - lo).  A list of densities: the element-wise union (:542-553).
    `manifold`: in a circular dimension the arc through the tangent offsets, left unwrapped (section 5e)."""
    if isinstance(p, (list, tuple)):
        if not p:
            raise ValueError("getKDERange: no densities")
        _same_kind(p)
        if len({_ndim(x) for x in p}) > 1:
            raise ValueError("getKDERange: densities of different dimensions")
        out = getKDERange(p[0], extend, manifold=manifold)
        for x in p[1:]:
            r = getKDERange(x, extend, manifold=manifold)
            out[:, 0] = np.where(out[:, 0] < r[:, 0], out[:, 0], r[:, 0])
            out[:, 1] = np.where(out[:, 1] > r[:, 1], out[:, 1], r[:, 1])
        return out
    man = _manifold(p, manifold)
    if _is_device(p):
        return _summary(p, extend=extend, range_=True, man=man)["range"]
    pts = _leaf_points(p)
    if man is not None:
        return _circ_range(pts, man, extend)
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    dr = np.float64(extend) * (hi - lo)
    return np.stack([lo - dr, hi + dr], axis=1)


def getKDERangeLinspace(p, extend=0.1, N=200, *, manifold=None):
    """`getKDERangeLinspace(p; extend, N)` (src/DualTree01.jl:552-556): the grid over getKDERange(p, extend).  1-D densities
    only: for D > 1 the reference's (v[1], v[2]) would be (lo_1, lo_2).  `manifold`: the grid over the circular range,
    unwrapped (monotone; wrap its points to read them as angles)."""
    if _ndim(p) != 1:
        raise ValueError("getKDERangeLinspace: 1-D densities only")
    v = getKDERange(p, extend, manifold=manifold)
    return grid(v[0, 0], v[0, 1], N)


def getKDEMax(p, N=200, *, values=False, device=0, manifold=None):
    """`getKDEMax(p; N)` (src/DualTree01.jl:558-570): per dimension, the grid point of the FIRST maximum of the 1-D marginal
    on the N-point grid over its range with extend 0.1.  values=True also returns the (D, N) grid values.
    `manifold`: the circular range, wrapped differences on the grid, the argmax wrapped to [-pi, pi) (section 5e).
    Every dimension is taken on its own, as the reference does: for a multimodal density the coordinates may come from
    different modes, so the point need not lie near any of them.  `getKDEMode` is the joint mode -- a local maximum of the
    D-dimensional density itself, by mean shift (section 5h)."""
    N = int(N)
    man = _manifold(p, manifold)
    if _is_device(p):
        r = _summary(p, N=N, argmax=True, values=values, man=man)
        return (r["argmax"], r["values"]) if values else r["argmax"]
    D = p.bt.dims
    m = np.zeros(D)
    vals = np.zeros((D, max(N, 0))) if values else None
    _lib.check(_lib.lib.kdehip_kde_max_manifold(C.byref(p._cstruct()), N, ptr(m, f64p), optr(vals, f64p), int(device),
                                                _mf.pointer(man)))
    return (m, vals) if values else m


def getKDEMean(p, *, manifold=None):
    """`getKDEMean(p)` (src/DualTree01.jl:572-575) = mean(getPoints(p), dims=2): unweighted, per dimension the sequential
    sum in original order from +0.0, then / N.  `manifold`: in a circular dimension wrap(a0 + mean of the tangent offsets)
    (section 5e)."""
    man = _manifold(p, manifold)
    if _is_device(p):
        return _summary(p, mean=True, man=man)["mean"]
    pts = _leaf_points(p)
    if man is not None:
        return _circ_mean(pts, man)
    s = np.cumsum(np.concatenate([np.zeros((pts.shape[0], 1)), pts], axis=1), axis=1)[:, -1]
    return s / np.float64(pts.shape[1])


def getKDEfit(p, *, manifold=None):
    """`getKDEfit(p)` (src/DualTree01.jl:576-578) = fit(MvNormal, getPoints(p)): (mu, Sigma) with mu = getKDEMean(p) and
    Sigma = (1/N) sum (x - mu)(x - mu)^T.  `manifold`: the circular mean and wrapped residuals (section 5e)."""
    man = _manifold(p, manifold)
    if _is_device(p):
        r = _summary(p, mean=True, cov=True, man=man)
        return r["mean"], r["cov"]
    mu = getKDEMean(p, manifold=man)
    X = _leaf_points(p) - mu[:, None]
    if man is not None:
        X[man.astype(bool)] = _wrap(X[man.astype(bool)])
    return mu, (X @ X.T) / np.float64(X.shape[1])


def intersIntgAppxIS(p, q, N=201, *, device=0, manifold=None):
    """`intersIntgAppxIS(p, q; N)` (src/DualTree01.jl:581-618), 1-D and 2-D: p and q evaluated by the direct sum on the
    grid over p's marginal ranges with extend 0.3, sum of p q times the cell size (rows in order in 2-D).
    `manifold`: p's circular range, p and q evaluated as `evaluateDualTree(..., manifold=)` (section 5e).
    The exact integral, in any dimension up to 8, is `intersIntg(p, q)` (overlap.py, section 5g)."""
    dev = _same_kind([p, q])
    man = _manifold(p, manifold)
    out = C.c_double(0.0)
    if dev:
        _lib.check(_lib.lib.kdehip_inters_intg_appx_is_device_manifold(p._h, q._h, int(N), C.byref(out), _mf.pointer(man)))
    else:
        _lib.check(_lib.lib.kdehip_inters_intg_appx_is_manifold(C.byref(p._cstruct()), C.byref(q._cstruct()), int(N),
                                                                C.byref(out), int(device), _mf.pointer(man)))
    return float(out.value)


def summary_device_batch(items, stream=None, *, manifold=None):
    """Summaries of many DeviceDensity in ONE call (kdehip_summary_device_batch[_manifold]): `items` = dicts with `density`
    and optionally `extend` (0.1), `Ngrid` (200), `manifold` and the device outputs (torch tensors or addresses, float64)
    `range` (2D, D x 2 column-major), `mean` (D), `cov` (D*D), `argmax` (D), `values` (D*Ngrid).  `manifold=`: one manifold
    for all items or one per item (None = Euclidean), as `mul_device_batch` takes it; an item's own `manifold` wins.
    Euclidean and circular items may be mixed.  Enqueues on `stream` and returns."""
    from .product import DeviceDensity
    items = list(items)
    n = len(items)
    for it in items:
        if not isinstance(it["density"], DeviceDensity):
            raise TypeError("summary_device_batch: items of DeviceDensity")
    mans = None
    if manifold is not None or any("manifold" in it for it in items):   # (a call without any manifold parses none)
        mans = _mf.per_item(items, manifold)
    arr = (_lib.CSummaryManifoldItem * max(1, n))()
    for k, it in enumerate(items):
        a = arr[k]
        a.density = it["density"]._h
        a.extend = float(it.get("extend", 0.1))
        a.Ngrid = int(it.get("Ngrid", 200))
        a.d_range, a.d_mean, a.d_cov = (addr(it.get(x)) for x in ("range", "mean", "cov"))
        a.d_argmax, a.d_values = addr(it.get("argmax")), addr(it.get("values"))
        if mans is not None:
            a.circular_mask = _mf.mask(mans[k])
    _lib.check(_lib.lib.kdehip_summary_device_batch_manifold(n, arr, addr(stream)))


def _marginal_device(p, dims, manifold=None, tree_manifold=None):
    """kdehip_density_marginal_device_tree (DeviceDensity.marginal)."""
    dl = _dims_list(dims, p.dims)
    man = _mf.select(_manifold(p, manifold), dl)
    tman = _mf.select(_manifold(p, tree_manifold, attr="tree_manifold"), dl)
    d = np.array([x + 1 for x in dl], dtype=np.int32)
    h = C.c_void_p()
    _lib.check(_lib.lib.kdehip_density_marginal_device_tree(C.byref(h), p._h, len(dl), ptr(d, i32p), _mf.pointer(tman)))
    return type(p)._built(h, p.device, manifold=man, tree_manifold=tman)
