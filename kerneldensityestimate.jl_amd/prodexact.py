"""The exact product of two densities: `prod_exact`, `product_components`, `log_intersIntg`, `mul_exact` and
`prod_exact_device_batch`, over kdehip_prod_exact[_device] / kdehip_prod_exact_device_batch /
kdehip_product_components[_device] (include/kdehip.h section 5p; kernels in csrc/prodexact.hip).  The library's own: the
reference has the Gibbs samplers only.

For p (points a_i, weights alpha_i, ONE bandwidth vector, variances u) and q (b_j, beta_j, v) the product p q is the mixture

    sum_ij alpha_i beta_j N(a_i - b_j; 0, u + v) N(x; a_i + (b_j - a_i) u / (u + v), u v / (u + v)),

so a draw is a pair of labels (i, j) by two inverse-CDF walks and one Gaussian: no sweeps to converge, no Niter.  The
normaliser log int p q comes out of the same sums in the log domain.  Both arguments are BallTreeDensity (host arrays, run on
`device`) or both DeviceDensity (on their own device); mixing the two is a TypeError.  Euclidean, fp64, two densities per
sweep; a list of more than two is folded through the mixture itself while that stays small.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .density import kde
from .loglik import _dims, _kind

MAX_FOLD_COMPONENTS = 65536  # an intermediate of a fold is a density of that many points at the most


def _npts(d):
    return d.bt.num_points if hasattr(d, "bt") else d.num_points


def _pair(p, q):
    kind = _kind(p, q)
    if _dims(p) != _dims(q):
        raise ValueError("prod_exact -- dimensions of two BallTreeDensities must match")
    return kind, _dims(p)


def _call(p, q, Np, seed, sample_offset, device, draw=True, logz=True):
    """kdehip_prod_exact or kdehip_prod_exact_device: (pts (Np, D) or None, ind (Np, 2) or None, logz or None)"""
    kind, D = _pair(p, q)
    Np = int(Np)
    if kind == "host":
        pts = np.zeros((max(Np, 0), D)) if draw else None
        ind = np.zeros((max(Np, 0), 2), dtype=np.int64) if draw else None
        lz = C.c_double(0.0)
        cp = p._cstruct()
        cq = cp if p is q else q._cstruct()
        _lib.check(_lib.lib.kdehip_prod_exact(C.byref(cp), C.byref(cq), Np, _lib.u64(seed), int(sample_offset),
                                              _lib.optr(pts, _lib.f64p), _lib.optr(ind, _lib.i64p),
                                              C.byref(lz) if logz else None, int(device)))
        return pts, ind, float(lz.value) if logz else None
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        d_pts = torch.zeros((max(1, Np), D), dtype=torch.float64, device=dev) if draw else None
        d_ind = torch.zeros((max(1, Np), 2), dtype=torch.int64, device=dev) if draw else None
        d_lz = torch.zeros(1, dtype=torch.float64, device=dev) if logz else None
        st = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib.kdehip_prod_exact_device(p._h, q._h, Np, _lib.u64(seed), int(sample_offset), _lib.addr(d_pts),
                                                     _lib.addr(d_ind), _lib.addr(d_lz), _lib.addr(st.cuda_stream)))
        st.synchronize()
        return (d_pts.cpu().numpy()[:Np].copy() if draw else None, d_ind.cpu().numpy()[:Np].copy() if draw else None,
                float(d_lz.cpu().numpy()[0]) if logz else None)


def product_components(p, q, *, device=0):
    """(means (D, N1 N2), weights (N1 N2,), sd (D,)): the mixture p q itself in ORIGINAL point order -- component
    c = i N2 + j (0-based) is the pair of p's point i and q's point j, its weight normalised (they sum to 1), sd the
    standard deviation sqrt(u v / (u + v)) every component shares: `kde(means, sd, weights)` is the product as a density.
    More than 2^20 components are refused (KDEHIP_ERR_UNSUPPORTED)."""
    kind, D = _pair(p, q)
    NC = _npts(p) * _npts(q)
    if kind == "host":
        means, w, var = np.zeros((NC, D)), np.zeros(NC), np.zeros(D)
        cp = p._cstruct()
        cq = cp if p is q else q._cstruct()
        _lib.check(_lib.lib.kdehip_product_components(C.byref(cp), C.byref(cq), _lib.ptr(means, _lib.f64p),
                                                      _lib.ptr(w, _lib.f64p), _lib.ptr(var, _lib.f64p), int(device)))
    else:
        if NC > 2 ** 20:  # (before the result is allocated; the library says the same)
            raise _lib.KdeHipError(_lib.ERR_UNSUPPORTED, "product_components: more than 2^20 components")
        import torch
        dev = torch.device("cuda", p.device)
        with torch.cuda.device(dev):
            d_means = torch.zeros((NC, D), dtype=torch.float64, device=dev)
            d_w = torch.zeros(NC, dtype=torch.float64, device=dev)
            d_var = torch.zeros(D, dtype=torch.float64, device=dev)
            st = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib.kdehip_product_components_device(p._h, q._h, _lib.addr(d_means), _lib.addr(d_w),
                                                                 _lib.addr(d_var), _lib.addr(st.cuda_stream)))
            st.synchronize()
            means, w, var = d_means.cpu().numpy(), d_w.cpu().numpy(), d_var.cpu().numpy()
    return np.ascontiguousarray(means.T), w, np.sqrt(var)


def log_intersIntg(p, q, *, device=0) -> float:
    """log of the exact integral of p q (= log intersIntg(p, q)), by log-sum-exp: finite where intersIntg underflows to 0;
    -inf only where one of the two has no point of positive weight."""
    return _call(p, q, 0, 0, 0, device, draw=False)[2]


def _fold(trees, Np, seed, sample_offset, device, return_logz):
    """p q r ... = ((p q) r) ...: every intermediate is `kde(*product_components)` of the two before it"""
    from .product import DeviceDensity
    resident = isinstance(trees[0], DeviceDensity)
    sizes = [_npts(t) for t in trees]
    acc, n_acc, made = trees[0], sizes[0], []
    try:
        for t, n in zip(trees[1:-1], sizes[1:-1]):
            if n_acc * n > MAX_FOLD_COMPONENTS:
                raise ValueError(f"prod_exact: an intermediate of the fold would have {n_acc * n} components (more than "
                                 f"{MAX_FOLD_COMPONENTS}); use prodAppxMSGibbsS for this product")
            means, w, sd = product_components(acc, t, device=device)
            host = kde(means, sd, w)
            acc = DeviceDensity(host, acc.device) if resident else host
            if resident:
                made.append(acc)
            n_acc *= n
        pts, ind, lz = _call(acc, trees[-1], Np, seed, sample_offset, device, logz=return_logz)
    finally:
        for d in made:
            d.close()
    # the first label is a component of the fold so far: c = (((i_0 n_1 + i_1) n_2 + i_2) ...), 0-based
    out = np.zeros((len(trees), ind.shape[0]), dtype=np.int64)
    out[-1] = ind[:, 1]
    c = ind[:, 0] - 1
    valid = ind[:, 0] > 0
    for m in range(len(trees) - 2, 0, -1):
        out[m] = np.where(valid, c % sizes[m] + 1, 0)
        c = c // sizes[m]
    out[0] = np.where(valid, c + 1, 0)
    return pts, out, lz


def prod_exact(p, q=None, Np=None, *, seed=None, sample_offset=0, device=0, return_logz=False):
    """(pts (D, Np), ind (2, Np)) -- with return_logz also log int p q --: Np exact draws of the product p q.  ind[0] / ind[1]
    are the 1-based original indices of the drawn kernels of p / q, pts the component's mean plus its noise.  Draw t uses the
    Philox numbers of index sample_offset + t (two uniforms, D normals), so a call with an offset continues an earlier one.
    Np defaults to Npts(p); seed=None draws one from the operating system.
    `prod_exact([p, q, r, ...])` folds left through `product_components` and `kde` while every intermediate has at most
    65,536 components (otherwise ValueError: use prodAppxMSGibbsS); ind is then (M, Np), one original index per input."""
    if isinstance(p, (list, tuple)):
        trees = list(p)
        if q is not None and Np is None:
            Np = q  # prod_exact([p, q, r], Np)
        elif q is not None:
            raise TypeError("prod_exact: a list of densities, then Np")
        if len(trees) < 2:
            raise ValueError("prod_exact: a product has at least two densities")
        for t in trees[1:]:
            _pair(trees[0], t)
    else:
        if q is None:
            raise TypeError("prod_exact: two densities, or a list of them")
        trees = [p, q]
        _pair(p, q)
    if Np is None:
        Np = _npts(trees[0])
    if seed is None:
        seed = _lib.random_seed()
    if len(trees) == 2:
        pts, ind, lz = _call(trees[0], trees[1], Np, seed, sample_offset, device, logz=return_logz)
        ind = np.ascontiguousarray(ind.T)
    else:
        pts, ind, lz = _fold(trees, Np, seed, sample_offset, device, return_logz)
    pts = np.ascontiguousarray(pts.T)
    return (pts, ind, lz) if return_logz else (pts, ind)


def prod_exact_device_batch(items, stream=None):
    """Many exact products of DeviceDensity pairs in ONE call (kdehip_prod_exact_device_batch): `items` = dicts with `p`, `q`,
    `Np` and any of `pts` (float64, Np rows of D) with `ind` (int64, Np rows of 2) and `logz` (float64, 1); optionally `seed`
    and `sample_offset`.  Items may mix D, sizes and Np.  Enqueue only on `stream`; every item's results are bit for bit those
    of the single call."""
    from .product import DeviceDensity
    items = list(items)
    n = len(items)
    arr = (_lib.CProdExactItem * max(1, n))()
    for k, it in enumerate(items):
        p, q = it["p"], it["q"]
        if not (isinstance(p, DeviceDensity) and isinstance(q, DeviceDensity)):
            raise TypeError("prod_exact_device_batch: items of DeviceDensity")
        Np = int(it["Np"])
        for name, per in (("pts", p.dims), ("ind", 2), ("logz", 0)):
            if it.get(name) is not None and int(it[name].numel()) < max(Np * per, 1 if per == 0 else 0):
                raise ValueError(f"prod_exact_device_batch: {name} is too small")
        a = arr[k]
        a.p, a.q, a.Np = p._h, q._h, Np
        a.seed, a.sample_offset = int(it.get("seed", 0)) & _lib.SEED_MASK, int(it.get("sample_offset", 0))
        a.d_pts, a.d_ind, a.d_logz = (_lib.addr(it.get(x)) for x in ("pts", "ind", "logz"))
    _lib.check(_lib.lib.kdehip_prod_exact_device_batch(n, arr, _lib.addr(stream)))


def mul_exact(p, q, Np=None, seed=None):
    """The exact `*` of two DeviceDensity: Np draws of `prod_exact` (None = Npts(p)) into HBM, then `kde!(pGM)` of that
    matrix by `DeviceDensity.from_device_points` (the LOOCV bandwidth search) -- nothing leaves the device.  Returns a
    DeviceDensity whose points are the draws of `prod_exact(p, q, Np, seed=seed)`.  `__mul__` and `mul_device` stay the
    samplers'."""
    from .product import DeviceDensity
    if not (isinstance(p, DeviceDensity) and isinstance(q, DeviceDensity)):
        raise TypeError("mul_exact: two DeviceDensity")
    _pair(p, q)
    Np = p.num_points if Np is None else int(Np)
    if seed is None:
        seed = _lib.random_seed()
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        d_pts = torch.zeros((Np, p.dims), dtype=torch.float64, device=dev)  # row t = draw t: D x Np column-major
        d_ind = torch.zeros((Np, 2), dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev)
        p.prod_exact(q, d_pts, d_ind, Np=Np, seed=seed, stream=st.cuda_stream)
        return DeviceDensity.from_device_points(d_pts, p.dims, Np, device=p.device, stream=st.cuda_stream)
