"""A density conditioned on some of its dimensions: `condition`, `conditional_weights`, `conditional_moments`,
`sample_conditional` and `conditional_device_batch`, over kdehip_conditional[_device] / kdehip_conditional_device_batch /
kdehip_condition_weights[_device] / kdehip_density_condition_device (include/kdehip.h section 5i; kernels in
csrc/conditional.hip).  The library's own: the reference has `marginal`, which drops dimensions; these fix them.

For a joint Gaussian-kernel density with one bandwidth vector v, the given dimensions G, the free ones F and a query y,

    a_i = -1/2 sum_{k in G} (y_k - c_ik)^2 / v_k,   omega_i = w_i e^{a_i} / sum_j w_j e^{a_j},
    p(x_F | x_G = y) = sum_i omega_i N(x_F; c_iF, v_F),   logz = log p_G(y)

-- `condition` returns that mixture as a density, `conditional_weights` the omega, `conditional_moments` its mean and
per-dimension variance, `sample_conditional` ONE draw of it per query (the message step of nonparametric belief propagation:
push each sample of x_G through p(x_F | x_G)).  `dims` are 0-based, distinct and in any order; the rows of `Y` follow `dims`
as given.  The density is a BallTreeDensity (host arrays, run on `device`) or a DeviceDensity (on its own device);
`manifold=` as the other entries take it, "inherit" included.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .density import getBW, kde
from .loglik import _dims
from .modes import _kind
from .summary import _leaf_points


def _given(dims, D):
    """(the dims as given, the order that sorts them, the mask, F ascending)"""
    dl = [dims] if np.isscalar(dims) else list(dims)
    for d in dl:
        if int(d) != d or not 0 <= int(d) < D:
            raise ValueError(f"condition: dims must be integers in 0..{D - 1}")
    dl = [int(d) for d in dl]
    if len(set(dl)) != len(dl):
        raise ValueError("condition: dims must be distinct")
    if D < 2:
        raise ValueError("condition: a 1-D density has no dimension left to condition on")
    if not 1 <= len(dl) <= D - 1:
        raise ValueError("condition: between 1 and ndims - 1 dimensions can be given")
    order = np.argsort(dl)
    free = [k for k in range(D) if k not in dl]
    return dl, order, sum(1 << d for d in dl), free


def _queries(Y, ng, order):
    """`Y` (ng, Nq) -- a vector is ONE query of ng values, or Nq queries when ng == 1 -- as Nq rows in the order of G"""
    if hasattr(Y, "data_ptr"):
        Y = Y.detach().cpu().numpy()
    A = np.asarray(Y, dtype=np.float64)
    if A.ndim == 0:
        A = A.reshape(1, 1)
    elif A.ndim == 1:
        A = A.reshape(1, -1) if ng == 1 else A.reshape(-1, 1)
    if A.ndim != 2 or A.shape[0] != ng:
        raise ValueError("condition: one value per given dimension and query")
    return np.ascontiguousarray(A[order, :].T)


def _call(p, dims, Y, *, logz=False, moments=False, draw=False, seed=0, sample_offset=0, device=0, manifold=None):
    """kdehip_conditional or kdehip_conditional_device: a dict of the numpy results that were asked for"""
    kind, D = _kind(p), _dims(p)
    dl, order, gmask, free = _given(dims, D)
    man = _mf.resolve(p, manifold, D)
    flat = _queries(Y, len(dl), order)
    Nq, nf = flat.shape[0], len(free)
    if kind == "host":
        bufs = {"logz": np.zeros(Nq) if logz else None,
                "mean": np.zeros((Nq, nf)) if moments else None, "var": np.zeros((Nq, nf)) if moments else None,
                "pts": np.zeros((Nq, nf)) if draw else None}
        ind = np.zeros(Nq, dtype=np.int64) if draw else None
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_conditional(C.byref(cd), gmask, _lib.ptr(flat, _lib.f64p), Nq, _lib.u64(seed),
                                               int(sample_offset), *[_lib.optr(bufs[k], _lib.f64p) for k in ("logz", "mean", "var", "pts")],
                                               _lib.optr(ind, _lib.i64p), int(device), _mf.pointer(man)))
        bufs["ind"] = ind
        return bufs
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        d_y = torch.from_numpy(flat).to(dev)
        bufs = {"logz": torch.zeros(max(1, Nq), **f64) if logz else None,
                "mean": torch.zeros((max(1, Nq), nf), **f64) if moments else None,
                "var": torch.zeros((max(1, Nq), nf), **f64) if moments else None,
                "pts": torch.zeros((max(1, Nq), nf), **f64) if draw else None,
                "ind": torch.zeros(max(1, Nq), dtype=torch.int64, device=dev) if draw else None}
        st = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib.kdehip_conditional_device(p._h, gmask, _lib.addr(d_y), Nq, _lib.u64(seed), int(sample_offset),
                                                      *[_lib.addr(bufs[k]) for k in ("logz", "mean", "var", "pts", "ind")],
                                                      _mf.pointer(man), _lib.addr(st.cuda_stream)))
        st.synchronize()
        return {k: None if v is None else v.cpu().numpy()[:Nq].copy() for k, v in bufs.items()}


def conditional_moments(p, dims, Y, *, device=0, manifold=None):
    """(logz (Nq,), mean (nf, Nq), var (nf, Nq)) of p(x_F | x_dims = Y[:, q]): logz = the log of the marginal over `dims` at
    the query, finite far beyond where that marginal underflows; var is the diagonal of the conditional covariance and never
    below the bandwidth.  var is accurate to an absolute error proportional to the squared range of the data in that
    dimension (section 5i).  A circular FREE dimension is refused (KDEHIP_ERR_UNSUPPORTED); circular given ones wrap."""
    r = _call(p, dims, Y, logz=True, moments=True, device=device, manifold=manifold)
    return r["logz"], np.ascontiguousarray(r["mean"].T), np.ascontiguousarray(r["var"].T)


def sample_conditional(p, dims, Y, seed=0, sample_offset=0, *, device=0, manifold=None):
    """(pts (nf, Nq), ind (Nq,)): ONE draw of p(x_F | x_dims = Y[:, q]) per query -- ind the 1-based original index of the
    drawn kernel, pts its centre in F plus bandwidth noise.  Query q uses the Philox numbers `sample` uses for index
    sample_offset + q, so two half calls with offsets continue one stream.  Where no point has a positive weight: NaN, 0."""
    r = _call(p, dims, Y, draw=True, seed=seed, sample_offset=sample_offset, device=device, manifold=manifold)
    return np.ascontiguousarray(r["pts"].T), r["ind"]


def conditional_weights(p, dims, Y, *, device=0, manifold=None):
    """(W (Nq, N), logz (Nq,)): W[q, o] = the weight omega of ORIGINAL point o in p(x_F | x_dims = Y[:, q]) -- what
    `kde(points[F], ks[F], W[q])` takes; every row sums to 1 and a point of weight 0 keeps exactly 0."""
    kind, D = _kind(p), _dims(p)
    dl, order, gmask, _ = _given(dims, D)
    man = _mf.resolve(p, manifold, D)
    flat = _queries(Y, len(dl), order)
    Nq = flat.shape[0]
    if kind == "host":
        N = p.bt.num_points
        W, logz = np.zeros((Nq, N)), np.zeros(Nq)
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_condition_weights(C.byref(cd), gmask, _lib.ptr(flat, _lib.f64p), Nq, _lib.ptr(W, _lib.f64p),
                                                     _lib.ptr(logz, _lib.f64p), int(device), _mf.pointer(man)))
        return W, logz
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        N = p.num_points
        d_y = torch.from_numpy(flat).to(dev)
        W = torch.zeros((max(1, Nq), N), dtype=torch.float64, device=dev)
        logz = torch.zeros(max(1, Nq), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib.kdehip_condition_weights_device(p._h, gmask, _lib.addr(d_y), Nq, _lib.addr(W), _lib.addr(logz),
                                                            _mf.pointer(man), _lib.addr(st.cuda_stream)))
        st.synchronize()
        return W.cpu().numpy()[:Nq].copy(), logz.cpu().numpy()[:Nq].copy()


def condition(p, dims, values, *, device=0, manifold=None, tree_manifold=None):
    """p(x_F | x_dims = values) as a density over the other dimensions F (ascending): the points' coordinates in F, the
    bandwidth of ORIGINAL point 0 in F (marginal's rule) and the weights omega.  A BallTreeDensity gives a BallTreeDensity
    (`kde(points[F], getBW(p)[F, 0], omega)`, omega from kdehip_condition_weights), a DeviceDensity a DeviceDensity
    (kdehip_density_condition_device): the same arrays.  `manifold` (one entry per dimension of p, or "inherit"): circular
    given dimensions wrap their differences; `tree_manifold` (likewise): the result's tree is built with tree_manifold[F];
    the result remembers manifold[F] and tree_manifold[F].  A `values` at which no point has a positive weight is an error."""
    kind, D = _kind(p), _dims(p)
    dl, order, gmask, free = _given(dims, D)
    man = _mf.resolve(p, manifold, D)
    tman = _mf.select(_mf.resolve(p, tree_manifold, D, attr="tree_manifold"), free)
    y = _queries(np.asarray(values, dtype=np.float64).reshape(-1, 1), len(dl), order)
    if y.shape[0] != 1:
        raise ValueError("condition: one value per given dimension")
    if kind == "device":
        h = C.c_void_p()
        _lib.check(_lib.lib.kdehip_density_condition_device(C.byref(h), p._h, gmask, _lib.ptr(y, _lib.f64p), _mf.pointer(man),
                                                            _mf.pointer(tman)))
        return type(p)._built(h, p.device, manifold=_mf.select(man, free), tree_manifold=tman)
    W, logz = conditional_weights(p, dl, np.asarray(values, dtype=np.float64).reshape(-1, 1), device=device, manifold=man)
    if not logz[0] > -np.inf:
        raise _lib.KdeHipError(_lib.ERR_ARG, "condition: no point of the density has a positive weight at y (logz = -Inf), or y holds a NaN")
    return kde(_leaf_points(p)[free, :], getBW(p)[free, 0], W[0], tree_manifold=tman)


def conditional_device_batch(items, stream=None):
    """Many conditionals of DeviceDensity items in ONE call (kdehip_conditional_device_batch): `items` = dicts with
    `density`, `dims`, `given` (a float64 device tensor of Nq rows of ng values, the columns in ASCENDING order of the given
    dimensions) and any of `logz` (float64, Nq), `mean`, `var` (float64, Nq rows of nf), `pts` (float64, Nq rows of nf) with
    `ind` (int64, Nq); optionally `seed`, `sample_offset` and `manifold`.  Enqueue only on `stream`; every item's results are
    bit for bit those of the single call."""
    from .product import DeviceDensity
    items = list(items)
    n = len(items)
    arr = (_lib.CConditionalItem * max(1, n))()
    for k, it in enumerate(items):
        d = it["density"]
        if not isinstance(d, DeviceDensity):
            raise TypeError("conditional_device_batch: items of DeviceDensity")
        dl, _, gmask, free = _given(it["dims"], d.dims)
        g = it["given"]
        if g.dim() != 2 or int(g.shape[1]) != len(dl) or not g.is_contiguous():
            raise ValueError("conditional_device_batch: given is Nq contiguous rows of ng values")
        Nq, nf = int(g.shape[0]), len(free)
        for name, per in (("logz", 1), ("mean", nf), ("var", nf), ("pts", nf), ("ind", 1)):
            if it.get(name) is not None and int(it[name].numel()) < Nq * per:
                raise ValueError(f"conditional_device_batch: {name} is too small")
        a = arr[k]
        a.bd, a.d_given, a.Nq = d._h, _lib.addr(g), Nq
        a.seed, a.sample_offset = int(it.get("seed", 0)) & _lib.SEED_MASK, int(it.get("sample_offset", 0))
        a.d_logz, a.d_mean, a.d_var = (_lib.addr(it.get(x)) for x in ("logz", "mean", "var"))
        a.d_pts, a.d_ind = _lib.addr(it.get("pts")), _lib.addr(it.get("ind"))
        a.given_mask = gmask
        a.circular_mask = _mf.mask(_mf.resolve(d, it.get("manifold"), d.dims))
    _lib.check(_lib.lib.kdehip_conditional_device_batch(n, arr, _lib.addr(stream)))
