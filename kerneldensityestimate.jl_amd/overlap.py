"""Exact overlap measures of two densities by kernel sums: `kernel_sum`, `intersIntg`, `ise`, `mmd` and their batches, over
kdehip_kernel_sum / kdehip_kernel_sum_device / kdehip_kernel_sum_device_batch (include/kdehip.h section 5g; kernels in
csrc/ksum.hip).  The library's own: the reference has `intersIntgAppxIS`, a grid sum in 1-D and 2-D.

All of them are compositions of ONE primitive,

    S(a, b; v) = sum_j b_j sum_i a_i exp(-1/2 sum_k diff_k(y_jk, x_ik)^2 / v_k)

over the leaf points and weights of `a` and `b`, in any dimension up to 8, at the cost of one all-pairs pass.  The full square
is summed -- no leave-one-out, whatever the identity of the arguments --, so `ise(p, p)` and `mmd(p, p, bw)` are exactly 0.
Both arguments are BallTreeDensity (host arrays, run on `device`) or both DeviceDensity (on their own device); mixing the
two is a TypeError.  `manifold=` as the other entries take it, "inherit" (the first density's record) included: a circular
dimension wraps its differences and keeps the Gaussian constant, as evaluation does.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .loglik import _dims, _kind


def _variances(var, D, what="var"):
    """None, or the D variances as a float64 array (one entry is repeated over the dimensions)"""
    if var is None:
        return None
    v = np.atleast_1d(np.asarray(var, dtype=np.float64)).ravel()
    if v.size not in (1, D):
        raise ValueError(f"{what} must have 1 or D entries")
    return np.ascontiguousarray(np.repeat(v, D) if v.size == 1 and D > 1 else v)


def _bw_variances(bw, D):
    """a bandwidth as `kde` takes `ks` (standard deviation, 1 or D entries), squared as `kde` squares it (sd * sd)"""
    if bw is None:
        raise TypeError("mmd: bw (the kernel's standard deviation) is required")
    sd = _variances(bw, D, "bw")
    return sd * sd


def _pair(a, b):
    kind = _kind(a, b)
    if _dims(a) != _dims(b):
        raise ValueError("kernel sum -- dimensions of two BallTreeDensities must match")
    return kind, _dims(a)


def kernel_sum(a, b, var=None, *, normalize=False, device=0, manifold=None) -> float:
    """S(a, b; var) (section 5g).  `var`: D variances (or one for all dimensions), or None = the sum of the two densities'
    leaf variances (they must not be per-point then).  `normalize`: divided by prod_k sqrt(2 pi var_k)."""
    kind, D = _pair(a, b)
    v = _variances(var, D)
    man = _mf.resolve(a, manifold, D)
    out = C.c_double(0.0)
    vp = _lib.optr(v, _lib.f64p)
    if kind == "host":
        ca = a._cstruct()
        cb = ca if a is b else b._cstruct()
        _lib.check(_lib.lib.kdehip_kernel_sum(C.byref(ca), C.byref(cb), vp, int(bool(normalize)), C.byref(out), int(device),
                                              _mf.pointer(man)))
    else:
        _lib.check(_lib.lib.kdehip_kernel_sum_device(a._h, b._h, vp, int(bool(normalize)), C.byref(out), _mf.pointer(man)))
    return float(out.value)


def intersIntg(p, q, *, device=0, manifold=None) -> float:
    """The exact integral of p q: kernel_sum(p, q, None, normalize=True), each pair of kernels a normal density of the
    difference of their centres with the summed variances.  What `intersIntgAppxIS` approximates, in any D <= 8."""
    return kernel_sum(p, q, None, normalize=True, device=device, manifold=manifold)


def _combine(pp, pq, qq):
    return pp - 2.0 * pq + qq


def ise(p, q, *, device=0, manifold=None) -> float:
    """The integrated squared error, integral of (p - q)^2 = intersIntg(p, p) - 2 intersIntg(p, q) + intersIntg(q, q):
    symmetric, and 0 for p == q."""
    _pair(p, q)
    kw = dict(device=device, manifold=manifold)
    return _combine(intersIntg(p, p, **kw), intersIntg(p, q, **kw), intersIntg(q, q, **kw))


def mmd(p, q, bw, *, device=0, manifold=None) -> float:
    """The biased squared maximum mean discrepancy under the Gaussian kernel of standard deviation `bw` (1 or D entries, as
    `kde`'s ks): S(p, p; bw^2) - 2 S(p, q; bw^2) + S(q, q; bw^2), not normalised."""
    _, D = _pair(p, q)
    v = _bw_variances(bw, D)
    kw = dict(device=device, manifold=manifold)
    return _combine(kernel_sum(p, p, v, **kw), kernel_sum(p, q, v, **kw), kernel_sum(q, q, v, **kw))


def kernel_sum_device_batch(items, d_out, stream=None):
    """S of many DeviceDensity pairs in ONE call (kdehip_kernel_sum_device_batch): `items` = dicts with `a`, `b` and
    optionally `var` (None), `normalize` (False) and `manifold` (None, a per-dimension sequence or "inherit"); d_out[i] (a
    float64 device tensor or the address of len(items) doubles) = item i's sum, bit for bit `kernel_sum`'s.  Items of any
    dimension count, Euclidean and circular, may be mixed.  Enqueues on `stream` and returns."""
    from .product import DeviceDensity
    items = list(items)
    n = len(items)
    arr = (_lib.CKsumItem * max(1, n))()
    keep = []  # the variances live until the call has copied them
    for k, it in enumerate(items):
        a, b = it["a"], it["b"]
        if not (isinstance(a, DeviceDensity) and isinstance(b, DeviceDensity)):
            raise TypeError("kernel_sum_device_batch: items of DeviceDensity")
        if a.dims != b.dims:
            raise ValueError("kernel sum -- dimensions of two BallTreeDensities must match")
        v = _variances(it.get("var"), a.dims)
        keep.append(v)
        arr[k].a, arr[k].b, arr[k].var = a._h, b._h, _lib.optr(v, _lib.f64p)
        arr[k].circular_mask = _mf.mask(_mf.resolve(a, it.get("manifold"), a.dims))
        arr[k].normalize = int(bool(it.get("normalize", False)))
    _lib.check(_lib.lib.kdehip_kernel_sum_device_batch(n, arr, _lib.addr(d_out), _lib.addr(stream)))


def _three_term_batch(name, pairs, var_of, normalize, manifold, manifolds):
    """term(p, p) - 2 term(p, q) + term(q, q) for many DeviceDensity pairs: ONE batch call, one synchronisation; an identical
    (a, b, var, manifold) item is sent once"""
    from .product import DeviceDensity
    pairs = [(p, q) for p, q in pairs]
    n = len(pairs)
    if n == 0:
        return np.zeros(0)
    if manifold is not None and manifolds is not None:
        raise ValueError(f"{name}: manifold= (one for all pairs) or manifolds= (one per pair), not both")
    if manifolds is not None and len(manifolds) != n:
        raise ValueError(f"{name}: one manifold per pair")
    per = [manifold] * n if manifolds is None else list(manifolds)
    items, index, slots = [], {}, []
    for (p, q), m in zip(pairs, per):
        if not (isinstance(p, DeviceDensity) and isinstance(q, DeviceDensity)):
            raise TypeError(f"{name}: pairs of DeviceDensity")
        if p.dims != q.dims:
            raise ValueError("kernel sum -- dimensions of two BallTreeDensities must match")
        v = var_of(p.dims)
        man = _mf.resolve(p, m, p.dims)
        tail = (None if v is None else v.tobytes(), _mf.mask(man))
        row = []
        for a, b in ((p, p), (p, q), (q, q)):
            key = (id(a), id(b)) + tail
            if key not in index:
                index[key] = len(items)
                items.append(dict(a=a, b=b, var=v, normalize=normalize, manifold=man))
            row.append(index[key])
        slots.append(row)
    import torch
    dev = torch.device("cuda", pairs[0][0].device)
    out = torch.empty(len(items), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        kernel_sum_device_batch(items, out, stream=st.cuda_stream)
        st.synchronize()
    v = out.cpu().numpy()
    s = np.asarray(slots)
    return _combine(v[s[:, 0]], v[s[:, 1]], v[s[:, 2]])


def ise_batch(pairs, manifold=None, manifolds=None):
    """ise(p_i, q_i) for many DeviceDensity pairs in ONE batch call and one synchronisation; a numpy array of n values, each
    bit for bit `ise(p_i, q_i)`.  `manifold`: one for all pairs; `manifolds`: one (or None) per pair."""
    return _three_term_batch("ise_batch", pairs, lambda D: None, True, manifold, manifolds)


def mmd_batch(pairs, bw, manifold=None, manifolds=None):
    """mmd(p_i, q_i, bw) likewise."""
    if bw is None:
        raise TypeError("mmd_batch: bw (the kernel's standard deviation) is required")
    return _three_term_batch("mmd_batch", pairs, lambda D: _bw_variances(bw, D), False, manifold, manifolds)
