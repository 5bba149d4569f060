"""Log-likelihoods of one density at another's points: `evalAvgLogL`, `entropy`, `kld`, `minkld` (reference
src/DualTree01.jl:450-510), and evaluation of resident densities, over kdehip_eval_avg_logl / kdehip_eval_avg_logl_device /
kdehip_eval_avg_logl_device_batch / kdehip_evaluate_device / kdehip_evaluate_device_at (include/kdehip.h section 5b;
kernels in csrc/evaluate.hip).

Leave-one-out is decided by identity, as in the reference (`bd == locations` on a mutable struct, :333): evalAvgLogL(p, p)
skips the self terms, evalAvgLogL(p, copy_of_p) does not -- so kld(p, p) is not 0.  Both arguments are BallTreeDensity
(host arrays, evaluated on `device`) or both DeviceDensity (on their own device); mixing the two is a TypeError.

`log_domain=True` (include/kdehip.h section 5f) forms every log p by log-sum-exp in the kernel: where the default returns
-inf because a p underflowed to 0, the result stays finite and ordered.  The default is the reference's arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .density import BallTreeDensity


def _kind(bd1, bd2):
    from .product import DeviceDensity
    if isinstance(bd1, BallTreeDensity) and isinstance(bd2, BallTreeDensity):
        return "host"
    if isinstance(bd1, DeviceDensity) and isinstance(bd2, DeviceDensity):
        return "device"
    raise TypeError("both densities must be BallTreeDensity, or both DeviceDensity")


def _dims(d):
    return d.bt.dims if isinstance(d, BallTreeDensity) else d.dims


def _mask(man):
    return 0 if man is None else int(sum(int(v) << k for k, v in enumerate(man)))


def evalAvgLogL(bd1, bd2, *, device=0, manifold=None, log_domain=False) -> float:
    """`evalAvgLogL(bd1, bd2)` (src/DualTree01.jl:450-470): sum over bd2's points of W log L, L = bd1 at those points
    (leave-one-out when `bd1 is bd2`), W = bd2's weights; -inf when an L == 0 carries weight.  `log_domain=True`: the sum
    over W != 0 of W log p with log p by log-sum-exp (section 5f), finite wherever bd1 has a weighted point.
    A bd1 with per-point bandwidths (multibandwidth == 1; a DeviceDensity whose leaves do not share one vector) is
    evaluated by the entries of section 5o; bd2 contributes points and weights only."""
    kind = _kind(bd1, bd2)
    if _dims(bd1) != _dims(bd2):
        raise ValueError("evaluate -- dimensions of two BallTreeDensities must match")
    out = C.c_double(0.0)
    loo = 1 if bd1 is bd2 else 0
    man = _mf.parse(manifold, _dims(bd1))  # (circular differences in those dimensions: include/kdehip.h section 5d)
    mp = _mf.pointer(man)
    if kind == "host":
        c1 = bd1._cstruct()
        c2 = c1 if loo else bd2._cstruct()
        if bd1.multibandwidth == 1:  # per-point bandwidths (section 5o)
            _lib.check(_lib.lib.kdehip_eval_avg_logl_varbw(C.byref(c1), C.byref(c2), loo, int(bool(log_domain)), C.byref(out),
                                                           int(device), mp))
            return float(out.value)
        fn = _lib.lib.kdehip_eval_avg_logl_log if log_domain else _lib.lib.kdehip_eval_avg_logl_manifold
        _lib.check(fn(C.byref(c1), C.byref(c2), loo, C.byref(out), int(device), mp))
    elif bd1._h and not _lib.lib.kdehip_density_uniform_bandwidth(bd1._h):
        import torch
        dev = torch.device("cuda", bd1.device)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            d_out = torch.empty(1, dtype=torch.float64, device=dev)
            _lib.check(_lib.lib.kdehip_eval_avg_logl_varbw_device(bd1._h, bd2._h, loo, int(bool(log_domain)), _lib.addr(d_out),
                                                                  _lib.addr(st.cuda_stream), mp))
            st.synchronize()
            return float(d_out.cpu()[0])
    else:
        fn = _lib.lib.kdehip_eval_avg_logl_log_device if log_domain else _lib.lib.kdehip_eval_avg_logl_device_manifold
        _lib.check(fn(bd1._h, bd2._h, loo, C.byref(out), mp))
    return float(out.value)


def entropy(bd, *, device=0, manifold=None, log_domain=False) -> float:
    """`entropy(bd)` (src/DualTree01.jl:505-508) = -evalAvgLogL(bd, bd)."""
    return -evalAvgLogL(bd, bd, device=device, manifold=manifold, log_domain=log_domain)


def kld(p1, p2, method="direct", *, device=0, manifold=None, log_domain=False) -> float:
    """`kld(p1, p2; method=:direct)` (src/DualTree01.jl:477-503) = evalAvgLogL(p1, p1) - evalAvgLogL(p2, p1)."""
    if method != "direct":
        raise ValueError(f"kld: method {method!r} is not supported (only 'direct'; the reference's 'unscented' builds "
                         "overlapping sigma-point blocks)")
    _kind(p1, p2)
    if _dims(p1) != _dims(p2):
        raise ValueError("evaluate -- dimensions of two BallTreeDensities must match")
    kw = dict(device=device, manifold=manifold, log_domain=log_domain)
    return evalAvgLogL(p1, p1, **kw) - evalAvgLogL(p2, p1, **kw)


def minkld(p, q, *, device=0, manifold=None, log_domain=False) -> float:
    """`minkld(p, q)` (src/DualTree01.jl:510) = min(|kld(p, q)|, |kld(q, p)|)."""
    kw = dict(device=device, manifold=manifold, log_domain=log_domain)
    return min(abs(kld(p, q, **kw)), abs(kld(q, p, **kw)))


def eval_avg_logl_device_batch(pairs, d_out, stream=None, manifolds=None, log_domain=False):
    """evalAvgLogL of many (bd, at) DeviceDensity pairs in ONE call (kdehip_eval_avg_logl_device_batch): d_out[i] (a
    float64 device tensor or address of len(pairs) doubles) = evalAvgLogL(bd_i, at_i), leave-one-out where `bd_i is
    at_i`.  `manifolds`: None, or one manifold (or None) per pair.  `log_domain=True`: every item in the log domain
    (kdehip_eval_avg_logl_log_device_batch).  Enqueues on `stream` and returns."""
    from .product import DeviceDensity
    pairs = list(pairs)
    n = len(pairs)
    if manifolds is not None and len(manifolds) != n:
        raise ValueError("eval_avg_logl_device_batch: one manifold per pair")
    arr = (_lib.CLoglManifoldItem * max(1, n))()
    for k, (bd, at) in enumerate(pairs):
        if not (isinstance(bd, DeviceDensity) and isinstance(at, DeviceDensity)):
            raise TypeError("eval_avg_logl_device_batch: pairs of DeviceDensity")
        arr[k].bd, arr[k].at, arr[k].leave_one_out = bd._h, at._h, 1 if bd is at else 0
        arr[k].circular_mask = 0 if manifolds is None else _mask(_mf.parse(manifolds[k], bd.dims))
    fn = _lib.lib.kdehip_eval_avg_logl_log_device_batch if log_domain else _lib.lib.kdehip_eval_avg_logl_device_batch_manifold
    _lib.check(fn(n, arr, _lib.addr(d_out), _lib.addr(stream)))


def kld_batch(pairs, manifold=None, manifolds=None, log_domain=False):
    """kld(p_i, q_i) for many DeviceDensity pairs: ONE batch call of 2n items (evalAvgLogL(p, p), evalAvgLogL(q, p) per
    pair), one synchronisation; returns a numpy array of n values, each bit for bit `kld(p_i, q_i)`.  `manifold`: one for
    all pairs; `manifolds`: one (or None) per pair; `log_domain` as in `kld`."""
    from .product import DeviceDensity
    pairs = [(p, q) for p, q in pairs]
    n = len(pairs)
    if n == 0:
        return np.zeros(0)
    for p, q in pairs:
        if not (isinstance(p, DeviceDensity) and isinstance(q, DeviceDensity)):
            raise TypeError("kld_batch: pairs of DeviceDensity")
        if p.dims != q.dims:
            raise ValueError("evaluate -- dimensions of two BallTreeDensities must match")
    import torch
    dev = torch.device("cuda", pairs[0][0].device)
    if manifold is not None and manifolds is not None:
        raise ValueError("kld_batch: manifold= (one for all pairs) or manifolds= (one per pair), not both")
    if manifolds is not None and len(manifolds) != n:
        raise ValueError("kld_batch: one manifold per pair")
    per = [manifold] * n if manifolds is None else list(manifolds)
    items, mans = [], []
    for (p, q), m in zip(pairs, per):
        items += [(p, p), (q, p)]
        mans += [m, m]
    out = torch.empty(2 * n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        eval_avg_logl_device_batch(items, out, stream=st.cuda_stream, manifolds=mans, log_domain=log_domain)
        st.synchronize()
    v = out.cpu().numpy()
    return v[0::2] - v[1::2]
