"""Reweighting and moving a density without re-forming its tree: `changeWeights!` / `movePoints!` (reference
src/BallTreeDensity01.jl:278-309; include/kdehip.h section 5r) and the Bayes update `w_i <- w_i L(x_i)` on top of them.

Every leaf takes a new weight or moves by its own offset, the statistics of the internal nodes are recomputed from their
children, the tree itself stays.  On the host that is `kdehip_density_refit` (csrc/balltree.cpp); on a `DeviceDensity` it is
`kdehip_density_refit_device` (csrc/refit.hip) and nothing but a few hundred bytes leaves HBM.  Both return a NEW density.
The surface is methods: `BallTreeDensity.changeWeights / movePoints / bayes_update` and the same three on `DeviceDensity`,
with `DeviceDensity.refit_batch` for many densities in one call.  The recorded `manifold` and `tree_manifold` of the source
carry over; the box formula and the move use `tree_manifold` (addop / diffop of the tree's operators)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import addr, f64p, i64p, optr, ptr

KEEP, WEIGHTS, LOGL = 0, 1, 2


# ---- host ----------------------------------------------------------------------------------------------------------------

def _vector(x, N, name):
    v = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    if v.size != N:
        raise ValueError(f"{name} must have one entry per point")
    return v


def _delta_flat(delta, D, N):
    d = np.asarray(delta, dtype=np.float64)
    if d.ndim == 1 and D == 1:
        d = d.reshape(1, -1)
    if d.shape != (D, N):
        raise ValueError("delta must be a (D, N) matrix, one column per point")
    return np.ascontiguousarray(d.T).ravel()  # column-major D x N


def refit_host(bd, new_weights=None, delta=None, tree_manifold="inherit"):
    """`kdehip_density_refit` on the twelve arrays of `bd`: new_weights (N, original order, used as given) and / or delta
    ((D, N), original order).  tree_manifold: the operators, "inherit" = those `bd` was built with."""
    from .density import _empty_density
    bt = bd.bt
    D, N = int(bt.dims), int(bt.num_points)
    if bt.centers is None or bd.bandwidthMin is None:
        raise ValueError("refit needs the twelve arrays of a density that kde built (density_from_arrays carries six)")
    tman = _mf.resolve(bd, tree_manifold, D, attr="tree_manifold")
    w = None if new_weights is None else _vector(new_weights, N, "weights")
    dl = None if delta is None else _delta_flat(delta, D, N)
    multibw = int(getattr(bd, "multibandwidth", 0)) == 1
    out = _empty_density(D, N, multibw)
    ot = out.bt
    _lib.check(_lib.lib.kdehip_density_refit(
        D, N, ptr(bt.centers, f64p), ptr(bt.ranges, f64p), ptr(bt.weights, f64p), ptr(bt.left_child, i64p),
        ptr(bt.right_child, i64p), ptr(bt.lowest_leaf, i64p), ptr(bt.highest_leaf, i64p), ptr(bt.permutation, i64p),
        ptr(bd.means, f64p), ptr(bd.bandwidth, f64p), ptr(bd.bandwidthMin, f64p), ptr(bd.bandwidthMax, f64p), int(multibw),
        optr(w, f64p), optr(dl, f64p), _mf.pointer(tman),
        ptr(ot.centers, f64p), ptr(ot.ranges, f64p), ptr(ot.weights, f64p), ptr(ot.left_child, i64p),
        ptr(ot.right_child, i64p), ptr(ot.lowest_leaf, i64p), ptr(ot.highest_leaf, i64p), ptr(ot.permutation, i64p),
        ptr(out.means, f64p), ptr(out.bandwidth, f64p), ptr(out.bandwidthMin, f64p), ptr(out.bandwidthMax, f64p)))
    out.tree_manifold = bd.tree_manifold if isinstance(tree_manifold, str) else _mf.parse(tree_manifold, D)
    return out


def bayes_weights(w, logl):
    """The Bayes update of section 5r in NumPy: (w', log_evidence, ess) with m = max l_i over w_i > 0,
    S = sum w_i exp(l_i - m), w' = w exp(l - m) / S, log_evidence = m + log S, ess = 1 / sum w'^2."""
    w = np.asarray(w, dtype=np.float64)
    l = np.asarray(logl, dtype=np.float64)
    if np.isnan(l).any() or (l == np.inf).any():
        raise ValueError("bayes_update: a log-likelihood is NaN or +Inf")
    pos = w > 0
    if not pos.any():
        raise ValueError("bayes_update: no point of the density has a positive weight")
    m = l[pos].max()
    if m == -np.inf:
        raise ValueError("bayes_update: the evidence is 0 (every log-likelihood of a weighted point is -Inf)")
    t = np.zeros_like(w)
    with np.errstate(under="ignore"):
        t[pos] = w[pos] * np.exp(l[pos] - m)
    S = t.sum()
    if not (S > 0 and np.isfinite(S)):
        raise ValueError("bayes_update: the evidence is 0 or not finite (every log-likelihood -Inf?)")
    wn = t / S
    return wn, float(m + np.log(S)), float(1.0 / np.sum(wn * wn))


def host_bayes_update(bd, logl):
    from .density import getWeights
    wn, le, ess = bayes_weights(getWeights(bd), _vector(logl, int(bd.bt.num_points), "logl"))
    return refit_host(bd, new_weights=wn), le, ess


# ---- device ---------------------------------------------------------------------------------------------------------------

def _device_vector(x, n, dev, name):
    """n float64 values on `dev`: a tensor stays where it is (made contiguous), anything else is uploaded"""
    import torch
    if hasattr(x, "data_ptr"):
        t = x.to(dev, torch.float64).reshape(-1).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())).to(dev)
    if t.numel() != n:
        raise ValueError(f"{name} must have one entry per point")
    return t


def _device_delta(delta, D, N, dev):
    import torch
    if hasattr(delta, "data_ptr"):
        d = delta.to(dev, torch.float64)
        if d.dim() == 1 and D == 1:
            d = d.reshape(1, -1)
        if tuple(d.shape) != (D, N):
            raise ValueError("delta must be a (D, N) matrix, one column per point")
        return d.t().contiguous()  # column-major D x N = the (N, D) row-major array
    return torch.from_numpy(_delta_flat(delta, D, N)).to(dev)


def _prepare_item(dd, values, kind, delta, dev):
    v = None if kind == KEEP else _device_vector(values, dd.num_points, dev, "weights" if kind == WEIGHTS else "logl")
    d = None if delta is None else _device_delta(delta, dd.dims, dd.num_points, dev)
    if v is None and d is None:
        raise ValueError("refit: neither values nor delta: nothing to do")
    return v, d


def _result(dd, handle):
    from .product import DeviceDensity
    return DeviceDensity._built(handle, dd.device, dd.bw, dd.nevals, dd.manifold, dd.tree_manifold)


def refit_device(dd, values=None, kind=KEEP, delta=None, leaf_order=False):
    """`kdehip_density_refit_device` on the handle of `dd`: (DeviceDensity, log_evidence, ess), the last two None unless
    kind is LOGL.  Tensors stay on the device, NumPy arrays are uploaded; the current stream is synchronised first (the entry
    is blocking and runs on the library's own stream)."""
    import torch
    dev = torch.device("cuda", dd.device)
    with torch.cuda.device(dev):
        v, d = _prepare_item(dd, values, kind, delta, dev)
        torch.cuda.current_stream(dev).synchronize()
        tman = _mf.resolve(dd, "inherit", dd.dims, attr="tree_manifold")
        h = C.c_void_p()
        le, ess = C.c_double(np.nan), C.c_double(np.nan)
        _lib.check(_lib.lib.kdehip_density_refit_device(C.byref(h), dd._h, addr(v), int(kind), int(bool(leaf_order)), addr(d),
                                                        _mf.pointer(tman), C.byref(le), C.byref(ess)))
    out = _result(dd, h)
    return (out, float(le.value), float(ess.value)) if kind == LOGL else (out, None, None)


def device_bayes_update(dd, logl, leaf_order=False):
    """`w_i <- w_i L(x_i)`.  logl: N log-likelihoods (tensor or array; by original point, or by leaf with leaf_order=True), or a
    DeviceDensity likelihood -- evaluated in the log domain at this density's points (kdehip_evaluate_log_device_at, which
    returns them in this density's original order) without leaving the device."""
    from .product import DeviceDensity
    if isinstance(logl, DeviceDensity):
        import torch
        if logl.dims != dd.dims:
            raise ValueError("the likelihood and the density must have the same dimension")
        dev = torch.device("cuda", dd.device)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            out = torch.empty(max(1, dd.num_points), dtype=torch.float64, device=dev)
            _lib.check(_lib.lib.kdehip_evaluate_log_device_at(logl._h, dd._h, addr(out), addr(st.cuda_stream), None))
        logl, leaf_order = out[:dd.num_points], False
    return refit_device(dd, logl, LOGL, None, leaf_order)


def refit_batch(items):
    """Many refits in one call (kdehip_density_refit_device_batch).  items: dicts with `density` and any of `weights` or `logl`
    (one of them at most), `delta`, `leaf_order`.  Returns [(DeviceDensity, log_evidence, ess)] -- the last two None unless
    the item has `logl`.  One bad item fails the whole call."""
    import torch
    items = list(items)
    if not items:
        return []
    dds = [it["density"] for it in items]
    if len({dd.device for dd in dds}) != 1:
        raise ValueError("refit_batch: the densities are on different devices")
    dev = torch.device("cuda", dds[0].device)
    n = len(items)
    arr = (_lib.CRefitItem * n)()
    keep = []
    les = np.full(n, np.nan)
    esss = np.full(n, np.nan)
    with torch.cuda.device(dev):
        for k, (it, dd) in enumerate(zip(items, dds)):
            if "weights" in it and "logl" in it:
                raise ValueError("refit_batch: an item has `weights` or `logl`, not both")
            kind = WEIGHTS if it.get("weights") is not None else LOGL if it.get("logl") is not None else KEEP
            v, d = _prepare_item(dd, it.get("weights") if kind == WEIGHTS else it.get("logl"), kind, it.get("delta"), dev)
            keep.append((v, d))
            tman = _mf.resolve(dd, "inherit", dd.dims, attr="tree_manifold")
            arr[k].p = dd._h
            arr[k].d_values = None if v is None else v.data_ptr()
            arr[k].d_delta = None if d is None else d.data_ptr()
            arr[k].log_evidence = C.cast(les[k:].ctypes.data, f64p)
            arr[k].ess = C.cast(esss[k:].ctypes.data, f64p)
            arr[k].kind = kind
            arr[k].leaf_order = int(bool(it.get("leaf_order", False)))
            arr[k].circular_mask = _mf.mask(tman)
        torch.cuda.current_stream(dev).synchronize()
        hs = (C.c_void_p * n)()
        _lib.check(_lib.lib.kdehip_density_refit_device_batch(n, arr, hs))
    out = []
    for k, dd in enumerate(dds):
        logl = arr[k].kind == LOGL
        out.append((_result(dd, C.c_void_p(hs[k])), float(les[k]) if logl else None, float(esss[k]) if logl else None))
    return out
