"""The curvature of a density: `evaluate_hess`, `laplace`, `fit_modes`, `getKDEModeFit` and `evaluate_hess_device_batch`, over
kdehip_evaluate_hess[_device] / kdehip_evaluate_hess_device_batch (include/kdehip.h section 5k; kernels in csrc/modes.hip).
The library's own: the reference's only second-order summary is `getKDEfit`, one moment-matched Gaussian for the whole density.

With d_ik, a_i, S_0 and S_k as in `modes` and t_i = w_i e^{a_i - m},

    S_kl = sum_i t_i d_ik d_il,   g_k = -S_k / (S_0 v_k),   H_kl = S_kl / (S_0 v_k v_l) - delta_kl / v_k - g_k g_l

is the Hessian of log p at x, and where -H is positive definite cov = (-H)^-1 is the covariance of the Gaussian with the
density's curvature there: the Laplace approximation of a mode.  The density is a BallTreeDensity (host arrays, run on
`device`) or a DeviceDensity (on its own device); `manifold=` as the other entries take it, "inherit" included.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from .loglik import _dims
from .modes import _device_points, _host_points, _kind, modes


def _curvature(p, pos, device, manifold, what, want):
    """the outputs named in `want` (of logp, grad, hess, cov, definite) as the ABI lays them out: Nq rows"""
    kind, D = _kind(p), _dims(p)
    man = _mf.resolve(p, manifold, D)
    shapes = dict(logp=(), grad=(D,), hess=(D, D), cov=(D, D), definite=())
    names = ("logp", "grad", "hess", "cov", "definite")
    if kind == "host":
        flat = _host_points(pos, D, what)
        Nq = flat.shape[0]
        out = {k: np.zeros((Nq,) + shapes[k], dtype=np.int32 if k == "definite" else np.float64) for k in want}
        args = [_lib.optr(out.get(k), _lib.i32p if k == "definite" else _lib.f64p) for k in names]
        cd = p._cstruct()
        _lib.check(_lib.lib.kdehip_evaluate_hess(C.byref(cd), _lib.ptr(flat, _lib.f64p), Nq, *args, int(device),
                                                 _mf.pointer(man)))
        return out
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        flat = _device_points(pos, D, dev, what)
        Nq = int(flat.shape[0])
        out = {k: torch.zeros((max(1, Nq),) + shapes[k], dtype=torch.int32 if k == "definite" else torch.float64, device=dev)
               for k in want}
        st = torch.cuda.current_stream(dev)
        _lib.check(_lib.lib.kdehip_evaluate_hess_device(p._h, _lib.addr(flat), Nq, *[_lib.addr(out.get(k)) for k in names],
                                                        _mf.pointer(man), _lib.addr(st.cuda_stream)))
        st.synchronize()
        return {k: v.cpu().numpy()[:Nq].copy() for k, v in out.items()}


def evaluate_hess(p, pos, *, log=True, device=0, manifold=None):
    """(val (Nq,), grad (D, Nq), hess (D, D, Nq)) at the columns of `pos` (D, Nq): log p, its gradient g and its Hessian H
    (section 5k).  With log=False: p, its gradient p g and its Hessian p (H + g g^T), formed on the host from the log-domain
    outputs (where p underflows they are 0 while the log-domain ones stay finite).  A DeviceDensity takes host points or a
    device tensor; the results are numpy arrays."""
    out = _curvature(p, pos, device, manifold, "evaluate_hess", ("logp", "grad", "hess"))
    val, grad, hess = out["logp"], np.ascontiguousarray(out["grad"].T), np.ascontiguousarray(out["hess"].transpose(1, 2, 0))
    if log:
        return val, grad, hess
    pv = np.exp(val)
    with np.errstate(invalid="ignore"):
        full = np.where(pv == 0.0, 0.0, pv * (hess + grad[:, None, :] * grad[None, :, :]))
        return pv, np.where(pv == 0.0, 0.0, pv * grad), full


def laplace(p, pos, *, device=0, manifold=None):
    """(cov (D, D, Nq), definite (Nq,) bool): cov = (-H)^-1 at the columns of `pos` by a Cholesky factorisation of -H on the
    device.  definite is False where a pivot fails -- the point is a saddle, a minimum or lies in a flat direction, not a
    maximum -- and all of cov[:, :, q] is NaN there.  At a mode cov - diag(v) is positive semidefinite: a mode is never
    narrower than the kernel."""
    out = _curvature(p, pos, device, manifold, "laplace", ("cov", "definite"))
    return np.ascontiguousarray(out["cov"].transpose(1, 2, 0)), out["definite"] != 0


def fit_modes(p, starts=None, *, device=0, manifold=None, **modes_kw):
    """(means (D, n), covs (D, D, n), mass (n,), logp (n,), definite (n,)): `modes(p, ...)`, then the curvature at every
    mode -- a Gaussian per mode, in descending logp.  means, mass and logp are `modes`' own arrays and covs is
    `laplace(p, means)`.  `mass` is the BASIN mass of `modes` (the weight of the starts that flowed into the mode), not a
    Laplace evidence."""
    _kind(p)
    man = _mf.resolve(p, manifold, _dims(p))
    means, logp, mass, _ = modes(p, starts, device=device, manifold=man, **modes_kw)
    covs, definite = laplace(p, means, device=device, manifold=man)
    return means, covs, mass, logp, definite


def getKDEModeFit(p, **kw):
    """(mode (D,), cov (D, D)): the highest joint mode of the density and the covariance of its Laplace approximation, the
    first of `fit_modes(p, **kw)` -- the per-mode counterpart of `getKDEfit`, which matches ONE Gaussian to the moments of
    the whole density and so, for a multimodal one, sits between the modes and spans them."""
    means, covs, _, _, _ = fit_modes(p, **kw)
    return means[:, 0], covs[:, :, 0]


def _device_tensor(t, name, dtype):
    """the kernels write 8-byte (definite: 4-byte) values at consecutive addresses of device memory: anything else is refused"""
    if not getattr(t, "is_cuda", False) or str(t.dtype) != "torch." + dtype or not t.is_contiguous():
        raise ValueError(f"evaluate_hess_device_batch: {name} must be a contiguous {dtype} device tensor")


def evaluate_hess_device_batch(items, stream=None):
    """The curvature of many DeviceDensity items in ONE call (kdehip_evaluate_hess_device_batch): `items` = dicts with
    `density`, `pos` (float64 device tensor of Nq rows of D) and any of the outputs `logp` (float64, Nq), `grad` (Nq, D),
    `hess` (Nq, D, D), `cov` (Nq, D, D), `definite` (int32, Nq) -- at least one; all contiguous --, optionally `manifold`.  Enqueue only on
    `stream`, no read-back: the call can be captured in a graph.  Every item's results are bit for bit the single call's."""
    from .product import DeviceDensity
    items = list(items)
    n = len(items)
    arr = (_lib.CHessItem * max(1, n))()
    for k, it in enumerate(items):
        d = it["density"]
        if not isinstance(d, DeviceDensity):
            raise TypeError("evaluate_hess_device_batch: items of DeviceDensity")
        pos = it["pos"]
        _device_tensor(pos, "pos", "float64")
        if pos.dim() != 2 or int(pos.shape[1]) != d.dims:
            raise ValueError("evaluate_hess_device_batch: pos is Nq rows of D")
        Nq, D = int(pos.shape[0]), d.dims
        outs = {name: it.get(name) for name in ("logp", "grad", "hess", "cov", "definite")}
        if all(v is None for v in outs.values()):
            raise ValueError("evaluate_hess_device_batch: an item asks for no output")
        for name, per in (("logp", 1), ("grad", D), ("hess", D * D), ("cov", D * D), ("definite", 1)):
            if outs[name] is not None:
                _device_tensor(outs[name], name, "int32" if name == "definite" else "float64")
                if int(outs[name].numel()) < Nq * per:
                    raise ValueError(f"evaluate_hess_device_batch: {name} holds Nq entries of its shape")
        arr[k].bd, arr[k].d_pos, arr[k].Nq = d._h, _lib.addr(pos), Nq
        arr[k].d_logp, arr[k].d_grad, arr[k].d_hess = _lib.addr(outs["logp"]), _lib.addr(outs["grad"]), _lib.addr(outs["hess"])
        arr[k].d_cov, arr[k].d_definite = _lib.addr(outs["cov"]), _lib.addr(outs["definite"])
        arr[k].circular_mask = _mf.mask(_mf.resolve(d, it.get("manifold"), d.dims))
    _lib.check(_lib.lib.kdehip_evaluate_hess_device_batch(n, arr, _lib.addr(stream)))
