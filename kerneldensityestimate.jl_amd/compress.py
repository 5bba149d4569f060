"""A density cut to M of its own points by kernel herding: the methods `compress` and `herding_order` of `BallTreeDensity`
and `DeviceDensity` and `DeviceDensity.compress_batch`, over kdehip_compress[_device] / kdehip_compress_device_batch /
kdehip_density_compress_device (include/kdehip.h section 5t; kernels in csrc/compress.hip).  The library's own: the reference
has no counterpart.

Herding picks, one after another, the points of p that best match p's kernel mean embedding under the Gaussian kernel of
standard deviation `bw` (as `mmd` takes it; None = sqrt(2) times p's bandwidth, the kernel under which the squared MMD is the
integrated squared error at p's own bandwidth up to the Gaussian constant).  The result has the picked points, weights 1 / M and
bandwidth `ks` (None = p's own).  The run is anytime: its first m picks are the run to m, so one run gives the whole curve
mmd2(m), and `mmd_tol` asks for the shortest prefix that reaches an MMD.

The surface is methods only: every function of this module is private.  `info` is a dict: `idx` (the picks, 1-based, by
original point, in pick order), `mmd2` (the squared MMD after 1 .. len(idx) picks, not normalised, as `mmd`), `zpick`, `rpick`,
`self_sum`, `M` (the points of the result) and `reached` (False when `mmd_tol` was asked for and not reached)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import addr, f64p, i64p, optr, ptr
from .loglik import _dims
from .modes import _kind
from .overlap import _variances

_STEPWISE = 1  # KDEHIP_COMPRESS_STEPWISE


def _npts(p, kind):
    return int(p.bt.num_points) if kind == "host" else int(p.num_points)


def _kernel_var(bw, D):
    """None (the library takes twice the leaf variance), or the D kernel variances bw * bw"""
    if bw is None:
        return None
    sd = _variances(bw, D, "bw")
    if not (np.isfinite(sd).all() and (sd > 0.0).all()):
        raise ValueError("bw must be finite and > 0")
    return sd * sd


def _ks(ks, D):
    """None (the density's own bandwidth), or D standard deviations"""
    if ks is None:
        return None
    sd = _variances(ks, D, "ks")
    if not (np.isfinite(sd).all() and (sd > 0.0).all()):
        raise ValueError("ks must be finite and > 0")
    return sd


def _count(M, N, what="M"):
    if M is None or int(M) != M or not 1 <= int(M) <= N:
        raise ValueError(f"{what} must be an integer in 1..N")
    return int(M)


def _curve(zpick, rpick, self_sum):
    """mmd2(m) = self_sum - (2 / m) sum_{t < m} zpick[t] + (m + 2 sum_{t < m} rpick[t]) / m^2 for m = 1 .. len(zpick)"""
    m = np.arange(1, len(zpick) + 1, dtype=np.float64)
    return self_sum - (2.0 / m) * np.cumsum(zpick) + (m + 2.0 * np.cumsum(rpick)) / (m * m)


def _info(idx, zpick, rpick, self_sum):
    return dict(idx=idx, mmd2=_curve(zpick, rpick, self_sum), zpick=zpick, rpick=rpick, self_sum=float(self_sum))


def _herd_host(p, M, var, man, flags, device):
    idx, z, r, s = np.zeros(M, dtype=np.int64), np.zeros(M), np.zeros(M), np.zeros(1)
    _lib.check(_lib.lib.kdehip_compress(C.byref(p._cstruct()), M, optr(var, f64p), flags, ptr(idx, i64p), ptr(z, f64p),
                                        ptr(r, f64p), ptr(s, f64p), int(device), _mf.pointer(man)))
    return _info(idx, z, r, s[0])


def _trace_tensors(M, dev):
    import torch
    return torch.empty(M, dtype=torch.int64, device=dev), torch.empty(2 * M + 1, dtype=torch.float64, device=dev)


def _trace_info(M, d_idx, d_tr):
    tr = d_tr.cpu().numpy()
    return _info(d_idx.cpu().numpy(), tr[:M].copy(), tr[M:2 * M].copy(), tr[2 * M])


def _herd_device(p, M, var, man, flags):
    """the picks and the traces of a resident density: 3 M + 1 numbers come to the host, no point does"""
    import torch
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        d_idx, d_tr = _trace_tensors(M, dev)
        torch.cuda.current_stream(dev).synchronize()  # (the entry is blocking and runs on the library's own stream)
        base = d_tr.data_ptr()
        _lib.check(_lib.lib.kdehip_compress_device(p._h, M, optr(var, f64p), flags, addr(d_idx), None, addr(base),
                                                   addr(base + 8 * M), addr(base + 16 * M), _mf.pointer(man)))
        return _trace_info(M, d_idx, d_tr)


def _arguments(p, M, mmd_tol, bw, manifold, stepwise):
    kind = _kind(p)
    D, N = _dims(p), _npts(p, kind)
    if M is None and mmd_tol is None:
        raise ValueError("compress: give M, mmd_tol, or both (M then bounds the run)")
    if mmd_tol is not None and not float(mmd_tol) >= 0.0:
        raise ValueError("mmd_tol must be >= 0")
    run = N if M is None else _count(M, N)
    return kind, D, run, _kernel_var(bw, D), _mf.resolve(p, manifold, D), _STEPWISE if stepwise else 0


def _prefix(info, mmd_tol):
    """the points of the result: the whole run, or the shortest prefix with mmd2(m) <= mmd_tol^2"""
    run = len(info["idx"])
    info["M"], info["reached"] = run, True
    if mmd_tol is None:
        return run
    hit = np.nonzero(info["mmd2"] <= float(mmd_tol) ** 2)[0]
    if hit.size:
        info["M"] = int(hit[0]) + 1
    else:
        info["reached"] = False
    return info["M"]


def _herding_order(p, M, bw=None, manifold=None, stepwise=False, device=0):
    kind, D, run, var, man, flags = _arguments(p, M, None, bw, manifold, stepwise)
    info = _herd_host(p, run, var, man, flags, device) if kind == "host" else _herd_device(p, run, var, man, flags)
    info["M"], info["reached"] = run, True
    return info["idx"], info


def _own_sd(p):
    """the first leaf's bandwidth as standard deviations: what the resident entry takes for ks = NULL"""
    N, D = p.bt.num_points, p.bt.dims
    return np.sqrt(np.ascontiguousarray(p.bandwidth[N * D:N * D + D]))


def _compress_host(p, M, mmd_tol, bw, ks, manifold, return_info, tree_manifold, stepwise, device):
    from .density import getPoints, kde
    kind, D, run, var, man, flags = _arguments(p, M, mmd_tol, bw, manifold, stepwise)
    sd = _ks(ks, D)
    tman = _mf.resolve(p, tree_manifold, D, attr="tree_manifold")
    info = _herd_host(p, run, var, man, flags, device)
    m = _prefix(info, mmd_tol)
    out = kde(getPoints(p)[:, info["idx"][:m] - 1], _own_sd(p) if sd is None else sd, np.full(m, 1.0 / m), tree_manifold=tman)
    return (out, info) if return_info else out


def _build_device(p, m, var, sd, man, tman):
    """kdehip_density_compress_device: the m picks gathered on the device, one copy down, the host builder, the block back up"""
    import torch
    h = C.c_void_p()
    dev = torch.device("cuda", p.device)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(_lib.lib.kdehip_density_compress_device(C.byref(h), p._h, m, optr(var, f64p), optr(sd, f64p), _mf.pointer(man),
                                                           _mf.pointer(tman)))
    return type(p)._built(h, p.device, None, None, man, tman)


def _compress_device(p, M, mmd_tol, bw, ks, manifold, return_info, tree_manifold, stepwise):
    kind, D, run, var, man, flags = _arguments(p, M, mmd_tol, bw, manifold, stepwise)
    sd = _ks(ks, D)
    tman = _mf.resolve(p, tree_manifold, D, attr="tree_manifold")
    if mmd_tol is None and not return_info and not stepwise:
        return _build_device(p, run, var, sd, man, tman)
    info = _herd_device(p, run, var, man, flags)
    out = _build_device(p, _prefix(info, mmd_tol), var, sd, man, tman)  # (anytime: the run to m is the prefix of the run to M)
    return (out, info) if return_info else out


def _compress(p, M=None, mmd_tol=None, bw=None, ks=None, manifold=None, return_info=False, tree_manifold=None, stepwise=False,
              device=0):
    if _kind(p) == "host":
        return _compress_host(p, M, mmd_tol, bw, ks, manifold, return_info, tree_manifold, stepwise, device)
    return _compress_device(p, M, mmd_tol, bw, ks, manifold, return_info, tree_manifold, stepwise)


def _compress_batch(densities, M, bw=None, ks=None, manifold=None, return_info=False, tree_manifold=None, stepwise=False):
    """Many DeviceDensity in ONE call (kdehip_compress_device_batch).  `densities`: DeviceDensity, or dicts with `density` and
    optionally `M`, `bw`, `ks`, `manifold`, `tree_manifold`, `stepwise` of their own.  Returns the list of new handles (with
    return_info: of (handle, info) pairs), each what `p.compress(M, ...)` returns."""
    import torch
    from .product import DeviceDensity
    items = [dict(it) if isinstance(it, dict) else dict(density=it) for it in densities]
    n = len(items)
    arr = (_lib.CCompressItem * max(1, n))()
    handles = (C.c_void_p * max(1, n))()
    keep = []
    for k, it in enumerate(items):
        p = it["density"]
        if not isinstance(p, DeviceDensity):
            raise TypeError("compress_batch: items of DeviceDensity")
        _, D, run, var, man, flags = _arguments(p, it.get("M", M), None, it.get("bw", bw), it.get("manifold", manifold),
                                                it.get("stepwise", stepwise))
        sd = _ks(it.get("ks", ks), D)
        tman = _mf.resolve(p, it.get("tree_manifold", tree_manifold), D, attr="tree_manifold")
        keep.append([p, run, var, sd, man, tman, None])
        arr[k].p, arr[k].var, arr[k].M, arr[k].flags = p._h, optr(var, f64p), run, flags
        arr[k].circular_mask = _mf.mask(man)
        arr[k].out = C.cast(C.addressof(handles) + k * C.sizeof(C.c_void_p), C.POINTER(C.c_void_p))
        arr[k].ks, arr[k].tree_manifold = optr(sd, f64p), _mf.pointer(tman)
    if n == 0:
        return []
    if len({kp[0].device for kp in keep}) != 1:
        raise ValueError("compress_batch: the densities are on different devices")
    dev = torch.device("cuda", keep[0][0].device)
    with torch.cuda.device(dev):
        if return_info:
            for k, kp in enumerate(keep):
                d_idx, d_tr = _trace_tensors(kp[1], dev)
                kp[6] = (d_idx, d_tr)
                base = d_tr.data_ptr()
                arr[k].d_idx, arr[k].d_zpick, arr[k].d_rpick = d_idx.data_ptr(), base, base + 8 * kp[1]
                arr[k].d_self_sum = base + 16 * kp[1]
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(_lib.lib.kdehip_compress_device_batch(n, arr))
    out = []
    for k, (p, run, _, _, man, tman, tr) in enumerate(keep):
        d = DeviceDensity._built(C.c_void_p(handles[k]), p.device, None, None, man, tman)
        if return_info:
            info = _trace_info(run, *tr)
            info["M"], info["reached"] = run, True
            d = (d, info)
        out.append(d)
    return out
