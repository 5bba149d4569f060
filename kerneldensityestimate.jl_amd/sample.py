"""Drawing from a density: `sample`, `rand`, `resample` (reference src/KDE01.jl:155-199, src/BallTreeDensity01.jl:312-334)
over kdehip_sample / kdehip_sample_device / kdehip_sample_device_batch / kdehip_resample_device (include/kdehip.h
section 2f; kernels in csrc/sample.hip).

Labels are 1-based original point indices (the reference's, and the product's `ind`).  Random numbers come from the
device Philox stream: sample s of a call draws the uniform and the D normals `philox_streams(seed, sample_offset + s, 1,
1, D)` returns, so a result is reproducible on the host and `sample_offset` continues an earlier call.  Samples come in
draw order; the reference returns them grouped by ascending label (same distribution).

`manifold=` (a per-dimension sequence of 'euclid' / 'circular', or "inherit" = the density's recorded `.manifold`): the
drawn coordinate of a circular dimension is wrapped to [-pi, pi) -- bit for bit the wrap of what the call without a
manifold returns; labels and the other dimensions are unchanged (include/kdehip.h section 5e).  `resample` then runs
`kde!(pts, addop, diffop)`: `manifold` for the bandwidth search, `tree_manifold` for the tree builder.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, manifold as _mf
from ._lib import SEED_MASK, addr, f64p, i64p, optr, ptr
from .density import BallTreeDensity, getBW, getPoints, kde
from .summary import _manifold as _man


def _seed(seed):
    return int(_lib.random_seed() if seed is None else seed) & SEED_MASK


def _labels(ind, Npts):
    a = np.ascontiguousarray(np.asarray(ind, dtype=np.int64).ravel())
    if a.size != Npts:
        raise ValueError("ind must hold Npts labels")
    return a


def sample(p, Npts, ind=None, *, seed=None, sample_offset=0, device=0, manifold=None):
    """`sample(p, Npts)` / `sample(p, Npts, ind)` (reference src/KDE01.jl:164-189): returns (points (D, Npts),
    ind (Npts,) 1-based).  `p`: a BallTreeDensity (host arrays, kdehip_sample on `device`) or a DeviceDensity (its own
    device; results come back as host arrays).  `ind`: given 1-based labels -- only the normals are drawn.  `manifold`:
    circular coordinates come back wrapped (kdehip_sample_manifold / kdehip_sample_device_manifold)."""
    from .product import DeviceDensity
    if not isinstance(p, (DeviceDensity, BallTreeDensity)):
        raise TypeError("sample: p must be a BallTreeDensity or a DeviceDensity")
    man = _man(p, manifold)
    Npts = int(Npts)  # (Npts < 0 is refused by the library: KdeHipError ERR_ARG)
    n = max(Npts, 0)
    s = _seed(seed)
    if isinstance(p, DeviceDensity):
        import torch
        D = p.dims
        dev = torch.device("cuda", p.device)
        P = torch.empty(D * max(n, 1), dtype=torch.float64, device=dev)
        I = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        T = None if ind is None else torch.from_numpy(_labels(ind, n)).to(dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            p.sample_device(P, I, Npts, seed=s, sample_offset=sample_offset, ind=T, stream=st.cuda_stream, manifold=man)
            st.synchronize()
        return P.cpu().numpy()[:D * n].reshape(n, D).T.copy(), I.cpu().numpy()[:n].copy()
    D = p.bt.dims
    pts = np.empty(D * n)
    out = np.empty(n, dtype=np.int64)
    lab = None if ind is None else _labels(ind, n)
    _lib.check(_lib.lib.kdehip_sample_manifold(C.byref(p._cstruct()), Npts, C.c_uint64(s), int(sample_offset), optr(lab, i64p),
                                               ptr(pts, f64p), ptr(out, i64p), int(device), _mf.pointer(man)))
    return pts.reshape(n, D).T.copy(), out


def rand(p, N=1, *, seed=None, manifold=None):
    """`rand(p, N=1)` (reference src/KDE01.jl:196-198): the points of `sample(p, N)`, (D, N)."""
    return sample(p, N, seed=seed, manifold=manifold)[0]


def resample(p, Np=None, ksType="lcv", *, seed=None, manifold=None, tree_manifold=None):
    """`resample(p, Np, ksType)` (reference src/BallTreeDensity01.jl:312-334).  Np None / <= 0 means Npts(p) (the
    reference's default calls an undefined `getNpts`; Npts(p) is its evident intent).
    ksType "lcv": `kde!(sample(p, Np)[0])` -- a DeviceDensity stays on the device (kdehip_resample_device) and gives a
    DeviceDensity, a BallTreeDensity gives a BallTreeDensity.
    ksType "discrete" (BallTreeDensity only): labels drawn by weight, the points themselves without noise, then
    `kde(points, getBW(p)[:, 0])`.  The reference's branch calls undefined functions; this is its evident intent (a
    zero-bandwidth copy of p sampled by weight, the kernel size of p's first point).
    `manifold` / `tree_manifold`: the wrapped draw, then `kde(pts, manifold=, tree_manifold=)` -- the reference's
    `kde!(pts, addop, diffop)` is both set to the same value (kdehip_resample_device_manifold for a DeviceDensity).  The
    noise-free "discrete" points are not wrapped; its `kde(points, ks)` takes `tree_manifold` only."""
    from .product import DeviceDensity
    if ksType not in ("lcv", "discrete"):
        raise ValueError("resample: ksType must be 'lcv' or 'discrete'")
    if isinstance(p, DeviceDensity):
        if ksType != "lcv":
            raise ValueError("resample: ksType 'discrete' needs the host arrays of a BallTreeDensity")
        return p.resample(Np, seed=seed, manifold=manifold, tree_manifold=tree_manifold)
    man, tman = _man(p, manifold), _man(p, tree_manifold, "tree_manifold")
    N = p.bt.num_points
    Np = N if Np is None or int(Np) <= 0 else int(Np)
    if ksType == "discrete":
        _, lab = sample(p, Np, seed=seed)
        return kde(getPoints(p)[:, lab - 1], getBW(p)[:, 0], tree_manifold=tman)
    pts, _ = sample(p, Np, seed=seed, manifold=man)
    return kde(pts, manifold=man, tree_manifold=tman)


def sample_device_batch(items, stream=None, *, manifold=None):
    """Many draws in ONE call (kdehip_sample_device_batch): `items` = dicts with `density` (DeviceDensity), `Npts`,
    `d_pts` (float64[D*Npts]), `d_ind` (int64[Npts]) device arrays (torch tensors or addresses) and optionally `seed`
    (default 0), `sample_offset` (0), `ind` (device int64[Npts] of 1-based labels).  One table build for the densities
    that have none yet, one draw launch per dimension count; every item gets what `DeviceDensity.sample_device` gives it.
    `manifold=`: one manifold for all items or one per item (None = Euclidean); an item's own `manifold` wins
    (kdehip_sample_device_batch_manifold).  Enqueues on `stream` and returns."""
    items = list(items)
    n = len(items)
    mans = None
    if manifold is not None or any("manifold" in it for it in items):   # (a call without any manifold parses none)
        mans = _mf.per_item(items, manifold)
    arr = (_lib.CSampleManifoldItem * max(1, n))()
    for k, it in enumerate(items):
        a = arr[k]
        if mans is not None:
            a.circular_mask = _mf.mask(mans[k])
        a.density = it["density"]._h
        a.Npts = int(it["Npts"])
        a.seed = int(it.get("seed", 0)) & SEED_MASK
        a.sample_offset = int(it.get("sample_offset", 0))
        a.d_ind_in = addr(it.get("ind"))
        a.d_pts = addr(it["d_pts"])
        a.d_ind = addr(it["d_ind"])
    _lib.check(_lib.lib.kdehip_sample_device_batch_manifold(n, arr, addr(stream)))
