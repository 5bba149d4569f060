"""Nearest neighbours on the ball tree: `knn` over kdehip_knn / kdehip_knn_device_at (include/kdehip.h section 5n; kernels in
csrc/knn.hip), and the two bandwidth-free estimators that rest on them, `entropy_knn` (Kozachenko-Leonenko) and `kld_knn`
(Wang-Kulkarni-Verdu): a cross-check on `entropy` and `kld`, which rest on the LOOCV bandwidth.

The search is exact: per query the k points with the smallest key (squared distance, original index), what brute force
returns, bit for bit.  A 128-leaf chunk of the density is skipped for a block of 256 queries once its bounding box lies
beyond every query's k-th neighbour within the nearest chunk, so -- as in `evaluate_tol` -- which queries share a block
matters to the speed (never to the result): `order="tree"` processes them in the leaf order of a tree over them.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib, manifold as _mf
from ._lib import f64p, i64p, ptr
from .density import BallTreeDensity, getPoints, kde
from .evaltol import _leaf_rows

_EULER_GAMMA = 0.5772156649015329


def _host_arrays(bd):
    """the host density behind `bd` (a BallTreeDensity, or a DeviceDensity: the one it was uploaded from or its download)"""
    if isinstance(bd, BallTreeDensity):
        return bd
    return bd._host if bd._host is not None else bd.download()


def _scale(bd, metric, D):
    """the per-dimension scale of a metric as a float64 array, or None for the squared Euclidean distance"""
    if isinstance(metric, str):
        if metric == "euclid":
            return None
        if metric != "bandwidth":
            raise ValueError('knn: metric is "euclid", "bandwidth" or a length-D vector of scales')
        h = _host_arrays(bd)
        N = h.bt.num_points
        v = h.bandwidth[N * D:2 * N * D].reshape(N, D)
        if not np.all(v == v[0]):
            raise ValueError('knn: metric="bandwidth" needs ONE bandwidth vector; this density has per-point bandwidths')
        return np.ascontiguousarray(1.0 / v[0])
    s = np.ascontiguousarray(metric, dtype=np.float64).reshape(-1)
    if s.shape[0] != D:
        raise ValueError("knn: an explicit metric has one scale per dimension")
    return s


def _finish(d2, idx, stats, squared, return_stats):
    dist = d2 if squared else np.sqrt(d2)
    return (dist, idx, (int(stats[0]), int(stats[1]))) if return_stats else (dist, idx)


def knn(bd, pos=None, k=1, lvFlag=False, metric="euclid", order="tree", device=0, manifold=None, squared=False,
        return_stats=False):
    """The k points of `bd` nearest to every query: `(dist, idx)`, each of shape (k, Nq) in the caller's order -- row j holds
    the (j+1)-th neighbour, `idx` its 1-based index among `getPoints(bd)`'s columns (the convention of `sample`'s labels).
    Ties in distance go to the lower index.  A query with a NaN or infinite coordinate gets NaN distances and index 0.

    pos: a (D, Nq) matrix, a vector of 1-D positions or a BallTreeDensity; lvFlag=True (or pos is bd) asks for the neighbours
    of bd's own points, each point itself left out BY INDEX (a duplicate of it stays a neighbour at distance 0).
    metric: "euclid"; "bandwidth" -- every squared difference divided by the density's variance in that dimension; or a
    length-D vector of scales s, the squared distance being sum_k s_k d_k^2.  squared=True returns the squared distances.
    manifold: circular differences in those dimensions (section 5d).  order="tree" / "given" as in `evaluate_tol`: the
    speed alone depends on it.  return_stats=True adds (tiles visited, tiles in all).  1 <= k <= 32.  A DeviceDensity `bd`
    goes to its `.knn`."""
    from .product import DeviceDensity
    if isinstance(bd, DeviceDensity):
        return bd.knn(None if lvFlag else pos, k=k, metric=metric, manifold=manifold, squared=squared,
                      return_stats=return_stats)
    if not isinstance(bd, BallTreeDensity):
        raise TypeError("knn: a BallTreeDensity or a DeviceDensity")
    if order not in ("tree", "given"):
        raise ValueError('knn: order is "tree" or "given"')
    D = bd.bt.dims
    k = int(k)
    cd = bd._cstruct()
    mp = _mf.pointer(_mf.parse(manifold, D))
    sc = _scale(bd, metric, D)
    sp = _lib.optr(sc, f64p)
    stats = np.zeros(2, dtype=np.int64)
    if lvFlag or pos is bd:
        Nq, rows, where = bd.bt.num_points, None, None
    elif isinstance(pos, BallTreeDensity):
        if pos.bt.dims != D:
            raise ValueError("bd and pos must have the same dimension")
        if order == "tree":
            rows, where = _leaf_rows(pos)
        else:
            rows, where = np.ascontiguousarray(getPoints(pos).T), None
        Nq = rows.shape[0]
    else:
        if pos is None:
            raise TypeError("knn: pos is required unless lvFlag=True")
        P = np.asarray(pos, dtype=np.float64)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        if P.shape[0] != D:
            raise ValueError("bd and pos must have the same dimension")
        if order == "tree" and P.shape[1] > 1 and np.all(np.isfinite(P)):
            rows, where = _leaf_rows(kde(P, [1.0]))
        else:  # (a tree cannot place a NaN or an infinite point: such queries keep the given order)
            rows, where = np.ascontiguousarray(P.T), None
        Nq = rows.shape[0]
    d2 = np.zeros((Nq, max(k, 1)))            # [Nq][k]: the transpose is the (k, Nq) result
    idx = np.zeros((Nq, max(k, 1)), dtype=np.int64)
    _lib.check(_lib.lib.kdehip_knn(C.byref(cd), None if rows is None else ptr(rows, f64p), 0 if rows is None else Nq, k,
                                   1 if rows is None else 0, sp, ptr(d2, f64p), ptr(idx, i64p), ptr(stats, i64p), int(device),
                                   mp))
    if where is not None:
        back = np.empty(Nq, dtype=np.int64)
        back[where] = np.arange(Nq)
        d2, idx = d2[back], idx[back]
    return _finish(np.ascontiguousarray(d2.T), np.ascontiguousarray(idx.T), stats, squared, return_stats)


def _sum(vals):
    """math.fsum of the terms, or numpy's sum where an infinite or NaN term decides the result anyway"""
    return math.fsum(vals.tolist()) if np.all(np.isfinite(vals)) else float(np.sum(vals))


def _digamma_int(n):
    """psi at the integer n >= 1: -gamma + sum_{m < n} 1 / m"""
    return -_EULER_GAMMA + sum(1.0 / m for m in range(1, int(n)))


def _log_unit_ball(D):
    """log V_D, V_D = pi^(D/2) / Gamma(D/2 + 1)"""
    return 0.5 * D * math.log(math.pi) - math.lgamma(0.5 * D + 1.0)


def _estimator_checks(name, p, manifold):
    """Euclidean only, uniform weights only"""
    D = p.bt.dims if isinstance(p, BallTreeDensity) else p.dims
    man = _mf.parse(manifold, D)
    if man is not None and man.any():
        raise ValueError(f"{name}: Euclidean dimensions only")
    h = _host_arrays(p)
    N = h.bt.num_points
    w = h.bt.weights[N:2 * N]
    if not np.all(w == w[0]):
        raise ValueError(f"{name}: uniform weights only")
    return D, N


def _kth_distance(bd, pos, k, device):
    """the distance of every query to its k-th neighbour, leave-one-out when pos is None"""
    dist, _ = knn(bd, pos, k=k, lvFlag=pos is None, device=device)
    return dist[k - 1]


def entropy_knn(p, k=4, *, device=0, manifold=None) -> float:
    """The Kozachenko-Leonenko entropy estimate of the sample behind `p`, in nats:

        psi(N) - psi(k) + log V_D + (D / N) sum_i log eps_i,

    eps_i the Euclidean distance of point i to its k-th nearest other point (`knn(p, lvFlag=True)`), V_D the volume of the
    D-dimensional unit ball.  No bandwidth enters.  Euclidean distance and uniform weights only: a circular manifold or
    non-uniform weights raise ValueError.  A point that has k duplicates has eps_i = 0: the result is -inf, as the formula
    says -- jitter the data or use `entropy`.  `p`: a BallTreeDensity or a DeviceDensity."""
    D, N = _estimator_checks("entropy_knn", p, manifold)
    eps = _kth_distance(p, None, int(k), device)
    with np.errstate(divide="ignore"):
        s = _sum(np.log(eps))
    return _digamma_int(N) - _digamma_int(k) + _log_unit_ball(D) + D / N * s


def kld_knn(p, q, k=4, *, device=0, manifold=None) -> float:
    """The Wang-Kulkarni-Verdu estimate of KL(p || q) from the samples behind the two densities, in nats:

        (D / n) sum_i log(nu_i / rho_i) + log(m / (n - 1)),

    rho_i the distance of p's point i to its k-th nearest other point of p, nu_i its distance to the k-th nearest point of q;
    n and m the point counts.  Exactly 0.0 when `q is p`.  Restrictions as `entropy_knn`, for both densities; both are
    BallTreeDensity or both DeviceDensity (the rule of `kld`).  Duplicates give +-inf or nan, as the formula says."""
    from .loglik import _dims, _kind
    _kind(p, q)
    if _dims(p) != _dims(q):
        raise ValueError("knn -- dimensions of two BallTreeDensities must match")
    D, n = _estimator_checks("kld_knn", p, manifold)
    if q is p:
        return 0.0
    _, m = _estimator_checks("kld_knn", q, manifold)
    k = int(k)
    rho = _kth_distance(p, None, k, device)
    nu = _kth_distance(q, p, k, device)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = _sum(np.log(nu) - np.log(rho))
    return D / n * s + math.log(m / (n - 1))
