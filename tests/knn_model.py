"""NumPy / plain-Python restatement of include/kdehip.h section 5n, written from its text: the k nearest leaves by the key
(d2, original index), and the plan that decides which (256-query block, 128-leaf chunk) tiles the search visits.  Everything
takes LEAF-ORDER arrays: `pts` (N, D) leaf centres, `orig` (N,) the 1-based original index of each leaf, `qry` (Nq, D)
queries in the order they are processed (leave-one-out: qry is pts, query q is leaf q).

Unlike tests/evaltol_model.py this model agrees with the device TO THE BIT, because the contract's distance is a chain of
correctly rounded operations: with no scale it is `acc + d * d` in plain fp64 (fma(t, 1, acc) rounds t + acc once); with a
scale each fma is formed exactly in integers and rounded once (`fma`)."""
import math
from fractions import Fraction

import numpy as np

CHUNK, BLOCK = 128, 256
EULER_GAMMA = 0.5772156649015329


def wrap(d):
    """csrc/circ_wrap.hpp: to [-pi, pi), every operation rounded on its own"""
    return d - 2.0 * math.pi * np.floor((d + math.pi) / (2.0 * math.pi))


def _int_exp(x):
    """x = m * 2^e exactly, m an integer"""
    m, e = math.frexp(x)
    return int(math.ldexp(m, 53)), e - 53


def fma(a, b, c):
    """round(a * b + c), rounded once, for finite arguments: the sum is formed exactly in integers, and Python's division of
    two integers is correctly rounded"""
    (ma, ea), (mb, eb), (mc, ec) = _int_exp(a), _int_exp(b), _int_exp(c)
    ep = ea + eb
    e = min(ep, ec)
    total = ((ma * mb) << (ep - e)) + (mc << (ec - e))
    return total / (1 << -e) if e < 0 else float(total << e)


def fma_fraction(a, b, c):
    """the same through rationals (slow: the check of `fma`)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


_fma = np.frompyfunc(fma, 3, 1)


def _two_sum(a, b):
    """a + b = s + e exactly (Knuth)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_array(t, s, acc):
    """`fma` element by element on arrays, t, s, acc >= 0 and far from overflow and underflow, without a Python call per
    element: t * s = p + e exactly (Dekker's product on Veltkamp's split), p + acc = s1 + e1 and e1 + e = y + ey exactly, and
    fl(s1 + y) is the rounding of the exact sum unless s1 + y lies within |ey| of a point halfway between two doubles -- those
    elements (none, as a rule) are redone by `fma`"""
    t, acc = np.asarray(t, dtype=np.float64), np.asarray(acc, dtype=np.float64)
    s = np.float64(s)
    p = t * s
    c = 134217729.0  # 2^27 + 1
    th = c * t
    th = th - (th - t)
    tl = t - th
    sh = c * s
    sh = sh - (sh - s)
    sl = s - sh
    e = ((th * sh - p) + th * sl + tl * sh) + tl * sl
    s1, e1 = _two_sum(p, acc)
    y, ey = _two_sum(e1, e)
    r, err = _two_sum(s1, y)
    h = np.spacing(r)
    near = (ey != 0.0) & ((np.abs(np.abs(err) - 0.5 * h) <= 4.0 * np.abs(ey)) | (np.abs(np.abs(err) - 0.25 * h) <= 4.0 * np.abs(ey)))
    if near.any():
        r = np.array(r)
        for i in zip(*np.nonzero(near)):
            r[i] = fma(float(t[i]), float(s), float(acc[i]))
    return r


def _chain(diffs, scale):
    """acc = fma(d_k * d_k, s_k, acc) from 0, k ascending; diffs: a list of D equal-shaped arrays"""
    acc = np.zeros_like(diffs[0])
    for k, d in enumerate(diffs):
        t = d * d
        acc = acc + t if scale is None else fma_array(t, float(scale[k]), acc)
    return acc


def dist2(pts, qry, scale=None, circ=()):
    """d2[q, i]"""
    diffs = []
    for k in range(pts.shape[1]):
        d = qry[:, k, None] - pts[None, :, k]
        diffs.append(wrap(d) if k in circ else d)
    return _chain(diffs, scale)


def boxes(pts):
    """step 1: lo (nc, D), hi (nc, D)"""
    nc = (pts.shape[0] + CHUNK - 1) // CHUNK
    lo = np.stack([pts[c * CHUNK:(c + 1) * CHUNK].min(axis=0) for c in range(nc)])
    hi = np.stack([pts[c * CHUNK:(c + 1) * CHUNK].max(axis=0) for c in range(nc)])
    return lo, hi


def dmin2(lo, hi, qry, scale=None, circ=()):
    """dmin2[q, c]: the distance's chain on the nearest corner, dmin_k = 0 in a circular dimension"""
    diffs = []
    for k in range(lo.shape[1]):
        d = np.maximum(0.0, np.maximum(lo[None, :, k] - qry[:, k, None], qry[:, k, None] - hi[None, :, k]))
        diffs.append(np.zeros_like(d) if k in circ else d)
    return _chain(diffs, scale)


def _topk(d2row, orig, k, skip=None):
    """the k smallest (d2, original index) of one query: (d2 (k,), idx (k,)); `skip`: a leaf position left out"""
    d = np.array(d2row, dtype=np.float64)
    if skip is not None:
        d[skip] = np.inf
    kth = np.partition(d, k - 1)[k - 1]  # only the leaves up to the k-th smallest distance, ties included, can be among the k
    keys = sorted((float(d[i]), int(orig[i])) for i in np.nonzero(d <= kth)[0] if i != skip)
    return np.array([a for a, _ in keys[:k]]), np.array([b for _, b in keys[:k]], dtype=np.int64)


def all_dist2(pts, qry, scale=None, circ=()):
    """dist2 of every pair with the non-finite queries at 0: what `knn` and `plan` take as `d2` to share one matrix"""
    live = np.isfinite(qry).all(axis=1)
    return dist2(pts, np.where(live[:, None], qry, 0.0), scale, circ)


def knn(pts, orig, qry, k, loo=False, scale=None, circ=(), d2=None, rows=None):
    """brute force: (d2 (Nq, k), idx (Nq, k)) in processing order; a non-finite query gets NaN and 0.  `rows` (leave-one-out
    of a large density, block by block): a slice of the leaves; qry is pts[rows] and query q is leaf rows.start + q"""
    Nq = qry.shape[0]
    r0 = 0 if rows is None else rows.start
    d2o, ido = np.full((Nq, k), np.nan), np.zeros((Nq, k), dtype=np.int64)
    live = np.isfinite(qry).all(axis=1)
    if d2 is None:
        d2 = all_dist2(pts, qry, scale, circ)
    for q in np.nonzero(live)[0]:
        d2o[q], ido[q] = _topk(d2[q], orig, k, r0 + q if loo else None)
    return d2o, ido


def plan(pts, orig, qry, k, loo=False, scale=None, circ=(), d2=None, rows=None):
    """steps 1-6: dict with cstar (Nq,), r (Nq,), need (Nq, nc) bool, visited (qblocks, nc) bool and stats.  `rows` as in `knn`,
    starting at a multiple of BLOCK: the query blocks of that slice (the stats of the slices add up)"""
    r0 = 0 if rows is None else rows.start
    assert r0 % BLOCK == 0
    if d2 is None:
        d2 = all_dist2(pts, qry, scale, circ)
    N, Nq = pts.shape[0], qry.shape[0]
    lo, hi = boxes(pts)
    nc = lo.shape[0]
    live = np.isfinite(qry).all(axis=1)
    qsafe = np.where(live[:, None], qry, 0.0)
    dm = dmin2(lo, hi, qsafe, scale, circ)
    cstar, r = np.full(Nq, -1), np.full(Nq, np.inf)
    need = np.zeros((Nq, nc), dtype=bool)
    for q in np.nonzero(live)[0]:
        row = dm[q].copy()
        own = (r0 + q) // CHUNK
        if loo and min(CHUNK, N - own * CHUNK) == 1:
            row[own] = np.inf  # the own chunk holds no other leaf: it does not count
        c = int(np.argmin(row))  # (the first of equal minima: the lowest c)
        cstar[q] = c
        sl = slice(c * CHUNK, min(N, (c + 1) * CHUNK))
        near = d2[q, sl]
        keep = [i for i in range(near.shape[0]) if not (loo and sl.start + i == r0 + q)]
        if len(keep) >= k:
            r[q] = np.sort(near[keep])[k - 1]
        need[q] = dm[q] <= r[q]
    visited = np.stack([need[q0:q0 + BLOCK].any(axis=0) for q0 in range(0, Nq, BLOCK)])
    return dict(cstar=cstar, r=r, need=need, visited=visited, stats=(int(visited.sum()), int(visited.size)))


# ---- the estimators' formulas, fed with k-th neighbour distances -----------------------------------------------------------
def digamma_int(n):
    return -EULER_GAMMA + sum(1.0 / m for m in range(1, int(n)))


def log_unit_ball(D):
    return 0.5 * D * math.log(math.pi) - math.lgamma(0.5 * D + 1.0)


def entropy_kl(eps, D, k):
    """Kozachenko-Leonenko from the leave-one-out k-th neighbour distances eps (N,)"""
    N = len(eps)
    return digamma_int(N) - digamma_int(k) + log_unit_ball(D) + D / N * math.fsum(np.log(eps).tolist())


def kld_wkv(rho, nu, D, m):
    """Wang-Kulkarni-Verdu from rho (n,) within p (leave-one-out) and nu (n,) from p's points into q's m points"""
    n = len(rho)
    return D / n * math.fsum((np.log(nu) - np.log(rho)).tolist()) + math.log(m / (n - 1))
