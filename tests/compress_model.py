"""Kernel herding as include/kdehip.h section 5t states it, in NumPy fp64: the model tests/test_compress_host.py pins and
tests/test_gpu_compress.py holds the kernels of csrc/compress.hip to.

It works on the points in their ORIGINAL order (the pick's tie-break is the original index, and the order of a sum is below
the tolerance the traces are compared at), forms z by row blocks and the kernel columns on demand -- no N x N matrix, so
N = 8193 costs a few megabytes --, and also returns every step's margin: the best score minus the second best among the
not-yet-chosen points (inf when one point is left)."""
import math

import numpy as np

TWO_PI = 2.0 * math.pi


def wrap(t):
    """circ_wrap of csrc/circ_wrap.hpp: to [-pi, pi)"""
    return t - TWO_PI * np.floor((t + math.pi) / TWO_PI)


def exponents(x, s, nh, man=None):
    """a(s, j) for the queries x (D, n) against the sources s (D, m): (n, m), sum_k d_k^2 nh_k with k ascending,
    d_k = x_jk - s_sk, wrapped in a circular dimension"""
    acc = np.zeros((x.shape[1], s.shape[1]))
    for k in range(x.shape[0]):
        d = x[k][:, None] - s[k][None, :]
        if man is not None and man[k]:
            d = wrap(d)
        acc = d * d * nh[k] + acc
    return acc


def kernel_mean(points, weights, var, man=None, rows=512):
    """z_j = sum_i alpha_i exp(a(i, j)), by blocks of `rows` queries"""
    pts = np.asarray(points, dtype=np.float64)
    nh = -0.5 / np.asarray(var, dtype=np.float64)
    z = np.empty(pts.shape[1])
    for j0 in range(0, pts.shape[1], rows):
        z[j0:j0 + rows] = np.exp(exponents(pts[:, j0:j0 + rows], pts, nh, man)) @ weights
    return z


def herd(points, weights, var, M, man=None, rows=512):
    """points (D, N) and weights (N) in original order, var the D kernel variances.  Returns a dict: idx (M, 1-based), zpick,
    rpick, self_sum, z (N), margin (M), mmd2 (M: the curve after 1 .. M picks)."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    N = pts.shape[1]
    assert 1 <= M <= N
    nh = -0.5 / np.asarray(var, dtype=np.float64)
    z = kernel_mean(pts, w, var, man, rows)
    self_sum = float(np.sum(w * z))
    r = np.zeros(N)
    free = np.ones(N, dtype=bool)
    idx, zpick, rpick, margin = np.zeros(M, dtype=np.int64), np.zeros(M), np.zeros(M), np.zeros(M)
    for t in range(M):
        inv = 1.0 / float(t + 1)
        score = np.where(free, z - r * inv, -np.inf)
        s = int(np.argmax(score))                     # the first maximum: ties go to the lower original index
        rest = score.copy()
        rest[s] = -np.inf
        margin[t] = score[s] - rest.max() if free.sum() > 1 else np.inf
        idx[t], zpick[t], rpick[t] = s + 1, z[s], r[s]
        free[s] = False
        r += np.exp(exponents(pts, pts[:, s:s + 1], nh, man))[:, 0]
    m = np.arange(1, M + 1, dtype=np.float64)
    mmd2 = self_sum - (2.0 / m) * np.cumsum(zpick) + (m + 2.0 * np.cumsum(rpick)) / (m * m)
    return dict(idx=idx, zpick=zpick, rpick=rpick, self_sum=self_sum, z=z, margin=margin, mmd2=mmd2)


def mmd2_direct(points, weights, chosen, var, man=None):
    """the squared MMD (not normalised) between (points, weights) and the equal-weight density on points[:, chosen], summed
    term by term: what the curve's last entry must equal"""
    pts = np.asarray(points, dtype=np.float64)
    nh = -0.5 / np.asarray(var, dtype=np.float64)
    q = pts[:, chosen]
    u = np.full(q.shape[1], 1.0 / q.shape[1])
    pp = float(weights @ np.exp(exponents(pts, pts, nh, man)) @ weights)
    pq = float(weights @ np.exp(exponents(pts, q, nh, man)) @ u)
    qq = float(u @ np.exp(exponents(q, q, nh, man)) @ u)
    return pp - 2.0 * pq + qq


def two_clusters(D, N, seed=None, grid=None):
    """(points (D, N), weights): two clusters of different widths, weights uniform in [0.5, 1.5] with every fifth one 0,
    normalised; grid: every coordinate rounded to a multiple of it"""
    rng = np.random.default_rng(4000 + 100 * D + N if seed is None else seed)
    centre = rng.uniform(-2.0, 2.0, size=(D, 2))
    lab = rng.integers(0, 2, size=N)
    pts = centre[:, lab] + rng.standard_normal((D, N)) * np.where(lab == 0, 0.8, 0.4)[None, :]
    if grid is not None:
        pts = np.round(pts / grid) * grid
    w = rng.uniform(0.5, 1.5, size=N)
    w[::5] = 0.0
    return np.ascontiguousarray(pts), w / w.sum()


def cut_pair(N=150, centre=math.pi - 0.1, seed=23):
    """a 2-D density on R x S1 whose angles straddle the cut at +-pi: (points, weights)"""
    rng = np.random.default_rng(seed)
    pts = np.vstack([rng.standard_normal(N), wrap(centre + 0.3 * rng.standard_normal(N))])
    w = rng.uniform(0.5, 1.5, size=N)
    w[::5] = 0.0
    return np.ascontiguousarray(pts), w / w.sum()
