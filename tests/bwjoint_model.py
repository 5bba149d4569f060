"""A numpy model of include/kdehip.h section 5q, written from its text: one step of the joint leave-one-out bandwidth
iteration in fp64 with a running maximum over S_i = { j : w_j > 0, j != i }, the iteration with its convergence and
degenerate tests, and the leave-one-out average log-likelihood it climbs.  No GPU.

A density is (points (D, N), weights (N,) summing to 1 -- zeros allowed --, variances (D,)); `man` is None or one 0 / 1 per
dimension (1 = circular).  The pair terms are formed in row blocks, so that N = 8193 needs no N x N array, and the sums over
the points whose order could matter are math.fsum."""
import math

import numpy as np

from tests.modes_model import log_norm, wrap

ROWS = 512  # queries per row block


def _sweep(pts, w, v, man=None):
    """per point i: (m_i, S0_i, T_ik (N, D)) over S_i; S_i empty: (-inf, 0, 0)"""
    pts = np.asarray(pts, dtype=np.float64)
    D, N = pts.shape
    w = np.asarray(w, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    circ = np.zeros(D, dtype=bool) if man is None else np.asarray(man, dtype=bool)
    src = w > 0.0
    m, S0, T = np.full(N, -np.inf), np.zeros(N), np.zeros((N, D))
    for r0 in range(0, N, ROWS):
        r1 = min(N, r0 + ROWS)
        d = pts[:, r0:r1, None] - pts[:, None, :]          # (D, rows, N): c_ik - c_jk
        for k in range(D):
            if circ[k]:
                d[k] = wrap(d[k])
        a = np.zeros((r1 - r0, N))
        for k in range(D):
            a += d[k] * d[k] * (-0.5 / v[k])
        inS = np.broadcast_to(src[None, :], a.shape).copy()
        inS[np.arange(r1 - r0), np.arange(r0, r1)] = False   # by INDEX: a duplicate stays
        am = np.where(inS, a, -np.inf)
        mm = am.max(axis=1)
        some = mm > -np.inf
        e = np.where(inS, w[None, :] * np.exp(np.where(inS, a, 0.0) - np.where(some, mm, 0.0)[:, None]), 0.0)
        m[r0:r1] = mm
        S0[r0:r1] = e.sum(axis=1)
        for k in range(D):
            T[r0:r1, k] = (e * d[k] * d[k]).sum(axis=1)
    return m, S0, T


def _logl(w, v, m, S0):
    """sum over w_i > 0 of w_i (m_i + log S0_i - log norm - log(1 - w_i)); -inf if some such S_i is empty"""
    use = w > 0.0
    if np.any(use & ~(m > -np.inf)):
        return -math.inf
    ln = log_norm(v)
    return math.fsum(float(w[i]) * (float(m[i]) + math.log(float(S0[i])) - ln - math.log(1.0 - float(w[i])))
                     for i in np.flatnonzero(use))


def loo_logl(dens, sd, man=None):
    """L at the bandwidth `sd` (standard deviations): log-domain evalAvgLogL(bd, bd), leave-one-out"""
    pts, w, _ = dens
    v = np.asarray(sd, dtype=np.float64) ** 2
    m, S0, _ = _sweep(pts, w, v, man)
    return _logl(np.asarray(w, dtype=np.float64), v, m, S0)


def step(dens, v, man=None):
    """(L(v), v_new (D,)): one sweep at the variances v.  v_new_k = (sum_Q w_i T_ik / S0_i) / W; NaN where W == 0"""
    pts, w, _ = dens
    w = np.asarray(w, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    m, S0, T = _sweep(pts, w, v, man)
    L = _logl(w, v, m, S0)
    Q = np.flatnonzero((w > 0.0) & (m > -np.inf))
    W = math.fsum(float(w[i]) for i in Q)
    vn = np.full(len(v), np.nan)
    if W > 0.0:
        for k in range(len(v)):
            vn[k] = math.fsum(float(w[i]) * float(T[i, k]) / float(S0[i]) for i in Q) / W
    return L, vn


def iterate(dens, start, tol, maxiter, man=None):
    """(bandwidth (D,) standard deviations, logl, iters, status, trace (|iters| + 1,)) from the start `start` (standard
    deviations; None: the density's own variances).  A step whose v_new has an entry that is 0 or not finite changes
    nothing: status = 1 and the iteration ends where it is."""
    v = np.asarray(dens[2], dtype=np.float64).copy() if start is None else np.asarray(start, dtype=np.float64) ** 2
    iters, status, trace = 0, 0, []
    closing = maxiter == 0
    while True:
        L, vn = step(dens, v, man)
        trace.append(L)
        if closing:
            break
        if not np.all(np.isfinite(vn) & (vn > 0.0)):
            status = 1
            break
        reach = float(np.max(np.abs(np.log(vn / v)))) / 2.0
        v = vn
        cnt = abs(iters) + 1
        conv = reach <= tol
        iters = cnt if conv else -cnt
        closing = conv or cnt >= maxiter
    return np.sqrt(v), trace[-1], iters, status, np.array(trace)


# ---- the data of the tests -------------------------------------------------------------------------------------------------
def two_clusters(D, N, seed=None):
    """(points (D, N), weights (N,) with every fifth one 0, summing to 1): two clusters of different widths per dimension"""
    rng = np.random.default_rng(1000 + 10 * D + N if seed is None else seed)
    sd = rng.uniform(0.3, 1.2, size=(D, 1))
    centre = rng.uniform(-2.0, 2.0, size=(D, 2))
    lab = rng.integers(0, 2, size=N)
    pts = centre[:, lab] + sd * rng.standard_normal((D, N)) * np.where(lab == 0, 1.0, 0.5)[None, :]
    w = rng.uniform(0.2, 1.0, size=N)
    w[::5] = 0.0
    return np.ascontiguousarray(pts), w / w.sum()


def silverman(pts):
    """a Silverman-style start: sd_k (4 / ((D + 2) N))^(1 / (D + 4))"""
    D, N = pts.shape
    return pts.std(axis=1, ddof=1) * (4.0 / ((D + 2.0) * N)) ** (1.0 / (D + 4.0))


def angle_data(N=30, shift=0.0):
    """(2, N): a Euclidean coordinate, and an angle cluster of sd 0.04 around pi - 0.08 of which exactly ONE point lies across
    the cut at +-pi.  On the circle that point is 0.1 from its neighbours; on the line it is 2 pi from all of them and alone
    (the self term is skipped), so its mean squared difference stays (2 pi)^2 whatever the bandwidth is and the angle's
    variance can never fall below (2 pi)^2 / N = 1.32: a standard deviation above 1.1."""
    rng = np.random.default_rng(9)
    ang = math.pi - 0.08 + 0.04 * rng.standard_normal(N)
    ang = np.minimum(ang, math.pi - 0.01)
    ang[N // 2] = math.pi + 0.02
    return np.vstack([rng.standard_normal(N), wrap(ang) + shift])


def improvement_data(D=6, N=300):
    """unweighted two-cluster data on which kde!(points)'s per-marginal bandwidth undersmooths the joint density"""
    rng = np.random.default_rng(62)
    lab = rng.integers(0, 2, size=N)
    centre = np.stack([np.full(D, -1.5), np.full(D, 1.5)], axis=1)
    return np.ascontiguousarray(centre[:, lab] + rng.standard_normal((D, N)) * np.where(lab == 0, 1.0, 0.6)[None, :])
