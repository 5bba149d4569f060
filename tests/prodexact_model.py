"""A numpy model of include/kdehip.h section 5p, written from its text: the exact product of two Gaussian-kernel densities
in fp64 with running maxima over S_q = { j : beta_j > 0 } and S_p = { i : alpha_i > 0 } and exactly rounded sums
(math.fsum), log int p q, the two labels of every draw by inverse CDFs in leaf order (the cumulative sums in extended
precision: they stand for the header's exact ones), the drawn points, and the mixture itself.  No GPU.

A density is (points (D, N), weights (N,), variances (D,)) IN LEAF ORDER with `perm` (N,), the 1-based original index of
every leaf, where labels are asked for.  The uniforms (Np, 2) and normals (Np, D) of a call come from the library's host
Philox twin, kdehip.philox_streams(seed, sample_offset, Np, 2, D)."""
import math

import numpy as np

from tests.modes_model import exponents

TWO_PI = 2.0 * math.pi


def log_norm(s):
    """log((2 pi)^(D/2) prod_k sqrt(s_k))"""
    return 0.5 * len(s) * math.log(TWO_PI) + 0.5 * math.fsum(math.log(t) for t in s)


def pair_exponents(p, q, fma=False):
    """e (N1, N2): e_ij = sum_k (a_ik - b_jk)^2 * (-0.5 / s_k), k ascending (fma: as modes_model.exponents)"""
    (A, _, u), (B, _, v) = p, q
    s = np.asarray(u) + np.asarray(v)
    return np.stack([exponents(A[:, i][:, None] - B, s, fma) for i in range(A.shape[1])])


def rows(p, q, fma=False, e=None):
    """(e, m (N1,), T (N1,), L (N1,)): m_i = max_{S_q} e_ij, T_i = sum_{S_q} beta_j e^{e_ij - m_i} (exactly rounded),
    L_i = log alpha_i + m_i + log T_i, -inf outside S_p; S_q empty: m = -inf, T = 0, L = -inf"""
    alpha, beta = np.asarray(p[1]), np.asarray(q[1])
    e = pair_exponents(p, q, fma) if e is None else e
    N1 = len(alpha)
    inq = beta > 0.0
    m, T, L = np.full(N1, -math.inf), np.zeros(N1), np.full(N1, -math.inf)
    if not inq.any():
        return e, m, T, L
    for i in range(N1):
        m[i] = float(np.max(e[i, inq]))
        T[i] = math.fsum((beta[inq] * np.exp(e[i, inq] - m[i])).tolist())
        if alpha[i] > 0.0:
            L[i] = math.log(alpha[i]) + m[i] + math.log(T[i])
    return e, m, T, L


def totals(L):
    """(M, R_i (N1,), R): M = max L_i, R_i = e^{L_i - M} (0 where L_i = -inf), R their exactly rounded sum"""
    M = float(np.max(L)) if len(L) else -math.inf
    if M == -math.inf:
        return M, np.zeros(len(L)), 0.0
    Ri = np.where(L > -math.inf, np.exp(np.where(L > -math.inf, L - M, 0.0)), 0.0)
    return M, Ri, math.fsum(Ri.tolist())


def logz(p, q, fma=False, L=None):
    """log int p q = M + log R - log((2 pi)^(D/2) prod sqrt(s_k)); -inf when S_p or S_q is empty"""
    L = rows(p, q, fma)[3] if L is None else L
    M, _, R = totals(L)
    return -math.inf if R == 0.0 else M + math.log(R) - log_norm(np.asarray(p[2]) + np.asarray(q[2]))


def _inverse_cdf(t, inS, u):
    """(leaf, gap): the first leaf of S whose cumulative sum of t exceeds u * total (the last leaf of S if none) and the
    relative distance of the threshold to the nearest boundary between two leaves of S (the last value is no boundary)"""
    C = np.cumsum(t[inS].astype(np.longdouble))
    thr = np.longdouble(u) * C[-1]
    above = np.flatnonzero(C > thr)
    leaf = int(inS[above[0]]) if len(above) else int(inS[-1])
    gap = float(np.min(np.abs(C[:-1] - thr)) / C[-1]) if len(C) > 1 else math.inf
    return leaf, gap


def draw_labels(p, perm_p, q, perm_q, U, fma=False, pre=None):
    """(ind (Np, 2), leaves (Np, 2), gap (Np,)) for the uniforms U (Np, 2): i by the inverse CDF of R over S_p with U[:, 0],
    j by the inverse CDF of beta_j e^{e_ij - m_i} over S_q with U[:, 1]; ind the 1-based original indices, gap the smaller
    of the two relative distances to a boundary.  S_p or S_q empty: ind 0, leaves -1, gap inf."""
    U = np.asarray(U, dtype=np.float64).reshape(-1, 2)
    Np = U.shape[0]
    alpha, beta = np.asarray(p[1]), np.asarray(q[1])
    e, m, T, L = rows(p, q, fma) if pre is None else pre
    _, Ri, R = totals(L)
    ind, leaves, gap = np.zeros((Np, 2), dtype=np.int64), np.full((Np, 2), -1, dtype=np.int64), np.full(Np, math.inf)
    if R == 0.0:
        return ind, leaves, gap
    inp, inq = np.flatnonzero(alpha > 0.0), np.flatnonzero(beta > 0.0)
    for t in range(Np):
        i, g0 = _inverse_cdf(Ri, inp, U[t, 0])
        tj = np.zeros(len(beta))
        tj[inq] = beta[inq] * np.exp(e[i, inq] - m[i])
        j, g1 = _inverse_cdf(tj, inq, U[t, 1])
        leaves[t] = (i, j)
        ind[t] = (perm_p[i], perm_q[j])
        gap[t] = min(g0, g1)
    return ind, leaves, gap


def component_mean(a, b, u, v):
    """a + (b - a) u / s, per dimension"""
    u, v = np.asarray(u), np.asarray(v)
    return a + (b - a) * (u / (u + v))


def points(p, q, leaves, normals):
    """pts (Np, D): the mean of component (i, j) plus sqrt(u v / s) n; NaN where a label is -1"""
    (A, _, u), (B, _, v) = p, q
    u, v = np.asarray(u), np.asarray(v)
    sd = np.sqrt(u * v / (u + v))
    out = np.full((len(leaves), A.shape[0]), math.nan)
    for t, (i, j) in enumerate(leaves):
        if i >= 0 and j >= 0:
            out[t] = component_mean(A[:, i], B[:, j], u, v) + sd * np.asarray(normals)[t]
    return out


def components(p, q, fma=False):
    """(means (N1 N2, D), weights (N1 N2,), var (D,)) in the ORDER THE DENSITIES ARE GIVEN IN (pass original-order arrays
    for the library's layout): component c = i N2 + j, weight e^{(log alpha_i + log beta_j + e_ij) - (M + log R)}, 0
    outside S_p x S_q"""
    (A, alpha, u), (B, beta, v) = p, q
    alpha, beta, u, v = np.asarray(alpha), np.asarray(beta), np.asarray(u), np.asarray(v)
    e, _, _, L = rows(p, q, fma)
    M, _, R = totals(L)
    N1, N2, D = A.shape[1], B.shape[1], A.shape[0]
    means = np.zeros((N1 * N2, D))
    w = np.zeros(N1 * N2)
    for i in range(N1):
        for j in range(N2):
            c = i * N2 + j
            means[c] = component_mean(A[:, i], B[:, j], u, v)
            if alpha[i] > 0.0 and beta[j] > 0.0 and R > 0.0:
                w[c] = math.exp((math.log(alpha[i]) + math.log(beta[j]) + e[i, j]) - (M + math.log(R)))
    return means, w, u * v / (u + v)


def mixture_moments(p, q):
    """(mean (D,), var (D,)) of the product as a distribution: the mixture's mean, and its per-dimension variance
    u v / s + sum_c w_c (mean_c - mean)^2"""
    means, w, var = components(p, q)
    mu = np.array([math.fsum((w * means[:, k]).tolist()) for k in range(means.shape[1])])
    va = np.array([var[k] + math.fsum((w * (means[:, k] - mu[k]) ** 2).tolist()) for k in range(means.shape[1])])
    return mu, va
