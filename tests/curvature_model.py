"""A numpy model of include/kdehip.h section 5k, written from its text: tests/modes_model.py's moments extended by the second
moments S_kl = sum_{i in S} t_i d_ik d_il and their absolute sums A_kl = sum_{i in S} t_i |d_ik d_il| (math.fsum), the
Hessian of log p they give, and its inverse by numpy.linalg.inv.  No GPU.

A density is (points (D, N), weights (N,), variances (D,)); `man` is None or one 0 / 1 per dimension (1 = circular)."""
import math

import numpy as np

from tests import modes_model as mm


def moments2(dens, x, man=None, fma=False):
    """(m, S_0, S (D,), A (D,), S2 (D, D), A2 (D, D)) at one query: modes_model.moments and, with t_i = w_i e^{a_i - m},
    S2_kl = sum t_i d_ik d_il and A2_kl = sum t_i |d_ik d_il|, the scale of the signed sum.  S empty: (-inf, 0, zeros)."""
    pts, w, v = dens
    D = pts.shape[0]
    d = mm.differences(x, pts, man)
    a = mm.exponents(d, v, fma)
    inS = np.asarray(w) > 0.0
    if not inS.any():
        return -math.inf, 0.0, np.zeros(D), np.zeros(D), np.zeros((D, D)), np.zeros((D, D))
    m = float(np.max(a[inS]))
    t = np.where(inS, w * np.exp(np.where(inS, a - m, 0.0)), 0.0)
    S0 = math.fsum(t.tolist())
    S = np.array([math.fsum((t * d[k]).tolist()) for k in range(D)])
    A = np.array([math.fsum((t * np.abs(d[k])).tolist()) for k in range(D)])
    S2, A2 = np.zeros((D, D)), np.zeros((D, D))
    for k in range(D):
        for l in range(k, D):
            S2[k, l] = S2[l, k] = math.fsum((t * d[k] * d[l]).tolist())
            A2[k, l] = A2[l, k] = math.fsum((t * np.abs(d[k] * d[l])).tolist())
    return m, S0, S, A, S2, A2


def hessian(dens, x, man=None, fma=False):
    """(log p, g (D,), gscale (D,), H (D, D), hscale (D, D)) at one query:
        g_k = -S_k / (S_0 v_k),  H_kl = S_kl / (S_0 v_k v_l) - delta_kl / v_k - g_k g_l
    gscale_k = A_k / (S_0 v_k) and hscale_kl = A_kl / (S_0 v_k v_l) + delta_kl / v_k + gscale_k gscale_l are what the roundings
    of the signed sums are relative to.  S empty: (-inf, 0, 0, 0, 0)."""
    v = np.asarray(dens[2], dtype=np.float64)
    D = len(v)
    m, S0, S, A, S2, A2 = moments2(dens, x, man, fma)
    if S0 == 0.0:
        return -math.inf, np.zeros(D), np.zeros(D), np.zeros((D, D)), np.zeros((D, D))
    lp = m + math.log(S0) - mm.log_norm(v)
    g, gs = -S / (S0 * v), A / (S0 * v)
    vv = np.outer(v, v)
    H = S2 / (S0 * vv) - np.diag(1.0 / v) - np.outer(g, g)
    hs = A2 / (S0 * vv) + np.diag(1.0 / v) + np.outer(gs, gs)
    return lp, g, gs, H, hs


def evaluate_hess(dens, X, man=None, fma=False):
    """(logp (Nq,), grad (D, Nq), gscale (D, Nq), hess (D, D, Nq), hscale (D, D, Nq)) at the columns of X"""
    D, Nq = X.shape
    logp, grad, gs = np.zeros(Nq), np.zeros((D, Nq)), np.zeros((D, Nq))
    hess, hs = np.zeros((D, D, Nq)), np.zeros((D, D, Nq))
    for q in range(Nq):
        logp[q], grad[:, q], gs[:, q], hess[:, :, q], hs[:, :, q] = hessian(dens, X[:, q], man, fma)
    return logp, grad, gs, hess, hs


def laplace(dens, X, man=None):
    """(cov (D, D, Nq), definite (Nq,)): cov = (-H)^-1 by numpy.linalg.inv where every eigenvalue of -H is > 0, else NaN"""
    D, Nq = X.shape
    cov, definite = np.full((D, D, Nq), np.nan), np.zeros(Nq, dtype=bool)
    for q in range(Nq):
        lp, _, _, H, _ = hessian(dens, X[:, q], man)
        if lp > -math.inf and np.all(np.linalg.eigvalsh(-H) > 0.0):
            cov[:, :, q] = np.linalg.inv(-H)
            definite[q] = True
    return cov, definite


def cov_bound(H, cov):
    """(kappa_2(H), 64 * 2^-53 * kappa_2(H) * max|cov|): the c D u kappa bound of a Cholesky inverse with c D = 64 at D <= 8"""
    kappa = float(np.linalg.cond(H, 2))
    return kappa, 64.0 * 2.0 ** -53 * kappa * float(np.max(np.abs(cov)))
