"""A numpy model of include/kdehip.h section 5i, written from its text: the weights of a Gaussian-kernel density conditioned
on some of its dimensions in fp64 with a running maximum over S = { i : w_i > 0 } and exactly rounded sums (math.fsum), the
log of the normaliser, the conditional mean and per-dimension variance, and the label of the one draw per query by the
inverse CDF in leaf order (the cumulative sums in extended precision: they stand for the header's exact ones).  No GPU.

A density is (points (D, N), weights (N,), variances (D,)) IN LEAF ORDER with `perm` (N,), the 1-based original index of
every leaf, where labels are asked for; `gdims` are the given dimensions, ascending; a query y has one value per given
dimension in that order; `man` is None or one 0 / 1 per dimension of the density (1 = circular)."""
import math

import numpy as np

from tests.modes_model import _circ, exponents, wrap

TWO_PI = 2.0 * math.pi


def free_dims(D, gdims):
    return [k for k in range(D) if k not in gdims]


def log_norm(v, gdims):
    """log((2 pi)^(ng/2) prod_{k in G} sqrt(v_k))"""
    return 0.5 * len(gdims) * math.log(TWO_PI) + 0.5 * math.fsum(math.log(v[k]) for k in gdims)


def terms(dens, gdims, y, man=None, fma=False):
    """(m, t (N,), S_0): a_i over the given dimensions (k ascending; fma as modes_model.exponents), m = max_S a_i,
    t_i = w_i e^{a_i - m} (0 outside S), S_0 = their exactly rounded sum.  S empty: (-inf, zeros, 0)."""
    pts, w, v = dens
    g = list(gdims)
    d = np.asarray(y, dtype=np.float64)[:, None] - pts[g]
    c = _circ(man, pts.shape[0])[g]
    if c.any():
        d[c] = wrap(d[c])
    a = exponents(d, np.asarray(v)[g], fma)
    inS = np.asarray(w) > 0.0
    if not inS.any():
        return -math.inf, np.zeros(len(w)), 0.0
    m = float(np.max(a[inS]))
    t = np.where(inS, w * np.exp(np.where(inS, a - m, 0.0)), 0.0)
    return m, t, math.fsum(t.tolist())


def logz(dens, gdims, y, man=None, fma=False):
    m, _, S0 = terms(dens, gdims, y, man, fma)
    return -math.inf if S0 == 0.0 else m + math.log(S0) - log_norm(dens[2], gdims)


def weights(dens, gdims, y, man=None):
    """omega (N,) in the density's own (leaf) order; S empty: zeros"""
    _, t, S0 = terms(dens, gdims, y, man)
    return t / S0 if S0 > 0.0 else t


def moments(dens, gdims, y, man=None):
    """(logz, mean (nf,), var (nf,)): mean_k = sum omega_i c_ik, var_k = v_k + sum omega_i (c_ik - mean_k)^2, k in F
    ascending; S empty: (-inf, NaN, NaN)"""
    pts, w, v = dens
    F = free_dims(pts.shape[0], gdims)
    m, t, S0 = terms(dens, gdims, y, man)
    if S0 == 0.0:
        return -math.inf, np.full(len(F), math.nan), np.full(len(F), math.nan)
    om = t / S0
    mean = np.array([math.fsum((om * pts[k]).tolist()) for k in F])
    var = np.array([v[k] + math.fsum((om * (pts[k] - mu) ** 2).tolist()) for k, mu in zip(F, mean)])
    return m + math.log(S0) - log_norm(v, gdims), mean, var


def draw_label(dens, perm, gdims, y, u, man=None):
    """(ind, leaf, gap): the first leaf i of S with C_i > u S_0, C_i = sum_{j <= i, j in S} t_j in leaf order -- the last leaf
    of S if none --, ind its 1-based original index, and gap = min_i |u S_0 - C_i| / S_0 over the boundaries between leaves
    of S (the last one, C = S_0, is no boundary: nothing lies beyond it).  S empty: (0, -1, inf)."""
    _, t, S0 = terms(dens, gdims, y, man)
    if S0 == 0.0:
        return 0, -1, math.inf
    inS = np.flatnonzero(np.asarray(dens[1]) > 0.0)
    C = np.cumsum(t[inS].astype(np.longdouble))
    T = np.longdouble(u) * C[-1]
    above = np.flatnonzero(C > T)
    leaf = int(inS[above[0]]) if len(above) else int(inS[-1])
    gap = float(np.min(np.abs(C[:-1] - T)) / C[-1]) if len(C) > 1 else math.inf
    return int(perm[leaf]), leaf, gap


def log_normal_mixture(pts, w, v, x):
    """log sum_i w_i N(x; c_i, diag v) of the mixture (pts (D, N), w (N,), v (D,)) at one point, by log-sum-exp"""
    d = np.asarray(x, dtype=np.float64)[:, None] - pts
    a = exponents(d, np.asarray(v))
    inS = np.asarray(w) > 0.0
    m = float(np.max(a[inS]))
    S0 = math.fsum((np.where(inS, w * np.exp(np.where(inS, a - m, 0.0)), 0.0)).tolist())
    return m + math.log(S0) - log_norm(v, list(range(len(v))))
