"""NumPy fp64 model of log-domain evaluation (include/kdehip.h section 5f), the CPU reference of
tests/test_logdensity_host.py and tests/test_gpu_logdensity.py: log p by log-sum-exp with an explicit max-shift over the
weighted sources only, no scipy.  The difference operator (and with it the wrap) is tests/circular_model.py's.

Densities are plain arrays, as in tests/circular_model.py: points (D, N), weights (N, any scale, zeros allowed; None =
uniform), bw = per-dimension VARIANCES (D)."""
import math

import numpy as np

from tests.circular_model import diff, normalise


def exponents(points, bw, pos, manifold=None):
    """a[q, i] = sum_k d_ik^2 * (-0.5 / v_k), d = diffop_k(x_qk, c_ik)"""
    points = np.asarray(points, dtype=np.float64)
    D = points.shape[0]
    bw = np.asarray(bw, dtype=np.float64)
    man = [0] * D if manifold is None else list(manifold)
    pos = np.asarray(pos, dtype=np.float64).reshape(D, -1)
    a = np.zeros((pos.shape[1], points.shape[1]))
    for k in range(D):
        d = diff(pos[k][:, None], points[k][None, :], man[k])
        a += d * d * (-0.5 / bw[k])
    return a


def eval_log(points, weights, bw, pos=None, manifold=None, loo=False, rows=None):
    """log p[q] = m + log(sum_{i in S} w_i exp(a_i - m)) - log(norm) [- log(1 - w_q)], m = max_{i in S} a_i,
    S = {i : w_i > 0} (loo: and i != q); S empty gives -inf.  rows: a slice of the queries -- the values of those alone (a
    large leave-one-out is evaluated block by block, never as one N x N array)."""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    w = normalise(weights, N)
    bw = np.asarray(bw, dtype=np.float64)
    pos = points if loo else np.asarray(pos, dtype=np.float64).reshape(D, -1)
    qs = np.arange(pos.shape[1])[slice(None) if rows is None else rows]
    a = exponents(points, bw, pos[:, qs], manifold)
    inS = np.broadcast_to(w[None, :] > 0.0, a.shape).copy()
    if loo:
        inS[np.arange(qs.size), qs] = False
    lognorm = math.log((2.0 * math.pi) ** (D / 2.0) * np.prod(np.sqrt(bw)))
    out = np.full(a.shape[0], -np.inf)
    for r, q in enumerate(qs):
        s = inS[r]
        if not s.any():
            continue
        m = a[r, s].max()
        out[r] = m + math.log(float(np.sum(w[s] * np.exp(a[r, s] - m)))) - lognorm
        if loo:
            out[r] -= math.log(1.0 - w[q])
    return out


def avg_logl_log(logp, W):
    """sum over W != 0 of W log p; -inf only if such a log p is -inf.  Returns (value, max |log p| over W != 0)."""
    logp, W = np.asarray(logp, dtype=np.float64), np.asarray(W, dtype=np.float64)
    use = W != 0.0
    if np.any(np.isneginf(logp[use])):
        return -np.inf, 0.0
    return float(np.dot(logp[use], W[use])), float(np.abs(logp[use]).max()) if use.any() else 0.0


def eval_avg_logl_log(p, q=None, manifold=None):
    """log-domain evalAvgLogL(p, q); p, q = (points, weights, bw); q None: the same object, leave-one-out"""
    if q is None:
        return avg_logl_log(eval_log(p[0], p[1], p[2], manifold=manifold, loo=True),
                            normalise(p[1], np.asarray(p[0]).shape[1]))
    return avg_logl_log(eval_log(p[0], p[1], p[2], q[0], manifold=manifold), normalise(q[1], np.asarray(q[0]).shape[1]))


def kld_log(p, q, manifold=None):
    """kld(p, q) = evalAvgLogL(p, p) [leave-one-out] - evalAvgLogL(q, p), both in the log domain"""
    return eval_avg_logl_log(p, None, manifold)[0] - eval_avg_logl_log(q, p, manifold)[0]
