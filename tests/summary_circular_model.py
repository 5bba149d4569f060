"""NumPy restatement of include/kdehip.h section 5e: the summaries of a density whose dimensions may be circular -- the CPU
model of tests/test_summary_circular_host.py, tests/test_gpu_summary_circular.py and tests/test_gpu_sample_circular.py.

Written from the header's text operation by operation: the wrap is the scalar expression tests/pymodel.py shares with the
library (applied element by element, no second formula), every sum is a Python loop from +0.0 in original order, grid() is
the one section 5c defines.  Points are (D, N) in original order; manifold is one 0 / 1 per dimension."""
import math

import numpy as np

from tests.pymodel import TWO_PI, wrapRad

PI = math.pi
_wrap = np.frompyfunc(wrapRad, 1, 1)


def wrap(t):
    return np.asarray(_wrap(np.asarray(t, dtype=np.float64)), dtype=np.float64)


def grid(lo, hi, N):
    """section 5c: x_k = lo + k h, h = (hi - lo) / (N - 1), x_{N-1} = hi, every operation rounded on its own"""
    lo, hi = np.float64(lo), np.float64(hi)
    h = (hi - lo) / np.float64(N - 1)
    x = np.array([lo + np.float64(k) * h for k in range(N)], dtype=np.float64)
    x[-1] = hi
    return x


def seqsum(v):
    s = np.float64(0.0)
    for x in v:
        s = s + np.float64(x)
    return s


def offsets(x, circular):
    """(a0, t) of one dimension: the reference angle (original point 1) and the tangent offsets; Euclidean: (None, x)"""
    x = np.asarray(x, dtype=np.float64)
    if not circular:
        return None, x
    a0 = x[0]
    return a0, wrap(x - a0)


def mean(points, manifold):
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    mu = np.empty(D)
    for k in range(D):
        a0, t = offsets(points[k], manifold[k])
        m = seqsum(t) / np.float64(N)
        mu[k] = wrapRad(float(a0 + m)) if manifold[k] else m
    return mu


def residuals(points, manifold, mu):
    r = np.asarray(points, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[:, None]
    for k in range(r.shape[0]):
        if manifold[k]:
            r[k] = wrap(r[k])
    return r


def fit(points, manifold):
    """(mu, Sigma): Sigma in np.longdouble from the fp64 residuals (the library sums in fp64: a tolerance)"""
    mu = mean(points, manifold)
    r = residuals(points, manifold, mu).astype(np.longdouble)
    return mu, (r @ r.T) / np.longdouble(r.shape[1])


def krange(points, manifold, extend):
    """(D, 2): per dimension (lo - dr, hi + dr); circular: the arc (a0 + lo_t - dr, a0 + hi_t + dr), unwrapped, and
    (mid - pi, mid + pi) around the midpoint of the unextended arc when it is longer than 2 pi"""
    points = np.asarray(points, dtype=np.float64)
    out = np.empty((points.shape[0], 2))
    ext = np.float64(extend)
    for k in range(points.shape[0]):
        a0, t = offsets(points[k], manifold[k])
        lo, hi = np.min(t), np.max(t)
        dr = ext * (hi - lo)
        if not manifold[k]:
            out[k] = lo - dr, hi + dr
            continue
        alo, ahi = a0 + lo, a0 + hi
        rlo, rhi = alo - dr, ahi + dr
        if rhi - rlo > np.float64(TWO_PI):
            mid = np.float64(0.5) * (alo + ahi)
            rlo, rhi = mid - np.float64(PI), mid + np.float64(PI)
        out[k] = rlo, rhi
    return out


def grid_values(points, weights, var1, manifold, Ngrid, extend=0.1):
    """getKDEMax's grids and values per dimension, the values in np.longdouble: weights w / sum(w), variance fl(sqrt(v_1))^2,
    norm sqrt(2 pi) sqrt(variance), the difference x - c_i wrapped in a circular dimension.  var1: the variances of original
    point 1 (D).  Returns (xs (D, Ngrid) float64 unwrapped, values (D, Ngrid) longdouble)."""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    w = w.astype(np.longdouble) / w.astype(np.longdouble).sum()
    rng = krange(points, manifold, extend)
    xs = np.empty((D, Ngrid))
    vals = np.empty((D, Ngrid), dtype=np.longdouble)
    for k in range(D):
        xs[k] = grid(rng[k, 0], rng[k, 1], Ngrid)
        sd = np.sqrt(np.float64(var1[k]))
        v = np.longdouble(sd * sd)
        d = xs[k][:, None] - points[k][None, :]
        if manifold[k]:
            d = wrap(d)
        d = d.astype(np.longdouble)
        vals[k] = (np.exp(-d * d / (2 * v)) * w[None, :]).sum(axis=1) / np.sqrt(2 * np.longdouble(np.pi) * v)
    return xs, vals


def argmax(xs, vals, manifold):
    """wrap(x_k) (x_k itself in a Euclidean dimension) of the first maximal k, per dimension"""
    out = np.empty(xs.shape[0])
    for k in range(xs.shape[0]):
        x = xs[k][int(np.argmax(vals[k]))]
        out[k] = wrapRad(float(x)) if manifold[k] else x
    return out


def top_two_gap(vals):
    """per dimension (largest - second largest grid value) / largest"""
    s = np.sort(np.asarray(vals), axis=1)
    return (s[:, -1] - s[:, -2]) / s[:, -1]


def inters(points_p, manifold, Ngrid, evaluate_p, evaluate_q):
    """intersIntgAppxIS, D = 1, 2: the grids over p's range with extend 0.3, dx_d = x_1 - x_0; evaluate_p / evaluate_q
    map (D, Nq) positions to values (the library's evaluateDualTree(..., manifold=)); the sums by math.fsum"""
    points_p = np.asarray(points_p, dtype=np.float64)
    D = points_p.shape[0]
    rng = krange(points_p, manifold, 0.3)
    xs = [grid(rng[d, 0], rng[d, 1], Ngrid) for d in range(D)]
    dx = [x[1] - x[0] for x in xs]
    if D == 1:
        pos = xs[0][None, :]
        return math.fsum(evaluate_p(pos) * evaluate_q(pos)) * dx[0]
    pos = np.stack([np.tile(xs[0], Ngrid), np.repeat(xs[1], Ngrid)])  # row i = (x1_j, x2_i)
    return math.fsum(evaluate_p(pos) * evaluate_q(pos)) * dx[0] * dx[1]
