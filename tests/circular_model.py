"""NumPy restatement of the reference's evaluation, log-likelihood and bandwidth search with a per-dimension `diffop`
(0 = Euclidean a - b, 1 = circular wrapRad(a - b), tests/pymodel.py) -- the CPU model of tests/test_circular_host.py and
tests/test_gpu_circular.py.  Written from the reference lines cited per function; with an all-Euclidean manifold it is
pinned against oracle.eval_direct and oracle.auto_bandwidth (tests/test_circular_host.py).

Densities are plain arrays: points (D, N), weights (N, any scale), bw = per-dimension VARIANCES (D)."""
import math

import numpy as np

from tests.pymodel import wrapRad

_wrap = np.frompyfunc(wrapRad, 1, 1)  # the scalar expression itself, element by element: no second formula


def diff(a, b, circular):
    """diffop[k](a, b) of src/DualTree01.jl:14-47: a - b, wrapped in a circular dimension"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return _wrap(d).astype(np.float64) if circular else d


def normalise(weights, N):
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    return w / w.sum()


def eval_direct(points, weights, bw, pos=None, manifold=None, loo=False, rows=None):
    """evalDirect -> maxDistKer! -> distGauss! (src/DualTree01.jl:14-47, 130-162) with the normalisation of evaluate
    (:325-335, untouched by the operators): p[q] = sum_i w_i exp(-1/2 sum_k diffop_k(x_qk, c_ik)^2 / bw_k) / norm; loo:
    at the density's own points without the self term (:141), divided by (1 - w_q) (:335).  rows: a slice of the queries --
    the values of those alone (a large leave-one-out is evaluated block by block, never as one N x N array)."""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    w = normalise(weights, N)
    bw = np.asarray(bw, dtype=np.float64)
    man = [0] * D if manifold is None else list(manifold)
    pos = points if loo else np.asarray(pos, dtype=np.float64).reshape(D, -1)
    q = np.arange(pos.shape[1])[slice(None) if rows is None else rows]
    pos = pos[:, q]
    acc = np.zeros((pos.shape[1], N))
    for k in range(D):
        d = diff(pos[k][:, None], points[k][None, :], man[k])
        acc += d * d * (-0.5 / bw[k])
    K = np.exp(acc) * w[None, :]
    if loo:
        K[np.arange(q.size), q] = 0.0
    norm = (2.0 * math.pi) ** (D / 2.0) * np.prod(np.sqrt(bw))
    p = K.sum(axis=1) / norm
    return p / (1.0 - w[q]) if loo else p


def avg_logl(L, W):
    """evalAvgLogL's rule on L and W (src/DualTree01.jl:456-466): an L == 0 with W != 0 makes it -Inf, the other zeros count
    as log 1.  Returns (value, sum |W log L|) -- the second is the tolerance scale tests/test_gpu_loglik.py uses."""
    L, W = np.asarray(L, dtype=np.float64), np.asarray(W, dtype=np.float64)
    zero = L == 0.0
    if np.any(W[zero] != 0.0):
        return -np.inf, 0.0
    logs = np.log(np.where(zero, 1.0, L))
    return float(np.dot(logs, W)), float(np.dot(np.abs(logs), np.abs(W)))


def eval_avg_logl(p, q=None, manifold=None):
    """evalAvgLogL(p, q) (:450-470); p, q = (points, weights, bw); q None: the same object, leave-one-out."""
    if q is None:
        L = eval_direct(p[0], p[1], p[2], manifold=manifold, loo=True)
        return avg_logl(L, normalise(p[1], np.asarray(p[0]).shape[1]))
    L = eval_direct(p[0], p[1], p[2], q[0], manifold=manifold)
    return avg_logl(L, normalise(q[1], np.asarray(q[0]).shape[1]))


# ---- kde!(points, addop, diffop) -> ksize -> golden -> nLOO_LL (src/KDE01.jl:3-27, src/CrossValidation.jl:15-120) -------
def _interval_stats(xs, lo, hi, ranges):
    """calcStatsBall! (src/BallTree01.jl:282-336) on the median-split 1-D tree of buildBall! (:371-394): every node is a rank
    interval [lo, hi] of the sorted marginal; returns (centre, half range) and collects the internal nodes' half ranges"""
    if lo == hi:
        return xs[lo], 0.0
    n = len(xs)
    split = ((lo + n + 1) + (hi + n + 1)) // 2 - (n + 1)  # the rounding on the reference's 1-based leaf ids
    cL, rL = _interval_stats(xs, lo, split, ranges)
    cR, rR = _interval_stats(xs, split + 1, hi, ranges)
    top, bottom = max(cL + rL, cR + rR), min(cL - rL, cR - rR)
    half = (top - bottom) / 2.0
    ranges.append(half)
    return bottom + half, half


def neighbor_min_max(x):
    """neighborMinMax (src/CrossValidation.jl:100-108) of the 1-D marginal's tree, which marginal(p, [i]) builds with the
    DEFAULT operators: Euclidean whatever the manifold"""
    xs = [float(v) for v in np.sort(np.asarray(x, dtype=np.float64))]
    ranges = []
    _, root = _interval_stats(xs, 0, len(xs) - 1, ranges)
    maxm = math.sqrt((2.0 * root) * (2.0 * root))
    minm = min(math.sqrt((2.0 * r) * (2.0 * r)) for r in ranges)
    return minm, maxm


def ksize_1d(x, circular):
    """ksize (src/CrossValidation.jl:110-120) of one marginal: golden (:44-98) over nLOO_LL (:15-24), whose entropy
    (src/DualTree01.jl:505-508) takes the operators.  Returns (standard deviation, evaluations, trace): the trace lists
    (x1, x2, f1, f2) at every comparison golden makes -- the near-tie check of the tests reads it."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    minm, maxm = neighbor_min_max(x)
    minm = max(minm, 1e-6)
    mid = (minm + maxm) / 2.0
    state = {"b": mid * mid, "n": 0}
    pts = x.reshape(1, N)
    # weights: ones -> / N (kde!(points, [1.0])) -> renormalised by the marginal's kde! (src/KDE01.jl:46, 152)
    w0 = np.full(N, 1.0 / N)
    w1 = w0 / np.cumsum(w0)[-1]

    def nloo(alpha):
        a2 = alpha * alpha
        b = state["b"] * a2  # bandwidth *= alpha^2 ... /= alpha^2: the reference's drift
        ll, _ = avg_logl(eval_direct(pts, w1, [b], manifold=[circular], loo=True), w1)
        state["b"] = b / a2
        state["n"] += 1
        return -ll

    ax, bx, cx, tol = 2.0 * minm / (minm + maxm), 1.0, 2.0 * maxm / (minm + maxm), 1e-2
    C = (3.0 - math.sqrt(5.0)) / 2.0
    R = 1.0 - C
    x0, x3 = ax, cx
    if abs(cx - bx) > abs(bx - ax):
        x1, x2 = bx, bx + C * (cx - bx)
    else:
        x1, x2 = bx - C * (bx - ax), bx
    f1, f2 = nloo(x1), nloo(x2)
    trace = []
    while abs(x3 - x0) > tol * (abs(x1) + abs(x2)):
        trace.append((x1, x2, f1, f2))
        if f2 < f1:
            x0, x1 = x1, x2
            x2 = R * x1 + C * x3
            f1, f2 = f2, nloo(x2)
        else:
            x3, x2 = x2, x1
            x1 = R * x2 + C * x0
            f2, f1 = f1, nloo(x1)
    trace.append((x1, x2, f1, f2))
    ks = (x1 if f1 < f2 else x2) * (minm + maxm) / 2.0
    return math.sqrt(ks * ks), state["n"], trace


def auto_bandwidth(points, manifold=None):
    """kde!(points, addop, diffop)'s bandwidth (src/KDE01.jl:3-27): per dimension, ksize of the marginal.  Returns
    (bw[D] standard deviations, total evaluations, per-dimension traces)."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim == 1:
        points = points.reshape(1, -1)
    D = points.shape[0]
    man = [0] * D if manifold is None else list(manifold)
    bw, total, traces = np.zeros(D), 0, []
    for d in range(D):
        bw[d], n, tr = ksize_1d(points[d], man[d])
        total += n
        traces.append(tr)
    return bw, total, traces


def min_tie_gap(traces):
    """the smallest relative gap |f1 - f2| / max(|f1|, |f2|) over every comparison the searches made"""
    gap = np.inf
    for tr in traces:
        for _, _, f1, f2 in tr:
            if np.isfinite(f1) and np.isfinite(f2):
                gap = min(gap, abs(f1 - f2) / max(abs(f1), abs(f2), 1e-300))
            elif f1 == f2:
                gap = 0.0
    return gap


# ---- the inputs both test files use ----------------------------------------------------------------------------------
def circular_case(seed, D, N, Nq, manifold, weighted):
    """points, weights, variances, queries: in a circular dimension a cluster that straddles the cut at +-pi, with part of
    the inputs moved to other representatives (+-2 pi, outside [-pi, pi)); Euclidean dimensions are plain normals"""
    rng = np.random.default_rng(seed)
    pts, pos = rng.standard_normal((D, N)), rng.standard_normal((D, Nq)) * 1.2
    for k in range(D):
        if manifold[k]:
            a = math.pi + 0.5 * rng.standard_normal(N)
            pts[k] = np.where(a >= math.pi, a - 2.0 * math.pi, a)            # wrapped into [-pi, pi): both sides of the cut
            pts[k, ::5] += 2.0 * math.pi * rng.integers(-1, 2, size=pts[k, ::5].size)  # other representatives
            pos[k] = rng.uniform(-2.0 * math.pi, 2.0 * math.pi, Nq)
    w = rng.uniform(0.2, 1.0, N) if weighted else None
    bw = rng.uniform(0.2, 0.6, D)  # standard deviations
    return pts, w, bw, pos


# seeds of bandwidth_case for which the model's own f1 / f2 gaps are far from a tie (tests/test_circular_host.py asserts it)
BANDWIDTH_CASES = [(1, 100, [1]), (2, 300, [0, 1]), (3, 65, [1, 0, 1]), (6, 129, [0, 0, 0, 1, 1, 1]), (2, 257, [1, 1])]


def bandwidth_case(D, N, manifold):
    rng = np.random.default_rng(1000 + 10 * D + N)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))
    for k in range(D):
        if manifold[k]:
            a = math.pi + 0.6 * rng.standard_normal(N)
            pts[k] = np.where(a >= math.pi, a - 2.0 * math.pi, a)
    return pts
