"""NumPy fp64 model of densities with per-point bandwidths (include/kdehip.h sections 4 and 5o), the CPU reference of
tests/test_varbw_host.py and tests/test_gpu_varbw.py: the builder's rows, log p by log-sum-exp with a normaliser per source,
leave-one-out, evalAvgLogL, and the two scale rules of `adaptive_scales`.  No scipy.  The difference operator (and with it
the wrap) is tests/circular_model.py's.

Densities are plain arrays: points (D, N), weights (N, any scale, zeros allowed; None = uniform), var = VARIANCES (D, N),
column i being point i's -- all in the caller's original order."""
import math

import numpy as np

from tests.circular_model import diff, normalise


# ---- the builder -----------------------------------------------------------------------------------------------------
def builder_rows(bd, var):
    """(bandwidth, bandwidthMin, bandwidthMax), each (2N, D) by node, that kdehip_make_density_varbw must give on the tree of
    `bd` (any density over the same points and weights: the tree does not depend on the bandwidth) for the variances var
    (D, N): leaf rows var through the permutation; internal rows by calcStatsDensity! (src/BallTreeDensity01.jl:156-185),
    children before parents, every operation rounded on its own."""
    bt = bd.bt
    N, D = bt.num_points, bt.dims
    var = np.asarray(var, dtype=np.float64)
    mu = np.asarray(bd.means, dtype=np.float64).reshape(2 * N, D)
    w = np.asarray(bt.weights, dtype=np.float64)
    bw, lo, hi = np.zeros((2 * N, D)), np.zeros((2 * N, D)), np.zeros((2 * N, D))
    for leaf in range(N, 2 * N):
        bw[leaf] = lo[leaf] = hi[leaf] = var[:, bt.permutation[leaf] - 1]
    eps = np.finfo(np.float64).eps

    def visit(node):  # 1-based id
        if node > N:
            return
        a, b = int(bt.left_child[node - 1]), int(bt.right_child[node - 1])
        if N == 1:
            a = b = 2  # the root summarises the one leaf with itself (src/BallTree01.jl:351-362)
        visit(a)
        if b != a:
            visit(b)
        wa, wb = w[a - 1], w[b - 1]
        wt = wa + wb + eps
        wa, wb = wa / wt, wb / wt
        ma, mb, m = mu[a - 1], mu[b - 1], mu[node - 1]
        bw[node - 1] = wa * (bw[a - 1] + ma * ma) + wb * (bw[b - 1] + mb * mb) - m * m
        hi[node - 1] = np.where(hi[a - 1] > hi[b - 1], hi[a - 1], hi[b - 1])
        lo[node - 1] = np.where(lo[a - 1] < lo[b - 1], lo[a - 1], lo[b - 1])

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        visit(1)
    finally:
        sys.setrecursionlimit(old)
    return bw, lo, hi


def subtree_extremes(bd, var):
    """(min, max) of the leaf variances below every internal node, (N, D) each, from lowest_leaf / highest_leaf alone"""
    bt = bd.bt
    N, D = bt.num_points, bt.dims
    leaf = np.asarray(var, dtype=np.float64)[:, bt.permutation[N:] - 1].T  # (N, D), leaf order
    lo, hi = np.zeros((N, D)), np.zeros((N, D))
    for node in range(1, N if N > 1 else 2):
        a, b = int(bt.lowest_leaf[node - 1]) - N - 1, int(bt.highest_leaf[node - 1]) - N - 1
        lo[node - 1], hi[node - 1] = leaf[a:b + 1].min(axis=0), leaf[a:b + 1].max(axis=0)
    return lo, hi


# ---- evaluation ------------------------------------------------------------------------------------------------------
def terms(points, weights, var, pos, manifold=None):
    """t[q, i] = a_qi + lc_i: a_qi = sum_k d_k^2 (-0.5 / v_ik), lc_i = log w_i - 1/2 sum_k log v_ik (-inf for w_i == 0)"""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    var = np.asarray(var, dtype=np.float64).reshape(D, N)
    w = normalise(weights, N)
    man = [0] * D if manifold is None else list(manifold)
    pos = np.asarray(pos, dtype=np.float64).reshape(D, -1)
    a = np.zeros((pos.shape[1], N))
    for k in range(D):
        d = diff(pos[k][:, None], points[k][None, :], man[k])
        a += d * d * (-0.5 / var[k])[None, :]
    with np.errstate(divide="ignore"):
        lc = np.log(w) - 0.5 * np.log(var).sum(axis=0)
    return a + lc[None, :], w


def eval_log(points, weights, var, pos=None, manifold=None, loo=False, rows=None):
    """log p[q] = m + log(sum_{i in S} exp(t_i - m)) - (D/2) log 2pi [- log(1 - w_q)], m = max_{i in S} t_i,
    S = {i : w_i > 0} (loo: and i != q); S empty gives -inf; a query with a NaN coordinate gives NaN.  rows: a slice of the
    queries -- the values of those alone."""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    pos = points if loo else np.asarray(pos, dtype=np.float64).reshape(D, -1)
    qs = np.arange(pos.shape[1])[slice(None) if rows is None else rows]
    with np.errstate(invalid="ignore"):
        t, w = terms(points, weights, var, pos[:, qs], manifold)
    inS = np.broadcast_to(w[None, :] > 0.0, t.shape).copy()
    if loo:
        inS[np.arange(qs.size), qs] = False
    lognorm0 = 0.5 * D * math.log(2.0 * math.pi)
    out = np.full(t.shape[0], -np.inf)
    for r, q in enumerate(qs):
        if np.any(np.isnan(pos[:, q])):
            out[r] = np.nan
            continue
        s = inS[r]
        if not s.any():
            continue
        m = t[r, s].max()
        out[r] = m + math.log(float(np.sum(np.exp(t[r, s] - m)))) - lognorm0
        if loo:
            out[r] -= math.log(1.0 - w[q])
    return out


def eval_direct(points, weights, var, pos=None, manifold=None, loo=False, rows=None):
    """p[q] = sum_{i (!= q if loo)} w_i / prod_k sqrt(v_ik) exp(a_qi) / (2 pi)^(D/2) [/ (1 - w_q)]: the plain sum, which
    underflows to 0 where eval_log stays finite"""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    var = np.asarray(var, dtype=np.float64).reshape(D, N)
    pos = points if loo else np.asarray(pos, dtype=np.float64).reshape(D, -1)
    qs = np.arange(pos.shape[1])[slice(None) if rows is None else rows]
    w = normalise(weights, N)
    man = [0] * D if manifold is None else list(manifold)
    a = np.zeros((qs.size, N))
    for k in range(D):
        d = diff(pos[k, qs][:, None], points[k][None, :], man[k])
        a += d * d * (-0.5 / var[k])[None, :]
    c = w / np.prod(np.sqrt(var), axis=0)
    e = c[None, :] * np.exp(a)
    if loo:
        e[np.arange(qs.size), qs] = 0.0
    p = e.sum(axis=1) / (2.0 * math.pi) ** (D / 2.0)
    p[np.any(np.isnan(pos[:, qs]), axis=0)] = np.nan
    return p / (1.0 - w[qs]) if loo else p


def avg_logl(L, W):
    """evalAvgLogL's rule on L and W (src/DualTree01.jl:456-466): an L == 0 with W != 0 makes it -inf, the other zeros
    count as log 1"""
    L, W = np.asarray(L, dtype=np.float64), np.asarray(W, dtype=np.float64)
    if np.any((L == 0.0) & (W != 0.0)):
        return -np.inf
    return float(np.dot(np.log(np.where(L == 0.0, 1.0, L)), W))


def avg_logl_log(logp, W):
    """the log-domain rule (section 5f): sum over W != 0 of W log p; -inf only if such a log p is -inf"""
    logp, W = np.asarray(logp, dtype=np.float64), np.asarray(W, dtype=np.float64)
    use = W != 0.0
    if np.any(np.isneginf(logp[use])):
        return -np.inf
    return float(np.dot(logp[use], W[use]))


def eval_avg_logl(p, q=None, manifold=None, log_domain=False):
    """evalAvgLogL(p, q); p = (points, weights, var), q = (points, weights); q None: the same object, leave-one-out"""
    at = p if q is None else q
    W = normalise(at[1], np.asarray(at[0]).shape[1])
    kw = dict(manifold=manifold, loo=True) if q is None else dict(pos=q[0], manifold=manifold)
    if log_domain:
        return avg_logl_log(eval_log(p[0], p[1], p[2], **kw), W)
    return avg_logl(eval_direct(p[0], p[1], p[2], **kw), W)


def entropy(p, **kw):
    return -eval_avg_logl(p, None, **kw)


def kld(p, q, **kw):
    """kld(p, q) = evalAvgLogL(p, p) [leave-one-out] - evalAvgLogL(q, p)"""
    return eval_avg_logl(p, None, **kw) - eval_avg_logl(q, (p[0], p[1]), **kw)


# ---- the scale rules -------------------------------------------------------------------------------------------------
def _uniform_var(var1, N):
    return np.repeat(np.asarray(var1, dtype=np.float64).reshape(-1, 1), N, axis=1)


def scales_abramson(points, weights, var1, alpha=0.5):
    """lambda_i = exp(-alpha (lp_i - sum_j w_j lp_j)), lp the pilot (one variance vector var1 (D)) at its own points with
    the self term"""
    points = np.asarray(points, dtype=np.float64)
    N = points.shape[1]
    lp = eval_log(points, weights, _uniform_var(var1, N), points)
    w = normalise(weights, N)
    return np.exp(-alpha * (lp - np.sum(w * lp)))


def scales_knn(points, weights, var1, k=8):
    """lambda_i proportional to the k-th smallest of sqrt(sum_k d_k^2 / v_k) over the other points (left out by index),
    normalised to weighted geometric mean 1"""
    points = np.asarray(points, dtype=np.float64)
    D, N = points.shape
    var1 = np.asarray(var1, dtype=np.float64).reshape(D)
    d2 = np.zeros((N, N))
    for kk in range(D):
        d = points[kk][:, None] - points[kk][None, :]
        d2 += d * d * (1.0 / var1[kk])
    d2[np.arange(N), np.arange(N)] = np.inf
    dk = np.sqrt(np.sort(d2, axis=1)[:, k - 1])
    w = normalise(weights, N)
    ld = np.log(dk)
    return np.exp(ld - np.sum(w * ld))


def two_scale_sample(seed, D, N=300):
    """the issue's sample: a tight mode 0.1 N(0, I) [N // 2 points] and a wide one 3 N(0, I) + 1"""
    rng = np.random.default_rng(seed)
    return np.concatenate([0.1 * rng.standard_normal((D, N // 2)), 3.0 * rng.standard_normal((D, N - N // 2)) + 1.0], axis=1)
