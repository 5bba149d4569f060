"""A numpy model of include/kdehip.h section 5h, written from its text: the moments of a Gaussian-kernel density at a query
in fp64 with a running maximum over S = { i : w_i > 0 } and exactly rounded sums (math.fsum), the gradient and the
mean-shift step they give, the iteration with freezing, and the greedy merge of the converged points.  No GPU.

A density is (points (D, N), weights (N,), variances (D,)); `man` is None or one 0 / 1 per dimension (1 = circular)."""
import math
from fractions import Fraction

import numpy as np

TWO_PI = 2.0 * math.pi


def wrap(t):
    """to [-pi, pi): the library's circ_wrap"""
    return t - TWO_PI * np.floor((t + math.pi) / TWO_PI)


def _circ(man, D):
    return np.zeros(D, dtype=bool) if man is None else np.asarray(man, dtype=bool)


def differences(x, pts, man=None):
    """d[k, i] = x_k - c_ik, wrapped where circular"""
    d = np.asarray(x, dtype=np.float64)[:, None] - pts
    c = _circ(man, pts.shape[0])
    if c.any():
        d[c] = wrap(d[c])
    return d


def log_norm(v):
    """log((2 pi)^(D/2) prod_k sqrt(v_k))"""
    return 0.5 * len(v) * math.log(TWO_PI) + 0.5 * math.fsum(math.log(t) for t in v)


def _fma(x, y, z):
    """x * y + z rounded once (exact rational arithmetic; float() of a Fraction rounds correctly)"""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def exponents(d, v, fma=False):
    """a_i = sum_k d_ik^2 * (-0.5 / v_k), k ascending.  fma=True: as the header words it, a_i <- fma(d_ik * d_ik, -0.5 / v_k,
    a_i) with the square rounded and the fma rounded once -- slow, for the few queries whose exponents are so large that
    the rounding of a product more or less shows in e^{a_i - m}"""
    D, N = d.shape
    a = np.zeros(N)
    for k in range(D):
        if fma:
            sq, h = d[k] * d[k], -0.5 / v[k]
            a = np.array([_fma(float(sq[i]), float(h), float(a[i])) for i in range(N)])
        else:
            a = a + (d[k] * d[k]) * (-0.5 / v[k])
    return a


def moments(dens, x, man=None, fma=False):
    """(m, S_0, S (D,), A (D,)) at one query: m = max_{i in S} a_i, S_0 = sum w_i e^{a_i - m}, S_k = sum w_i e^{a_i - m} d_ik
    and A_k = sum w_i e^{a_i - m} |d_ik|, the scale of the signed sum S_k.  S empty: (-inf, 0, 0, 0).  fma: see exponents."""
    pts, w, v = dens
    D = pts.shape[0]
    d = differences(x, pts, man)
    a = exponents(d, v, fma)
    inS = np.asarray(w) > 0.0
    if not inS.any():
        return -math.inf, 0.0, np.zeros(D), np.zeros(D)
    m = float(np.max(a[inS]))
    t = np.where(inS, w * np.exp(np.where(inS, a - m, 0.0)), 0.0)
    S0 = math.fsum(t.tolist())
    S = np.array([math.fsum((t * d[k]).tolist()) for k in range(D)])
    A = np.array([math.fsum((t * np.abs(d[k])).tolist()) for k in range(D)])
    return m, S0, S, A


def log_p(dens, x, man=None):
    m, S0, _, _ = moments(dens, x, man)
    return -math.inf if S0 == 0.0 else m + math.log(S0) - log_norm(dens[2])


def evaluate_grad(dens, X, man=None, log=True, fma=False):
    """(val (Nq,), grad (D, Nq), scale (D, Nq)) at the columns of X: log p and its gradient -S_k / (S_0 v_k) (or p and
    p times it); scale = A_k / (S_0 v_k) (times p), what the rounding of the signed sum is relative to"""
    v = np.asarray(dens[2])
    D, Nq = X.shape
    val, grad, scale = np.zeros(Nq), np.zeros((D, Nq)), np.zeros((D, Nq))
    for q in range(Nq):
        m, S0, S, A = moments(dens, X[:, q], man, fma)
        if S0 == 0.0:
            val[q] = -math.inf if log else 0.0
            continue
        lp = m + math.log(S0) - log_norm(v)
        p = math.exp(lp)
        val[q] = lp if log else p
        grad[:, q] = -S / (S0 * v) * (1.0 if log else p)
        scale[:, q] = A / (S0 * v) * (1.0 if log else p)
    return val, grad, scale


def step(dens, x, man=None):
    """(the point after one mean-shift step, dx = S_k / S_0, A_k / S_0); S empty: the point itself and zeros"""
    m, S0, S, A = moments(dens, x, man)
    D = len(x)
    if S0 == 0.0:
        return np.array(x, dtype=np.float64), np.zeros(D), np.zeros(D)
    dx = S / S0
    xn = np.asarray(x, dtype=np.float64) - dx
    c = _circ(man, D)
    if c.any():
        xn[c] = wrap(xn[c])
    return xn, dx, A / S0


def moments_many(dens, X, man=None):
    """(m (K,), S_0 (K,), S (D, K)) at the columns of X at once, with numpy's pairwise sums in place of math.fsum: what the
    iteration below runs on (a start takes tens of steps); `moments` is the exactly rounded one the tests compare with"""
    pts, w, v = dens
    D = pts.shape[0]
    d = X[:, :, None] - pts[:, None, :]  # (D, K, N)
    c = _circ(man, D)
    if c.any():
        d[c] = wrap(d[c])
    a = np.zeros(d.shape[1:])
    for k in range(D):
        a = a + (d[k] * d[k]) * (-0.5 / v[k])
    inS = np.asarray(w) > 0.0
    if not inS.any():
        K = X.shape[1]
        return np.full(K, -math.inf), np.zeros(K), np.zeros((D, K))
    m = np.max(a[:, inS], axis=1)
    t = np.where(inS[None, :], w[None, :] * np.exp(np.where(inS[None, :], a - m[:, None], 0.0)), 0.0)
    return m, np.sum(t, axis=1), np.sum(t[None, :, :] * d, axis=2)


def meanshift(dens, starts, tol, maxiter, man=None):
    """(x (D, K), logp (K,), iters (K,), trace (steps + 1, K)): every start steps until max_k |S_k / S_0| / sqrt(v_k) <= tol --
    the step just taken is the last, the point is frozen -- or for maxiter steps; iters = the steps taken, negative if the
    last was still above tol; a start with S empty is frozen at once with 0 steps.  trace[s] = log p at the points before
    step s (a frozen start repeats its last value), trace[-1] = log p at the returned points."""
    v = np.asarray(dens[2])
    sd = np.sqrt(v)
    D, K = starts.shape
    x = np.array(starts, dtype=np.float64)
    iters = np.zeros(K, dtype=np.int64)
    frozen = np.zeros(K, dtype=bool)
    c = _circ(man, D)
    trace = []

    def logp_of(m, S0):
        with np.errstate(divide="ignore"):
            return np.where(S0 > 0.0, m + np.log(np.where(S0 > 0.0, S0, 1.0)) - log_norm(v), -math.inf)

    for _ in range(maxiter):
        if frozen.all():
            break
        m, S0, S = moments_many(dens, x, man)
        trace.append(logp_of(m, S0))
        empty = S0 == 0.0
        frozen |= empty
        live = ~frozen
        dx = np.where(live[None, :], S / np.where(empty, 1.0, S0)[None, :], 0.0)
        xn = x - dx
        if c.any():
            xn[c] = wrap(xn[c])
        x = np.where(live[None, :], xn, x)
        cnt = np.abs(iters) + 1
        done = live & (np.max(np.abs(dx) / sd[:, None], axis=0) <= tol)
        iters = np.where(live, np.where(done, cnt, -cnt), iters)
        frozen |= done
    m, S0, _ = moments_many(dens, x, man)
    trace.append(logp_of(m, S0))
    return x, trace[-1], iters, np.array(trace)


def merge(x, logp, iters, sd, tol_merge, man=None):
    """(indices of the founders, labels): the converged points (iters >= 0) in descending logp, ties by index; a point joins
    the first kept mode within tol_merge in max_k |diff_k| / sd_k (wrapped where circular), else it founds a new mode; an
    unconverged point is labelled -1"""
    D, K = x.shape
    c = _circ(man, D)
    labels = np.full(K, -1, dtype=np.int64)
    order = sorted((k for k in range(K) if iters[k] >= 0), key=lambda k: (-logp[k], k))
    kept = []
    for k in order:
        home = -1
        for j, f in enumerate(kept):
            d = x[:, k] - x[:, f]
            d = np.where(c, wrap(d), d)
            if float(np.max(np.abs(d) / sd)) <= tol_merge:
                home = j
                break
        if home < 0:
            home = len(kept)
            kept.append(k)
        labels[k] = home
    return kept, labels


def modes(dens, tol=1e-9, maxiter=500, tol_merge=1e-3, man=None):
    """(modes (D, n), logp (n,), mass (n,), labels (N,)) from the density's own points"""
    pts, w, v = dens
    x, logp, iters, _ = meanshift(dens, pts, tol, maxiter, man)
    kept, labels = merge(x, logp, iters, np.sqrt(np.asarray(v)), tol_merge, man)
    mass = np.array([math.fsum(np.asarray(w)[labels == j].tolist()) for j in range(len(kept))])
    return x[:, kept], logp[kept], mass, labels


def three_clusters(D, N, shift=None):
    """The convergence data: three clusters of sd 0.3 at 0, +3 e_1 and -3 e_2 (-3 e_1 when D = 1), point i in cluster i % 3,
    bandwidth sd 0.4, weights uniform(0.05, 1) with every fifth weight 0; seed 1000 D + N.  `shift` (D,) is added to the
    centres.  Returns (points (D, N), bandwidth sd (D,), weights (N,))."""
    rng = np.random.default_rng(1000 * D + N)
    centres = np.zeros((D, 3))
    centres[0, 1] = 3.0
    centres[1 if D > 1 else 0, 2] = -3.0
    pts = centres[:, np.arange(N) % 3] + 0.3 * rng.standard_normal((D, N))
    w = rng.uniform(0.05, 1.0, size=N)
    w[::5] = 0.0
    if shift is not None:
        pts = pts + np.asarray(shift, dtype=np.float64)[:, None]
    return pts, np.full(D, 0.4), w
