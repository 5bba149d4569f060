"""A numpy model of include/kdehip.h section 5s, written from its text: the cost between the points of two densities, the
log-domain Sinkhorn iteration of a cross item (alternating updates) and of a self item (the symmetric average), the results of
an item, the barycentric map and the Sinkhorn divergence.  fp64, every log-sum-exp with its maximum taken out, and the sums
over the points whose order could matter (err, mass, the dual sums, the transport cost) by math.fsum.  No GPU.

A density is (points (D, N), weights (N,) -- zeros allowed); `s` is the scale (D,), `man` None or one 0 / 1 per dimension
(1 = circular)."""
import math

import numpy as np

from tests.modes_model import wrap


def diffs(x, y, man=None):
    """(D, N, M): diff_k(x_i, y_j), wrapped in a circular dimension"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = x[:, :, None] - y[:, None, :]
    if man is not None:
        for k in np.flatnonzero(np.asarray(man, dtype=bool)):
            d[k] = wrap(d[k])
    return d


def cost(x, y, s, man=None):
    """c (N, M) = 1/2 sum_k diff_k^2 / s_k^2"""
    d = diffs(x, y, man)
    s = np.asarray(s, dtype=np.float64)
    c = np.zeros(d.shape[1:])
    for k in range(d.shape[0]):
        c += d[k] * d[k] * (0.5 / (s[k] * s[k]))
    return c


def default_scale(vp, vq):
    """sqrt(v_p + v_q) per dimension, from the two densities' variances"""
    return np.sqrt(np.asarray(vp, dtype=np.float64) + np.asarray(vq, dtype=np.float64))


def _neg_lse(Z):
    """-LSE over axis 1 of Z (rows of -inf entries excluded by their value); +inf for a row that is all -inf"""
    m = Z.max(axis=1)
    ok = m > -np.inf
    out = np.full(Z.shape[0], np.inf)
    with np.errstate(under="ignore"):
        out[ok] = -(m[ok] + np.log(np.exp(Z[ok] - m[ok, None]).sum(axis=1)))
    return out


def _logw(w):
    out = np.full(len(w), -np.inf)
    out[w > 0] = np.log(w[w > 0])
    return out


def _dot(w, v):
    use = np.flatnonzero(w > 0)
    return math.fsum(float(w[i]) * float(v[i]) for i in use)


def iterate(p, q, s, reg, tol, maxiter, man=None):
    """One item of section 5s.  p = (x (D, N), a (N,)), q = (y, b), or q None: the self item of p.  Returns a dict: value,
    transport_cost, err, mass, iters, phi (N,), gamma (M,), delta (D, N), map (D, N), and `errs`: err at every pass, the
    stopping one last."""
    x, a = np.asarray(p[0], dtype=np.float64), np.asarray(p[1], dtype=np.float64)
    self_item = q is None
    y, b = (x, a) if self_item else (np.asarray(q[0], dtype=np.float64), np.asarray(q[1], dtype=np.float64))
    eps = float(reg)
    d = diffs(x, y, man)
    c = cost(x, y, s, man)
    A = -c / eps
    la, lb = _logw(a), _logw(b)
    phi, gamma = np.zeros(len(a)), np.zeros(len(b))
    steps, errs = 0, []
    while True:
        tau = _neg_lse(A + (lb + gamma)[None, :])
        r = np.exp(phi - tau)
        err = _dot(a, np.abs(r - 1.0))
        mass = _dot(a, r)
        errs.append(err)
        if (steps >= 1 and err <= tol) or steps == maxiter:
            break
        if self_item:
            phi = 0.5 * (phi + tau)
            gamma = phi
        else:
            phi = tau
            gamma = _neg_lse(A.T + (la + phi)[None, :])
        steps += 1
    value = eps * (_dot(a, phi) + _dot(b, gamma) - (mass - 1.0))
    Z = A + (lb + gamma)[None, :]
    m = Z.max(axis=1)
    with np.errstate(under="ignore"):
        e = np.exp(Z - m[:, None])                       # (N, M); 0 for a weightless y_j
    S0 = e.sum(axis=1)
    delta = np.stack([-(e * d[k]).sum(axis=1) / S0 for k in range(d.shape[0])])   # diff(y_j, x_i) = -diff(x_i, y_j)
    T = x + delta
    if man is not None:
        for k in np.flatnonzero(np.asarray(man, dtype=bool)):
            T[k] = wrap(T[k])
    # <pi, c>, pi_ij = a_i b_j exp(phi_i + gamma_j + A_ij): row i is a_i exp(phi_i + m_i) sum_j e_ij c_ij
    rows = (e * c).sum(axis=1)
    use = np.flatnonzero(a > 0)
    tcost = math.fsum(float(a[i]) * math.exp(float(phi[i] + m[i])) * float(rows[i]) for i in use)
    return dict(value=value, transport_cost=tcost, err=err, mass=mass, iters=steps if err <= tol else -steps, phi=phi, gamma=gamma,
                delta=delta, map=T, errs=np.array(errs))


def iterate_blocked(p, q, s, reg, tol, maxiter, man=None, rows=1024):
    """`iterate`, the same formulas `rows` rows of the cost at a time: no array larger than (rows, max(N, M)) per dimension is
    ever formed, so a self item of 8193 points costs megabytes where the dense model needs gigabytes.  The second half-step
    takes the rows of the transposed cost from diff(y_j, x_i) = -diff(x_i, y_j).  Held to `iterate` by
    tests/test_transport_host.py; `errs` is returned as in `iterate`."""
    x, a = np.asarray(p[0], dtype=np.float64), np.asarray(p[1], dtype=np.float64)
    self_item = q is None
    y, b = (x, a) if self_item else (np.asarray(q[0], dtype=np.float64), np.asarray(q[1], dtype=np.float64))
    eps = float(reg)
    N, M = len(a), len(b)
    la, lb = _logw(a), _logw(b)

    def half(u, v, l):
        """-LSE_j (l_j - c(u_i, v_j) / eps) for every column i of u"""
        out = np.empty(u.shape[1])
        for i0 in range(0, u.shape[1], rows):
            A = -cost(u[:, i0:i0 + rows], v, s, man) / eps
            out[i0:i0 + rows] = _neg_lse(A + l[None, :])
        return out

    phi, gamma = np.zeros(N), np.zeros(M)
    steps, errs = 0, []
    while True:
        tau = half(x, y, lb + gamma)
        r = np.exp(phi - tau)
        err = _dot(a, np.abs(r - 1.0))
        mass = _dot(a, r)
        errs.append(err)
        if (steps >= 1 and err <= tol) or steps == maxiter:
            break
        if self_item:
            phi = 0.5 * (phi + tau)
            gamma = phi
        else:
            phi = tau
            gamma = half(y, x, la + phi)
        steps += 1
    value = eps * (_dot(a, phi) + _dot(b, gamma) - (mass - 1.0))
    delta, m, rowsum = np.empty(x.shape), np.empty(N), np.empty(N)
    for i0 in range(0, N, rows):
        xb = x[:, i0:i0 + rows]
        d = diffs(xb, y, man)
        c = cost(xb, y, s, man)
        Z = -c / eps + (lb + gamma)[None, :]
        mb = Z.max(axis=1)
        with np.errstate(under="ignore"):
            e = np.exp(Z - mb[:, None])
        S0 = e.sum(axis=1)
        for k in range(d.shape[0]):
            delta[k, i0:i0 + rows] = -(e * d[k]).sum(axis=1) / S0
        m[i0:i0 + rows] = mb
        rowsum[i0:i0 + rows] = (e * c).sum(axis=1)
    T = x + delta
    if man is not None:
        for k in np.flatnonzero(np.asarray(man, dtype=bool)):
            T[k] = wrap(T[k])
    use = np.flatnonzero(a > 0)
    tcost = math.fsum(float(a[i]) * math.exp(float(phi[i] + m[i])) * float(rowsum[i]) for i in use)
    return dict(value=value, transport_cost=tcost, err=err, mass=mass, iters=steps if err <= tol else -steps, phi=phi, gamma=gamma,
                delta=delta, map=T, errs=np.array(errs))


def plan(p, q, s, reg, phi, gamma, man=None):
    """pi (N, M) = a_i b_j exp(phi_i + gamma_j + A_ij), from potentials alone"""
    A = -cost(p[0], q[0], s, man) / float(reg)
    with np.errstate(under="ignore", divide="ignore"):
        return np.exp(A + (_logw(np.asarray(p[1])) + phi)[:, None] + (_logw(np.asarray(q[1])) + gamma)[None, :])


def divergence(p, q, s, reg, tol, maxiter, man=None):
    """S(p, q) = value(p, q) - value(p, p) / 2 - value(q, q) / 2, and the three items"""
    pq, pp, qq = iterate(p, q, s, reg, tol, maxiter, man), iterate(p, None, s, reg, tol, maxiter, man), \
        iterate(q, None, s, reg, tol, maxiter, man)
    return pq["value"] - 0.5 * pp["value"] - 0.5 * qq["value"], (pq, pp, qq)


def unregularised_1d(x, y, s):
    """W = 1/2 mean((x_sorted - y_sorted)^2 / s^2): two sets of equally many, equally weighted points on the line"""
    xs, ys = np.sort(np.ravel(x)), np.sort(np.ravel(y))
    return 0.5 * float(np.mean((xs - ys) ** 2)) / float(s) ** 2


def unregularised_1d_weighted(x, a, y, b, s):
    """the same for weighted points: the monotone coupling of the two sorted sets (north-west corner rule), which is
    optimal for a convex cost on the line"""
    ox, oy = np.argsort(np.ravel(x)), np.argsort(np.ravel(y))
    xs, ys, ra, rb = np.ravel(x)[ox], np.ravel(y)[oy], np.asarray(a, dtype=np.float64)[ox].copy(), np.asarray(b, dtype=np.float64)[oy].copy()
    i = j = 0
    terms = []
    while i < len(xs) and j < len(ys):
        t = min(ra[i], rb[j])
        if t > 0.0:
            terms.append(t * 0.5 * (xs[i] - ys[j]) ** 2 / float(s) ** 2)
        ra[i] -= t
        rb[j] -= t
        if ra[i] <= 0.0:
            i += 1
        elif rb[j] <= 0.0:
            j += 1
    return math.fsum(terms)


# ---- the data of the tests -------------------------------------------------------------------------------------------------
def two_clusters_pair(D, N, M, shift=0.5, seed=None):
    """((x (D, N), a), (y (D, M), b)): draws from ONE two-cluster mixture (different widths per dimension), q's shifted by
    `shift` in every dimension; every fifth weight is 0 on both sides, the weights of a side sum to 1"""
    rng = np.random.default_rng(3000 + 100 * D + 7 * N + M if seed is None else seed)
    sd = rng.uniform(0.3, 1.2, size=(D, 1))
    centre = rng.uniform(-2.0, 2.0, size=(D, 2))

    def draw(n, off):
        lab = rng.integers(0, 2, size=n)
        pts = centre[:, lab] + sd * rng.standard_normal((D, n)) * np.where(lab == 0, 1.0, 0.5)[None, :] + off
        w = rng.uniform(0.2, 1.0, size=n)
        w[::5] = 0.0
        return np.ascontiguousarray(pts), w / w.sum()

    return draw(N, 0.0), draw(M, shift)


def silverman(pts):
    D, N = pts.shape
    return pts.std(axis=1, ddof=1) * (4.0 / ((D + 2.0) * N)) ** (1.0 / (D + 4.0))


def angle_pair(N=60, M=50, centre=math.pi - 0.1, seed=17):
    """a 2-D pair, [euclid, circular]: both angle clusters straddle the cut at +-pi (q's 0.3 further round), so that the
    wrapped and the plain differences disagree for many pairs"""
    rng = np.random.default_rng(seed)
    x = np.vstack([rng.standard_normal(N), wrap(centre + 0.25 * rng.standard_normal(N))])
    y = np.vstack([0.5 + rng.standard_normal(M), wrap(centre + 0.3 + 0.25 * rng.standard_normal(M))])
    return (np.ascontiguousarray(x), np.full(N, 1.0 / N)), (np.ascontiguousarray(y), np.full(M, 1.0 / M))
