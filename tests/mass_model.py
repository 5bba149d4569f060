"""The model of include/kdehip.h section 5l in pure Python: the box mass, the marginal cdf and pdf and a quantile of a
Gaussian-kernel density with one bandwidth vector, by the contract's own factor with `math.erfc`, every term kept and ONE
`math.fsum` per value.  A density is (points (D, N), weights (N,), variances (D,)), as tests/test_gpu_ksum.py's `_arrays`
returns it.  Not a test module.

How good the model is (measured once against 40-digit arithmetic on D in {1, 3, 6, 8}, N = 130, two clusters, one zero
weight, 24 boxes at least half a bandwidth wide or infinite, a and b as the model rounds them): within 3.1e-16 relative,
far inside the 1e-12 the GPU tests allow."""
import math

import numpy as np


def scale(v):
    """s = 1 / sqrt(2 v), the root and the division correctly rounded"""
    return 1.0 / math.sqrt(2.0 * v)


def factor(a, b):
    """the mass of a unit kernel between a and b (in units of sqrt(2 v) from its centre): section 5l's three forms"""
    if not a < b:
        return 0.0
    if a >= 0.0:
        return (math.erfc(a) - math.erfc(b)) / 2.0
    if b <= 0.0:
        return (math.erfc(-b) - math.erfc(-a)) / 2.0
    return 1.0 - (math.erfc(-a) + math.erfc(b)) / 2.0


def box_mass_one(dens, lo, hi, dims):
    """the mass of ONE box: lo, hi hold one value per entry of `dims` (0-based, in that order); NaN if a bound is"""
    pts, w, v = dens
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if any(math.isnan(x) for x in lo + hi):
        return math.nan
    s = [scale(float(v[d])) for d in dims]
    terms = []
    for i in range(pts.shape[1]):
        if w[i] == 0.0:
            continue
        f = 1.0
        for j, d in enumerate(dims):
            c = float(pts[d, i])
            f *= factor((lo[j] - c) * s[j], (hi[j] - c) * s[j])
        terms.append(float(w[i]) * f)
    return math.fsum(terms)


def box_mass(dens, lo, hi, dims=None):
    """masses (Nq,) of the boxes lo[:, q], hi[:, q] (nb, Nq) over `dims` (None: all dimensions)"""
    D = dens[0].shape[0]
    dims = list(range(D)) if dims is None else list(dims)
    lo, hi = np.broadcast_arrays(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    lo, hi = lo.reshape(len(dims), -1), hi.reshape(len(dims), -1)
    return np.array([box_mass_one(dens, lo[:, q], hi[:, q], dims) for q in range(lo.shape[1])])


def cdf(dens, x, dim):
    """F_dim(x) = (sum_i w_i erfc(-(x - c_i) s)) / 2 for a scalar x"""
    pts, w, v = dens
    s = scale(float(v[dim]))
    return math.fsum(float(w[i]) * math.erfc(-((float(x) - float(pts[dim, i])) * s)) for i in range(pts.shape[1])) / 2.0


def pdf(dens, x, dim):
    """f_dim(x) = (sum_i w_i exp(-t_i^2)) * s / sqrt(pi)"""
    pts, w, v = dens
    s = scale(float(v[dim]))
    return math.fsum(float(w[i]) * math.exp(-((float(x) - float(pts[dim, i])) * s) ** 2) for i in range(pts.shape[1])) \
        * (s / math.sqrt(math.pi))


def quantile(dens, alpha, dim, tol=1e-12, max_iter=100):
    """(x, resid, iters, converged) by the iteration of section 5l (bracket, Newton, the rtsafe rule) on the model's F and f"""
    pts, w, v = dens
    if not 0.0 < alpha < 1.0:
        return math.nan, math.nan, 0, False
    live = [float(pts[dim, i]) for i in range(pts.shape[1]) if w[i] > 0.0]
    if not live:
        return math.nan, math.nan, 0, False
    sigma = math.sqrt(float(v[dim]))
    xl, xh = min(live) - 39.0 * sigma, max(live) + 39.0 * sigma
    x = 0.5 * (xl + xh)
    dxold = dx = xh - xl
    iters = 0
    while True:
        F, f = cdf(dens, x, dim), pdf(dens, x, dim)
        iters += 1
        r = F - alpha
        if abs(r) <= tol:
            return x, r, iters, True
        if iters >= max_iter:
            return x, r, iters, False
        if r < 0.0:
            xl = x
        else:
            xh = x
        step = r / f if f > 0.0 else math.inf
        xn = x - step
        newton = f > 0.0 and xl < xn < xh and abs(2.0 * step) <= abs(dxold)
        dxold = dx
        if newton:
            dx, x = step, xn
        else:
            dx = 0.5 * (xh - xl)
            x = xl + dx
