"""Pure Python / NumPy model of the kernel sum of include/kdehip.h section 5g and of the closed forms built on it -- the
yardstick of tests/test_ksum_host.py and tests/test_gpu_ksum.py.

    S(A, B; v) = sum_j b_j sum_i a_i exp(-1/2 sum_k diff_k(y_jk, x_ik)^2 / v_k)

A double loop over (j, i): the outer one in Python, the inner one element by element through NumPy, every term kept and the
whole sum taken ONCE by math.fsum (exactly rounded, so the model has no summation order and no summation error).  The wrap
of a circular dimension is tests/pymodel.py wrapRad itself, applied to the difference.

Densities are plain arrays: points (D, N), weights (N, summing to 1), var = per-dimension VARIANCES (D)."""
import math

import numpy as np

from tests.pymodel import wrapRad

_wrap = np.frompyfunc(wrapRad, 1, 1)  # the scalar expression itself, element by element: no second formula


def terms(xa, wa, xb, wb, v, manifold=None):
    """every b_j a_i exp(...) of the double sum, as one flat list"""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    wa, wb = np.asarray(wa, dtype=np.float64), np.asarray(wb, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    D, N = xa.shape
    assert xb.shape[0] == D and v.shape == (D,) and wa.shape == (N,) and wb.shape == (xb.shape[1],)
    man = [0] * D if manifold is None else [int(m) for m in manifold]
    out = []
    for j in range(xb.shape[1]):
        acc = np.zeros(N)
        for k in range(D):
            d = xb[k, j] - xa[k]
            if man[k]:
                d = _wrap(d).astype(np.float64)
            acc += d * d * (-0.5 / v[k])
        out.extend((wb[j] * (wa * np.exp(acc))).tolist())
    return out


def S(xa, wa, xb, wb, v, manifold=None):
    return math.fsum(terms(xa, wa, xb, wb, v, manifold))


def norm(v):
    """prod_k sqrt(2 pi v_k)"""
    return math.prod(math.sqrt(2.0 * math.pi * float(vk)) for vk in v)


def kernel_sum(a, b, v=None, normalize=False, manifold=None):
    """a, b = (points, weights, var); v None: the sum of the two densities' variances"""
    v = np.asarray(a[2], dtype=np.float64) + np.asarray(b[2], dtype=np.float64) if v is None else np.asarray(v, dtype=np.float64)
    s = S(a[0], a[1], b[0], b[1], v, manifold)
    return s / norm(v) if normalize else s


def inters_intg(p, q, manifold=None):
    """the exact integral of p q: every pair of kernels is a normal density of the difference of the centres, variances added"""
    return kernel_sum(p, q, None, True, manifold)


def ise(p, q, manifold=None):
    """(value, sum of the three terms' magnitudes)"""
    pp, pq, qq = inters_intg(p, p, manifold), inters_intg(p, q, manifold), inters_intg(q, q, manifold)
    return pp - 2.0 * pq + qq, pp + 2.0 * pq + qq


def mmd(p, q, bw, manifold=None):
    """biased MMD^2 under the Gaussian kernel of standard deviation bw (1 or D entries); (value, magnitudes)"""
    D = np.asarray(p[0]).shape[0]
    sd = np.broadcast_to(np.asarray(bw, dtype=np.float64).ravel(), (D,))
    v = sd * sd
    pp, pq, qq = (kernel_sum(a, b, v, False, manifold) for a, b in ((p, p), (p, q), (q, q)))
    return pp - 2.0 * pq + qq, pp + 2.0 * pq + qq


def normal_pdf(d, var):
    return math.exp(-0.5 * d * d / var) / math.sqrt(2.0 * math.pi * var)
