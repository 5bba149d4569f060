"""The exact product of two densities (include/kdehip.h section 5p) without a GPU: the new symbols, every refusal the host
entries make before they touch a device, the Python front end's refusals, and the model of tests/prodexact_model.py
against a brute-force enumeration of the closed form.

The refusals that read a resident handle (different dimensions, per-point bandwidths, pts without ind of resident
densities) need real handles: they are in tests/test_gpu_prodexact.py; here the resident entries are refused for their
NULL handles."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import prodexact_model as pm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_prod_exact", "kdehip_prod_exact_device", "kdehip_prod_exact_device_batch", "kdehip_product_components",
       "kdehip_product_components_device"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def _err():
    return L.kdehip_last_error().decode()


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    assert hdr.index("(5o)") < hdr.index("(5p)")
    section = hdr[hdr.index("(5p)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name  # declared under (5p)
    assert "kdehip_prod_exact_item" in section
    assert C.sizeof(_lib.CProdExactItem) == 64
    flat = " ".join(section.replace(" * ", " ").split())
    for words in ("within a relative 1e-9 of a boundary may resolve to the neighbouring leaf", "No atomics",
                  "Everything else about a label is exact", "circular dimensions, partialDimMask, more than two densities",
                  "fp32", "finite where the integral itself, 5g, underflows to 0"):
        assert words in flat, words
    for name in ("prod_exact", "product_components", "log_intersIntg", "mul_exact", "prod_exact_device_batch"):
        assert callable(getattr(kdehip, name)), name
    assert callable(kdehip.DeviceDensity.prod_exact)


def test_version_stays_600():
    assert kdehip.version() == 600


def test_the_julia_shim_binds_the_host_entry():
    shim.test_every_ccall_matches_the_header()
    assert set(NEW) <= set(shim.header_params())
    code = shim.strip_code(open(shim.SHIM).read())
    for name in ("function hip_prod_exact(", "function hip_log_intersIntg("):
        assert name in code, name
    assert code.count("ccall((:kdehip_prod_exact, libkdehip)") == 2


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _prod(p, q, Np=4, pts=True, ind=True, logz=True):
    D = 2 if p is None else p.bt.dims
    n = max(Np, 1)
    x, idx, lz = np.zeros((n, D)), np.zeros((n, 2), dtype=np.int64), np.zeros(1)
    return L.kdehip_prod_exact(None if p is None else C.byref(p._cstruct()), None if q is None else C.byref(q._cstruct()), Np, 7, 0,
                               _lib.ptr(x, _lib.f64p) if pts else None, _lib.ptr(idx, _lib.i64p) if ind else None,
                               _lib.ptr(lz, _lib.f64p) if logz else None, NO_SUCH_DEVICE)


def _comp(p, q, means=True, weights=True, var=True):
    N1, N2, D = (4, 4, 2) if p is None or q is None else (p.bt.num_points, q.bt.num_points, p.bt.dims)
    m, w, v = np.zeros((N1 * N2, D)), np.zeros(N1 * N2), np.zeros(D)
    f = _lib.f64p
    return L.kdehip_product_components(None if p is None else C.byref(p._cstruct()), None if q is None else C.byref(q._cstruct()),
                                       _lib.ptr(m, f) if means else None, _lib.ptr(w, f) if weights else None,
                                       _lib.ptr(v, f) if var else None, NO_SUCH_DEVICE)


def test_null_arguments_are_refused():
    p, q = _density(), _density(seed=4)
    for rc in (_prod(None, q), _prod(p, None), _comp(None, q), _comp(p, None)):
        assert rc == _lib.ERR_ARG and "null" in _err()
    assert _prod(p, q, pts=False, ind=False, logz=False) == _lib.ERR_ARG and "null" in _err()  # nothing asked for
    for rc in (_prod(p, q, ind=False), _prod(p, q, pts=False)):                                  # together or not at all
        assert rc == _lib.ERR_ARG and "pts and ind are given together" in _err()
    for kw in (dict(means=False), dict(weights=False), dict(var=False)):
        assert _comp(p, q, **kw) == _lib.ERR_ARG and "null" in _err()
    d = C.c_void_p(256)
    assert L.kdehip_prod_exact_device(None, None, 1, 7, 0, d, d, d, None) == _lib.ERR_ARG and "null density" in _err()
    assert L.kdehip_product_components_device(None, None, d, d, d, None) == _lib.ERR_ARG and "null density" in _err()
    assert L.kdehip_prod_exact_device_batch(1, None, None) == _lib.ERR_ARG and "bad item list" in _err()
    assert L.kdehip_prod_exact_device_batch(-1, None, None) == _lib.ERR_ARG
    items = (_lib.CProdExactItem * 1)()  # null handles
    assert L.kdehip_prod_exact_device_batch(1, items, None) == _lib.ERR_ARG and "null density" in _err()


def test_a_negative_count_is_refused():
    p, q = _density(), _density(seed=4)
    assert _prod(p, q, Np=-1) == _lib.ERR_ARG and "Np" in _err()


def test_different_dimensions_are_a_mismatch():
    p, q = _density(D=2), _density(D=3)
    for rc in (_prod(p, q), _comp(p, q)):
        assert rc == _lib.ERR_DIM_MISMATCH and "dimensions of two BallTreeDensities must match" in _err()


def test_dimensions_outside_one_to_eight_are_unsupported():
    p = _density(D=9, N=5)
    for rc in (_prod(p, p), _comp(p, p)):
        assert rc == _lib.ERR_UNSUPPORTED and "KDEHIP_MAX_DIMS" in _err()


@pytest.mark.parametrize("which", [0, 1])
def test_per_point_bandwidths_are_unsupported(which):
    pair = [_density(seed=5), _density(seed=6)]
    bad = pair[which]
    N, D = bad.bt.num_points, bad.bt.dims
    bad.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    for rc in (_prod(*pair), _comp(*pair)):
        assert rc == _lib.ERR_UNSUPPORTED and "per-point" in _err()


def test_too_many_components_are_unsupported():
    p, q = _density(D=1, N=1025), _density(D=1, N=1024, seed=4)
    assert _comp(p, q) == _lib.ERR_UNSUPPORTED and "2^20" in _err()


def test_nothing_to_do_is_ok():
    p, q = _density(), _density(seed=4)
    assert _prod(p, q, Np=0, logz=False) == _lib.KDEHIP_OK
    assert L.kdehip_prod_exact_device_batch(0, None, None) == _lib.KDEHIP_OK


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p, q = _density(D=3), _density(D=3, N=7, seed=4)
    for rc in (_prod(p, q), _prod(p, q, logz=False), _prod(p, q, pts=False, ind=False), _prod(p, q, Np=0), _prod(p, p),
               _comp(p, q)):
        assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE) and "device" in _err().lower()


def test_python_front_end_refusals():
    p2, p3 = _density(D=2), _density(D=3)
    for fn in (kdehip.prod_exact, kdehip.product_components, kdehip.log_intersIntg):
        with pytest.raises(ValueError, match="dimensions"):
            fn(p2, p3)
        with pytest.raises(TypeError):
            fn(p2, np.zeros((2, 4)))
    with pytest.raises(TypeError):
        kdehip.prod_exact(p2)
    with pytest.raises(ValueError, match="at least two"):
        kdehip.prod_exact([p2])
    with pytest.raises(ValueError, match="dimensions"):
        kdehip.prod_exact([p2, p2, p3])
    big = _density(D=1, N=300)
    with pytest.raises(ValueError, match="prodAppxMSGibbsS"):
        kdehip.prod_exact([big, big, big], 10, seed=1)  # the intermediate would have 90,000 components
    with pytest.raises(TypeError):
        kdehip.mul_exact(p2, p2)  # resident densities only
    with pytest.raises(TypeError):
        kdehip.prod_exact_device_batch([dict(p=p2, q=p2, Np=1)])


# ---- the model against brute force ------------------------------------------------------------------------------------------
def _normal_pdf(d, var):
    return math.exp(-0.5 * d * d / var) / math.sqrt(2.0 * math.pi * var)


def _brute(p, q):
    """the closed form term by term: weights alpha_i beta_j prod_k N(a_ik - b_jk; 0, u_k + v_k) normalised by their sum,
    means (a v + b u) / (u + v), and log of the sum"""
    (A, alpha, u), (B, beta, v) = p, q
    N1, N2, D = A.shape[1], B.shape[1], A.shape[0]
    w, means = np.zeros(N1 * N2), np.zeros((N1 * N2, D))
    for i in range(N1):
        for j in range(N2):
            w[i * N2 + j] = alpha[i] * beta[j] * math.prod(_normal_pdf(A[k, i] - B[k, j], u[k] + v[k]) for k in range(D))
            means[i * N2 + j] = [(A[k, i] * v[k] + B[k, j] * u[k]) / (u[k] + v[k]) for k in range(D)]
    Z = math.fsum(w.tolist())
    return means, w / Z, math.log(Z)


def _pair(D, N1, N2, weighted, seed):
    rng = np.random.default_rng(seed)
    def one(N):
        w = rng.uniform(0.1, 1.0, size=N) if weighted else np.ones(N)
        if weighted:
            w[1] = 0.0
        return rng.standard_normal((D, N)), w / w.sum(), rng.uniform(0.1, 0.5, size=D)
    return one(N1), one(N2)


@pytest.mark.parametrize("D,N1,N2,weighted", [(1, 4, 4, False), (3, 5, 4, True)])
def test_model_equals_the_enumerated_closed_form(D, N1, N2, weighted):
    p, q = _pair(D, N1, N2, weighted, 100 * D + N1)
    means, w, var = pm.components(p, q)
    bmeans, bw, blogz = _brute(p, q)
    assert np.all(np.abs(w - bw) <= 1e-12) and np.all(np.abs(means - bmeans) <= 1e-12)
    assert abs(math.fsum(w.tolist()) - 1.0) <= 1e-14
    assert abs(pm.logz(p, q) - blogz) <= 1e-12 * max(1.0, abs(blogz))
    assert np.all(np.abs(var - p[2] * q[2] / (p[2] + q[2])) <= 1e-16)
    if weighted:
        assert not w.reshape(N1, N2)[1].any() and not w.reshape(N1, N2)[:, 1].any()  # exactly 0 outside S_p x S_q
    mu, va = pm.mixture_moments(p, q)
    assert np.all(np.abs(mu - (bw[:, None] * bmeans).sum(axis=0)) <= 1e-12)
    assert np.all(va >= var)


def test_model_labels_follow_the_cumulative_weights():
    p, q = _pair(3, 5, 4, True, 9)
    perm_p, perm_q = np.array([3, 1, 5, 2, 4]), np.array([2, 4, 1, 3])
    _, w, _ = pm.components(p, q)
    W = w.reshape(5, 4)
    rowsum = W.sum(axis=1)
    Ci = np.cumsum(rowsum)
    for u0, u1 in ((1e-12, 1e-12), (0.3, 0.7), (0.77, 0.21), (1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53)):
        ind, leaves, gap = pm.draw_labels(p, perm_p, q, perm_q, [[u0, u1]])
        i, j = leaves[0]
        assert i == min(int(np.searchsorted(Ci, u0 * Ci[-1], side="right")), 4) or gap[0] < 1e-9
        Cj = np.cumsum(W[i])
        assert j == min(int(np.searchsorted(Cj, u1 * Cj[-1], side="right")), 3) or gap[0] < 1e-9
        assert p[1][i] > 0.0 and q[1][j] > 0.0                       # never a weightless leaf
        assert tuple(ind[0]) == (perm_p[i], perm_q[j])
    n = np.array([[0.5, -1.0, 2.0]])
    x = pm.points(p, q, leaves, n)
    s = p[2] + q[2]
    assert np.allclose(x[0], (p[0][:, i] * q[2] + q[0][:, j] * p[2]) / s + np.sqrt(p[2] * q[2] / s) * n[0], rtol=1e-14)


def test_model_empty_sets():
    p, q = _pair(2, 4, 3, False, 1)
    none = (q[0], np.zeros(3), q[2])
    assert pm.logz(p, none) == -math.inf
    ind, leaves, gap = pm.draw_labels(p, np.arange(1, 5), none, np.arange(1, 4), [[0.5, 0.5]])
    assert not ind.any() and (leaves == -1).all()
    assert np.isnan(pm.points(p, none, leaves, np.zeros((1, 2)))).all()
    assert not pm.components(p, none)[1].any()
    nonep = (p[0], np.zeros(4), p[2])
    assert pm.logz(nonep, q) == -math.inf and not pm.draw_labels(nonep, np.arange(1, 5), q, np.arange(1, 4), [[0.5, 0.5]])[0].any()


def test_model_logz_is_finite_where_the_integral_underflows():
    p, q = _pair(2, 4, 3, False, 2)
    far = (q[0] + 40.0 * math.sqrt(float(np.max(p[2] + q[2]))) * 2.0, q[1], q[2])
    lz = pm.logz(p, far, fma=True)
    assert math.isfinite(lz) and lz < -745.0
