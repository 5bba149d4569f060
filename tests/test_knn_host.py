"""Nearest neighbours on the ball tree (include/kdehip.h section 5n) without a GPU: the two new symbols, every refusal the
entries make before they touch a device, the front end's ValueErrors, and the model of tests/knn_model.py -- which the GPU
tests take their expected values from -- against closed forms.

The closed forms: the Kozachenko-Leonenko formula on 4,096 standard-normal points in 2-D, k = 4, against the entropy of the
law, log(2 pi e) = 2.8379; the Wang-Kulkarni-Verdu formula on two samples of one law against 0.  The margin, 0.1 nat, is
about four standard deviations of either estimator at this N (the sample mean of -log p alone has standard deviation
sqrt(D / 2 / N) = 0.016; the neighbour-distance term adds its own, and a bias of order 1 / sqrt(N))."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import knn_model as km

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_knn", "kdehip_knn_device_at"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    assert hdr.index("(5n)") > hdr.index("(5m)")
    section = hdr[hdr.index("(5n)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name
    for words in ("dmin2", "r_q", "KDEHIP_KNN_MAX_K 32", "Not here"):
        assert words in section, words
    for name in ("knn", "entropy_knn", "kld_knn"):
        assert callable(getattr(kdehip, name)), name
    assert callable(kdehip.DeviceDensity.knn)
    shim = open(os.path.join(ROOT, "kerneldensityestimate.jl_amd", "julia", "KernelDensityEstimateHIP.jl")).read()
    assert ":kdehip_knn" in shim


def _small(D=2, N=20, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [0.3])


def _knn(p, k=1, Nq=1, loo=0, scale=None, man=None, d2=True, idx=True, dev=NO_SUCH_DEVICE):
    D = p.bt.dims
    n = max(Nq, 1, p.bt.num_points) * max(k, 1)
    pos, od, oi, stats = np.zeros((max(Nq, 1), D)), np.zeros(n), np.zeros(n, dtype=np.int64), np.full(2, 7, dtype=np.int64)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    mb = None if man is None else np.ascontiguousarray(man, dtype=np.uint8)
    rc = L.kdehip_knn(C.byref(p._cstruct()), _lib.ptr(pos, _lib.f64p), Nq, k, loo, _lib.optr(sc, _lib.f64p),
                      _lib.ptr(od, _lib.f64p) if d2 else None, _lib.ptr(oi, _lib.i64p) if idx else None,
                      _lib.ptr(stats, _lib.i64p), dev, _lib.optr(mb, _lib.u8p))
    return rc, stats


def test_every_refusal_has_its_code_and_touches_no_device():
    p = _small()  # D = 2, N = 20
    for k in (0, 33, 21, -1):
        assert _knn(p, k=k)[0] == _lib.ERR_ARG and "k" in L.kdehip_last_error().decode(), k
    assert _knn(p, k=20, loo=1)[0] == _lib.ERR_ARG  # leave-one-out: k <= N - 1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _knn(p, scale=[1.0, bad])[0] == _lib.ERR_ARG and "scale" in L.kdehip_last_error().decode(), bad
    assert _knn(p, man=[0, 2])[0] == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()
    assert _knn(_small(D=9))[0] == _lib.ERR_UNSUPPORTED
    assert _knn(p, d2=False)[0] == _lib.ERR_ARG and _knn(p, idx=False)[0] == _lib.ERR_ARG
    assert _knn(p, Nq=-1)[0] == _lib.ERR_ARG
    od, oi = np.zeros(1), np.zeros(1, dtype=np.int64)
    assert L.kdehip_knn(None, None, 0, 1, 0, None, _lib.ptr(od, _lib.f64p), _lib.ptr(oi, _lib.i64p), None, NO_SUCH_DEVICE,
                        None) == _lib.ERR_ARG
    rc, stats = _knn(p, Nq=0)  # no queries: nothing to do, no device
    assert rc == _lib.KDEHIP_OK and stats.tolist() == [0, 0]
    # what is allowed gets as far as the device, which does not exist: k = N, k = N - 1 with leave-one-out, a circular byte
    for kw in (dict(k=20), dict(k=19, loo=1), dict(k=8, scale=[0.5, 2.0]), dict(man=[0, 1])):
        rc, _ = _knn(p, **kw)
        assert rc not in (_lib.KDEHIP_OK, _lib.ERR_UNSUPPORTED, _lib.ERR_DIM_MISMATCH), kw
        assert "knn" not in L.kdehip_last_error().decode() and "manifold" not in L.kdehip_last_error().decode(), kw
    # the resident entry: NULL handles and NULL outputs
    a = C.c_void_p(256)
    assert L.kdehip_knn_device_at(None, None, 1, None, a, a, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_knn_device_at(a, a, 1, None, None, a, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_knn_device_at(a, a, 1, None, a, None, None, None, None) == _lib.ERR_ARG


def test_the_front_end_refuses_what_it_cannot_read():
    p = _small()
    N, D = p.bt.num_points, p.bt.dims
    with pytest.raises(ValueError):
        kdehip.knn(p, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        kdehip.knn(p, np.zeros((2, 4)), order="sorted")
    with pytest.raises(ValueError):
        kdehip.knn(p, np.zeros((2, 4)), metric="manhattan")
    with pytest.raises(ValueError):
        kdehip.knn(p, np.zeros((2, 4)), metric=[1.0, 1.0, 1.0])
    with pytest.raises(TypeError):
        kdehip.knn(np.zeros((2, 4)), np.zeros((2, 4)))
    for k in (0, 33):
        with pytest.raises(kdehip.KdeHipError):
            kdehip.knn(p, np.zeros((2, 4)), k=k, device=NO_SUCH_DEVICE)
    # metric="bandwidth" reads ONE bandwidth vector
    per_point = _small(seed=5)
    per_point.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    with pytest.raises(ValueError, match="per-point"):
        kdehip.knn(per_point, np.zeros((2, 4)), metric="bandwidth", device=NO_SUCH_DEVICE)
    with pytest.raises(kdehip.KdeHipError):  # ... and with one it gets as far as the device
        kdehip.knn(p, np.zeros((2, 4)), metric="bandwidth", device=NO_SUCH_DEVICE)
    # the estimators: Euclidean, uniform weights
    rng = np.random.default_rng(9)
    weighted = kdehip.kde(rng.standard_normal((2, 20)), [0.3], rng.uniform(0.5, 1.0, size=20))
    for fn in (lambda d, **kw: kdehip.entropy_knn(d, device=NO_SUCH_DEVICE, **kw),
               lambda d, **kw: kdehip.kld_knn(d, p, device=NO_SUCH_DEVICE, **kw),
               lambda d, **kw: kdehip.kld_knn(p, d, device=NO_SUCH_DEVICE, **kw)):
        with pytest.raises(ValueError, match="uniform weights"):
            fn(weighted)
    with pytest.raises(ValueError, match="Euclidean"):
        kdehip.entropy_knn(p, manifold=[0, 1], device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError, match="Euclidean"):
        kdehip.kld_knn(p, _small(seed=4), manifold=["circular", "euclid"], device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        kdehip.kld_knn(p, _small(D=3))
    with pytest.raises(TypeError):
        kdehip.kld_knn(p, np.zeros((2, 4)))
    assert kdehip.kld_knn(p, p, device=NO_SUCH_DEVICE) == 0.0  # q is p: exactly 0, nothing computed


def test_the_models_distance_is_the_contracts_chain():
    """fma rounds once: a product whose low half decides the rounding of the sum"""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0
    assert km.fma(a, b, c) == 2.0 ** -29 + 2.0 ** -60 and a * b + c == 2.0 ** -29
    rng = np.random.default_rng(1)
    for x, y, z in (rng.standard_normal((2000, 3)) * 10.0 ** rng.integers(-8, 8, size=(2000, 3))).tolist():
        for zz in (z, 0.0, -x * y):  # (the last: the sum is the product's rounding error alone)
            assert km.fma(x, y, zz) == km.fma_fraction(x, y, zz)
    pts, qry = rng.standard_normal((7, 3)), rng.standard_normal((4, 3))
    plain = km.dist2(pts, qry)
    assert np.array_equal(plain, km.dist2(pts, qry, scale=np.ones(3)))  # s_k = 1: the plain chain's bits
    scaled = km.dist2(pts, qry, scale=np.array([0.3, 1.7, 2.9]))
    assert np.allclose(scaled, ((qry[:, None, :] - pts[None, :, :]) ** 2 * [0.3, 1.7, 2.9]).sum(axis=2), rtol=1e-14, atol=0)
    # the wrap: a query just inside -pi is close to a point just inside +pi
    d = km.dist2(np.array([[math.pi - 0.01]]), np.array([[-math.pi + 0.01]]), circ=(0,))
    assert abs(d[0, 0] - 0.02 ** 2) < 1e-12


def test_the_models_plan_never_loses_a_neighbour():
    """needed chunks hold every one of the k nearest, ties included: the exactness argument, on the model"""
    rng = np.random.default_rng(2)
    pts = np.round(rng.standard_normal((300, 2)), 1)  # rounded: many ties
    pts = pts[np.lexsort((pts[:, 1], pts[:, 0]))]      # a compact leaf order
    orig = rng.permutation(300) + 1
    qry = np.round(rng.standard_normal((40, 2)), 1)
    for k in (1, 8, 32):
        d2, idx = km.knn(pts, orig, qry, k)
        pl = km.plan(pts, orig, qry, k)
        where = np.argsort(orig)  # original index - 1 -> leaf position
        for q in range(qry.shape[0]):
            assert pl["need"][q, where[idx[q] - 1] // 128].all()
        assert 0 < pl["stats"][0] <= pl["stats"][1] == 3


def test_the_models_entropy_formula_against_the_normal_law():
    """model value with this seed: 2.84679 (log(2 pi e) = 2.83788)"""
    rng = np.random.default_rng(4096)
    pts = rng.standard_normal((4096, 2))
    eps = np.empty(4096)
    for q0 in range(0, 4096, 512):  # brute force in slabs: the 5-th smallest of a row is the 4-th neighbour (the 1st is itself)
        eps[q0:q0 + 512] = np.sqrt(np.partition(km.dist2(pts, pts[q0:q0 + 512]), 4, axis=1)[:, 4])
    h = km.entropy_kl(eps, 2, 4)
    print("Kozachenko-Leonenko, 4096 standard-normal points in 2-D, k = 4:", h, "log(2 pi e):", math.log(2 * math.pi * math.e))
    assert abs(h - math.log(2 * math.pi * math.e)) < 0.1


def test_the_models_divergence_formula_on_two_samples_of_one_law():
    """model value with this seed: -0.01791 (the law's value is 0)"""
    rng = np.random.default_rng(4097)
    p, q = rng.standard_normal((4096, 2)), rng.standard_normal((4096, 2))
    rho, nu = np.empty(4096), np.empty(4096)
    for q0 in range(0, 4096, 512):
        rho[q0:q0 + 512] = np.sqrt(np.partition(km.dist2(p, p[q0:q0 + 512]), 4, axis=1)[:, 4])
        nu[q0:q0 + 512] = np.sqrt(np.partition(km.dist2(q, p[q0:q0 + 512]), 3, axis=1)[:, 3])
    d = km.kld_wkv(rho, nu, 2, 4096)
    print("Wang-Kulkarni-Verdu, two samples of 4096 standard-normal points in 2-D, k = 4:", d)
    assert abs(d) < 0.1
