"""Circular dimensions in evaluation, log-likelihoods and the bandwidth search (include/kdehip.h section 5d) without a GPU:
the NumPy model of tests/circular_model.py pinned against the oracle with an all-Euclidean manifold, the model's own
golden-section comparisons far from a tie at the seeds the GPU tests use, the argument checks every new entry makes before
it touches a device, and the new symbols."""
import ctypes as C
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from oracle import oracle
from tests import circular_model as cm

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_evaluate_manifold", "kdehip_evaluate_device_manifold", "kdehip_evaluate_device_at_manifold",
       "kdehip_eval_avg_logl_manifold", "kdehip_eval_avg_logl_device_manifold", "kdehip_eval_avg_logl_device_batch_manifold",
       "kdehip_auto_bandwidth_manifold", "kdehip_make_density_auto_manifold", "kdehip_density_from_device_points_manifold"]


@pytest.mark.parametrize("D,N,Nq,weighted", [(1, 100, 33, False), (2, 257, 300, True), (3, 130, 129, False), (6, 65, 70, True)])
def test_model_evaluation_equals_the_oracle_when_euclidean(D, N, Nq, weighted):
    pts, w, bw, pos = cm.circular_case(10 * D + N, D, N, Nq, [1] * D, weighted)  # (the circular DATA, Euclidean operators)
    o = oracle.OracleDensity(pts, bw, w)
    for man in (None, [0] * D):
        assert np.allclose(cm.eval_direct(pts, w, bw ** 2, pos, man), oracle.eval_direct(o, pos), rtol=1e-12, atol=1e-300)
        assert np.allclose(cm.eval_direct(pts, w, bw ** 2, manifold=man, loo=True), oracle.eval_direct(o, loo=True), rtol=1e-12)


@pytest.mark.parametrize("D,N", [(1, 100), (2, 300), (3, 64), (2, 129), (4, 65)])
def test_model_bandwidth_equals_the_oracle_when_euclidean(D, N):
    rng = np.random.default_rng(100 + D)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.3, 3.0, size=(D, 1)) + rng.uniform(-2, 2, size=(D, 1))
    bw, nev, _ = cm.auto_bandwidth(pts, [0] * D)
    obw, onev = oracle.auto_bandwidth(pts)
    assert np.allclose(bw, obw, rtol=1e-9, atol=0), (bw, obw)
    assert nev == onev


@pytest.mark.parametrize("D,N,man", cm.BANDWIDTH_CASES)
def test_model_searches_are_far_from_a_tie(D, N, man):
    """two correct implementations may differ by rounding in f1, f2 (1e-12 relative at most: the bound on the likelihoods
    they are sums of); a comparison decided by a gap a thousand times wider, 1e-9, cannot flip"""
    pts = cm.bandwidth_case(D, N, man)
    _, _, traces = cm.auto_bandwidth(pts, man)
    assert cm.min_tie_gap(traces) > 1e-9
    _, _, traces = cm.auto_bandwidth(pts, [0] * D)
    assert cm.min_tie_gap(traces) > 1e-9


def test_the_wrap_matters_in_the_model():
    """a symmetric 1-D cluster on the cut, evaluated at the cut: the Euclidean sum sees half of it"""
    rng = np.random.default_rng(5)
    a = math.pi + 0.3 * rng.standard_normal(400)
    a = np.concatenate([a, 2.0 * math.pi - a])  # symmetric about pi
    pts = np.where(a >= math.pi, a - 2.0 * math.pi, a).reshape(1, -1)
    at = np.array([[-math.pi]])
    circ = cm.eval_direct(pts, None, [0.04], at, [1])[0]
    eucl = cm.eval_direct(pts, None, [0.04], at, [0])[0]
    assert 1.9 < circ / eucl < 2.1


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kdehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def test_bad_manifold_bytes_are_refused_before_the_device():
    p, q = _density(seed=1), _density(seed=2)
    cp, cq = p._cstruct(), q._cstruct()
    bad, badp = _u8([0, 2])
    out = np.zeros(20)
    res = C.c_double(0.0)
    pos = np.zeros(4)
    L = _lib.lib
    assert L.kdehip_evaluate_manifold(C.byref(cp), _lib.ptr(pos, _lib.f64p), 2, 0, _lib.ptr(out, _lib.f64p), NO_SUCH_DEVICE, badp) == _lib.ERR_ARG
    assert "manifold" in L.kdehip_last_error().decode()
    assert L.kdehip_eval_avg_logl_manifold(C.byref(cp), C.byref(cq), 0, C.byref(res), NO_SUCH_DEVICE, badp) == _lib.ERR_ARG
    assert "manifold" in L.kdehip_last_error().decode()
    pts = np.zeros(2 * 10) + np.arange(20)
    bw = np.zeros(2)
    assert L.kdehip_auto_bandwidth_manifold(2, 10, _lib.ptr(pts, _lib.f64p), _lib.ptr(bw, _lib.f64p), None, NO_SUCH_DEVICE, badp) == _lib.ERR_ARG
    assert "manifold" in L.kdehip_last_error().decode()
    d = kdehip.density._empty_density(2, 10)
    bt = d.bt
    f, i = _lib.f64p, _lib.i64p
    rc = L.kdehip_make_density_auto_manifold(
        2, 10, _lib.ptr(pts, f), _lib.ptr(bw, f), None, NO_SUCH_DEVICE, _lib.ptr(bt.centers, f), _lib.ptr(bt.ranges, f),
        _lib.ptr(bt.weights, f), _lib.ptr(bt.left_child, i), _lib.ptr(bt.right_child, i), _lib.ptr(bt.lowest_leaf, i),
        _lib.ptr(bt.highest_leaf, i), _lib.ptr(bt.permutation, i), _lib.ptr(d.means, f), _lib.ptr(d.bandwidth, f),
        _lib.ptr(d.bandwidthMin, f), _lib.ptr(d.bandwidthMax, f), badp)
    assert rc == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()
    h = C.c_void_p()
    assert L.kdehip_density_from_device_points_manifold(C.byref(h), C.c_void_p(256), 2, 10, NO_SUCH_DEVICE, None, None, None, badp) == _lib.ERR_ARG
    assert "manifold" in L.kdehip_last_error().decode()


def test_valid_and_null_manifolds_get_as_far_as_the_device():
    """NULL, all zeros and a valid circular manifold pass the argument checks: the call then fails on the device ordinal"""
    p, q = _density(seed=1), _density(seed=2)
    cp, cq = p._cstruct(), q._cstruct()
    out, res, pos = np.zeros(20), C.c_double(0.0), np.zeros(4)
    L = _lib.lib
    for vals in (None, [0, 0], [1, 0], [1, 1]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for rc in (L.kdehip_evaluate_manifold(C.byref(cp), _lib.ptr(pos, _lib.f64p), 2, 0, _lib.ptr(out, _lib.f64p), NO_SUCH_DEVICE, mp),
                   L.kdehip_eval_avg_logl_manifold(C.byref(cp), C.byref(cq), 0, C.byref(res), NO_SUCH_DEVICE, mp),
                   L.kdehip_eval_avg_logl_manifold(C.byref(cp), C.byref(cp), 1, C.byref(res), NO_SUCH_DEVICE, mp)):
            assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in L.kdehip_last_error().decode().lower()


def test_the_existing_refusals_hold_with_a_manifold():
    p, q3 = _density(D=2), _density(D=3)
    keep, mp = _u8([1, 0])
    res = C.c_double(0.0)
    L = _lib.lib
    assert L.kdehip_eval_avg_logl_manifold(C.byref(p._cstruct()), C.byref(q3._cstruct()), 0, C.byref(res), NO_SUCH_DEVICE, mp) == _lib.ERR_DIM_MISMATCH
    assert L.kdehip_eval_avg_logl_manifold(None, None, 0, C.byref(res), NO_SUCH_DEVICE, mp) == _lib.ERR_ARG
    assert L.kdehip_evaluate_manifold(None, None, 0, 0, None, NO_SUCH_DEVICE, mp) == _lib.ERR_ARG
    assert L.kdehip_evaluate_device_manifold(None, None, 3, 0, None, None, mp) == _lib.ERR_ARG
    assert L.kdehip_evaluate_device_at_manifold(None, None, None, None, mp) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_device_manifold(None, None, 0, None, mp) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_device_batch_manifold(1, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_device_batch_manifold(-1, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_device_batch_manifold(0, None, None, None) == _lib.KDEHIP_OK
    items = (_lib.CLoglManifoldItem * 1)()  # null handles
    assert L.kdehip_eval_avg_logl_device_batch_manifold(1, items, C.c_void_p(256), None) == _lib.ERR_ARG
    assert L.kdehip_auto_bandwidth_manifold(2, 1, _lib.ptr(np.zeros(2), _lib.f64p), _lib.ptr(np.zeros(2), _lib.f64p), None, NO_SUCH_DEVICE, mp) == _lib.ERR_ARG
    assert L.kdehip_auto_bandwidth_manifold(9, 5, _lib.ptr(np.zeros(45), _lib.f64p), _lib.ptr(np.zeros(9), _lib.f64p), None, NO_SUCH_DEVICE, None) == _lib.ERR_UNSUPPORTED


def test_python_front_end_refusals():
    p = _density()
    with pytest.raises(ValueError):
        kdehip.kde(np.zeros((2, 5)) + np.arange(5), [0.3], manifold=["euclid", "circular"])  # explicit bandwidth
    with pytest.raises(ValueError):
        kdehip.evaluateDualTree(p, np.zeros((2, 3)), manifold=[1])          # one entry per dimension
    with pytest.raises(ValueError):
        kdehip.evalAvgLogL(p, p, manifold=[1, 0, 0])
    with pytest.raises(ValueError):
        kdehip.auto_bandwidth(np.zeros((2, 5)), manifold=[1])
    with pytest.raises(KeyError):
        kdehip.entropy(p, manifold=["euclid", "torus"])
