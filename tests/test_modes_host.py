"""Gradients and joint modes (include/kdehip.h section 5h) without a GPU: the five new symbols, every refusal the entries make
before they touch a device, the Python front end's refusals, the Julia shim's calls, and the model of tests/modes_model.py
pinned against its own finite differences and against cases whose answer is known.

The refusals that read a resident handle (a mask bit at or above ndims, per-point bandwidths of a resident density) need
real handles: they are in tests/test_gpu_modes.py; here the resident entries are refused for their NULL handles."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import modes_model as mm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_evaluate_grad", "kdehip_evaluate_grad_device", "kdehip_meanshift", "kdehip_meanshift_device",
       "kdehip_meanshift_device_batch"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
TOL = C.byref(C.c_double(1e-9))  # the entries take tol by pointer


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name
    section = hdr[hdr.index("(5h)"):]
    for name in NEW:
        assert name + "(" in section, name  # declared under (5h)
    assert "kdehip_meanshift_item" in section
    for name in ("evaluate_grad", "meanshift", "meanshift_device_batch", "modes", "getKDEMode"):
        assert callable(getattr(kdehip, name)), name
    assert callable(kdehip.DeviceDensity.evaluate_grad)
    assert "getKDEMode" in kdehip.getKDEMax.__doc__ and "getKDEMax" in kdehip.getKDEMode.__doc__


def test_version_stays_600():
    assert kdehip.version() == 600


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _grad(p, Nq=3, pos=True, val=True, grad=True, man=None):
    D = 2 if p is None else p.bt.dims
    P = np.zeros((max(Nq, 1), D))
    v, g = np.zeros(max(Nq, 1)), np.zeros((max(Nq, 1), D))
    return L.kdehip_evaluate_grad(None if p is None else C.byref(p._cstruct()), _lib.ptr(P, _lib.f64p) if pos else None, Nq, 1,
                                  _lib.ptr(v, _lib.f64p) if val else None, _lib.ptr(g, _lib.f64p) if grad else None,
                                  NO_SUCH_DEVICE, man)


def _shift(p, K=3, start=True, tol=1e-9, maxiter=5, man=None, x=True, logp=True, iters=True):
    D = 2 if p is None else p.bt.dims
    n = max(K, 1)
    S, X, lp, it = np.zeros((n, D)), np.zeros((n, D)), np.zeros(n), np.zeros(n, dtype=np.int32)
    return L.kdehip_meanshift(None if p is None else C.byref(p._cstruct()), _lib.ptr(S, _lib.f64p) if start else None, K,
                              None if tol is None else C.byref(C.c_double(tol)), maxiter, _lib.ptr(X, _lib.f64p) if x else None, _lib.ptr(lp, _lib.f64p) if logp else None,
                              _lib.ptr(it, _lib.i32p) if iters else None, NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p = _density()
    assert _grad(None) == _lib.ERR_ARG
    assert _grad(p, val=False, grad=False) == _lib.ERR_ARG  # nothing asked for
    assert _grad(p, pos=False) == _lib.ERR_ARG
    assert _shift(None) == _lib.ERR_ARG
    for miss in ("x", "logp", "iters"):
        assert _shift(p, **{miss: False}) == _lib.ERR_ARG
    assert _shift(p, tol=None) == _lib.ERR_ARG
    one = np.zeros(4)
    d1, i1 = _lib.ptr(one, _lib.f64p), _lib.ptr(np.zeros(4, dtype=np.int32), _lib.i32p)
    assert L.kdehip_evaluate_grad_device(None, None, 1, 1, C.c_void_p(256), C.c_void_p(256), None, None) == _lib.ERR_ARG
    assert L.kdehip_meanshift_device(None, None, 1, TOL, 5, d1, d1, i1, None) == _lib.ERR_ARG
    assert L.kdehip_meanshift_device_batch(1, None, TOL, 5, None) == _lib.ERR_ARG
    assert L.kdehip_meanshift_device_batch(-1, None, TOL, 5, None) == _lib.ERR_ARG
    items = (_lib.CMeanshiftItem * 1)()  # a null handle
    assert L.kdehip_meanshift_device_batch(1, items, TOL, 5, None) == _lib.ERR_ARG


def test_negative_counts_are_refused():
    p = _density()
    assert _grad(p, Nq=-1) == _lib.ERR_ARG
    assert _shift(p, K=-1) == _lib.ERR_ARG
    assert _shift(p, maxiter=-1) == _lib.ERR_ARG
    assert _shift(p, K=7, start=False) == _lib.ERR_ARG   # the density's own points: nstart must be npts
    items = (_lib.CMeanshiftItem * 1)()
    assert L.kdehip_meanshift_device_batch(1, items, TOL, -1, None) == _lib.ERR_ARG
    assert L.kdehip_meanshift_device_batch(0, None, TOL, -1, None) == _lib.ERR_ARG


@pytest.mark.parametrize("bad", [-1e-300, -1.0, np.inf, -np.inf, np.nan])
def test_a_bad_tolerance_is_refused(bad):
    p = _density()
    assert _shift(p, tol=bad) == _lib.ERR_ARG and "tol" in L.kdehip_last_error().decode()
    items = (_lib.CMeanshiftItem * 1)()
    assert L.kdehip_meanshift_device_batch(1, items, C.byref(C.c_double(bad)), 5, None) == _lib.ERR_ARG
    assert L.kdehip_meanshift_device_batch(0, None, C.byref(C.c_double(bad)), 5, None) == _lib.ERR_ARG


def test_a_manifold_byte_above_one_is_refused():
    p = _density()
    keep, bad = _u8([0, 2])
    for rc in (_grad(p, man=bad), _shift(p, man=bad), _shift(p, K=20, start=False, man=bad)):
        assert rc == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()


def test_dimensions_outside_one_to_eight_are_unsupported():
    p = _density(D=9, N=5)
    assert _grad(p) == _lib.ERR_UNSUPPORTED
    assert _shift(p) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_are_unsupported_in_evaluates_words():
    p = _density(seed=5)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    out = np.zeros(1)
    cd = p._cstruct()
    pos = np.zeros((1, D))
    assert L.kdehip_evaluate(C.byref(cd), _lib.ptr(pos, _lib.f64p), 1, 0, _lib.ptr(out, _lib.f64p), NO_SUCH_DEVICE) == _lib.ERR_UNSUPPORTED
    words = L.kdehip_last_error().decode()
    for rc in (_grad(p), _shift(p), _shift(p, K=N, start=False)):
        assert rc == _lib.ERR_UNSUPPORTED and L.kdehip_last_error().decode() == words


def test_nothing_to_do_is_ok():
    p = _density()
    assert _grad(p, Nq=0) == _lib.KDEHIP_OK
    assert _grad(p, Nq=0, pos=False) == _lib.KDEHIP_OK
    assert _shift(p, K=0) == _lib.KDEHIP_OK
    assert L.kdehip_meanshift_device_batch(0, None, TOL, 5, None) == _lib.KDEHIP_OK
    assert L.kdehip_meanshift_device_batch(0, None, None, 5, None) == _lib.ERR_ARG  # (tol is read first)


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p = _density()
    for vals in (None, [0, 0], [1, 0]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for rc in (_grad(p, man=mp), _grad(p, val=False, man=mp), _grad(p, grad=False, man=mp), _shift(p, man=mp),
                   _shift(p, K=20, start=False, man=mp), _shift(p, tol=0.0, maxiter=0, man=mp)):
            assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in L.kdehip_last_error().decode().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake._host = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    fake.manifold = None
    return fake


class _Tensor:
    """what the front end takes for a device tensor"""
    def data_ptr(self):
        return 256


def test_python_front_end_refusals():
    p, fake = _density(), _fake_device_density()
    pos = np.zeros((2, 3))
    for fn in (lambda: kdehip.evaluate_grad(pos, pos), lambda: kdehip.meanshift(None), lambda: kdehip.modes(pos),
               lambda: kdehip.getKDEMode([p]),
               lambda: kdehip.evaluate_grad(p, _Tensor()), lambda: kdehip.meanshift(p, _Tensor()),  # host density, device points
               lambda: kdehip.modes(p, _Tensor()),
               lambda: kdehip.meanshift_device_batch([dict(density=p, x=None, logp=None, iters=None)], 1e-9, 5)):
        with pytest.raises(TypeError):  # mixed, or a host density where a resident one is needed: the error `kld` raises
            fn()
    with pytest.raises(ValueError):
        kdehip.evaluate_grad(p, np.zeros((3, 4)))   # D rows
    with pytest.raises(ValueError):
        kdehip.meanshift(p, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        kdehip.evaluate_grad(p, pos, manifold=[1])  # one entry per dimension
    with pytest.raises(ValueError):
        kdehip.meanshift(p, pos, manifold=[0, 2])
    with pytest.raises(ValueError):
        kdehip.evaluate_grad(fake, pos, manifold=[0, 2])
    for kw in (dict(tol=-1.0), dict(tol=math.nan), dict(tol=math.inf), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            kdehip.meanshift(p, pos, **kw)
        with pytest.raises(ValueError):
            kdehip.modes(fake, pos, **kw)
    with pytest.raises(ValueError):
        kdehip.meanshift_device_batch([], -1.0, 5)
    with pytest.raises(ValueError):
        kdehip.meanshift_device_batch([], 1e-9, -5)


def test_julia_shim_calls_the_new_entries_as_the_header_declares_them():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    m = re.search(r"ccall\(\(:kdehip_evaluate_grad,\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
    assert m
    types = [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert len(types) == len(params["kdehip_evaluate_grad"])
    for jt, ct in zip(types, params["kdehip_evaluate_grad"]):
        assert ct in shim.JULIA_TO_C[jt], (jt, ct)
    for fn in ("hip_evaluate_grad", "hip_meanshift", "hip_modes", "hip_getKDEMode"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    body = code[code.index("function hip_evaluate_grad("):]
    assert "manifold_bytes(" in body[:body.index("\nend")]


# ---- the model itself ----------------------------------------------------------------------------------------------------
def _model_density(D, N, seed, man=None):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 1.5, size=(D, 1))
    w = rng.uniform(0.05, 1.0, size=N)
    w[::5] = 0.0
    sd = rng.uniform(0.3, 0.6, size=D)
    return pts, w / w.sum(), sd * sd


@pytest.mark.parametrize("D,man", [(1, None), (3, None), (6, None), (2, [0, 1])])
def test_model_gradient_is_the_central_difference_of_its_own_log_p(D, man):
    dens = _model_density(D, 40, 10 + D)
    rng = np.random.default_rng(D)
    X = rng.standard_normal((D, 5))
    _, grad, _ = mm.evaluate_grad(dens, X, man)
    h = 1e-5
    for q in range(X.shape[1]):
        for k in range(D):
            e = np.zeros(D)
            e[k] = h
            fd = (mm.log_p(dens, X[:, q] + e, man) - mm.log_p(dens, X[:, q] - e, man)) / (2.0 * h)
            assert abs(grad[k, q] - fd) <= 1e-6 * max(1.0, abs(grad[k, q])), (q, k, grad[k, q], fd)


def test_model_one_point_is_its_own_mode_after_one_step():
    dens = (np.array([[0.25], [-1.25]]), np.array([1.0]), np.array([0.04, 0.09]))  # (dyadic: the differences are exact)
    xn, dx, _ = mm.step(dens, np.array([1.0, 0.5]))
    assert np.array_equal(xn, dens[0][:, 0])
    x, logp, iters, _ = mm.meanshift(dens, np.array([[1.0], [0.5]]), 1e-9, 10)
    assert np.array_equal(x[:, 0], dens[0][:, 0]) and iters[0] == 2  # the second step has length 0
    assert abs(logp[0] + mm.log_norm(dens[2])) <= 1e-15


def test_model_joint_mode_of_two_far_points_is_the_heavier():
    sd = 0.5
    dens = (np.array([[0.0, 20.0 * sd]]), np.array([0.25, 0.75]), np.array([sd * sd]))
    modes, logp, mass, labels = mm.modes(dens)
    assert modes.shape == (1, 2) and labels.tolist() == [1, 0]
    assert abs(modes[0, 0] - 20.0 * sd) <= 1e-12 and mass.tolist() == [0.75, 0.25] and logp[0] > logp[1]


def test_model_mode_of_a_cluster_across_the_cut_of_the_circle():
    rng = np.random.default_rng(8)
    ang = mm.wrap(math.pi + 0.04 * rng.standard_normal(30))  # around +-pi: both signs occur
    assert ang.min() < -3.0 and ang.max() > 3.0
    w = np.full(30, 1.0 / 30)
    v = np.array([0.01])
    # tol = 1e-13: every start ends within 1e-13 bandwidths of the fixed point, so whichever of them founds the mode (their
    # log p are equal to rounding) the two runs agree far below 1e-12; the rounding of a step is some 1e-16 bandwidths
    m1 = mm.modes((ang[None, :], w, v), tol=1e-13, man=[1])[0]
    assert m1.shape == (1, 1) and -math.pi <= m1[0, 0] < math.pi and abs(abs(m1[0, 0]) - math.pi) < 0.05
    m2 = mm.modes((ang[None, :] + mm.TWO_PI, w, v), tol=1e-13, man=[1])[0]
    assert m2.shape == (1, 1) and abs(mm.wrap(m2[0, 0] - m1[0, 0])) <= 1e-12
    assert mm.modes((ang[None, :], w, v), tol=1e-13)[0].shape == (1, 2)  # on the line the cluster is two, 2 pi apart


def test_model_iteration_agrees_with_the_exactly_rounded_step():
    """the vectorised iteration (pairwise sums) and the fsum step are the same map to rounding"""
    pts, sd, w = mm.three_clusters(1, 129)
    dens = (pts, w / w.sum(), sd * sd)
    x1, _, iters, _ = mm.meanshift(dens, pts[:, :7], 0.0, 1)
    assert iters.tolist() == [-1] * 7
    for q in range(7):
        xn, dx, scale = mm.step(dens, pts[:, q])
        assert np.all(np.abs(x1[:, q] - xn) <= 1e-14 * scale)


@pytest.mark.parametrize("D,N", [(1, 129), (2, 257), (3, 300), (6, 300), (8, 300), (2, 700)])
def test_model_convergence_data_has_three_modes(D, N):
    """what tests/test_gpu_modes.py takes for granted about its convergence data, shape by shape"""
    pts, sd, w = mm.three_clusters(D, N)
    dens = (pts, w / w.sum(), sd * sd)
    x, logp, iters, trace = mm.meanshift(dens, pts, 1e-9, 200)
    assert iters.min() > 0 and iters.max() <= 47
    assert np.all(np.diff(trace, axis=0) >= -1e-12 * np.maximum(1.0, np.abs(trace[:-1])))
    kept, labels = mm.merge(x, logp, iters, sd, 1e-3)
    assert len(kept) == 3 and labels.min() == 0


def test_model_exponent_in_fma_order_is_the_plain_one_to_rounding():
    dens = _model_density(3, 20, 4)
    x = np.array([30.0, -20.0, 25.0])
    d = mm.differences(x, dens[0])
    a, b = mm.exponents(d, dens[2]), mm.exponents(d, dens[2], fma=True)
    assert np.all(a < -1000.0) and np.all(np.abs(a - b) <= 8 * 2.0 ** -53 * np.abs(a))
    assert mm._fma(2.0 ** 27 + 1.0, 2.0 ** 27 + 1.0, -(2.0 ** 54)) == 2.0 ** 28 + 1.0  # the product is not rounded first
