"""Joint bandwidth selection (include/kdehip.h section 5q) without a GPU: the three new symbols, every refusal the entries make
before they touch a device, the Python front end's refusals, the Julia shim's calls, and the model of tests/bwjoint_model.py
pinned against cases whose answer is known, against its own log-likelihood and against that log-likelihood's differences.

The refusals that read a resident handle (a mask bit at or above ndims, per-point bandwidths of a resident density) need real
handles: they are in tests/test_gpu_bwjoint.py; here the resident entries are refused for their NULL handles."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import bwjoint_model as bm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_bandwidth_joint", "kdehip_bandwidth_joint_device", "kdehip_bandwidth_joint_device_batch"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
TOL = C.byref(C.c_double(1e-3))  # the entries take tol by pointer
SHAPES = [(1, 129), (2, 257), (3, 300), (6, 300), (8, 130), (2, 700)]  # what tests/test_gpu_bwjoint.py runs


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    section = hdr[hdr.index("(5q)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name  # declared under (5q)
    assert "kdehip_bwjoint_item" in section
    for name in ("joint_bandwidth", "kde_joint", "joint_bandwidth_device_batch"):
        assert callable(getattr(kdehip, name)), name
    assert callable(kdehip.DeviceDensity.joint_bandwidth)


def test_version_stays_600():
    assert kdehip.version() == 600


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _joint(p, start=None, tol=1e-3, maxiter=5, man=None, bw=True, logl=True, iters=True, status=True, trace=True):
    D = 2 if p is None else p.bt.dims
    s = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
    b, ll, tr = np.zeros(D), np.zeros(1), np.zeros(max(maxiter, 0) + 1)
    it, st = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    return L.kdehip_bandwidth_joint(None if p is None else C.byref(p._cstruct()), _lib.optr(s, _lib.f64p),
                                    None if tol is None else C.byref(C.c_double(tol)), maxiter,
                                    _lib.ptr(b, _lib.f64p) if bw else None, _lib.ptr(ll, _lib.f64p) if logl else None,
                                    _lib.ptr(it, _lib.i32p) if iters else None, _lib.ptr(st, _lib.i32p) if status else None,
                                    _lib.ptr(tr, _lib.f64p) if trace else None, NO_SUCH_DEVICE, man)


def _resident_null(tol=TOL, maxiter=5):
    d1, i1 = _lib.ptr(np.zeros(8), _lib.f64p), _lib.ptr(np.zeros(2, dtype=np.int32), _lib.i32p)
    return L.kdehip_bandwidth_joint_device(None, None, tol, maxiter, d1, d1, i1, i1, None, None)


def test_null_arguments_are_refused():
    p = _density()
    assert _joint(None) == _lib.ERR_ARG
    for miss in ("bw", "logl", "iters", "status"):
        assert _joint(p, **{miss: False}) == _lib.ERR_ARG
    assert _joint(p, tol=None) == _lib.ERR_ARG
    assert _resident_null() == _lib.ERR_ARG
    assert L.kdehip_bandwidth_joint_device_batch(1, None, TOL, 5) == _lib.ERR_ARG
    assert L.kdehip_bandwidth_joint_device_batch(-1, None, TOL, 5) == _lib.ERR_ARG
    items = (_lib.CBwJointItem * 1)()  # a null handle
    assert L.kdehip_bandwidth_joint_device_batch(1, items, TOL, 5) == _lib.ERR_ARG
    assert L.kdehip_bandwidth_joint_device_batch(1, items, None, 5) == _lib.ERR_ARG


@pytest.mark.parametrize("bad", [-1e-300, -1.0, np.inf, -np.inf, np.nan])
def test_a_bad_tolerance_is_refused(bad):
    p = _density()
    assert _joint(p, tol=bad) == _lib.ERR_ARG and "tol" in L.kdehip_last_error().decode()
    items = (_lib.CBwJointItem * 1)()
    assert L.kdehip_bandwidth_joint_device_batch(1, items, C.byref(C.c_double(bad)), 5) == _lib.ERR_ARG
    assert L.kdehip_bandwidth_joint_device_batch(0, None, C.byref(C.c_double(bad)), 5) == _lib.ERR_ARG


def test_a_negative_step_count_is_refused():
    p = _density()
    assert _joint(p, maxiter=-1) == _lib.ERR_ARG
    assert L.kdehip_bandwidth_joint_device_batch(0, None, TOL, -1) == _lib.ERR_ARG


def test_fewer_than_two_points_are_refused():
    one = kdehip.kde(np.zeros((2, 1)), [0.3])
    assert _joint(one) == _lib.ERR_ARG and "two points" in L.kdehip_last_error().decode()


@pytest.mark.parametrize("bad", [0.0, -0.5, np.inf, np.nan, 1e-200, 1e200])
def test_a_bad_start_entry_is_refused(bad):
    """not finite or <= 0 -- and a start whose square, the variance the iteration holds, is 0 or not finite"""
    p = _density()
    assert _joint(p, start=[0.3, bad]) == _lib.ERR_ARG and "start" in L.kdehip_last_error().decode()


def test_a_manifold_byte_above_one_is_refused():
    p = _density()
    keep, bad = _u8([0, 2])
    assert _joint(p, man=bad) == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()


def test_dimensions_outside_one_to_eight_are_unsupported():
    assert _joint(_density(D=9, N=5)) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_are_unsupported_in_evaluates_words():
    p = _density(seed=5)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    out = np.zeros(1)
    cd = p._cstruct()
    pos = np.zeros((1, D))
    assert L.kdehip_evaluate(C.byref(cd), _lib.ptr(pos, _lib.f64p), 1, 0, _lib.ptr(out, _lib.f64p), NO_SUCH_DEVICE) == _lib.ERR_UNSUPPORTED
    words = L.kdehip_last_error().decode()
    for rc in (_joint(p), _joint(p, start=[0.3, 0.3])):
        assert rc == _lib.ERR_UNSUPPORTED and L.kdehip_last_error().decode() == words


def test_nothing_to_do_is_ok():
    assert L.kdehip_bandwidth_joint_device_batch(0, None, TOL, 5) == _lib.KDEHIP_OK
    assert L.kdehip_bandwidth_joint_device_batch(0, None, None, 5) == _lib.ERR_ARG  # (tol is read first)


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p = _density()
    for vals in (None, [0, 0], [1, 0]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for rc in (_joint(p, man=mp), _joint(p, start=[0.2, 0.4], man=mp), _joint(p, trace=False, man=mp),
                   _joint(p, tol=0.0, maxiter=0, man=mp)):
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


def test_python_front_end_refusals():
    p, fake = _density(), _fake_device_density()
    for fn in (lambda: kdehip.joint_bandwidth(np.zeros((2, 3))), lambda: kdehip.joint_bandwidth(None),
               lambda: kdehip.joint_bandwidth([p]),
               lambda: kdehip.joint_bandwidth_device_batch([dict(density=p)], 1e-3, 5)):
        with pytest.raises(TypeError):  # a wrong kind, or a host density where a resident one is needed
            fn()
    for d in (p, fake):
        with pytest.raises(ValueError):
            kdehip.joint_bandwidth(d, start=[0.3])             # one entry per dimension
        with pytest.raises(ValueError):
            kdehip.joint_bandwidth(d, manifold=[1])
        with pytest.raises(ValueError):
            kdehip.joint_bandwidth(d, manifold=[0, 2])
        for kw in (dict(tol=-1.0), dict(tol=math.nan), dict(tol=math.inf), dict(maxiter=-1)):
            with pytest.raises(ValueError):
                kdehip.joint_bandwidth(d, **kw)
    with pytest.raises(ValueError):
        fake.joint_bandwidth(tol=-1.0)
    with pytest.raises(ValueError):
        kdehip.kde_joint(np.zeros((2, 5)), tol=-1.0)
    with pytest.raises(ValueError):
        kdehip.kde_joint(np.zeros((2, 5)), start=[0.3, 0.3, 0.3])
    with pytest.raises(ValueError):
        kdehip.kde_joint(np.zeros((2, 5)), start=[0.3, 0.3], manifold=[0])
    with pytest.raises(ValueError):
        kdehip.joint_bandwidth_device_batch([], -1.0, 5)
    with pytest.raises(ValueError):
        kdehip.joint_bandwidth_device_batch([], 1e-3, -5)
    with pytest.raises(ValueError):
        kdehip.joint_bandwidth_device_batch([dict(density=fake, start=[0.3])], 1e-3, 5)
    assert kdehip.joint_bandwidth_device_batch([], 1e-3, 5) == []


def test_julia_shim_calls_the_new_entry_as_the_header_declares_it():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    m = re.search(r"ccall\(\(:kdehip_bandwidth_joint,\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
    assert m
    types = [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert len(types) == len(params["kdehip_bandwidth_joint"]) == 11
    for jt, ct in zip(types, params["kdehip_bandwidth_joint"]):
        assert ct in shim.JULIA_TO_C[jt], (jt, ct)
    for fn in ("hip_joint_bandwidth", "hip_kde_joint"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    body = code[code.index("function hip_joint_bandwidth("):]
    assert "manifold_bytes(" in body[:body.index("\nend")]
    body = code[code.index("function hip_kde_joint("):]
    assert "hip_joint_bandwidth(" in body[:body.index("\nend")]


# ---- the model itself ----------------------------------------------------------------------------------------------------
TWO = (np.array([[0.0, 3.0], [0.0, 4.0]]), np.array([0.5, 0.5]), None)


def test_model_two_points_give_their_differences_after_one_step():
    """T_ik / S0_i = d_k^2 whatever v is: (9, 16) after the first step, and the second has length 0"""
    L0, vn = bm.step(TWO, np.array([0.7, 1.9]))
    assert vn.tolist() == [9.0, 16.0]
    bw, logl, iters, status, trace = bm.iterate(TWO, [1.0, 1.0], 1e-3, 200)
    assert bw.tolist() == [3.0, 4.0] and iters == 2 and status == 0 and len(trace) == 3
    assert trace[1] == trace[2] == logl
    # each point's leave-one-out density is one Gaussian at the other point, one standard deviation away in each dimension
    assert abs(logl - (-1.0 - math.log(2.0 * math.pi * 12.0))) <= 1e-14


@pytest.mark.parametrize("D,N", SHAPES + [(2, 8193)])
def test_model_trace_never_decreases(D, N):
    pts, w = bm.two_clusters(D, N)
    big = N > 1000  # (one sweep of 8193 points takes the model seconds: the GPU test of that size takes one step)
    bw, logl, iters, status, trace = bm.iterate((pts, w, None), bm.silverman(pts), 1e-3, 2 if big else 200)
    assert status == 0 and (big or iters > 0) and len(trace) == abs(iters) + 1
    assert np.all(np.diff(trace) >= -1e-12 * max(1.0, abs(logl))), np.diff(trace).min()
    assert trace[-1] > trace[0]


@pytest.mark.parametrize("D,N", [(1, 129), (3, 300), (6, 300)])
def test_model_logl_is_the_leave_one_out_likelihood_at_the_returned_bandwidth(D, N):
    pts, w = bm.two_clusters(D, N)
    bw, logl, iters, status, trace = bm.iterate((pts, w, None), bm.silverman(pts), 1e-3, 200)
    assert abs(logl - bm.loo_logl((pts, w, None), bw)) <= 1e-12 * max(1.0, abs(logl))
    assert abs(trace[0] - bm.loo_logl((pts, w, None), bm.silverman(pts))) <= 1e-12 * max(1.0, abs(trace[0]))


def test_model_loo_logl_is_the_log_domain_evalAvgLogL_model():
    """L is evalAvgLogL(bd, bd) of section 5f, as tests/logdensity_model.py restates it"""
    from tests import logdensity_model as lm
    pts, w = bm.two_clusters(3, 300)
    sd = bm.silverman(pts)
    want = lm.eval_avg_logl_log((pts, w, sd * sd))[0]
    assert abs(bm.loo_logl((pts, w, None), sd) - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("D,N,man", [(2, 60, None), (3, 80, None), (2, 60, [0, 1])])
def test_model_fixed_point_is_a_stationary_point_of_the_likelihood(D, N, man):
    pts, w = bm.two_clusters(D, N)
    dens = (pts, w, None)
    bw, logl, iters, status, _ = bm.iterate(dens, bm.silverman(pts), 1e-10, 5000, man)
    assert iters > 0 and status == 0
    h = 1e-4
    for k in range(D):
        up, dn = bw.copy(), bw.copy()
        up[k] *= math.exp(h)
        dn[k] *= math.exp(-h)
        fd = (bm.loo_logl(dens, up, man) - bm.loo_logl(dens, dn, man)) / (2.0 * h)
        assert abs(fd) < 1e-6, (k, fd)


def test_model_a_duplicate_pair_is_each_others_neighbour():
    """the self term is skipped by INDEX: two coincident points see each other at distance 0"""
    pts = np.array([[0.0, 0.0, 5.0], [1.0, 1.0, -2.0]])
    w = np.array([0.25, 0.25, 0.5])
    v = np.array([0.04, 0.04])
    m, S0, T = bm._sweep(pts, w, v)
    assert m[0] == 0.0 and m[1] == 0.0            # the twin, at distance 0, sets the maximum
    assert abs(S0[0] - 0.25) <= 1e-15 and np.all(T[:2] < 1e-100)   # the far point underflows
    assert m[2] < -100.0


def test_model_degenerate_data_freeze_the_iteration():
    pts, w = bm.two_clusters(2, 40)
    pts[1] = 0.75                                  # a dimension in which all points coincide
    start = np.array([0.3, 0.2])
    bw, logl, iters, status, trace = bm.iterate((pts, w, None), start, 1e-3, 50)
    assert status == 1 and iters == 0 and np.array_equal(bw, start) and len(trace) == 1 and np.isfinite(logl)
    one = np.zeros(40)
    one[7] = 1.0                                   # one point of positive weight
    bw, logl, iters, status, trace = bm.iterate((bm.two_clusters(2, 40)[0], one, None), start, 1e-3, 50)
    assert status == 1 and iters == 0 and np.array_equal(bw, start) and logl == -math.inf


def test_model_angle_cluster_across_the_cut_of_the_circle():
    """the premise of the GPU test of the same name"""
    pts = bm.angle_data()
    N = pts.shape[1]
    assert np.sum(pts[1] < 0.0) == 1 and pts[1].max() < math.pi and pts[1].min() >= -math.pi
    dens = (pts, np.full(N, 1.0 / N), None)
    circle = bm.iterate(dens, [0.5, 0.5], 1e-3, 200, [0, 1])
    line = bm.iterate(dens, [0.5, 0.5], 1e-3, 200)
    assert circle[2] > 0 and line[2] > 0 and circle[0][1] < 0.2 and line[0][1] > 1.0
    shifted = bm.iterate((bm.angle_data(shift=2.0 * math.pi), dens[1], None), [0.5, 0.5], 1e-3, 200, [0, 1])
    assert np.all(np.abs(shifted[0] - circle[0]) <= 1e-12)


def test_model_improves_on_the_marginal_bandwidth_in_six_dimensions():
    """the premise of the GPU test of the same name: from the bandwidth the oracle's kde!(points) selects, the joint
    iteration gains at least 1.0 nat per point on the 6-D data (3.99 when this was written)"""
    from oracle import oracle
    pts = bm.improvement_data()
    w = np.full(pts.shape[1], 1.0 / pts.shape[1])
    sd = oracle.auto_bandwidth(pts)[0]
    bw, logl, iters, status, trace = bm.iterate((pts, w, None), sd, 1e-3, 200)
    print(f"6-D, N = 300: L(marginal bw) = {trace[0]:.4f}, L(joint bw) = {logl:.4f}, {iters} sweeps")
    assert status == 0 and iters > 0
    assert logl - bm.loo_logl((pts, w, None), sd) >= 1.0
