"""Densities with per-point bandwidths (include/kdehip.h sections 4 and 5o) without a GPU: the host builder
kdehip_make_density_varbw against `kde()` and the NumPy model of tests/varbw_model.py, the refusals every new entry makes
before it touches a device, and the Python front end's argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import varbw_model as vm

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_make_density_varbw", "kdehip_evaluate_varbw", "kdehip_evaluate_varbw_device_at", "kdehip_evaluate_varbw_device",
       "kdehip_eval_avg_logl_varbw", "kdehip_eval_avg_logl_varbw_device", "kdehip_density_uniform_bandwidth"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name
    assert "(5o)" in hdr
    for name in ("kde_varbw", "adaptive_scales", "kde_adaptive"):
        assert callable(getattr(kdehip, name)), name


def _points(seed, D, N):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)), rng


TREE_FIELDS = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")


@pytest.mark.parametrize("D,N,weighted", [(1, 1, False), (1, 2, True), (2, 3, False), (3, 130, True), (6, 257, False),
                                          (2, 1500, True)])  # (1500: the top levels build on worker threads)
def test_equal_columns_give_the_bandwidth_of_kde_bit_for_bit(D, N, weighted):
    pts, rng = _points(10 * D + N, D, N)
    sd = rng.uniform(0.2, 0.6, size=D)
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    p = kdehip.kde(pts, sd, w)
    v = kdehip.kde_varbw(pts, np.repeat(sd[:, None], N, axis=1), w)
    assert v.multibandwidth == 1 and p.multibandwidth == 0
    assert np.array_equal(v.bandwidth, p.bandwidth)
    assert np.array_equal(v.means, p.means)
    for f in TREE_FIELDS:
        assert np.array_equal(getattr(v.bt, f), getattr(p.bt, f)), f
    assert v.bandwidthMin.shape == v.bandwidthMax.shape == (2 * N * D,)
    assert np.array_equal(v.bandwidthMin[N * D:], p.bandwidthMin) and np.array_equal(v.bandwidthMax[N * D:], p.bandwidthMax)
    assert np.array_equal(kdehip.getBW(v), kdehip.getBW(p))


@pytest.mark.parametrize("D,N,weighted,tman", [(1, 1, False, None), (1, 2, True, None), (2, 3, False, None),
                                                (3, 130, True, None), (6, 257, False, None), (2, 1500, True, None),
                                                (2, 200, False, ["circular", "euclid"])])
def test_per_point_rows_equal_the_model(D, N, weighted, tman):
    pts, rng = _points(20 * D + N, D, N)
    sd = rng.uniform(0.2, 0.6, size=D)
    bw = sd[:, None] * rng.uniform(0.5, 2.0, size=(D, N))
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    p = kdehip.kde(pts, sd, w, tree_manifold=tman)
    v = kdehip.kde_varbw(pts, bw, w, tree_manifold=tman)
    assert v.multibandwidth == 1
    # the tree, boxes, weights and means do not depend on the bandwidth
    assert np.array_equal(v.means, p.means)
    for f in TREE_FIELDS:
        assert np.array_equal(getattr(v.bt, f), getattr(p.bt, f)), f
    var = bw * bw
    got = [a.reshape(2 * N, D) for a in (v.bandwidth, v.bandwidthMin, v.bandwidthMax)]
    # leaf rows: bw^2 through the permutation, exactly
    leaf = var[:, v.bt.permutation[N:] - 1].T
    for a in got:
        assert np.array_equal(a[N:], leaf)
    assert np.array_equal(kdehip.getBW(v) ** 2, np.sqrt(var) ** 2)
    # internal rows: the model's moment match (the same expressions in the same order: bit for bit), and the slot past the
    # last internal node stays 0
    want = vm.builder_rows(p, var)
    nint = max(N - 1, 1)
    for a, b, what in zip(got, want, ("bandwidth", "bandwidthMin", "bandwidthMax")):
        assert np.array_equal(a[:nint], b[:nint]), what
        assert np.all(a[nint:N] == 0.0), what
    # Min / Max: the subtree's extremes, exactly
    lo, hi = vm.subtree_extremes(p, var)
    assert np.array_equal(got[1][:nint], lo[:nint]) and np.array_equal(got[2][:nint], hi[:nint])


def _build_raw(D, N, pts, bw):
    """kdehip_make_density_varbw on fresh arrays filled with a canary: (rc, arrays)"""
    f = lambda n: np.full(n, -7.0)
    i = lambda n: np.full(n, -7, dtype=np.int64)
    arrs = [f(2 * N * D), f(2 * N * D), f(2 * N), i(2 * N), i(2 * N), i(2 * N), i(2 * N), i(2 * N), f(2 * N * D), f(2 * N * D),
            f(2 * N * D), f(2 * N * D)]
    flat, bflat = np.ascontiguousarray(pts.T).ravel(), np.ascontiguousarray(bw.T).ravel()
    rc = _lib.lib.kdehip_make_density_varbw(
        D, N, _lib.ptr(flat, _lib.f64p), _lib.ptr(bflat, _lib.f64p), None,
        *[_lib.ptr(a, _lib.f64p if a.dtype == np.float64 else _lib.i64p) for a in arrs], None)
    return rc, arrs


@pytest.mark.parametrize("bad", [0.0, -0.3, np.inf, -np.inf, np.nan])
def test_a_bandwidth_that_is_not_finite_and_positive_is_refused_before_anything_is_written(bad):
    pts, rng = _points(3, 2, 17)
    bw = rng.uniform(0.2, 0.6, size=(2, 17))
    rc, _ = _build_raw(2, 17, pts, bw)
    assert rc == _lib.KDEHIP_OK
    bw[1, 16] = bad  # the last entry: every earlier one is fine
    rc, arrs = _build_raw(2, 17, pts, bw)
    assert rc == _lib.ERR_ARG and "bandwidth" in _lib.lib.kdehip_last_error().decode()
    for a in arrs:
        assert np.all(a == -7), "an output array was written"
    with pytest.raises(ValueError):
        kdehip.kde_varbw(pts, bw)


def test_builder_refuses_null_pointers_and_bad_manifolds():
    pts, rng = _points(4, 2, 5)
    flat = np.ascontiguousarray(pts.T).ravel()
    bw = np.full(10, 0.3)
    out = np.zeros(40)
    idx = np.zeros(10, dtype=np.int64)
    fp, ip = _lib.ptr(out, _lib.f64p), _lib.ptr(idx, _lib.i64p)
    L = _lib.lib
    args = [2, 5, _lib.ptr(flat, _lib.f64p), _lib.ptr(bw, _lib.f64p), None, fp, fp, fp, ip, ip, ip, ip, ip, fp, fp, fp, fp, None]
    for k in (2, 3, 5, 8, 13, 15, 16):
        a = list(args)
        a[k] = None
        assert L.kdehip_make_density_varbw(*a) == _lib.ERR_ARG, k
    a = list(args)
    a[0] = 0
    assert L.kdehip_make_density_varbw(*a) == _lib.ERR_ARG
    man = np.array([0, 2], dtype=np.uint8)
    a = list(args)
    a[17] = _lib.ptr(man, _lib.u8p)
    assert L.kdehip_make_density_varbw(*a) == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()


# ---- the entries of section 5o: every refusal comes before a device is touched ---------------------------------------------
def _density(D=2, N=20, seed=3):
    pts, rng = _points(seed, D, N)
    return kdehip.kde_varbw(pts, rng.uniform(0.2, 0.6, size=(D, N)))


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _evaluate(bd, Nq=2, loo=0, log=0, man=None, out=True, pos=True):
    D = 2 if bd is None else bd.bt.dims
    P, res = np.zeros(D * max(Nq, 1)), np.zeros(64)
    cb = None if bd is None else C.byref(bd._cstruct())
    return _lib.lib.kdehip_evaluate_varbw(cb, _lib.ptr(P, _lib.f64p) if pos else None, Nq, loo, log,
                                          _lib.ptr(res, _lib.f64p) if out else None, NO_SUCH_DEVICE, man)


def _logl(bd, at, loo, log=0, man=None, out=True):
    res = C.c_double(0.0)
    cb = None if bd is None else C.byref(bd._cstruct())
    ca = None if at is None else (cb if at is bd else C.byref(at._cstruct()))
    return _lib.lib.kdehip_eval_avg_logl_varbw(cb, ca, int(loo), log, C.byref(res) if out else None, NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p = _density()
    L = _lib.lib
    for log in (0, 1):
        assert _evaluate(None, log=log) == _lib.ERR_ARG
        assert _evaluate(p, log=log, out=False) == _lib.ERR_ARG
        assert _evaluate(p, log=log, pos=False) == _lib.ERR_ARG
        assert _evaluate(p, Nq=-1, log=log) == _lib.ERR_ARG
        assert _logl(None, p, 0, log) == _lib.ERR_ARG
        assert _logl(p, None, 0, log) == _lib.ERR_ARG
        assert _logl(p, p, 1, log, out=False) == _lib.ERR_ARG
        assert L.kdehip_evaluate_varbw_device_at(None, None, 0, log, C.c_void_p(256), None, None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_varbw_device(None, C.c_void_p(256), 3, log, C.c_void_p(256), None, None) == _lib.ERR_ARG
        assert L.kdehip_eval_avg_logl_varbw_device(None, None, 0, log, C.c_void_p(256), None, None) == _lib.ERR_ARG
        assert L.kdehip_eval_avg_logl_varbw_device(None, None, 0, log, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_density_uniform_bandwidth(None) == 0


def test_leave_one_out_needs_the_same_density():
    p, q = _density(seed=1), _density(seed=2)
    for log in (0, 1):
        assert _logl(p, q, 1, log) == _lib.ERR_ARG and "leave_one_out" in _lib.lib.kdehip_last_error().decode()


def test_dimension_mismatch_is_refused():
    p, q = _density(D=2), _density(D=3)
    for log in (0, 1):
        assert _logl(p, q, 0, log) == _lib.ERR_DIM_MISMATCH
    for fn in (kdehip.evalAvgLogL, kdehip.kld, kdehip.minkld):
        with pytest.raises(ValueError):
            fn(p, q)
    with pytest.raises(ValueError):
        kdehip.evaluateDualTree(p, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        kdehip.evaluate_log(p, np.zeros((3, 4)))


def test_nine_dimensions_are_unsupported():
    p = _density(D=9, N=5)
    for log in (0, 1):
        assert _evaluate(p, log=log) == _lib.ERR_UNSUPPORTED
        assert _evaluate(p, loo=1, log=log) == _lib.ERR_UNSUPPORTED
        assert _logl(p, p, 1, log) == _lib.ERR_UNSUPPORTED
        assert _logl(p, _density(D=9, N=7, seed=4), 0, log) == _lib.ERR_UNSUPPORTED


def test_a_manifold_byte_above_one_is_refused():
    p, q = _density(seed=1), _density(seed=2)
    keep, bad = _u8([0, 2])
    for log in (0, 1):
        for rc in (_evaluate(p, log=log, man=bad), _evaluate(p, loo=1, log=log, man=bad), _logl(p, q, 0, log, man=bad),
                   _logl(p, p, 1, log, man=bad)):
            assert rc == _lib.ERR_ARG and "manifold" in _lib.lib.kdehip_last_error().decode()


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'.  A density with one
    bandwidth vector is as welcome as a per-point one."""
    rng = np.random.default_rng(8)
    for p, q in ((_density(seed=1), _density(seed=2)), (kdehip.kde(rng.standard_normal((2, 9)), [0.3]), _density(seed=2))):
        for vals in (None, [0, 0], [1, 0]):
            keep, mp = (None, None) if vals is None else _u8(vals)
            for log in (0, 1):
                for rc in (_evaluate(p, log=log, man=mp), _evaluate(p, loo=1, log=log, man=mp), _logl(p, q, 0, log, man=mp),
                           _logl(p, p, 1, log, man=mp), _logl(p, None, 1, log, man=mp)):
                    assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
                    assert "device" in _lib.lib.kdehip_last_error().decode().lower()
    assert _evaluate(_density(), Nq=0) == _lib.KDEHIP_OK  # nothing to do


def test_the_old_entries_keep_refusing_per_point_densities():
    p = _density()
    cb = C.byref(p._cstruct())
    pos, res = np.zeros(4), np.zeros(4)
    L = _lib.lib
    assert L.kdehip_evaluate_manifold(cb, _lib.ptr(pos, _lib.f64p), 2, 0, _lib.ptr(res, _lib.f64p), NO_SUCH_DEVICE, None) \
        == _lib.ERR_UNSUPPORTED
    assert "per-point bandwidths are not supported" in L.kdehip_last_error().decode()
    assert L.kdehip_evaluate_log(cb, _lib.ptr(pos, _lib.f64p), 2, 0, _lib.ptr(res, _lib.f64p), NO_SUCH_DEVICE, None) \
        == _lib.ERR_UNSUPPORTED


# ---- the Python front end ------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    pts, rng = _points(6, 2, 30)
    pilot = kdehip.kde(pts, [0.3])
    with pytest.raises(ValueError, match="alpha"):
        kdehip.adaptive_scales(pilot, alpha=1.5)
    with pytest.raises(ValueError, match="alpha"):
        kdehip.adaptive_scales(pilot, alpha=-0.1)
    for k in (0, 33):
        with pytest.raises(ValueError, match="k must"):
            kdehip.adaptive_scales(pilot, method="knn", k=k)
    with pytest.raises(ValueError, match="method"):
        kdehip.adaptive_scales(pilot, method="silverman")
    with pytest.raises(TypeError):
        kdehip.adaptive_scales(pts)
    with pytest.raises(ValueError, match="alpha"):
        kdehip.kde_adaptive(pts, [0.3], alpha=2.0)
    with pytest.raises(ValueError, match="k must"):
        kdehip.kde_adaptive(pts, [0.3], method="knn", k=40)
    with pytest.raises(ValueError, match=r"\(D, N\)"):
        kdehip.kde_varbw(pts, np.full((2, 29), 0.3))
    with pytest.raises(ValueError, match=r"\(D, N\)"):
        kdehip.kde_varbw(pts, [0.3, 0.3])
    with pytest.raises(ValueError, match="weights"):
        kdehip.kde_varbw(pts, np.full((2, 30), 0.3), np.ones(29))
    with pytest.raises(ValueError):
        kdehip.kde_varbw(pts, np.full((2, 30), 0.3), tree_manifold=["circular"])  # one entry per dimension


def test_marginal_of_a_per_point_density_carries_the_selected_rows():
    pts, rng = _points(7, 3, 40)
    bw = rng.uniform(0.2, 0.6, size=(3, 40))
    w = rng.uniform(0.1, 1.0, size=40)
    p = kdehip.kde_varbw(pts, bw, w)
    m = kdehip.marginal(p, [2, 0])
    assert m.multibandwidth == 1 and m.bt.dims == 2
    assert np.array_equal(kdehip.getPoints(m), pts[[2, 0]])
    assert np.allclose(kdehip.getBW(m), kdehip.getBW(p)[[2, 0]], rtol=1e-15, atol=0.0)
    assert np.allclose(kdehip.getBW(m), bw[[2, 0]], rtol=1e-15)
    assert np.allclose(kdehip.getWeights(m), w / w.sum(), rtol=1e-15)
    # a density with one vector keeps the old rule
    assert kdehip.marginal(kdehip.kde(pts, [0.3]), [1]).multibandwidth == 0


def test_with_the_direct_switch_off_evaluate_tol_keeps_refusing():
    p = _density()
    kdehip.setForceEvalDirect(False)
    try:
        with pytest.raises(kdehip.KdeHipError, match="per-point bandwidths are not supported"):
            kdehip.evaluateDualTree(p, np.zeros((2, 3)), device=NO_SUCH_DEVICE)
    finally:
        kdehip.setForceEvalDirect(True)
