"""Conditioning a density on some of its dimensions (include/kdehip.h section 5i) without a GPU: the new symbols, every
refusal the entries make before they touch a device, the Python front end's refusals, and the model of
tests/conditional_model.py pinned on cases whose answer is known.

The refusals that read a resident handle (a mask bit at or above ndims, per-point bandwidths of a resident density, pts
without ind, densities on different devices) need real handles: they are in tests/test_gpu_conditional.py; here the resident
entries are refused for their NULL handles."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import conditional_model as cm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_conditional", "kdehip_conditional_device", "kdehip_conditional_device_batch", "kdehip_condition_weights",
       "kdehip_condition_weights_device", "kdehip_density_condition_device"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    assert hdr.index("(5h)") < hdr.index("(5i)")
    section = hdr[hdr.index("(5i)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name  # declared under (5i)
    assert "kdehip_conditional_item" in section
    assert C.sizeof(_lib.CConditionalItem) == 88
    for words in ("proportional to R_k^2", "within a relative 1e-9 of some C_i may resolve to the neighbouring leaf of S",
                  "Everything else about the label is exact"):
        assert words in " ".join(section.replace(" * ", " ").split()), words
    for name in ("condition", "conditional_weights", "conditional_moments", "sample_conditional", "conditional_device_batch"):
        assert callable(getattr(kdehip, name)), name
    for name in ("condition", "conditional_weights", "conditional_moments", "sample_conditional"):
        assert callable(getattr(kdehip.DeviceDensity, name)), name


def test_version_stays_600():
    assert kdehip.version() == 600


def test_the_julia_shim_still_matches_the_header():
    """the header gained declarations: every ccall of the shim is still checked against it type by type"""
    shim.test_every_ccall_matches_the_header()
    assert set(NEW) <= set(shim.header_params())


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _cond(p, mask=1, Nq=2, given=True, logz=True, mean=True, var=True, pts=True, ind=True, man=None):
    D = 2 if p is None else p.bt.dims
    n = max(Nq, 1)
    Y, lz, a = np.zeros((n, D)), np.zeros(n), [np.zeros((n, D)) for _ in range(3)]
    idx = np.zeros(n, dtype=np.int64)
    f = _lib.f64p
    return L.kdehip_conditional(None if p is None else C.byref(p._cstruct()), mask, _lib.ptr(Y, f) if given else None, Nq, 7, 0,
                                _lib.ptr(lz, f) if logz else None, _lib.ptr(a[0], f) if mean else None,
                                _lib.ptr(a[1], f) if var else None, _lib.ptr(a[2], f) if pts else None,
                                _lib.ptr(idx, _lib.i64p) if ind else None, NO_SUCH_DEVICE, man)


def _wts(p, mask=1, Nq=2, given=True, w=True, logz=True, man=None):
    D, N = (2, 20) if p is None else (p.bt.dims, p.bt.num_points)
    n = max(Nq, 1)
    Y, W, lz = np.zeros((n, D)), np.zeros((n, N)), np.zeros(n)
    f = _lib.f64p
    return L.kdehip_condition_weights(None if p is None else C.byref(p._cstruct()), mask, _lib.ptr(Y, f) if given else None, Nq,
                                      _lib.ptr(W, f) if w else None, _lib.ptr(lz, f) if logz else None, NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p = _density()
    assert _cond(None) == _lib.ERR_ARG
    assert _cond(p, given=False) == _lib.ERR_ARG
    assert _cond(p, logz=False, mean=False, var=False, pts=False, ind=False) == _lib.ERR_ARG  # nothing asked for
    assert _cond(p, ind=False) == _lib.ERR_ARG and _cond(p, pts=False) == _lib.ERR_ARG      # together or not at all
    assert _wts(None) == _lib.ERR_ARG and _wts(p, given=False) == _lib.ERR_ARG and _wts(p, w=False) == _lib.ERR_ARG
    d = C.c_void_p(256)
    assert L.kdehip_conditional_device(None, 1, d, 1, 7, 0, d, d, d, d, d, None, None) == _lib.ERR_ARG
    assert L.kdehip_condition_weights_device(None, 1, d, 1, d, d, None, None) == _lib.ERR_ARG
    assert L.kdehip_conditional_device_batch(1, None, None) == _lib.ERR_ARG
    assert L.kdehip_conditional_device_batch(-1, None, None) == _lib.ERR_ARG
    items = (_lib.CConditionalItem * 1)()  # a null handle
    assert L.kdehip_conditional_device_batch(1, items, None) == _lib.ERR_ARG
    y = np.zeros(1)
    h = C.c_void_p()
    assert L.kdehip_density_condition_device(None, None, 1, _lib.ptr(y, _lib.f64p), None, None) == _lib.ERR_ARG
    assert L.kdehip_density_condition_device(C.byref(h), None, 1, _lib.ptr(y, _lib.f64p), None, None) == _lib.ERR_ARG
    assert h.value is None


def test_a_negative_count_is_refused():
    p = _density()
    assert _cond(p, Nq=-1) == _lib.ERR_ARG and _wts(p, Nq=-1) == _lib.ERR_ARG


@pytest.mark.parametrize("D,mask", [(2, 0), (2, 3), (2, 4), (2, 5), (3, 7), (3, 8), (3, 0x80000001), (1, 1), (1, 0)])
def test_a_bad_given_mask_is_refused(D, mask):
    p = _density(D=D)
    assert _cond(p, mask=mask) == _lib.ERR_ARG and "condition" in L.kdehip_last_error().decode()
    assert _wts(p, mask=mask) == _lib.ERR_ARG


def test_a_manifold_byte_above_one_is_refused():
    p = _density()
    keep, bad = _u8([0, 2])
    for rc in (_cond(p, man=bad), _wts(p, man=bad)):
        assert rc == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()


def test_dimensions_outside_one_to_eight_are_unsupported():
    p = _density(D=9, N=5)
    assert _cond(p) == _lib.ERR_UNSUPPORTED and _wts(p) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_are_unsupported():
    p = _density(seed=5)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    for rc in (_cond(p), _wts(p)):
        assert rc == _lib.ERR_UNSUPPORTED and "per-point" in L.kdehip_last_error().decode()


def test_moments_over_a_circular_free_dimension_are_unsupported():
    p = _density(D=3)
    keep, free_circ = _u8([0, 0, 1])
    for kw in (dict(), dict(var=False), dict(mean=False), dict(logz=False, pts=False, ind=False)):
        assert _cond(p, mask=1, man=free_circ, **kw) == _lib.ERR_UNSUPPORTED
        assert "circular free" in L.kdehip_last_error().decode()
    # the same manifold is fine without moments, and with them when the circular dimension is a given one
    for rc in (_cond(p, mask=1, man=free_circ, mean=False, var=False), _cond(p, mask=4, man=free_circ),
               _wts(p, mask=1, man=free_circ)):
        assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE) and "device" in L.kdehip_last_error().decode().lower()


def test_nothing_to_do_is_ok():
    p = _density()
    assert _cond(p, Nq=0) == _lib.KDEHIP_OK and _cond(p, Nq=0, given=False) == _lib.KDEHIP_OK
    assert _wts(p, Nq=0) == _lib.KDEHIP_OK
    assert L.kdehip_conditional_device_batch(0, None, None) == _lib.KDEHIP_OK


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p = _density(D=3)
    for vals in (None, [0, 0, 0], [1, 0, 0]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for rc in (_cond(p, man=mp), _cond(p, mask=6, mean=False, var=False, man=mp), _cond(p, mask=3, man=mp),
                   _cond(p, mask=5, mean=False, var=False, pts=False, ind=False, man=mp),
                   _cond(p, logz=False, mean=False, var=False, man=mp), _wts(p, man=mp), _wts(p, mask=3, logz=False, man=mp)):
            assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in L.kdehip_last_error().decode().lower()


def test_python_front_end_refusals():
    p3, p1 = _density(D=3), _density(D=1)
    Y = np.zeros((1, 4))
    for fn in (kdehip.conditional_weights, kdehip.conditional_moments, kdehip.sample_conditional):
        with pytest.raises(ValueError, match="distinct"):
            fn(p3, [0, 0], np.zeros((2, 4)))
        with pytest.raises(ValueError, match="ndims - 1"):
            fn(p3, [0, 1, 2], np.zeros((3, 4)))  # all dims given
        with pytest.raises(ValueError, match="ndims - 1"):
            fn(p3, [], np.zeros((0, 4)))
        with pytest.raises(ValueError, match="1-D"):
            fn(p1, [0], Y)
        with pytest.raises(ValueError, match="dims must be integers"):
            fn(p3, [3], Y)
        with pytest.raises(ValueError, match="one value per given dimension"):
            fn(p3, [0, 1], Y)
        with pytest.raises(ValueError):
            fn(p3, [0], Y, manifold=[0, 1])  # one entry per dimension
        with pytest.raises(TypeError):
            fn(np.zeros((3, 4)), [0], Y)
    with pytest.raises(ValueError, match="distinct"):
        kdehip.condition(p3, [1, 1], [0.0, 0.0])
    with pytest.raises(ValueError, match="1-D"):
        kdehip.condition(p1, [0], [0.0])
    with pytest.raises(ValueError, match="one value per given dimension"):
        kdehip.condition(p3, [0, 2], [0.0])
    with pytest.raises(TypeError):
        kdehip.conditional_device_batch([dict(density=p3, dims=[0], given=None)])


# ---- the model itself ----------------------------------------------------------------------------------------------------
def _log_normal(y, c, v):
    return -0.5 * len(v) * math.log(2.0 * math.pi) - 0.5 * sum(math.log(t) for t in v) - 0.5 * sum((a - b) ** 2 / t for a, b, t in zip(y, c, v))


@pytest.mark.parametrize("gdims", [[0], [2], [0, 1], [1, 2]])
def test_model_one_point(gdims):
    c, v = np.array([[0.25], [-1.25], [2.0]]), np.array([0.04, 0.09, 0.25])
    dens, perm = (c, np.array([1.0]), v), np.array([1])
    y = np.array([0.5, -1.0, 1.5])[gdims]
    F = cm.free_dims(3, gdims)
    lz, mean, var = cm.moments(dens, gdims, y)
    assert abs(lz - _log_normal(y, c[gdims, 0], v[gdims])) <= 1e-15 * max(1.0, abs(lz))
    assert np.array_equal(mean, c[F, 0]) and np.array_equal(var, v[F])
    assert cm.weights(dens, gdims, y).tolist() == [1.0]
    for u in (1e-300, 0.5, 1.0 - 2.0 ** -53):
        assert cm.draw_label(dens, perm, gdims, y, u)[:2] == (1, 0)
    assert abs(cm.logz(dens, gdims, y) - lz) == 0.0


def test_model_two_far_clusters():
    rng = np.random.default_rng(2)
    N = 60
    left = np.arange(N) % 2 == 0
    pts = np.where(left, -10.0, 10.0)[None, :] + 0.3 * rng.standard_normal((2, N))
    pts[1] = np.where(left, 1.0, -2.0) + 0.1 * rng.standard_normal(N)
    w = rng.uniform(0.1, 1.0, size=N)
    dens, perm = (pts, w / w.sum(), np.array([0.09, 0.04])), rng.permutation(N) + 1
    for y, side, centre in ((-10.0, left, 1.0), (10.0, ~left, -2.0)):
        om = cm.weights(dens, [0], [y])
        assert math.fsum(om[side].tolist()) > 1.0 - 1e-12 and abs(math.fsum(om.tolist()) - 1.0) <= 1e-15
        _, mean, var = cm.moments(dens, [0], [y])
        assert abs(mean[0] - centre) < 0.1 and 0.04 <= var[0] < 0.04 + 0.1
        for u in (0.01, 0.37, 0.99):
            ind, leaf, gap = cm.draw_label(dens, perm, [0], [y], u)
            assert side[leaf] and ind == perm[leaf] and gap > 0.0


def test_model_weightless_points_and_the_empty_set():
    pts = np.array([[0.0, 1.0, 2.0, 3.0], [5.0, 6.0, 7.0, 8.0]])
    v, perm = np.array([0.25, 0.25]), np.array([3, 1, 4, 2])
    dens = (pts, np.array([0.0, 0.5, 0.0, 0.5]), v)
    om = cm.weights(dens, [0], [1.0])
    assert om[0] == 0.0 and om[2] == 0.0 and om[1] > om[3] > 0.0
    assert cm.draw_label(dens, perm, [0], [1.0], 1e-9)[:2] == (1, 1)           # the first leaf of S, never leaf 0
    assert cm.draw_label(dens, perm, [0], [1.0], 1.0 - 2.0 ** -53)[:2] == (2, 3)
    none = (pts, np.zeros(4), v)
    lz, mean, var = cm.moments(none, [0], [1.0])
    assert lz == -math.inf and np.isnan(mean).all() and np.isnan(var).all()
    assert cm.draw_label(none, perm, [0], [1.0], 0.5)[:2] == (0, -1) and not cm.weights(none, [0], [1.0]).any()


@pytest.mark.parametrize("D,gdims", [(2, [0]), (2, [1]), (3, [0, 2]), (6, [3, 4, 5]), (4, [1])])
def test_model_chain_rule(D, gdims):
    """log p([y; x]) = logz(y) + log p_cond(x): the joint density is the marginal of G times the conditional on F"""
    rng = np.random.default_rng(10 * D + len(gdims))
    N = 50
    pts = rng.standard_normal((D, N))
    w = rng.uniform(0.05, 1.0, size=N)
    w[::5] = 0.0
    v = rng.uniform(0.1, 0.4, size=D)
    dens = (pts, w / w.sum(), v)
    F = cm.free_dims(D, gdims)
    for _ in range(5):
        z = rng.standard_normal(D)
        joint = cm.log_normal_mixture(pts, dens[1], v, z)
        om = cm.weights(dens, gdims, z[gdims])
        cond = cm.log_normal_mixture(pts[F], om, v[F], z[F])
        assert abs(joint - (cm.logz(dens, gdims, z[gdims]) + cond)) <= 1e-13 * max(1.0, abs(joint))


def test_model_circular_given_dimension_wraps():
    rng = np.random.default_rng(4)
    N = 40
    ang = cm.wrap(math.pi + 0.05 * rng.standard_normal(N))  # a cluster across the cut
    assert ang.min() < -3.0 and ang.max() > 3.0
    pts = np.vstack([ang, rng.standard_normal(N)])
    dens = (pts, np.full(N, 1.0 / N), np.array([0.01, 0.04]))
    a = cm.weights(dens, [0], [math.pi - 0.01], man=[1, 0])
    b = cm.weights(dens, [0], [-math.pi + 0.01], man=[1, 0])
    assert a.min() > 1e-6 and b.min() > 1e-6       # both queries see the whole cluster
    line = cm.weights(dens, [0], [math.pi - 0.01])   # on the line half of it is 2 pi away
    assert line[ang < 0].max() < 1e-300
    shifted = (pts + np.array([[2.0 * math.pi], [0.0]]), dens[1], dens[2])
    assert np.allclose(cm.weights(shifted, [0], [math.pi - 0.01], man=[1, 0]), a, rtol=1e-9, atol=0.0)
