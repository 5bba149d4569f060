"""The curvature of a density (include/kdehip.h section 5k) without a GPU: the three new symbols, every refusal the entries
make before they touch a device, the Python front end's refusals, the Julia shim's call, and the model of
tests/curvature_model.py pinned against closed forms and against central differences of modes_model.evaluate_grad.

The refusals that read a resident handle (a mask bit at or above ndims, per-point bandwidths of a resident density) need real
handles: they are in tests/test_gpu_curvature.py; here the resident entries are refused for their NULL handles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import curvature_model as cm
from tests import modes_model as mm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_evaluate_hess", "kdehip_evaluate_hess_device", "kdehip_evaluate_hess_device_batch"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    section = hdr[hdr.index("(5k)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name  # declared under (5k)
    assert "kdehip_hess_item" in section and "V^-1 - V^-1 C V^-1" in section
    assert [f for f, _ in _lib.CHessItem._fields_] == ["bd", "d_pos", "Nq", "d_logp", "d_grad", "d_hess", "d_cov", "d_definite",
                                                       "circular_mask", "reserved_"]
    assert C.sizeof(_lib.CHessItem) == 72
    for name in ("evaluate_hess", "laplace", "fit_modes", "getKDEModeFit", "evaluate_hess_device_batch"):
        assert callable(getattr(kdehip, name)), name
    for name in ("evaluate_hess", "laplace", "fit_modes"):
        assert callable(getattr(kdehip.DeviceDensity, name)), name
    assert "not a Laplace evidence" in " ".join(kdehip.fit_modes.__doc__.split()) and "getKDEfit" in kdehip.getKDEModeFit.__doc__


def test_version_stays_600():
    assert kdehip.version() == 600


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


OUTS = ("logp", "grad", "hess", "cov", "definite")


def _hess(p, Nq=3, pos=True, outs=OUTS, man=None):
    D = 2 if p is None else p.bt.dims
    n = max(Nq, 1)
    P = np.zeros((n, D))
    bufs = dict(logp=np.zeros(n), grad=np.zeros((n, D)), hess=np.zeros((n, D, D)), cov=np.zeros((n, D, D)),
                definite=np.zeros(n, dtype=np.int32))
    args = [_lib.ptr(bufs[k], _lib.i32p if k == "definite" else _lib.f64p) if k in outs else None for k in OUTS]
    return L.kdehip_evaluate_hess(None if p is None else C.byref(p._cstruct()), _lib.ptr(P, _lib.f64p) if pos else None, Nq,
                                  *args, NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p = _density()
    assert _hess(None) == _lib.ERR_ARG
    assert _hess(p, outs=()) == _lib.ERR_ARG  # nothing asked for
    assert _hess(p, pos=False) == _lib.ERR_ARG
    a = C.c_void_p(256)
    assert L.kdehip_evaluate_hess_device(None, None, 1, a, a, a, a, a, None, None) == _lib.ERR_ARG
    assert L.kdehip_evaluate_hess_device_batch(1, None, None) == _lib.ERR_ARG
    assert L.kdehip_evaluate_hess_device_batch(-1, None, None) == _lib.ERR_ARG
    items = (_lib.CHessItem * 1)()  # a null handle
    assert L.kdehip_evaluate_hess_device_batch(1, items, None) == _lib.ERR_ARG


def test_a_negative_count_is_refused():
    assert _hess(_density(), Nq=-1) == _lib.ERR_ARG


def test_a_manifold_byte_above_one_is_refused():
    keep, bad = _u8([0, 2])
    assert _hess(_density(), man=bad) == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()


def test_dimensions_outside_one_to_eight_are_unsupported():
    assert _hess(_density(D=9, N=5)) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_are_unsupported_in_evaluates_words():
    p = _density(seed=5)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    out = np.zeros(1)
    pos = np.zeros((1, D))
    assert L.kdehip_evaluate(C.byref(p._cstruct()), _lib.ptr(pos, _lib.f64p), 1, 0, _lib.ptr(out, _lib.f64p),
                             NO_SUCH_DEVICE) == _lib.ERR_UNSUPPORTED
    words = L.kdehip_last_error().decode()
    assert _hess(p) == _lib.ERR_UNSUPPORTED and L.kdehip_last_error().decode() == words


def test_nothing_to_do_is_ok():
    p = _density()
    assert _hess(p, Nq=0) == _lib.KDEHIP_OK
    assert _hess(p, Nq=0, pos=False) == _lib.KDEHIP_OK
    assert L.kdehip_evaluate_hess_device_batch(0, None, None) == _lib.KDEHIP_OK


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p = _density()
    for vals in (None, [0, 0], [1, 0]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for outs in (OUTS, ("hess",), ("cov",), ("definite",), ("logp", "grad")):
            assert _hess(p, outs=outs, man=mp) in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
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
    for fn in (lambda: kdehip.evaluate_hess(pos, pos), lambda: kdehip.laplace(None, pos), lambda: kdehip.fit_modes(pos),
               lambda: kdehip.getKDEModeFit([p]),
               lambda: kdehip.evaluate_hess(p, _Tensor()), lambda: kdehip.laplace(p, _Tensor()),  # host density, device points
               lambda: kdehip.evaluate_hess_device_batch([dict(density=p, pos=None, hess=None)])):
        with pytest.raises(TypeError):
            fn()
    with pytest.raises(ValueError):
        kdehip.evaluate_hess(p, np.zeros((3, 4)))   # D rows
    with pytest.raises(ValueError):
        kdehip.laplace(p, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        kdehip.evaluate_hess(p, pos, manifold=[1])  # one entry per dimension
    with pytest.raises(ValueError):
        kdehip.laplace(p, pos, manifold=[0, 2])
    with pytest.raises(ValueError):
        kdehip.evaluate_hess(fake, pos, manifold=[0, 2])
    with pytest.raises(ValueError):
        kdehip.fit_modes(p, tol=-1.0)
    with pytest.raises(ValueError):
        kdehip.fit_modes(fake, pos, maxiter=-1)


def test_a_batch_refuses_tensors_that_are_not_on_a_device():
    """the type, device and layout of every tensor are checked before the library is called"""
    import torch
    fake = _fake_device_density()
    pos = torch.zeros((3, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        kdehip.evaluate_hess_device_batch([dict(density=fake, pos=pos, hess=torch.zeros((3, 2, 2), dtype=torch.float64))])


def test_julia_shim_calls_the_new_entry_as_the_header_declares_it():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    m = re.search(r"ccall\(\(:kdehip_evaluate_hess,\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
    assert m
    types = [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert len(types) == len(params["kdehip_evaluate_hess"]) == 10
    for jt, ct in zip(types, params["kdehip_evaluate_hess"]):
        assert ct in shim.JULIA_TO_C[jt], (jt, ct)
    for fn in ("hip_evaluate_hess", "hip_fit_modes"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    body = code[code.index("function hip_evaluate_hess("):]
    assert "manifold_bytes(" in body[:body.index("\nend")]
    body = code[code.index("function hip_fit_modes("):]
    assert "hip_modes(" in body[:body.index("\nend")]  # merged in Julia, as hip_modes is


# ---- the model itself ----------------------------------------------------------------------------------------------------
def _model_density(D, N, seed):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 1.5, size=(D, 1))
    w = rng.uniform(0.05, 1.0, size=N)
    w[::5] = 0.0
    sd = rng.uniform(0.3, 0.6, size=D)
    return pts, w / w.sum(), sd * sd


def test_model_one_point_has_the_kernels_curvature_everywhere():
    v = np.array([0.04, 0.09, 0.25])
    dens = (np.array([[0.25], [-1.25], [0.5]]), np.array([1.0]), v)
    for x in ([0.25, -1.25, 0.5], [1.0, 0.5, -2.0], [10.25, -11.25, 25.5]):
        lp, g, gs, H, hs = cm.hessian(dens, np.array(x))
        assert np.all(np.abs(H + np.diag(1.0 / v)) <= 4 * 2.0 ** -53 * hs)
    cov, definite = cm.laplace(dens, np.array([[1.0], [0.5], [-2.0]]))
    assert definite.tolist() == [True] and np.all(np.abs(cov[:, :, 0] - np.diag(v)) <= 1e-12)


@pytest.mark.parametrize("a,v", [(1.0, 0.25), (0.5, 0.25), (0.3, 0.25), (2.0, 9.0)])
def test_model_two_equal_points_at_plus_and_minus_a(a, v):
    dens = (np.array([[-a, a]]), np.array([0.5, 0.5]), np.array([v]))
    lp, g, gs, H, hs = cm.hessian(dens, np.array([0.0]))
    want = a * a / (v * v) - 1.0 / v
    assert g[0] == 0.0 and abs(H[0, 0] - want) <= 4 * 2.0 ** -53 * hs[0, 0]
    cov, definite = cm.laplace(dens, np.array([[0.0]]))
    if a * a > v:  # a minimum between two modes
        assert not definite[0] and np.isnan(cov[0, 0, 0])
    elif a * a < v:  # one mode, wider than the kernel
        assert definite[0] and abs(cov[0, 0, 0] - 1.0 / (1.0 / v - a * a / (v * v))) <= 1e-12 * cov[0, 0, 0] and cov[0, 0, 0] > v
    else:
        assert H[0, 0] == 0.0


@pytest.mark.parametrize("D,man", [(1, None), (3, None), (6, None), (8, None), (2, [0, 1])])
def test_model_hessian_is_the_central_difference_of_the_models_gradient(D, man):
    dens = _model_density(D, 40, 10 + D)
    rng = np.random.default_rng(D)
    X = rng.standard_normal((D, 5))
    _, _, _, hess, hscale = cm.evaluate_hess(dens, X, man)
    assert np.array_equal(hess, hess.transpose(1, 0, 2))
    sd = np.sqrt(dens[2])
    for l in range(D):
        e = np.zeros((D, 1))
        e[l] = 1e-5 * sd[l]
        fd = (mm.evaluate_grad(dens, X + e, man)[1] - mm.evaluate_grad(dens, X - e, man)[1]) / (2.0 * e[l])
        assert np.all(np.abs(hess[:, l, :] - fd) <= 1e-6 * hscale[:, l, :]), (l, float(np.max(np.abs(hess[:, l, :] - fd) / hscale[:, l, :])))


def test_model_first_moments_are_modes_models():
    dens = _model_density(3, 40, 7)
    x = np.array([0.3, -0.2, 0.5])
    m, S0, S, A = mm.moments(dens, x)
    m2, S02, S2, A2, _, _ = cm.moments2(dens, x)
    assert m == m2 and S0 == S02 and np.array_equal(S, S2) and np.array_equal(A, A2)
    lp, g, gs, _, _ = cm.hessian(dens, x)
    val, grad, scale = mm.evaluate_grad(dens, x[:, None])
    assert lp == val[0] and np.array_equal(g, grad[:, 0]) and np.array_equal(gs, scale[:, 0])


def test_model_covariance_of_a_mode_is_never_narrower_than_the_kernel():
    pts, sd, w = mm.three_clusters(3, 300)
    dens = (pts, w / w.sum(), sd * sd)
    modes = mm.modes(dens)[0]
    cov, definite = cm.laplace(dens, modes)
    assert modes.shape == (3, 3) and definite.all()
    for j in range(3):
        assert np.linalg.eigvalsh(cov[:, :, j] - np.diag(dens[2])).min() >= -1e-12
