"""Exact overlap measures (include/kdehip.h section 5g) without a GPU: the three new symbols, every refusal the entries make
before they touch a device, the Python front end's refusals, the Julia shim's calls, and the model of tests/ksum_model.py
pinned against sums written out by hand.

The refusals that read a resident handle (a mask bit at or above ndims, per-point bandwidths of a resident density) need
real handles: they are in tests/test_gpu_ksum.py; here the resident entries are refused for their NULL handles."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import ksum_model as km
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_kernel_sum", "kdehip_kernel_sum_device", "kdehip_kernel_sum_device_batch"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name
    assert "(5g)" in hdr and "kdehip_ksum_item" in hdr
    for name in ("kernel_sum", "intersIntg", "ise", "mmd", "kernel_sum_device_batch", "ise_batch", "mmd_batch"):
        assert callable(getattr(kdehip, name)), name
    assert "intersIntg" in kdehip.intersIntgAppxIS.__doc__


def test_version_stays_600():
    assert kdehip.version() == 600


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _ksum(a, b, var=None, man=None, out=True, normalize=1):
    res = C.c_double(0.0)
    ca = None if a is None else C.byref(a._cstruct())
    cb = None if b is None else (ca if b is a else C.byref(b._cstruct()))
    v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    return _lib.lib.kdehip_kernel_sum(ca, cb, _lib.optr(v, _lib.f64p), normalize, C.byref(res) if out else None,
                                      NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p, q = _density(), _density(seed=4)
    L = _lib.lib
    assert _ksum(None, q) == _lib.ERR_ARG
    assert _ksum(p, None) == _lib.ERR_ARG
    assert _ksum(p, q, out=False) == _lib.ERR_ARG
    res = C.c_double(0.0)
    assert L.kdehip_kernel_sum_device(None, None, None, 1, C.byref(res), None) == _lib.ERR_ARG
    assert L.kdehip_kernel_sum_device(None, None, None, 1, None, None) == _lib.ERR_ARG
    assert L.kdehip_kernel_sum_device_batch(1, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_kernel_sum_device_batch(-1, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_kernel_sum_device_batch(0, None, None, None) == _lib.KDEHIP_OK  # nothing to do
    items = (_lib.CKsumItem * 1)()  # null handles
    assert L.kdehip_kernel_sum_device_batch(1, items, None, None) == _lib.ERR_ARG
    assert L.kdehip_kernel_sum_device_batch(1, items, C.c_void_p(256), None) == _lib.ERR_ARG


def test_dimension_mismatch_is_refused():
    p, q = _density(D=2), _density(D=3)
    assert _ksum(p, q) == _lib.ERR_DIM_MISMATCH
    assert _ksum(p, q, var=[1.0, 1.0]) == _lib.ERR_DIM_MISMATCH
    for fn in (kdehip.kernel_sum, kdehip.intersIntg, kdehip.ise, lambda a, b: kdehip.mmd(a, b, 0.5)):
        with pytest.raises(ValueError):
            fn(p, q)


def test_nine_dimensions_are_unsupported():
    p, q = _density(D=9, N=5), _density(D=9, N=7, seed=4)
    assert _ksum(p, p) == _lib.ERR_UNSUPPORTED
    assert _ksum(p, q) == _lib.ERR_UNSUPPORTED
    assert _ksum(p, q, var=[1.0] * 9) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_need_explicit_variances():
    p, q = _density(seed=5), _density(seed=6)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    for a, b in ((p, q), (q, p), (p, p)):
        assert _ksum(a, b) == _lib.ERR_UNSUPPORTED and "bandwidth" in _lib.lib.kdehip_last_error().decode()
        assert _ksum(a, b, var=[0.2, 0.3]) != _lib.ERR_UNSUPPORTED  # (only points and weights are read)


@pytest.mark.parametrize("bad", [0.0, -1.0, np.inf, -np.inf, np.nan])
def test_a_bad_variance_is_refused(bad):
    p, q = _density(seed=1), _density(seed=2)
    for var in ([bad, 1.0], [1.0, bad]):
        assert _ksum(p, q, var=var) == _lib.ERR_ARG and "variance" in _lib.lib.kdehip_last_error().decode()
        assert _ksum(p, p, var=var, normalize=0) == _lib.ERR_ARG


def test_a_manifold_byte_above_one_is_refused():
    p, q = _density(seed=1), _density(seed=2)
    keep, bad = _u8([0, 2])
    for rc in (_ksum(p, q, man=bad), _ksum(p, p, man=bad), _ksum(p, q, var=[1.0, 2.0], man=bad)):
        assert rc == _lib.ERR_ARG and "manifold" in _lib.lib.kdehip_last_error().decode()


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p, q = _density(seed=1), _density(seed=2)
    for vals in (None, [0, 0], [1, 0]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for rc in (_ksum(p, q, man=mp), _ksum(p, p, man=mp), _ksum(p, q, var=[0.5, 2.0], man=mp, normalize=0)):
            assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in _lib.lib.kdehip_last_error().decode().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    fake.manifold = None
    return fake


def test_python_front_end_refusals():
    p, fake = _density(), _fake_device_density()
    for fn in (lambda: kdehip.kernel_sum(p, fake), lambda: kdehip.kernel_sum(fake, p, [1.0, 1.0]),
               lambda: kdehip.intersIntg(p, fake), lambda: kdehip.ise(fake, p), lambda: kdehip.mmd(p, fake, 0.3),
               lambda: kdehip.ise(np.zeros((2, 3)), p),
               lambda: kdehip.ise_batch([(p, fake)]), lambda: kdehip.ise_batch([(p, p)]),
               lambda: kdehip.mmd_batch([(p, p)], 0.3),
               lambda: kdehip.kernel_sum_device_batch([dict(a=p, b=p)], None)):
        with pytest.raises(TypeError):  # mixed, or host densities where resident ones are needed: the error `kld` raises
            fn()
    q = _density(seed=2)
    with pytest.raises(TypeError):
        kdehip.mmd(p, q)  # bw has no default
    with pytest.raises(TypeError):
        kdehip.mmd(p, q, None)
    with pytest.raises(TypeError):
        kdehip.mmd_batch([(fake, fake)], None)
    with pytest.raises(ValueError, match="bw"):
        kdehip.mmd(p, q, [0.1, 0.2, 0.3])  # 1 or D entries
    with pytest.raises(ValueError, match="var"):
        kdehip.kernel_sum(p, q, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        kdehip.intersIntg(p, q, manifold=[1])  # one entry per dimension
    with pytest.raises(ValueError):
        kdehip.ise(p, q, manifold=[0, 2])
    with pytest.raises(ValueError):
        kdehip.ise_batch([(fake, fake)], manifold=[0, 1], manifolds=[[0, 1]])
    with pytest.raises(ValueError):
        kdehip.mmd_batch([(fake, fake)], 0.3, manifolds=[])
    with pytest.raises(ValueError):
        kdehip.ise_batch([(fake, _fake_device_density(D=3))])


def test_julia_shim_calls_the_new_entry_as_the_header_declares_it():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    m = re.search(r"ccall\(\(:kdehip_kernel_sum,\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
    assert m
    types = [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert len(types) == len(params["kdehip_kernel_sum"])
    for jt, ct in zip(types, params["kdehip_kernel_sum"]):
        assert ct in shim.JULIA_TO_C[jt], (jt, ct)
    for fn in ("hip_kernel_sum", "hip_intersIntg", "hip_ise", "hip_mmd"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    body = code[code.index("function hip_kernel_sum("):]
    assert "manifold_bytes(" in body[:body.index("\nend")]


# ---- the model itself ----------------------------------------------------------------------------------------------------
def test_model_intersIntg_is_the_four_term_sum_of_normal_densities():
    xa, wa, va = np.array([[0.3, -1.1]]), np.array([0.25, 0.75]), np.array([0.04])
    xb, wb, vb = np.array([[0.5, 2.0]]), np.array([0.6, 0.4]), np.array([0.09])
    v = 0.04 + 0.09
    want = (0.25 * 0.6 * km.normal_pdf(0.3 - 0.5, v) + 0.25 * 0.4 * km.normal_pdf(0.3 - 2.0, v)
            + 0.75 * 0.6 * km.normal_pdf(-1.1 - 0.5, v) + 0.75 * 0.4 * km.normal_pdf(-1.1 - 2.0, v))
    got = km.inters_intg((xa, wa, va), (xb, wb, vb))
    assert abs(got - want) <= 4e-16 * want
    # ... and it is the integral: a Riemann sum of p q on a fine grid
    x = np.linspace(-6.0, 7.0, 260001)
    pdf = lambda pts, w, var: sum(wi * np.exp(-0.5 * (x - c) ** 2 / var) / math.sqrt(2 * math.pi * var) for c, wi in zip(pts[0], w))  # noqa: E731
    riemann = float(np.sum(pdf(xa, wa, va[0]) * pdf(xb, wb, vb[0])) * (x[1] - x[0]))
    assert abs(riemann - want) <= 1e-9 * want


def test_model_ise_and_mmd_of_a_density_with_itself_are_zero():
    rng = np.random.default_rng(1)
    for D in (1, 3):
        p = (rng.standard_normal((D, 17)), np.full(17, 1.0 / 17), rng.uniform(0.1, 0.4, size=D))
        assert km.ise(p, p)[0] == 0.0
        assert km.mmd(p, p, 0.5)[0] == 0.0
        q = (p[0] + 0.3, p[1], p[2])
        e, mag = km.ise(p, q)
        assert e > 0.0 and km.ise(q, p)[0] == pytest.approx(e, rel=1e-12) and mag > e
        assert km.mmd(p, q, [0.5] * D)[0] > 0.0


def test_model_wraps_the_difference_in_a_circular_dimension():
    a = (np.array([[3.1]]), np.array([1.0]), np.array([0.01]))
    b = (np.array([[-3.1]]), np.array([1.0]), np.array([0.01]))
    d = 2.0 * math.pi - 6.2
    circ = km.inters_intg(a, b, [1])
    assert abs(circ - km.normal_pdf(d, 0.02)) <= 1e-12 * circ
    assert km.inters_intg(a, b) < 1e-300 < circ
    shifted = (a[0] + 2.0 * math.pi, a[1], a[2])
    assert abs(km.inters_intg(shifted, b, [1]) - circ) <= 1e-12 * circ
