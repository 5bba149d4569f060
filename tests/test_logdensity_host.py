"""Log-domain evaluation (include/kdehip.h section 5f) without a GPU: the NumPy model of tests/logdensity_model.py pinned
against the oracle's direct evaluation where nothing underflows, the model's own behaviour where the direct sum does
underflow, the refusals every new entry makes before it touches a device, the Python front end's refusals and the Julia
shim's new calls.

The refusal of a batch mask bit at or beyond ndims needs resident handles (the entry reads the item's ndims from them), so
it is in tests/test_gpu_logdensity.py; here the batch is refused for its NULL handles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from oracle import oracle
from tests import circular_model as cm
from tests import logdensity_model as lm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_evaluate_log", "kdehip_evaluate_log_device", "kdehip_evaluate_log_device_at", "kdehip_eval_avg_logl_log",
       "kdehip_eval_avg_logl_log_device", "kdehip_eval_avg_logl_log_device_batch"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    return np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("D,N,Nq,weighted", [(1, 100, 33, False), (2, 257, 300, True), (3, 130, 129, False), (6, 65, 70, True)])
def test_model_equals_the_log_of_the_oracle_where_nothing_underflows(D, N, Nq, weighted):
    pts, w, sd, pos = cm.circular_case(10 * D + N, D, N, Nq, [0] * D, weighted)
    o = oracle.OracleDensity(pts, sd, w)
    p = oracle.eval_direct(o, pos)
    assert np.all(p > 1e-200)  # (far from the underflow range: the case means what it says)
    assert np.all(_rel(lm.eval_log(pts, w, sd ** 2, pos), np.log(p)))
    ploo = oracle.eval_direct(o, loo=True)
    assert np.all(ploo > 1e-200)
    assert np.all(_rel(lm.eval_log(pts, w, sd ** 2, loo=True), np.log(ploo)))
    # ... and the log-likelihood built on it equals the direct model's
    W = cm.normalise(w, N)
    want, _ = cm.avg_logl(ploo, W)
    got, big = lm.avg_logl_log(lm.eval_log(pts, w, sd ** 2, loo=True), W)
    assert abs(got - want) <= 1e-12 * big


def test_model_stays_finite_and_ordered_where_the_direct_sum_underflows():
    rng = np.random.default_rng(2)
    pts = rng.standard_normal((2, 50)) * 0.05
    var = np.array([0.05 ** 2, 0.05 ** 2])
    near, far = pts + np.array([[5.0], [0.0]]), pts + np.array([[10.0], [0.0]])  # 100 and 200 standard deviations away
    assert np.all(cm.eval_direct(pts, None, var, near) == 0.0)
    lp_near, lp_far = lm.eval_log(pts, None, var, near), lm.eval_log(pts, None, var, far)
    assert np.all(np.isfinite(lp_near)) and np.all(np.isfinite(lp_far)) and np.all(lp_far < lp_near)
    assert np.all(lp_near < -4000.0)
    p, q1, q2 = (pts, None, var), (far, None, var), (near, None, var)
    assert cm.eval_avg_logl(q1, p)[0] == -np.inf
    k1, k2 = lm.kld_log(p, q1), lm.kld_log(p, q2)
    assert np.isfinite(k1) and np.isfinite(k2) and k1 > k2 > 0.0


def test_model_ignores_weightless_sources_and_reports_an_empty_set():
    pts = np.array([[0.0, 0.001, 6.0, 6.1]])
    w = np.array([0.0, 0.0, 1.0, 3.0])
    var = np.array([0.01])
    lp = lm.eval_log(pts, w, var, np.array([[0.0]]))
    want = lm.eval_log(pts[:, 2:], w[2:], var, np.array([[0.0]]))
    assert np.isfinite(lp[0]) and lp[0] == want[0]
    assert lm.eval_log(pts[:, :1], None, var, loo=True)[0] == -np.inf  # one point, leave-one-out: nothing left
    assert lm.avg_logl_log([-np.inf, -1.0], [0.0, 1.0]) == (-1.0, 1.0)
    assert lm.avg_logl_log([-np.inf, -1.0], [0.5, 0.5])[0] == -np.inf


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name
    assert "(5f)" in hdr


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _evaluate_log(bd, Nq=2, loo=0, man=None, out=True):
    D = 2 if bd is None else bd.bt.dims
    pos, res = np.zeros(D * max(Nq, 1)), np.zeros(64)
    cb = None if bd is None else C.byref(bd._cstruct())
    return _lib.lib.kdehip_evaluate_log(cb, _lib.ptr(pos, _lib.f64p), Nq, loo, _lib.ptr(res, _lib.f64p) if out else None,
                                        NO_SUCH_DEVICE, man)


def _logl_log(bd, at, loo, man=None, out=True):
    res = C.c_double(0.0)
    cb = None if bd is None else C.byref(bd._cstruct())
    ca = None if at is None else (cb if at is bd else C.byref(at._cstruct()))
    return _lib.lib.kdehip_eval_avg_logl_log(cb, ca, int(loo), C.byref(res) if out else None, NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p = _density()
    L = _lib.lib
    assert _evaluate_log(None) == _lib.ERR_ARG
    assert _evaluate_log(p, out=False) == _lib.ERR_ARG
    assert L.kdehip_evaluate_log(C.byref(p._cstruct()), None, 2, 0, _lib.ptr(np.zeros(2), _lib.f64p), NO_SUCH_DEVICE, None) == _lib.ERR_ARG
    assert _logl_log(None, p, 0) == _lib.ERR_ARG
    assert _logl_log(p, None, 0) == _lib.ERR_ARG
    assert _logl_log(p, p, 1, out=False) == _lib.ERR_ARG
    assert _logl_log(p, _density(seed=4), 1) == _lib.ERR_ARG and "leave_one_out" in L.kdehip_last_error().decode()
    assert L.kdehip_evaluate_log_device(None, None, 3, 0, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_evaluate_log_device_at(None, None, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_log_device(None, None, 0, None, None) == _lib.ERR_ARG
    res = C.c_double(0.0)
    assert L.kdehip_eval_avg_logl_log_device(None, None, 0, C.byref(res), None) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_log_device_batch(1, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_log_device_batch(-1, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_eval_avg_logl_log_device_batch(0, None, None, None) == _lib.KDEHIP_OK  # nothing to do
    items = (_lib.CLoglManifoldItem * 1)()  # null handles, and a mask bit no density could have
    items[0].circular_mask = 1 << 9
    assert L.kdehip_eval_avg_logl_log_device_batch(1, items, C.c_void_p(256), None) == _lib.ERR_ARG


def test_dimension_mismatch_is_refused():
    p, q = _density(D=2), _density(D=3)
    assert _logl_log(p, q, 0) == _lib.ERR_DIM_MISMATCH
    for fn in (kdehip.evalAvgLogL, kdehip.kld, kdehip.minkld):
        with pytest.raises(ValueError):
            fn(p, q, log_domain=True)
    with pytest.raises(ValueError):
        kdehip.evaluate_log(p, np.zeros((3, 4)))


def test_nine_dimensions_are_unsupported():
    p = _density(D=9, N=5)
    assert _evaluate_log(p) == _lib.ERR_UNSUPPORTED
    assert _evaluate_log(p, loo=1) == _lib.ERR_UNSUPPORTED
    assert _logl_log(p, p, 1) == _lib.ERR_UNSUPPORTED
    assert _logl_log(p, _density(D=9, N=7, seed=4), 0) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_are_unsupported():
    p, q = _density(seed=5), _density(seed=6)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    assert _evaluate_log(p) == _lib.ERR_UNSUPPORTED and "bandwidth" in _lib.lib.kdehip_last_error().decode()
    assert _logl_log(p, q, 0) == _lib.ERR_UNSUPPORTED
    assert _logl_log(q, p, 0) != _lib.ERR_UNSUPPORTED  # (`at` contributes only points and weights)


def test_a_manifold_byte_above_one_is_refused():
    p, q = _density(seed=1), _density(seed=2)
    keep, bad = _u8([0, 2])
    for rc in (_evaluate_log(p, man=bad), _evaluate_log(p, loo=1, man=bad), _logl_log(p, q, 0, man=bad), _logl_log(p, p, 1, man=bad)):
        assert rc == _lib.ERR_ARG and "manifold" in _lib.lib.kdehip_last_error().decode()


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p, q = _density(seed=1), _density(seed=2)
    for vals in (None, [0, 0], [1, 0]):
        keep, mp = (None, None) if vals is None else _u8(vals)
        for rc in (_evaluate_log(p, man=mp), _evaluate_log(p, loo=1, man=mp), _logl_log(p, q, 0, man=mp),
                   _logl_log(p, p, 1, man=mp), _logl_log(p, None, 1, man=mp)):
            assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in _lib.lib.kdehip_last_error().decode().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    return fake


def test_python_front_end_refusals():
    p, fake = _density(), _fake_device_density()
    for fn in (lambda: kdehip.evalAvgLogL(p, fake, log_domain=True), lambda: kdehip.evalAvgLogL(fake, p, log_domain=True),
               lambda: kdehip.kld(p, fake, log_domain=True), lambda: kdehip.minkld(fake, p, log_domain=True),
               lambda: kdehip.entropy(np.zeros((2, 3)), log_domain=True),
               lambda: kdehip.kld_batch([(p, fake)], log_domain=True), lambda: kdehip.kld_batch([(p, p)], log_domain=True),
               lambda: kdehip.eval_avg_logl_device_batch([(p, p)], None, log_domain=True),
               lambda: kdehip.evaluate_log(fake, np.zeros((2, 3))), lambda: kdehip.evaluate_log(p, fake),
               lambda: fake.evaluate_log(p)):
        with pytest.raises(TypeError):
            fn()
    with pytest.raises(ValueError, match="not supported"):
        kdehip.kld(p, _density(seed=2), "unscented", log_domain=True)
    with pytest.raises(ValueError):
        kdehip.evaluate_log(p, np.zeros((2, 3)), manifold=[1])  # one entry per dimension
    with pytest.raises(ValueError):
        kdehip.evalAvgLogL(p, p, manifold=[1, 0, 0], log_domain=True)


def test_julia_shim_calls_the_new_entries_as_the_header_declares_them():
    """the pattern of tests/test_julia_shim_syntax.py on the log-domain calls: every new host entry is reached by a ccall
    whose argument types fit the header, the manifold goes through the shim's one reader, and the file stays balanced"""
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    for name in ("kdehip_evaluate_log", "kdehip_eval_avg_logl_log"):
        m = re.search(r"ccall\(\(:" + name + r",\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
        assert m, name
        types = [t.strip() for t in m.group(1).split(",") if t.strip()]
        assert len(types) == len(params[name]), (name, types, params[name])
        for jt, ct in zip(types, params[name]):
            assert ct in shim.JULIA_TO_C[jt], (name, jt, ct)
    for fn in ("hip_evaluate_log", "hip_evalAvgLogL_log", "hip_entropy_log", "hip_kld_log", "hip_minkld_log"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    for fn in ("hip_evaluate_log", "hip_evalAvgLogL_log"):
        body = code[code.index("function " + fn + "("):]
        body = body[:body.index("\nend")]
        assert "manifold_bytes(" in body, fn
