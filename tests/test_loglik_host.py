"""`evalAvgLogL` / `entropy` / `kld` / `minkld` without a GPU (include/kdehip.h section 5b): the argument checks the entries
make before they touch a device, and the Python front end's refusals (mixed density kinds, kld's unscented method)."""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _call(bd, at, loo, device=NO_SUCH_DEVICE, out=True):
    res = C.c_double(0.0)
    cb = None if bd is None else C.byref(bd._cstruct())
    ca = None if at is None else (cb if at is bd else C.byref(at._cstruct()))
    return _lib.lib.kdehip_eval_avg_logl(cb, ca, int(loo), C.byref(res) if out else None, int(device))


def test_null_arguments_are_refused():
    p = _density()
    assert _call(None, p, 0) == _lib.ERR_ARG
    assert _call(p, None, 0) == _lib.ERR_ARG  # (a NULL `at` stands for bd only with leave_one_out)
    assert _call(p, p, 1, out=False) == _lib.ERR_ARG
    assert _call(p, None, 1, out=False) == _lib.ERR_ARG
    assert _lib.lib.kdehip_eval_avg_logl_device(None, None, 0, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_eval_avg_logl_device_batch(1, None, None, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_eval_avg_logl_device_batch(-1, None, None, None) == _lib.ERR_ARG
    items = (_lib.CLoglItem * 1)()  # null handles
    assert _lib.lib.kdehip_eval_avg_logl_device_batch(1, items, C.c_void_p(256), None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_evaluate_device(None, None, 3, 0, None, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_evaluate_device_at(None, None, None, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_eval_avg_logl_device_batch(0, None, None, None) == _lib.KDEHIP_OK  # nothing to do


def test_dimension_counts_above_the_compiled_limit_are_unsupported():
    p = _density(D=9, N=5)
    assert _call(p, p, 1) == _lib.ERR_UNSUPPORTED
    assert _call(p, None, 1) == _lib.ERR_UNSUPPORTED
    assert _call(p, _density(D=9, N=7, seed=4), 0) == _lib.ERR_UNSUPPORTED


def test_per_point_bandwidths_on_the_evaluated_density_are_unsupported():
    p, q = _density(seed=5), _density(seed=6)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    assert _call(p, q, 0) == _lib.ERR_UNSUPPORTED
    assert "bandwidth" in _lib.lib.kdehip_last_error().decode()
    assert _call(p, p, 1) == _lib.ERR_UNSUPPORTED
    # `at` contributes only its points and weights: its bandwidths are not checked
    assert _call(q, p, 0) != _lib.ERR_UNSUPPORTED


def test_leave_one_out_needs_the_same_density():
    p, q = _density(seed=1), _density(seed=2)
    assert _call(p, q, 1) == _lib.ERR_ARG
    assert "leave_one_out" in _lib.lib.kdehip_last_error().decode()


def test_dimension_mismatch_is_refused():
    p, q = _density(D=2), _density(D=3)
    assert _call(p, q, 0) == _lib.ERR_DIM_MISMATCH
    with pytest.raises(ValueError):
        kdehip.evalAvgLogL(p, q)
    with pytest.raises(ValueError):
        kdehip.kld(p, q)
    with pytest.raises(ValueError):
        kdehip.minkld(q, p)


def test_a_valid_pair_only_fails_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p, q = _density(seed=1), _density(seed=2)
    for rc in (_call(p, q, 0), _call(p, p, 1), _call(p, None, 1), _call(p, p, 0)):
        assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
        assert "device" in _lib.lib.kdehip_last_error().decode().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    return fake


def test_mixed_density_kinds_are_a_type_error():
    p, fake = _density(), _fake_device_density()
    for fn in (lambda: kdehip.evalAvgLogL(p, fake), lambda: kdehip.evalAvgLogL(fake, p), lambda: kdehip.kld(p, fake),
               lambda: kdehip.kld(fake, p), lambda: kdehip.minkld(p, fake), lambda: kdehip.entropy(np.zeros((2, 3))),
               lambda: kdehip.kld_batch([(p, fake)]), lambda: kdehip.kld_batch([(p, p)])):
        with pytest.raises(TypeError):
            fn()


def test_unscented_kld_is_not_supported():
    p, q = _density(seed=1), _density(seed=2)
    with pytest.raises(ValueError, match="not supported"):
        kdehip.kld(p, q, method="unscented")
    with pytest.raises(ValueError, match="not supported"):
        kdehip.kld(p, q, "unscented")
