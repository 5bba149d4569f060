"""`sample` / `rand` / `resample` without a GPU (include/kdehip.h section 2f): the argument checks kdehip_sample makes before
it touches a device, and the label rule of the numpy model the GPU tests use against a literal restatement of the
reference's sorted-merge loop (src/KDE01.jl:173-180)."""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import f64p, i64p, ptr


def _call(p, Npts, ind_in=None, device=0):
    n = max(int(Npts), 0)
    pts = np.zeros(max(1, p.bt.dims * n))
    ind = np.zeros(max(1, n), dtype=np.int64)
    lab = None if ind_in is None else np.ascontiguousarray(ind_in, dtype=np.int64)
    return _lib.lib.kdehip_sample(C.byref(p._cstruct()), int(Npts), C.c_uint64(1), 0,
                                  None if lab is None else ptr(lab, i64p), ptr(pts, f64p), ptr(ind, i64p), int(device))


def _density(D=2, N=20, weights=None):
    rng = np.random.default_rng(3)
    return kdehip.kde(rng.standard_normal((D, N)), [0.3], weights)


def _set_weight(p, orig_index, value):
    """writes the leaf weight of original point `orig_index` (0-based)"""
    N = p.bt.num_points
    k = int(np.nonzero(p.bt.permutation[N:] - 1 == orig_index)[0][0])
    p.bt.weights[N + k] = value


def test_zero_samples_do_nothing_and_negative_counts_are_refused():
    p = _density()
    assert _call(p, 0) == _lib.KDEHIP_OK
    assert _call(p, -1) == _lib.ERR_ARG
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.sample(p, -3, seed=1)
    assert e.value.code == _lib.ERR_ARG
    pts, ind = kdehip.sample(p, 0, seed=1)
    assert pts.shape == (2, 0) and ind.shape == (0,)


@pytest.mark.parametrize("bad", [-0.25, np.nan, np.inf, -np.inf])
def test_weights_that_are_negative_or_not_finite_are_refused(bad):
    p = _density()
    _set_weight(p, 4, bad)
    assert _call(p, 5) == _lib.ERR_ARG
    assert "weight" in _lib.lib.kdehip_last_error().decode()


def test_weights_without_a_positive_total_are_refused():
    p = _density(N=6)
    for i in range(6):
        _set_weight(p, i, 0.0)
    assert _call(p, 5) == _lib.ERR_ARG
    assert "total" in _lib.lib.kdehip_last_error().decode()
    q = _density(N=4)
    for i in range(4):
        _set_weight(q, i, 1e308)  # finite weights whose sum overflows
    assert _call(q, 5) == _lib.ERR_ARG


def test_dimension_counts_above_the_compiled_limit_are_unsupported():
    p = _density(D=9, N=5)
    assert _call(p, 3) == _lib.ERR_UNSUPPORTED


def test_given_labels_out_of_range_are_refused_on_the_host():
    p = _density(N=10)
    assert _call(p, 3, ind_in=[1, 11, 2]) == _lib.ERR_ARG
    assert _call(p, 2, ind_in=[0, 3]) == _lib.ERR_ARG
    with pytest.raises(kdehip.KdeHipError):
        kdehip.sample(p, 2, ind=[5, -1], seed=0)


def test_a_broken_permutation_is_refused():
    p = _density(N=8)
    N = p.bt.num_points
    p.bt.permutation[N + 1] = p.bt.permutation[N]  # a repeated original index
    assert _call(p, 3) == _lib.ERR_ARG


def test_argument_errors_come_before_any_device_is_touched():
    """An ordinal no machine has: every refusal above is still the argument's, not KDEHIP_ERR_NO_DEVICE / device range."""
    p = _density(N=6)
    _set_weight(p, 0, -1.0)
    assert _call(p, 4, device=9999) == _lib.ERR_ARG
    assert _call(_density(D=9, N=4), 2, device=9999) == _lib.ERR_UNSUPPORTED
    assert _call(_density(N=6), 2, ind_in=[7, 1], device=9999) == _lib.ERR_ARG


def _reference_merge(w, t_sorted):
    """src/KDE01.jl:168-180 with 0-based i: w = cumsum(w) ./ w[end]; t = [sort(rand(Npts)); 10]; walk the points once,
    emitting label i while w[i] > t[ii]."""
    w = np.cumsum(w)
    w = w / w[-1]
    t = list(t_sorted) + [10.0]
    out = []
    ii = 0
    for i in range(len(w)):
        while w[i] > t[ii]:
            out.append(i)
            ii += 1
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("N,Npts,zeros", [(1, 50, 0), (2, 100, 0), (7, 1000, 2), (200, 5000, 30), (1000, 20000, 0)])
def test_numpy_label_rule_equals_the_reference_merge_on_sorted_uniforms(N, Npts, zeros):
    rng = np.random.default_rng(N + Npts)
    w = rng.uniform(0.0, 1.0, size=N)
    if zeros:
        w[rng.choice(N, size=zeros, replace=False)] = 0.0
        if w.sum() == 0.0:
            w[0] = 1.0
    u, _ = kdehip.philox_streams(11, 0, Npts, 1, 1)
    # the model of tests/test_gpu_sample.py
    C_ = np.cumsum(w)
    C_ /= C_[-1]
    lab = np.searchsorted(C_, u, side="right")
    ref = _reference_merge(w, np.sort(u))
    assert np.array_equal(np.sort(lab), ref)
    assert not np.isin(lab, np.nonzero(w == 0.0)[0]).any()


def test_philox_stream_of_a_sample_call_is_the_documented_one():
    """u of sample g = the uniform kdehip_philox_fill_uniform gives for (g, K = 1); offsets continue the stream."""
    u, n = kdehip.philox_streams(5, 0, 100, 1, 3)
    u2, n2 = kdehip.philox_streams(5, 40, 60, 1, 3)
    assert np.array_equal(u[40:], u2) and np.array_equal(n[120:], n2)
    assert ((u > 0) & (u < 1)).all()
