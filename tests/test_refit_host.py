"""Reweighting and moving a density without re-forming its tree (include/kdehip.h section 5r) without a GPU: the host entry
kdehip_density_refit behind `BallTreeDensity.changeWeights / movePoints / bayes_update`, against a rebuild by `kde` (H1), the
NumPy model of tests/refit_model.py (H2, H3), its own input (H4), its refusals (H5) and the Bayes formula (H6).  Arrays are
compared BIT FOR BIT (their bytes), not by value."""
import ctypes as C
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip import refit as rf
from kdehip._lib import f64p, i64p, u8p
from tests import refit_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kdehip_density_refit", "kdehip_density_refit_device", "kdehip_density_refit_device_batch"]
TOPOLOGY = ("left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in hdr, name
    assert "(5r)" in hdr
    for cls in (kdehip.BallTreeDensity, kdehip.DeviceDensity):
        for name in ("changeWeights", "movePoints", "bayes_update"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(kdehip.DeviceDensity.refit_batch)


def _points(seed, D, N):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)), rng


_same_bits = rm.same_bits


def _same_tree(got, src):
    """leaf order and child arrays are the input's"""
    g, s = rm.arrays_of(got), rm.arrays_of(src)
    for f in TOPOLOGY:
        assert g[f].tobytes() == s[f].tobytes(), f


def _dyadic_weights(rng, N):
    """k_i / 2^20 with sum k_i = 2^20 and some k_i = 0: every partial sum of kde's normalisation is exact, the total is 1.0"""
    total = 1 << 20
    if N == 1:
        return np.array([1.0])
    k = rng.integers(0, 1 << 10, size=N)
    if N >= 3:
        k[rng.choice(N, size=max(1, N // 10), replace=False)] = 0
    k[N - 1] = 0
    k[N - 1] = total - int(k.sum())
    assert k.min() >= 0 and int(k.sum()) == total and (N < 3 or (k == 0).any())
    return k.astype(np.float64) / total


# ---- H1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 5, 129, 1000])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_h1_reweighting_equals_a_rebuild_bit_for_bit(D, N):
    pts, rng = _points(100 * D + N, D, N)
    sd = rng.choice([0.125, 0.25, 0.5], size=D)  # dyadic: sqrt(sd^2)^2 == sd^2, so getBW hands kde the same variances
    p = kdehip.kde(pts, sd)
    w = _dyadic_weights(rng, N)
    got = p.changeWeights(w)
    want = kdehip.kde(kdehip.getPoints(p), kdehip.getBW(p)[:, 0], w)
    _same_bits(got, want)
    _same_tree(got, p)
    assert got.multibandwidth == 0


# ---- H2 ----------------------------------------------------------------------------------------------------------------------
def _free_weights(rng, N):
    w = rng.uniform(0.0, 3.0, size=N)
    if N >= 3:
        w[rng.choice(N, size=max(1, N // 7), replace=False)] = 0.0
    return w


@pytest.mark.parametrize("D,N", [(1, 2), (2, 3), (3, 129), (8, 300), (2, 1000)])
def test_h2_arbitrary_weights_equal_the_model(D, N):
    pts, rng = _points(7 * D + N, D, N)
    p = kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D), rng.uniform(0.1, 1.0, size=N))
    w = _free_weights(rng, N)
    assert w.sum() != 1.0
    got = p.changeWeights(w)
    _same_bits(got, rm.refit(rm.arrays_of(p), D, N, new_weights=w))
    _same_tree(got, p)
    assert np.array_equal(kdehip.getWeights(got), w)  # used as given: not normalised


@pytest.mark.parametrize("D,N", [(1, 3), (3, 130), (6, 257)])
def test_h2_per_point_bandwidths_with_their_extremes(D, N):
    pts, rng = _points(11 * D + N, D, N)
    p = kdehip.kde_varbw(pts, rng.uniform(0.1, 0.9, size=(D, N)), rng.uniform(0.1, 1.0, size=N))
    w = _free_weights(rng, N)
    got = p.changeWeights(w)
    assert got.multibandwidth == 1 and got.bandwidthMin.shape == (2 * N * D,)
    _same_bits(got, rm.refit(rm.arrays_of(p), D, N, new_weights=w, varbw=True))
    moved = p.movePoints(rng.standard_normal((D, N)))
    _same_tree(moved, p)
    assert moved.bandwidthMin.tobytes() == p.bandwidthMin.tobytes() and moved.bandwidthMax.tobytes() == p.bandwidthMax.tobytes()


# ---- H3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(1, 1), (6, 1), (1, 2), (2, 5), (3, 129), (8, 200), (2, 1000)])
def test_h3_moved_points_equal_the_model(D, N):
    pts, rng = _points(13 * D + N, D, N)
    p = kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D), rng.uniform(0.1, 1.0, size=N))
    delta = rng.standard_normal((D, N)) * 0.3
    got = p.movePoints(delta)
    _same_bits(got, rm.refit(rm.arrays_of(p), D, N, delta=delta))
    _same_tree(got, p)
    assert np.array_equal(kdehip.getPoints(got), kdehip.getPoints(p) + delta)
    both = rf.refit_host(p, new_weights=_free_weights(rng, N), delta=delta)
    _same_bits(both, rm.refit(rm.arrays_of(p), D, N, new_weights=kdehip.getWeights(both), delta=delta), "both at once")


def test_h3_a_circular_dimension_wraps_across_the_cut():
    rng = np.random.default_rng(5)
    N = 200
    x = rng.standard_normal(N)
    th = rm.PI - np.abs(rng.standard_normal(N)) * 0.2  # just below +pi ...
    th[::2] = -rm.PI + np.abs(rng.standard_normal(N // 2)) * 0.2  # ... and just above -pi: one cluster across the cut
    pts = np.stack([x, th])
    tman = ["euclid", "circular"]
    p = kdehip.kde(pts, [0.3, 0.2], rng.uniform(0.1, 1.0, size=N), tree_manifold=tman)
    delta = np.stack([rng.standard_normal(N) * 0.1, rng.uniform(-0.5, 0.5, size=N)])
    got = p.movePoints(delta)  # (the tree's own operators by default)
    assert np.array_equal(got.tree_manifold, p.tree_manifold)
    _same_bits(got, rm.refit(rm.arrays_of(p), 2, N, delta=delta, circ=[False, True]))
    th_new = kdehip.getPoints(got)[1]
    assert (th_new >= -rm.PI).all() and (th_new < rm.PI).all()
    assert (np.abs(th + delta[1]) > rm.PI).any()  # some sums did leave [-pi, pi)
    _same_bits(p.movePoints(delta, tree_manifold=tman), got, "explicit operators")
    _same_bits(p.changeWeights(kdehip.getWeights(p)), p, "the circular boxes are recomputed to the same bits")


# ---- H4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(1, 1), (1, 2), (3, 129), (8, 1000)])
def test_h4_a_zero_delta_returns_the_input_bits(D, N):
    pts, rng = _points(17 * D + N, D, N)
    p = kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D), rng.uniform(0.1, 1.0, size=N) if N > 1 else None)
    _same_bits(p.movePoints(np.zeros((D, N))), p)
    _same_bits(p.changeWeights(kdehip.getWeights(p)), p, "its own weights")


# ---- H5 ----------------------------------------------------------------------------------------------------------------------
def _raw_call(p, D=None, N=None, new_weights=None, delta=None, tman=None, null=None):
    """kdehip_density_refit on p's arrays through ctypes; `null`: the index of an array argument passed as NULL.  Returns
    (rc, message, whether any output byte was written)."""
    a = rm.arrays_of(p)
    ins = [a[f] for f in ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf",
                          "permutation", "means", "bandwidth", "bandwidthMin", "bandwidthMax")]
    outs = [np.full_like(x, 77) for x in ins]
    snap = [o.copy() for o in outs]

    def pp(x):
        return None if x is None else x.ctypes.data_as(f64p if x.dtype == np.float64 else i64p if x.dtype == np.int64 else u8p)
    args_in = [pp(x) for x in ins]
    args_out = [pp(x) for x in outs]
    if null is not None:
        (args_in if null < 12 else args_out)[null % 12] = None
    rc = _lib.lib.kdehip_density_refit(p.bt.dims if D is None else D, p.bt.num_points if N is None else N, *args_in, 0,
                                       pp(new_weights), pp(delta), pp(tman), *args_out)
    msg = _lib.lib.kdehip_last_error().decode()
    return rc, msg, any(o.tobytes() != s.tobytes() for o, s in zip(outs, snap))


def test_h5_refusals():
    D, N = 3, 50
    pts, rng = _points(3, D, N)
    p = kdehip.kde(pts, [0.3])
    w = np.full(N, 0.5)
    dl = np.zeros(D * N)
    rc, msg, wrote = _raw_call(p, new_weights=w, delta=dl)
    assert rc == _lib.KDEHIP_OK and wrote
    for null in (0, 7, 11, 12, 20, 23):
        rc, msg, wrote = _raw_call(p, new_weights=w, null=null)
        assert rc == _lib.ERR_ARG and "null" in msg and not wrote, null
    rc, msg, wrote = _raw_call(p)
    assert rc == _lib.ERR_ARG and "new_weights" in msg and "delta" in msg and "null" in msg and not wrote
    for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[N - 1] = bad
        rc, msg, wrote = _raw_call(p, new_weights=wb, delta=dl)
        assert rc == _lib.ERR_ARG and "new_weights" in msg and not wrote, bad
    for bad in (np.nan, np.inf, -np.inf):
        db = dl.copy()
        db[D * N - 1] = bad
        rc, msg, wrote = _raw_call(p, new_weights=w, delta=db)
        assert rc == _lib.ERR_ARG and "delta" in msg and not wrote, bad
    for badD in (0, -1, _lib.MAX_DIMS + 1):
        rc, msg, wrote = _raw_call(p, D=badD, new_weights=w)
        assert rc == _lib.ERR_UNSUPPORTED and "ndims" in msg and not wrote, badD
    rc, msg, wrote = _raw_call(p, new_weights=w, tman=np.array([0, 2, 0], dtype=np.uint8))
    assert rc == _lib.ERR_ARG and "tree_manifold" in msg and not wrote
    # the Python front end's own argument errors
    with pytest.raises(ValueError):
        p.changeWeights(np.ones(N + 1))
    with pytest.raises(ValueError):
        p.movePoints(np.zeros((D, N + 1)))
    with pytest.raises(kdehip.KdeHipError) as e:
        p.changeWeights(-np.ones(N))
    assert e.value.code == _lib.ERR_ARG


# ---- H6 ----------------------------------------------------------------------------------------------------------------------
def bayes_reference(w, logl):
    """the formula in extended precision: (w', log_evidence, ess)"""
    w = np.asarray(w, dtype=np.longdouble)
    l = np.asarray(logl, dtype=np.longdouble)
    m = l[w > 0].max()
    t = np.where(w > 0, w * np.exp(np.where(w > 0, l - m, 0)), 0)
    S = t.sum()
    wn = t / S
    return wn.astype(np.float64), float(m + np.log(S)), float(1 / np.sum(wn * wn))


def test_h6_host_bayes_update():
    D, N = 2, 500
    pts, rng = _points(23, D, N)
    w0 = rng.uniform(0.1, 1.0, size=N)
    w0[::9] = 0.0
    p = kdehip.kde(pts, [0.4], w0)
    logl = rng.uniform(-1000.0, 0.0, size=N) - 2000.0  # spans 1e3; exp(logl) itself underflows to 0 everywhere
    assert np.exp(logl).max() == 0.0
    logl[5] = -np.inf
    q, le, ess = p.bayes_update(logl)
    wn, le_ref, ess_ref = bayes_reference(kdehip.getWeights(p), logl)
    got = kdehip.getWeights(q)
    # (1e-300: a weight below 2.2e-308 is subnormal in fp64 and holds fewer than 53 bits -- no relative bound can apply to it;
    # the absolute part of tests/test_gpu_conditional.py's bound for its weights)
    assert np.all(np.abs(got - wn) <= 1e-12 * np.abs(wn) + 1e-300)
    assert got[5] == 0.0 and (got[::9] == 0.0).all() and abs(got.sum() - 1.0) < 1e-12
    assert abs(le - le_ref) <= 1e-12 * max(1.0, abs(le_ref))
    assert abs(ess - ess_ref) <= 1e-12 * ess_ref
    _same_bits(q, p.changeWeights(got), "the update is changeWeights of its weights")
    for bad in (np.nan, np.inf):
        lb = logl.copy()
        lb[7] = bad
        with pytest.raises(ValueError):
            p.bayes_update(lb)
    with pytest.raises(ValueError):
        p.bayes_update(np.full(N, -np.inf))
