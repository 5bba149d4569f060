"""Reweighting and moving a RESIDENT density without re-forming its tree (csrc/refit.hip, include/kdehip.h section 5r):
`DeviceDensity.changeWeights / movePoints / bayes_update / refit_batch` against the host entry kdehip_density_refit -- which
tests/test_refit_host.py pins to a rebuild by `kde` and to the NumPy model -- BIT FOR BIT (G1), as an input of the sampler and
of the other consumers (G2, G3: the test of the packers' recomputed facts), the Bayes update against the formula in extended
precision with the bounds of the host test (G4), batches (G5), the two index conventions (G6), repeatability (G7), the
scaling law (G8), a density of one point (G9), a source with a bandwidth per point (G10), a tree built with circular
operators, built and uploaded, alone and in a batch with a Euclidean item (G11), and more chunks than the fold's tile holds
(G12).  The refit of an UPLOADED density has no arrays to download: it is compared as an input of the consumers.

Shapes: two leaves is the smallest tree; 129 and 1025 cross a power of two (uneven heights); 5000 has heights wider than a
workgroup, so it runs one launch per height as well as the one-workgroup top.  Every source is built once and never changed."""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip import refit as rf
from tests import refit_model as rm
from tests.test_refit_host import bayes_reference

pytestmark = pytest.mark.gpu

NS, DS = [2, 3, 129, 1025, 5000], [1, 6, 8]


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


_BUILT, _HOST = {}, {}


def _points(rng, D, N):
    return rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))


def _built(D, N):
    """(resident density built by the library from device points, its downloaded arrays): made once, shared, never changed"""
    if (D, N) not in _BUILT:
        rng = np.random.default_rng(1000 * D + N)
        d_pts = _dev(_points(rng, D, N).T)  # column-major D x N
        _torch().cuda.synchronize()
        dd = kdehip.DeviceDensity.from_device_points(d_pts, D, N)
        _BUILT[(D, N)] = (dd, dd.download())
    return _BUILT[(D, N)]


def _uploaded(D, N):
    """(a density the caller built and uploaded, the host density)"""
    if (D, N) not in _HOST:
        rng = np.random.default_rng(77 * D + N)
        hp = kdehip.kde(_points(rng, D, N), rng.uniform(0.2, 0.6, size=D), rng.uniform(0.1, 1.0, size=N))
        _HOST[(D, N)] = (kdehip.DeviceDensity(hp), hp)
    return _HOST[(D, N)]


def _weights(rng, N):
    w = rng.uniform(0.05, 2.0, size=N)
    if N > 4:
        w[::7] = 0.0
    return w


# ---- G1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DS)
def test_g1_a_built_source_equals_the_host_refit_bit_for_bit(D, N):
    dd, hp = _built(D, N)
    rng = np.random.default_rng(D + 10 * N)
    w, delta = _weights(rng, N), rng.standard_normal((D, N)) * 0.3
    rm.same_bits(dd.changeWeights(w).download(), hp.changeWeights(w), "weights")
    rm.same_bits(dd.changeWeights(_dev(w)).download(), hp.changeWeights(w), "weights from a tensor")
    rm.same_bits(dd.movePoints(delta).download(), hp.movePoints(delta), "delta")
    rm.same_bits(dd.movePoints(_dev(delta)).download(), hp.movePoints(delta), "delta from a tensor")
    both, le, ess = rf.refit_device(dd, w, rf.WEIGHTS, delta)
    assert le is None and ess is None
    rm.same_bits(both.download(), rf.refit_host(hp, new_weights=w, delta=delta), "both in one call")
    again = both.changeWeights(w[::-1].copy())  # a refit of a refit: the table is the source's
    rm.same_bits(again.download(), rf.refit_host(hp, new_weights=w[::-1].copy(), delta=delta), "refit of a refit")
    rm.same_bits(dd.download(), hp, "the source is not written")


# ---- G2 ----------------------------------------------------------------------------------------------------------------------
def _product(a, other, seed):
    return kdehip.prodAppxMSGibbsS_resident([a, other], Np=96, Niter=2, seed=seed, precision=64)


def _same_product(res, host_refit, other, what):
    up = kdehip.DeviceDensity(host_refit)
    (p1, i1), (p2, i2) = _product(res, other, 11), _product(up, other, 11)
    assert i1.tobytes() == i2.tobytes(), what
    assert p1.tobytes() == p2.tobytes(), what


def _runs_of_zeros(hp, N):
    """a tenth of the weights exactly 0, in a RUN of leaf positions: whole subtrees without weight, so internal nodes with
    weight 0 and variance 0 -- the packers' `bad` flag and the generic arithmetic"""
    rng = np.random.default_rng(N)
    w = rng.uniform(0.1, 1.0, size=N)
    w[hp.bt.permutation[N:N + max(2, N // 10)] - 1] = 0.0
    return w


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", [2, 6])
def test_g2_the_result_as_an_input_of_the_sampler(D, N):
    dd, hp = _built(D, N)
    other = _uploaded(D, 200)[0]
    rng = np.random.default_rng(3 * D + N)
    w, delta = _weights(rng, N), rng.standard_normal((D, N)) * 0.2
    _same_product(dd.changeWeights(w), hp.changeWeights(w), other, "weights")
    _same_product(dd.movePoints(delta), hp.movePoints(delta), other, "delta")


@pytest.mark.parametrize("D,N", [(2, 1025), (6, 129), (6, 5000)])
@pytest.mark.parametrize("source", ["built", "uploaded"])
def test_g2_zero_runs_and_a_weight_ratio_of_1e12(D, N, source):
    dd, hp = _built(D, N) if source == "built" else _uploaded(D, N)
    other = _uploaded(D, 200)[0]
    wz = _runs_of_zeros(hp, N)
    hz = hp.changeWeights(wz)
    assert (hz.bandwidth[:(N - 1) * D] == 0.0).any()  # (some internal node has no weight below it)
    _same_product(dd.changeWeights(wz), hz, other, "zero runs")
    rng = np.random.default_rng(N + D)
    wr = rng.uniform(0.5, 1.0, size=N)
    wr[::3] *= 1e-12
    _same_product(dd.changeWeights(wr), hp.changeWeights(wr), other, "ratio 1e12")
    delta = rng.standard_normal((D, N)) * 0.2
    _same_product(dd.movePoints(delta), hp.movePoints(delta), other, "delta")


# ---- G3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,source", [(1, 129, "built"), (6, 1025, "built"), (8, 5000, "uploaded"), (2, 3, "uploaded")])
def test_g3_other_consumers_agree_with_the_uploaded_host_refit(D, N, source):
    dd, hp = _built(D, N) if source == "built" else _uploaded(D, N)
    rng = np.random.default_rng(5 * D + N)
    w, delta = _weights(rng, N), rng.standard_normal((D, N)) * 0.2
    res = rf.refit_device(dd, w, rf.WEIGHTS, delta)[0]
    up = kdehip.DeviceDensity(rf.refit_host(hp, new_weights=w, delta=delta))
    pos = _points(rng, D, 300)
    assert res.evaluate(pos).tobytes() == up.evaluate(pos).tobytes()
    assert res.evaluate_log(pos).tobytes() == up.evaluate_log(pos).tobytes()
    assert res.evaluate_log(lvFlag=True).tobytes() == up.evaluate_log(lvFlag=True).tobytes()
    (x1, l1), (x2, l2) = kdehip.sample(res, 500, seed=9), kdehip.sample(up, 500, seed=9)
    assert l1.tobytes() == l2.tobytes() and x1.tobytes() == x2.tobytes()
    assert kdehip.ise(res, up) == 0.0


# ---- G4, G7 ------------------------------------------------------------------------------------------------------------------
def _check_bayes(dd, hp, logl_host, res, le, ess):
    wn, le_ref, ess_ref = bayes_reference(kdehip.getWeights(hp), logl_host)
    hq = res.download()
    got = kdehip.getWeights(hq)
    print(f"bayes: max rel weight error {np.max(np.abs(got - wn) / np.maximum(wn, 1e-300)):.3e}, log evidence {le!r} vs "
          f"{le_ref!r}, ess {ess!r} vs {ess_ref!r}")
    assert np.all(np.abs(got - wn) <= 1e-12 * np.abs(wn) + 1e-300)  # (the absolute part: subnormal weights, as on the host)
    assert abs(le - le_ref) <= 1e-12 * max(1.0, abs(le_ref))
    assert abs(ess - ess_ref) <= 1e-12 * ess_ref
    # the arithmetic with a tolerance and the exact refit, held apart: the arrays are the host's for the weights it made
    rm.same_bits(hq, hp.changeWeights(got), "the update is changeWeights of its weights")


@pytest.mark.parametrize("D,N", [(2, 129), (6, 5000)])
def test_g4_g7_device_bayes_update_from_a_tensor(D, N):
    dd, hp = _built(D, N)
    rng = np.random.default_rng(31 * D + N)
    logl = rng.uniform(-1000.0, 0.0, size=N) - 2000.0  # spans 1e3: the unshifted exp underflows everywhere
    logl[1] = -np.inf
    res, le, ess = dd.bayes_update(_dev(logl))
    _check_bayes(dd, hp, logl, res, le, ess)
    res2, le2, ess2 = dd.bayes_update(logl)  # G7: a repeat (from a host array this time) gives identical bits
    assert np.float64(le).tobytes() == np.float64(le2).tobytes() and np.float64(ess).tobytes() == np.float64(ess2).tobytes()
    rm.same_bits(res2.download(), res.download(), "repeat")


def test_g4_device_bayes_update_from_a_density_likelihood():
    D, N = 3, 1025
    dd, hp = _built(D, N)
    like = _uploaded(D, 200)[0]
    res, le, ess = dd.bayes_update(like)
    logl = like.evaluate_log(dd)  # at dd's points, in dd's original order
    _check_bayes(dd, hp, logl, res, le, ess)


def _raw_single(dd, values, kind):
    h = C.c_void_p(12345)
    le, ess = C.c_double(0.0), C.c_double(0.0)
    _torch().cuda.synchronize()
    rc = _lib.lib.kdehip_density_refit_device(C.byref(h), dd._h, _lib.addr(values), kind, 0, None, None, C.byref(le), C.byref(ess))
    return rc, h.value, _lib.lib.kdehip_last_error().decode()


def test_g4_refused_log_likelihoods_and_weights_leave_no_handle():
    D, N = 2, 1025
    dd, hp = _built(D, N)
    good = np.linspace(-5.0, 0.0, N)
    cases = {"all -Inf": np.full(N, -np.inf), "a NaN": good.copy(), "a +Inf": good.copy()}
    cases["a NaN"][N - 1] = np.nan
    cases["a +Inf"][500] = np.inf
    for what, logl in cases.items():
        rc, h, msg = _raw_single(dd, _dev(logl), rf.LOGL)
        assert rc == _lib.ERR_ARG and h is None, (what, msg)
        with pytest.raises(kdehip.KdeHipError) as e:
            dd.bayes_update(logl)
        assert e.value.code == _lib.ERR_ARG, what
    for bad in (-1.0, np.nan, np.inf):
        w = np.ones(N)
        w[3] = bad
        rc, h, msg = _raw_single(dd, _dev(w), rf.WEIGHTS)
        assert rc == _lib.ERR_ARG and h is None and "weight" in msg, bad
    delta = np.zeros((D, N))
    delta[1, 7] = np.nan
    with pytest.raises(kdehip.KdeHipError) as e:
        dd.movePoints(delta)
    assert e.value.code == _lib.ERR_ARG and "delta" in str(e.value)
    no_weight = dd.changeWeights(np.zeros(N))
    rc, h, msg = _raw_single(no_weight, _dev(good), rf.LOGL)
    assert rc == _lib.ERR_ARG and h is None and "positive weight" in msg
    rc, h, msg = _raw_single(dd, None, rf.KEEP)  # nothing to do: refused before any device work
    assert rc == _lib.ERR_ARG and h is None
    rm.same_bits(dd.download(), hp, "the source is untouched by refused calls")


# ---- G5 ----------------------------------------------------------------------------------------------------------------------
def _batch_items():
    rng = np.random.default_rng(55)
    shapes = [(1, 2), (6, 129), (8, 1025), (3, 300), (2, 64)]
    srcs = [_built(D, N)[0] for D, N in shapes]
    return [
        {"density": srcs[0], "weights": np.array([0.25, 3.0])},
        {"density": srcs[1], "logl": rng.uniform(-50.0, 0.0, size=129)},
        {"density": srcs[2], "delta": rng.standard_normal((8, 1025)) * 0.1},
        {"density": srcs[3], "weights": rng.uniform(0.0, 1.0, size=300), "delta": rng.standard_normal((3, 300)), "leaf_order": True},
        {"density": srcs[4], "logl": _dev(rng.uniform(-900.0, -100.0, size=64)), "leaf_order": True},
    ]


def test_g5_a_mixed_batch_equals_the_single_calls_bit_for_bit():
    items = _batch_items()
    out = kdehip.DeviceDensity.refit_batch(items)
    assert len(out) == len(items)
    for it, (res, le, ess) in zip(items, out):
        kind = rf.WEIGHTS if "weights" in it else rf.LOGL if "logl" in it else rf.KEEP
        one, le1, ess1 = rf.refit_device(it["density"], it.get("weights", it.get("logl")), kind, it.get("delta"),
                                         it.get("leaf_order", False))
        rm.same_bits(res.download(), one.download(), f"kind {kind}")
        if kind == rf.LOGL:
            assert np.float64(le).tobytes() == np.float64(le1).tobytes() and np.float64(ess).tobytes() == np.float64(ess1).tobytes()
        else:
            assert le is None and ess is None and le1 is None


def test_g5_one_bad_item_fails_the_whole_batch_and_creates_no_handle():
    a, b = _built(6, 129)[0], _built(2, 64)[0]
    good, bad = _dev(np.ones(129)), _dev(np.full(64, -np.inf))
    arr = (_lib.CRefitItem * 2)()
    arr[0].p, arr[0].d_values, arr[0].kind = a._h, good.data_ptr(), rf.WEIGHTS
    arr[1].p, arr[1].d_values, arr[1].kind = b._h, bad.data_ptr(), rf.LOGL
    hs = (C.c_void_p * 2)(111, 222)
    _torch().cuda.synchronize()
    rc = _lib.lib.kdehip_density_refit_device_batch(2, arr, hs)
    assert rc == _lib.ERR_ARG and hs[0] is None and hs[1] is None
    assert "item 1" in _lib.lib.kdehip_last_error().decode()
    with pytest.raises(kdehip.KdeHipError):
        kdehip.DeviceDensity.refit_batch([{"density": a, "weights": np.ones(129)}, {"density": b, "logl": np.full(64, np.nan)}])


# ---- G6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(1, 3), (6, 1025)])
def test_g6_leaf_order_values_give_the_bits_of_original_order(D, N):
    dd, hp = _built(D, N)
    rng = np.random.default_rng(2 * D + N)
    leaf = hp.bt.permutation[N:] - 1  # the original index of every leaf position
    w, logl, delta = _weights(rng, N), rng.uniform(-30.0, 0.0, size=N), rng.standard_normal((D, N))
    a = rf.refit_device(dd, w, rf.WEIGHTS, delta)[0]
    b = rf.refit_device(dd, w[leaf], rf.WEIGHTS, delta[:, leaf], leaf_order=True)[0]
    rm.same_bits(b.download(), a.download(), "weights and delta")
    (a, le_a, ess_a), (b, le_b, ess_b) = dd.bayes_update(logl), dd.bayes_update(logl[leaf], leaf_order=True)
    rm.same_bits(b.download(), a.download(), "logl")
    assert np.float64(le_a).tobytes() == np.float64(le_b).tobytes() and np.float64(ess_a).tobytes() == np.float64(ess_b).tobytes()


# ---- G8 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-30, 30])
def test_g8_exact_rescaling_of_points_bandwidths_and_delta(k):
    D, N = 4, 300
    rng = np.random.default_rng(8)
    pts, sd, w0 = _points(rng, D, N), rng.choice([0.125, 0.25, 0.5], size=D), rng.uniform(0.1, 1.0, size=N)
    w, delta, logl = _weights(rng, N), rng.standard_normal((D, N)) * 0.3, rng.uniform(-40.0, 0.0, size=N)

    def run(scale):
        # (a built source without a bandwidth search: the marginal over all dimensions of an uploaded density)
        src = kdehip.DeviceDensity(kdehip.kde(np.ldexp(pts, scale), np.ldexp(sd, scale), w0)).marginal(list(range(D)))
        moved = rf.refit_device(src, w, rf.WEIGHTS, np.ldexp(delta, scale))[0].download()
        upd, le, ess = src.bayes_update(logl)
        return rm.arrays_of(moved), rm.arrays_of(upd.download()), le, ess

    (m0, u0, le0, ess0), (m1, u1, le1, ess1) = run(0), run(k)
    assert np.float64(le0).tobytes() == np.float64(le1).tobytes() and np.float64(ess0).tobytes() == np.float64(ess1).tobytes()
    for base, scaled in ((m0, m1), (u0, u1)):
        for f in ("weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation"):
            assert base[f].tobytes() == scaled[f].tobytes(), f
        for f in ("centers", "ranges", "means"):
            assert np.ldexp(base[f], k).tobytes() == scaled[f].tobytes(), f
        for f in ("bandwidth", "bandwidthMin", "bandwidthMax"):
            assert np.ldexp(base[f], 2 * k).tobytes() == scaled[f].tobytes(), f


# ---- G9: one point -----------------------------------------------------------------------------------------------------------
def _all_dims(dd):
    """a BUILT twin of an uploaded density without a bandwidth search (as G8): its marginal over all dimensions"""
    return dd.marginal(list(range(dd.dims)))


def _same_consumers(res, host_refit, pos, manifold=None):
    """G3's checks of a result whose arrays cannot be downloaded (the source was uploaded): as an input of evaluate,
    evaluate_log and sample it gives the bits of the uploaded host refit"""
    with kdehip.DeviceDensity(host_refit) as up:
        kw = {} if manifold is None else dict(manifold=manifold)
        assert res.evaluate(pos, **kw).tobytes() == up.evaluate(pos, **kw).tobytes()
        assert res.evaluate_log(pos, **kw).tobytes() == up.evaluate_log(pos, **kw).tobytes()
        if res.num_points > 1:
            assert res.evaluate_log(lvFlag=True, **kw).tobytes() == up.evaluate_log(lvFlag=True, **kw).tobytes()
        (x1, l1), (x2, l2) = kdehip.sample(res, 300, seed=9), kdehip.sample(up, 300, seed=9)
        assert l1.tobytes() == l2.tobytes() and x1.tobytes() == x2.tobytes()


@pytest.mark.parametrize("source", ["built", "uploaded"])
@pytest.mark.parametrize("D", [1, 6])
def test_g9_a_density_of_one_point(D, source):
    """N = 1: the tree is its root with the one leaf as both children (the `left[0] != 2` case of ensure_table), no internal
    node of two children.  Id 1 is the root AND "slot N": the arrays of a moved built density once kept the source's box there
    (the copy that preserves the unused slot N of larger trees), which the comparison of `centers` after a move holds now."""
    rng = np.random.default_rng(900 + D)
    hp = kdehip.kde(_points(rng, D, 1), rng.uniform(0.2, 0.6, size=D))
    assert hp.bt.left_child[0] == 2
    w, delta, logl = np.array([0.75]), rng.standard_normal((D, 1)), np.array([-3.5])
    pos = _points(rng, D, 40)
    wants = [hp.changeWeights(w), hp.movePoints(delta), rf.refit_host(hp, new_weights=w, delta=delta)]
    hb, le_h, ess_h = hp.bayes_update(logl)
    with kdehip.DeviceDensity(hp) as up:
        dd = _all_dims(up) if source == "built" else up
        try:
            if source == "built":
                rm.same_bits(dd.download(), hp, "the built twin is the host density")
            gots = [dd.changeWeights(w), dd.movePoints(delta), rf.refit_device(dd, w, rf.WEIGHTS, delta)[0]]
            db, le, ess = dd.bayes_update(logl)
            assert abs(le - le_h) <= 1e-12 * max(1.0, abs(le_h)) and abs(ess - 1.0) <= 1e-12 and abs(ess_h - 1.0) <= 1e-12
            for got, want, what in zip(gots + [db], wants + [hb], ("weights", "delta", "both", "bayes")):
                if source == "built":
                    if what == "bayes":
                        _check_bayes(dd, hp, logl, got, le, ess)
                    else:
                        rm.same_bits(got.download(), want, what)
                    assert got.evaluate(pos).tobytes() == kdehip.evaluateDualTree(got.download(), pos).tobytes(), what
                else:
                    _same_consumers(got, want, pos)
                got.close()
        finally:
            if dd is not up:
                dd.close()


# ---- G10: a source with a bandwidth per point ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(2, 129), (6, 1025)])
def test_g10_a_per_point_bandwidth_source(D, N):
    """`kde_varbw` as H2 of the host test builds it, uploaded: the leaves keep their own variances through the copy, and the
    internal nodes' are recomputed from them"""
    rng = np.random.default_rng(11 * D + N)
    hp = kdehip.kde_varbw(_points(rng, D, N), rng.uniform(0.1, 0.9, size=(D, N)), rng.uniform(0.1, 1.0, size=N))
    assert hp.multibandwidth == 1
    w, delta = _weights(rng, N), rng.standard_normal((D, N)) * 0.2
    pos = _points(rng, D, 300)
    with kdehip.DeviceDensity(hp) as dd:
        with dd.changeWeights(w) as a:
            _same_consumers(a, hp.changeWeights(w), pos)
        with dd.movePoints(delta) as b:
            _same_consumers(b, hp.movePoints(delta), pos)
        with rf.refit_device(dd, w, rf.WEIGHTS, delta)[0] as ab:
            _same_consumers(ab, rf.refit_host(hp, new_weights=w, delta=delta), pos)


# ---- G11: a tree built with circular operators --------------------------------------------------------------------------------
TMAN = ["euclid", "circular"]


def _across_the_cut(N=200):
    """H3's data: one cluster of angles on both sides of the cut at +-pi, and moves that carry some of them across it"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(N)
    th = rm.PI - np.abs(rng.standard_normal(N)) * 0.2
    th[::2] = -rm.PI + np.abs(rng.standard_normal(N // 2)) * 0.2
    pts = np.stack([x, th])
    w0 = rng.uniform(0.1, 1.0, size=N)
    delta = np.stack([rng.standard_normal(N) * 0.1, rng.uniform(-0.5, 0.5, size=N)])
    assert (np.abs(th + delta[1]) > rm.PI).any() and (np.abs(th + delta[1]) < rm.PI).any()
    return pts, w0, delta, _weights(rng, N)


def test_g11_a_circular_tree_built_on_the_device():
    """the `circ_wrap` branch of leaf_kernel and the circular boxes of refit_node, against the host entry bit for bit"""
    pts, _, delta, w = _across_the_cut()
    N = pts.shape[1]
    d_pts = _dev(pts.T)
    _torch().cuda.synchronize()
    with kdehip.DeviceDensity.from_device_points(d_pts, 2, N, tree_manifold=TMAN) as dd:
        hp = dd.download()
        assert list(hp.tree_manifold) == [0, 1]
        assert (hp.bt.ranges[:(N - 1) * 2][1::2] < 1.0).all()   # the premise: the boxes of the angle are the short way round
        moved = dd.movePoints(delta)
        assert np.array_equal(moved.tree_manifold, dd.tree_manifold)
        want = hp.movePoints(delta)
        rm.same_bits(moved.download(), want, "delta")
        th = kdehip.getPoints(want)[1]
        assert (th >= -rm.PI).all() and (th < rm.PI).all()
        rm.same_bits(dd.changeWeights(w).download(), hp.changeWeights(w), "weights")
        rm.same_bits(rf.refit_device(dd, w, rf.WEIGHTS, delta)[0].download(), rf.refit_host(hp, new_weights=w, delta=delta), "both")
        rm.same_bits(dd.changeWeights(kdehip.getWeights(hp)).download(), hp, "the circular boxes are recomputed to the same bits")
        rm.same_bits(moved.movePoints(-delta).changeWeights(w).download(), want.movePoints(-delta).changeWeights(w), "a refit of a refit")
        # a batch mixes it with a Euclidean item of the same D: circular_mask differs per item
        flat, hflat = _built(2, 129)
        rng = np.random.default_rng(77)
        d2 = rng.standard_normal((2, 129)) * 3.0   # (moves beyond pi, which a Euclidean item must not wrap)
        out = kdehip.DeviceDensity.refit_batch([dict(density=dd, weights=w, delta=delta), dict(density=flat, delta=d2),
                                                dict(density=dd, delta=delta)])
        rm.same_bits(out[0][0].download(), rf.refit_host(hp, new_weights=w, delta=delta), "batch: circular")
        rm.same_bits(out[1][0].download(), hflat.movePoints(d2), "batch: Euclidean")
        rm.same_bits(out[2][0].download(), want, "batch: circular again")
        assert (np.abs(kdehip.getPoints(out[1][0].download())) > rm.PI).any()


def test_g11_a_circular_tree_uploaded():
    pts, w0, delta, w = _across_the_cut()
    hp = kdehip.kde(pts, [0.3, 0.2], w0, tree_manifold=TMAN)
    rng = np.random.default_rng(6)
    pos = np.stack([rng.standard_normal(300), rng.uniform(-rm.PI, rm.PI, size=300)])
    with kdehip.DeviceDensity(hp) as dd:
        for man in (None, TMAN):
            with dd.movePoints(delta) as a:
                assert np.array_equal(a.tree_manifold, hp.tree_manifold)
                _same_consumers(a, hp.movePoints(delta), pos, man)
            with dd.changeWeights(w) as b:
                _same_consumers(b, hp.changeWeights(w), pos, man)
            with rf.refit_device(dd, w, rf.WEIGHTS, delta)[0] as ab:
                _same_consumers(ab, rf.refit_host(hp, new_weights=w, delta=delta), pos, man)
        flat = _uploaded(2, 200)
        out = kdehip.DeviceDensity.refit_batch([dict(density=dd, delta=delta), dict(density=flat[0], delta=delta * 8.0)])
        _same_consumers(out[0][0], hp.movePoints(delta), pos, TMAN)
        _same_consumers(out[1][0], flat[1].movePoints(delta * 8.0), pos)


# ---- G12: more than 1024 chunks ---------------------------------------------------------------------------------------------------
def test_g12_the_fold_makes_a_second_trip_through_its_tile():
    """(1, 131201): 1026 chunks of 128 leaves, so fold_kernel stages 1024 chunk partials, adds them, and comes back for two"""
    D, N = 1, 131201
    assert (N + 127) // 128 == 1026
    dd, hp = _built(D, N)
    rng = np.random.default_rng(131201)
    logl = rng.uniform(-1000.0, 0.0, size=N) - 2000.0
    logl[1] = -np.inf
    res, le, ess = dd.bayes_update(_dev(logl))
    _check_bayes(dd, hp, logl, res, le, ess)
    w, delta = _weights(rng, N), rng.standard_normal((D, N)) * 0.3
    rm.same_bits(dd.changeWeights(w).download(), hp.changeWeights(w), "weights")
    rm.same_bits(dd.movePoints(delta).download(), hp.movePoints(delta), "delta")
