"""Joint bandwidth selection on the GPU (csrc/bwjoint.hip, include/kdehip.h section 5q): `joint_bandwidth`, `kde_joint`,
`DeviceDensity.joint_bandwidth` and `joint_bandwidth_device_batch` against tests/bwjoint_model.py (fp64, exactly rounded sums
over the points), and against each other bit for bit.

Tolerances, none of them taken from the code under test:
  bandwidth  relative 1e-9 per iterate: the bound the project holds its LOOCV bandwidths to against the oracle
  logl, trace  1e-9 * max(1, |L|) against the model; 1e-12 * max(1, |L|) against `evalAvgLogL(p', p', log_domain=True)`, the
             bound tests/test_gpu_logdensity.py holds that quantity to against its model
  monotone   1e-12 * max(1, |L|): the rounding of two sums of N terms of size |L|
The sizes: 129 and 257 leave a second chunk / a second query block with one leaf, 300 and 700 give two to three finish
blocks, every fifth weight is 0 (weightless leaves as sources and as queries), and N = 8193 is where a group of the sweep
walks two chunks and the carried sums are rescaled."""
import ctypes as C
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import bwjoint_model as bm
from tests.helpers import chunks_per_group

pytestmark = pytest.mark.gpu

SHAPES = [(1, 129), (2, 257), (3, 300), (6, 300), (8, 130), (2, 700)]
_CASES = {}


def _case(D, N):
    """a weighted density of one shape at a Silverman-style bandwidth, and the model's view of it (the density's own points
    and normalised weights): built once, shared, never changed"""
    if (D, N) not in _CASES:
        pts, w = bm.two_clusters(D, N)
        start = bm.silverman(pts)
        p = kdehip.kde(pts, start, w)
        _CASES[(D, N)] = dict(p=p, pts=pts, w=w, start=start, dens=(kdehip.getPoints(p), kdehip.getWeights(p), None), model={})
    return _CASES[(D, N)]


def _model(c, maxiter):
    if maxiter not in c["model"]:
        c["model"][maxiter] = bm.iterate(c["dens"], c["start"], 0.0, maxiter)
    return c["model"][maxiter]


def _close_bw(got, want):
    rel = np.abs(got - want) / want
    print(f"bandwidth: max relative difference {rel.max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(rel <= 1e-9), float(rel.max())


def _close_logl(got, want, rel=1e-9):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"log-likelihood: max scaled difference {err.max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= rel), float(err.max())


def _check_against_model(c, maxiter):
    bw, info = kdehip.joint_bandwidth(c["p"], c["start"], tol=0.0, maxiter=maxiter, return_info=True)
    wbw, wlogl, witers, wstatus, wtrace = _model(c, maxiter)
    assert witers == -maxiter and wstatus == 0
    assert info["iters"] == -maxiter and info["status"] == 0
    assert info["trace"].shape == (maxiter + 1,) and info["trace"][-1] == info["logl"]
    _close_bw(bw, wbw)
    _close_logl(info["trace"], wtrace)
    _close_logl(info["logl"], wlogl)
    return bw, info


# ---- 1. every iterate against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("maxiter", [1, 5])
@pytest.mark.parametrize("D,N", SHAPES)
def test_iterates_equal_the_model(D, N, maxiter):
    _check_against_model(_case(D, N), maxiter)


def test_several_chunks_a_group():
    """N = 8193: the 65 chunks go to 33 groups of two (one of one), so the carried t_k are rescaled between chunks"""
    assert chunks_per_group(8193, 8193) == 2
    _check_against_model(_case(2, 8193), 1)


def test_the_start_with_no_steps():
    c = _case(3, 300)
    bw, info = kdehip.joint_bandwidth(c["p"], c["start"], tol=0.0, maxiter=0, return_info=True)
    assert np.array_equal(bw, c["start"]) and info["iters"] == 0 and info["status"] == 0 and info["trace"].shape == (1,)
    _close_logl(info["logl"], bm.loo_logl(c["dens"], c["start"]))
    own, oinfo = kdehip.joint_bandwidth(c["p"], None, tol=0.0, maxiter=0, return_info=True)  # the density's own bandwidth
    assert np.array_equal(own, kdehip.getBW(c["p"])[:, 0]) and oinfo["logl"] == info["logl"]


# ---- 2. a case whose answer is known ------------------------------------------------------------------------------------
def test_two_points_give_their_differences_exactly():
    p = kdehip.kde(np.array([[0.0, 3.0], [0.0, 4.0]]), [1.0, 1.0])
    bw, info = kdehip.joint_bandwidth(p, return_info=True)
    assert bw.tolist() == [3.0, 4.0] and info["iters"] == 2 and info["status"] == 0
    assert abs(info["logl"] - (-1.0 - math.log(2.0 * math.pi * 12.0))) <= 1e-12
    assert info["trace"].shape == (3,) and info["trace"][1] == info["trace"][2] == info["logl"]


# ---- 3. monotone, and consistent with evalAvgLogL -----------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(3, 300), (6, 300)])
def test_the_trace_never_decreases_and_logl_is_evalAvgLogL(D, N):
    c = _case(D, N)
    bw, info = kdehip.joint_bandwidth(c["p"], c["start"], tol=1e-3, maxiter=200, return_info=True)
    L = info["logl"]
    assert 0 < info["iters"] <= 200 and info["status"] == 0 and info["trace"].shape == (info["iters"] + 1,)
    steps = np.diff(info["trace"])
    print(f"{info['iters']} sweeps, L {info['trace'][0]:.6f} -> {L:.6f}, smallest step {steps.min():.3e}")
    assert np.all(steps >= -1e-12 * max(1.0, abs(L))), float(steps.min())
    q = kdehip.kde(c["pts"], bw, c["w"])
    _close_logl(L, kdehip.evalAvgLogL(q, q, log_domain=True), rel=1e-12)


# ---- 4. the improvement over kde!(points) -------------------------------------------------------------------------------
def _loo(p):
    return kdehip.evalAvgLogL(p, p, log_domain=True)


def test_kde_joint_improves_on_the_marginal_bandwidth_in_six_dimensions():
    pts = bm.improvement_data()
    marginal, joint = _loo(kdehip.kde(pts)), _loo(kdehip.kde_joint(pts))
    print(f"6-D, N = 300: leave-one-out log-likelihood {marginal:.4f} (kde!(points)) -> {joint:.4f} (kde_joint)")
    assert joint >= marginal + 1.0


def test_kde_joint_is_never_below_the_marginal_bandwidth():
    pts = _case(2, 257)["pts"]
    marginal, joint = _loo(kdehip.kde(pts)), _loo(kdehip.kde_joint(pts))
    print(f"2-D, N = 257: leave-one-out log-likelihood {marginal:.6f} (kde!(points)) -> {joint:.6f} (kde_joint)")
    assert joint >= marginal


# ---- 5. the same bits by every route ------------------------------------------------------------------------------------
def _same(a, b):
    return (np.array_equal(a[0], b[0]) and a[1]["logl"] == b[1]["logl"] and a[1]["iters"] == b[1]["iters"]
            and a[1]["status"] == b[1]["status"])


def test_host_resident_and_batch_give_the_same_bits():
    cases = [_case(3, 300), _case(1, 129), _case(6, 300)]
    kw = dict(tol=1e-3, maxiter=60)
    host = [kdehip.joint_bandwidth(c["p"], c["start"], return_info=True, **kw) for c in cases]
    again = kdehip.joint_bandwidth(cases[0]["p"], cases[0]["start"], return_info=True, **kw)
    assert _same(again, host[0]) and np.array_equal(again[1]["trace"], host[0][1]["trace"])   # run after run
    devs = [kdehip.DeviceDensity(c["p"]) for c in cases]
    try:
        for c, d, h in zip(cases, devs, host):
            res = d.joint_bandwidth(c["start"], return_info=True, **kw)
            assert _same(res, h) and np.array_equal(res[1]["trace"], h[1]["trace"])
        batch = kdehip.joint_bandwidth_device_batch([dict(density=d, start=c["start"]) for c, d in zip(cases, devs)], **kw)
        assert len(batch) == 3
        for b, h in zip(batch, host):     # items that converge at different sweeps share the launches
            assert _same(b, h)
        assert len({h[1]["iters"] for h in host}) > 1
        # ... and from the density's own bandwidth
        own = kdehip.joint_bandwidth(cases[0]["p"], return_info=True, **kw)
        assert _same(devs[0].joint_bandwidth(return_info=True, **kw), own)
        assert _same(kdehip.joint_bandwidth_device_batch([dict(density=devs[0])], **kw)[0], own)
    finally:
        for d in devs:
            d.close()


# ---- 6. circular ----------------------------------------------------------------------------------------------------------
def test_an_angle_cluster_across_the_cut_of_the_circle():
    """bm.angle_data: one point of the cluster lies across the cut -- on the line it is 2 pi from every other point, which
    keeps the angle's bandwidth above (2 pi) / sqrt(N) = 1.1 (tests/test_bwjoint_host.py checks that premise on the model)"""
    man = ["euclid", "circular"]
    start = [0.5, 0.5]
    p = kdehip.kde(bm.angle_data(), start)
    bw, info = kdehip.joint_bandwidth(p, manifold=man, return_info=True)
    assert info["status"] == 0 and info["iters"] > 0 and bw[1] < 0.2
    line = kdehip.joint_bandwidth(p)
    print(f"the angle's bandwidth: {bw[1]:.4f} on the circle, {line[1]:.4f} on the line")
    assert line[1] > 1.0
    shifted = kdehip.joint_bandwidth(kdehip.kde(bm.angle_data(shift=2.0 * math.pi), start), manifold=man)
    assert np.all(np.abs(shifted - bw) <= 1e-12), np.abs(shifted - bw)
    _close_bw(bw, bm.iterate((kdehip.getPoints(p), kdehip.getWeights(p), None), start, 1e-3, 200, [0, 1])[0])


def test_circular_data_in_which_nothing_wraps_gives_the_euclidean_bits():
    c = _case(2, 257)
    pts = c["pts"] / np.abs(c["pts"]).max() * 1.5            # every difference inside [-pi, pi)
    p = kdehip.kde(pts, bm.silverman(pts), c["w"])
    e = kdehip.joint_bandwidth(p, tol=1e-3, maxiter=40, return_info=True)
    for man in ([1, 1], [0, 1]):
        assert _same(kdehip.joint_bandwidth(p, tol=1e-3, maxiter=40, manifold=man, return_info=True), e)


# ---- 7. degenerate data ---------------------------------------------------------------------------------------------------
def test_a_constant_dimension_freezes_the_iteration_at_the_start():
    pts = _case(2, 257)["pts"].copy()
    pts[1] = 0.75
    start = np.array([0.3, 0.2])
    p = kdehip.kde(pts, start)
    bw, info = kdehip.joint_bandwidth(p, start, return_info=True)
    assert info["status"] == 1 and info["iters"] == 0 and np.array_equal(bw, start)
    assert np.isfinite(info["logl"]) and info["trace"].tolist() == [info["logl"]]
    with kdehip.DeviceDensity(p) as d:
        assert _same(d.joint_bandwidth(start, return_info=True), (bw, info))


def test_one_weighted_point_has_no_neighbour():
    pts = _case(2, 257)["pts"]
    w = np.zeros(257)
    w[7] = 1.0
    start = np.array([0.3, 0.2])
    bw, info = kdehip.joint_bandwidth(kdehip.kde(pts, start, w), start, return_info=True)
    assert info["status"] == 1 and info["iters"] == 0 and info["logl"] == -math.inf and np.array_equal(bw, start)


# ---- 8. the refusals that read a handle -----------------------------------------------------------------------------------
def test_resident_arguments_are_refused_before_the_device_is_used():
    rng = np.random.default_rng(32)
    p = kdehip.kde(rng.standard_normal((2, 130)), [0.3])
    q = kdehip.kde(rng.standard_normal((2, 130)), [0.3])
    q.bandwidth[(130 + 3) * 2] *= 2.0  # leaf 3 gets a bandwidth of its own
    L = _lib.lib
    tol = C.byref(C.c_double(1e-3))
    out = [np.zeros(8), np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]
    o = (_lib.ptr(out[0], _lib.f64p), _lib.ptr(out[1], _lib.f64p), _lib.ptr(out[2], _lib.i32p), _lib.ptr(out[3], _lib.i32p))
    bad = np.array([0, 2], dtype=np.uint8)
    neg = np.array([0.3, -1.0])
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert L.kdehip_bandwidth_joint_device(dq._h, None, tol, 5, *o, None, None) == _lib.ERR_UNSUPPORTED
        assert "per-point" in L.kdehip_last_error().decode()
        assert L.kdehip_bandwidth_joint_device(dp._h, None, tol, 5, *o, None, _lib.ptr(bad, _lib.u8p)) == _lib.ERR_ARG
        assert L.kdehip_bandwidth_joint_device(dp._h, _lib.ptr(neg, _lib.f64p), tol, 5, *o, None, None) == _lib.ERR_ARG
        assert L.kdehip_bandwidth_joint_device(dp._h, None, tol, 5, None, *o[1:], None, None) == _lib.ERR_ARG
        items = (_lib.CBwJointItem * 2)()
        for k in range(2):
            items[k].bd = dp._h
            items[k].bw_out, items[k].logl, items[k].iters, items[k].status = o
        items[1].circular_mask = 1 << 2  # a dimension the density does not have
        assert L.kdehip_bandwidth_joint_device_batch(2, items, tol, 5) == _lib.ERR_ARG
        assert "circular_mask" in L.kdehip_last_error().decode()
        items[1].circular_mask = 0
        items[1].bd = dq._h
        assert L.kdehip_bandwidth_joint_device_batch(2, items, tol, 5) == _lib.ERR_UNSUPPORTED
        items[1].bd = dp._h
        items[1].logl = None
        assert L.kdehip_bandwidth_joint_device_batch(2, items, tol, 5) == _lib.ERR_ARG
        with pytest.raises(kdehip.KdeHipError) as e:
            dq.joint_bandwidth()
        assert e.value.code == _lib.ERR_UNSUPPORTED
