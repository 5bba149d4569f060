"""Circular dimensions in the summaries (include/kdehip.h section 5e) without a GPU: the model of
tests/summary_circular_model.py against the Euclidean formulas where nothing wraps, the straddling case that motivates the
feature, the host (numpy) path of `getKDEMean` / `getKDEfit` / `getKDERange` against the model, and the refusals that need
no device."""
import ctypes as C
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import f64p, ptr, u8p
from tests import summary_circular_model as M
from tests.pymodel import wrapRad


def _straddling(N=300, seed=0, D=1):
    rng = np.random.default_rng(seed)
    return M.wrap(math.pi + 0.2 * rng.standard_normal((D, N)))


def test_model_is_the_euclidean_formulas_when_no_offset_wraps():
    rng = np.random.default_rng(1)
    pts = rng.uniform(-1.2, 1.2, size=(3, 97))   # every offset and residual within (-pi, pi): wrap is the identity
    p = kdehip.kde(pts, [0.3])
    circ, eu = [1, 1, 1], [0, 0, 0]
    assert np.array_equal(M.wrap(pts), pts)
    # a0 + (mean of x - a0) is the Euclidean mean up to the rounding of the shifted sum
    assert np.allclose(M.mean(pts, circ), kdehip.getKDEMean(p), rtol=0, atol=1e-14)
    assert np.array_equal(M.mean(pts, eu), kdehip.getKDEMean(p))
    assert np.array_equal(M.krange(pts, eu, 0.1), kdehip.getKDERange(p, 0.1))
    assert np.allclose(M.krange(pts, circ, 0.1), kdehip.getKDERange(p, 0.1), rtol=0, atol=1e-14)
    mu, S = M.fit(pts, circ)
    _, S0 = kdehip.getKDEfit(p)
    assert np.allclose(S.astype(np.float64), S0, rtol=1e-12, atol=0)
    assert np.array_equal(M.grid(-1.5, 2.25, 200), kdehip.summary.grid(-1.5, 2.25, 200))
    assert np.array_equal(M.grid(0.0, 1.0, 2), [0.0, 1.0])


def test_straddling_mean_points_at_pi_not_at_zero():
    """angles wrap(pi + 0.2 randn), N = 300: the standard error of the mean is 0.2 / sqrt(300) = 0.012, so 0.05 is four of
    them; the Euclidean mean of two clusters at +-pi lands near 0 -- the opposite direction"""
    pts = _straddling()
    assert pts.min() < -3.0 and pts.max() > 3.0   # the set does straddle the cut
    p = kdehip.kde(pts, [0.1])
    mu = kdehip.getKDEMean(p, manifold=["circular"])
    assert np.array_equal(mu, M.mean(pts, [1]))
    assert -math.pi <= mu[0] < math.pi
    assert abs(wrapRad(mu[0] - math.pi)) < 0.05
    assert abs(kdehip.getKDEMean(p)[0]) < 0.5
    assert abs(M.mean(pts, [0])[0]) < 0.5
    # the fit sees a spread of 0.2, the Euclidean one a spread of about pi
    _, S = kdehip.getKDEfit(p, manifold=["circular"])
    assert abs(math.sqrt(S[0, 0]) - 0.2) < 0.03
    assert math.sqrt(kdehip.getKDEfit(p)[1][0, 0]) > 2.5
    # and the range hugs the cluster, unwrapped across the cut
    r = kdehip.getKDERange(p, 0.1, manifold=["circular"])
    assert np.array_equal(r, M.krange(pts, [1], 0.1))
    assert r[0, 1] - r[0, 0] < 2.0 and r[0, 0] < r[0, 1]
    assert kdehip.getKDERange(p, 0.1)[0, 1] - kdehip.getKDERange(p, 0.1)[0, 0] > 6.0


@pytest.mark.parametrize("kind", ["straddle", "shifted", "wide"])
def test_host_path_is_the_model(kind):
    rng = np.random.default_rng(5)
    N = 65
    pts = np.stack([_straddling(N, seed=2)[0], rng.standard_normal(N) * 2.0, M.wrap(-3.0 + 0.3 * rng.standard_normal(N))])
    if kind == "shifted":
        pts[0] += 4 * math.pi   # any representative works
    if kind == "wide":
        pts[2] = rng.uniform(-math.pi, math.pi, N)   # more than a half circle: the 2 pi clamp of the range
    man = [1, 0, 1]
    p = kdehip.kde(pts, [0.2, 0.5, 0.3])
    assert np.array_equal(kdehip.getPoints(p), pts)
    assert np.array_equal(kdehip.getKDEMean(p, manifold=man), M.mean(pts, man))
    for extend in (0.0, 0.1, 0.3):
        r = kdehip.getKDERange(p, extend, manifold=["circular", "euclid", "circular"])
        assert np.array_equal(r, M.krange(pts, man, extend))
        assert np.all((r[:, 1] - r[:, 0])[[0, 2]] <= 2 * math.pi + 1e-14)   # at most one turn
    if kind == "wide":
        r = kdehip.getKDERange(p, 0.3, manifold=man)
        assert abs((r[2, 1] - r[2, 0]) - 2 * math.pi) < 1e-14
    mu, S = kdehip.getKDEfit(p, manifold=man)
    mmu, mS = M.fit(pts, man)
    assert np.array_equal(mu, mmu)
    assert np.max(np.abs(S - mS)) <= 1e-12 * float(np.max(np.abs(mS)))
    # all-Euclidean and None are today's results
    assert np.array_equal(kdehip.getKDEMean(p, manifold=[0, 0, 0]), kdehip.getKDEMean(p))
    assert np.array_equal(kdehip.getKDERange(p, 0.1, manifold=None), kdehip.getKDERange(p, 0.1))
    p1 = kdehip.marginal(p, [0])
    assert np.array_equal(kdehip.getKDERangeLinspace(p1, 0.1, 7, manifold=[1]),
                          M.grid(*M.krange(pts[:1], [1], 0.1)[0], 7))


def test_marginal_builds_its_tree_with_the_selected_operators():
    pts = np.stack([_straddling(40, seed=3)[0], np.linspace(-1, 1, 40)])
    p = kdehip.kde(pts, [0.2, 0.4], tree_manifold=["circular", "euclid"])
    m = kdehip.marginal(p, [0], tree_manifold="inherit")
    want = kdehip.kde(pts[:1], kdehip.getBW(p)[[0], 0], kdehip.getWeights(p), tree_manifold=["circular"])
    assert np.array_equal(m.tree_manifold, [1])
    for k in ("centers", "ranges", "permutation"):
        assert np.array_equal(getattr(m.bt, k), getattr(want.bt, k)), k
    assert np.array_equal(m.means, want.means) and np.array_equal(m.bandwidth, want.bandwidth)
    assert kdehip.marginal(p, [1], tree_manifold="inherit").tree_manifold is None


def test_refusals_need_no_device():
    pts = _straddling(20, seed=4, D=2)
    p = kdehip.kde(pts, [0.2])
    for f in (kdehip.getKDEMean, kdehip.getKDEfit, kdehip.getKDERange, kdehip.getKDEMax):
        with pytest.raises(ValueError):
            f(p, manifold=[1])           # the wrong length
        with pytest.raises(ValueError):
            f(p, manifold=[1, 2])        # a byte above 1
    with pytest.raises(ValueError):
        kdehip.sample(p, 4, seed=1, manifold=[1, 0, 0])
    with pytest.raises(ValueError):
        kdehip.resample(p, 4, seed=1, tree_manifold=[3, 0])
    with pytest.raises(ValueError):
        kdehip.intersIntgAppxIS(p, p, 10, manifold=["circular"])
    with pytest.raises(ValueError):
        kdehip.marginal(p, [0], tree_manifold=[2, 0])
    # the library itself refuses a byte above 1 before it touches a device (device -1 would be the next error)
    bad = np.array([1, 2], dtype=np.uint8)
    out, ind = np.zeros(2), np.zeros(4, dtype=np.int64)
    cs = p._cstruct()
    calls = [
        lambda: _lib.lib.kdehip_kde_max_manifold(C.byref(cs), 10, ptr(out, f64p), None, 0, ptr(bad, u8p)),
        lambda: _lib.lib.kdehip_inters_intg_appx_is_manifold(C.byref(cs), C.byref(cs), 10, ptr(out, f64p), 0, ptr(bad, u8p)),
        lambda: _lib.lib.kdehip_sample_manifold(C.byref(cs), 2, C.c_uint64(1), 0, None, ptr(np.zeros(4), f64p),
                                                ptr(ind, _lib.i64p), 0, ptr(bad, u8p)),
    ]
    for call in calls:
        with pytest.raises(kdehip.KdeHipError) as e:
            _lib.check(call())
        assert e.value.code == _lib.ERR_ARG


def test_small_things():
    """gibbs1 with a manifold runs on one GPU: asking for more is an error, not a silent single-GPU run"""
    pts = np.random.default_rng(0).standard_normal((1, 8))
    t = kdehip.kde(pts, [0.3])
    with pytest.raises(ValueError):
        kdehip.gibbs1(2, [t, t], 4, 1, np.zeros(4), np.ones((2, 4), dtype=np.int64), np.zeros(64), np.zeros(64),
                      manifold=["circular"], ngpus=2)
