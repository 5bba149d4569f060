"""Circular dimensions in the summaries and in `marginal` on the GPU (csrc/summary.hip, csrc/pack_device.hip,
include/kdehip.h section 5e) against tests/summary_circular_model.py.

The mean and the range are specified operation by operation: bit for bit the model's.  The covariance and the grid values
take the tolerances of the Euclidean checks in tests/test_gpu_summary.py (1e-12 of the largest entry of a np.longdouble
covariance; 1e-12 relative per grid value).  The argmax is the model's grid point; every case asserts that the model's two
largest grid values are further apart than that tolerance, so that a tie cannot hide a wrong index.  Sizes: one point, two,
around the wavefront (63, 64, 65), more than one staged chunk of 256 (257, 300); grids of 2, 3, 200 and 257 (two blocks).
Data: angles straddling +-pi, the same plus 4 pi (any representative works), and angles over the whole circle (the 2 pi
clamp of the range; its two-point grid is one angle twice, so that case checks the values only).  One case has
N = 256 * 256 + 1, where a group of the grid kernel holds two chunks."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import f64p, ptr, u8p
from tests import summary_circular_model as M
from tests.helpers import assert_chunks_per_group

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 257, 300)
DS = (1, 2, 3, 6)
KINDS = ("straddle", "shifted", "wide")
GRIDS = (2, 3, 200, 257)
GRID_TOL = 1e-12     # tests/test_gpu_summary.py, the grid values
COV_TOL = 1e-12      # tests/test_gpu_summary.py, getKDEfit
SEPARATION = 1e-11   # the top two grid values of every argmax case differ by more than this (relative): above GRID_TOL

ARRAYS_BT = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
ARRAYS_BD = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")


def manifolds(D):
    """all-circular, mixed (every other dimension), all-Euclidean"""
    mixed = [(k + 1) % 2 for k in range(D)]
    return [[1] * D, mixed, [0] * D] if D > 1 else [[1], [0]]


@functools.lru_cache(maxsize=None)
def case(D, N, kind, man):
    """(host density, points (D, N), weights or None): circular dimensions hold angles of `kind`, the others a Gaussian"""
    rng = np.random.default_rng(1000 * D + 7 * N + 101 * KINDS.index(kind) + sum(man))
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 3.0, size=(D, 1)) + rng.uniform(-2, 2, size=(D, 1))
    for k in range(D):
        if not man[k]:
            continue
        if kind == "wide":
            # a bump on a background that spans 5.6 rad: with extend 0.1 the range laps and is cut to one turn, whose
            # midpoint is the bump (so that a coarse grid has its maximum inside, not at the two ends -- one angle)
            c = rng.uniform(-math.pi, math.pi)
            x = c + np.where(rng.random(N) < 0.7, 0.4 * rng.standard_normal(N), rng.uniform(-2.8, 2.8, N))
            if N >= 3:   # (point 1, the reference angle, sits in the bump: every offset stays within half a turn)
                x[0], x[1], x[2] = c + 0.1, c - 2.8, c + 2.8
            pts[k] = M.wrap(x)
        else:
            pts[k] = M.wrap(math.pi + 0.2 * rng.standard_normal(N)) + (4 * math.pi if kind == "shifted" else 0.0)
    w = rng.uniform(0.05, 1.0, size=N) if N % 2 == 0 else None   # (weights also break the symmetry of a two-point grid)
    p = kdehip.kde(pts, rng.uniform(0.1, 0.7, size=D), w)
    pts = kdehip.getPoints(p)
    pts.setflags(write=False)
    return p, pts, w


@functools.lru_cache(maxsize=None)
def resident(D, N, kind, man):
    return kdehip.DeviceDensity(case(D, N, kind, man)[0])


def full_turn_pair(x, circular):
    """a range cut to one turn starts and ends at the SAME angle: a grid of two points holds that angle twice, its two
    values are equal by periodicity whatever the seed -- such a dimension checks its values and has no argmax to tell
    apart"""
    return bool(circular) and len(x) == 2 and x[1] - x[0] > 2 * math.pi - 1e-9


def grid_model(D, N, kind, man, Ngrid):
    """the model's grids, values, argmax and the dimensions whose argmax is checked; asserts the separation of the top two
    values in each of those (a grid whose points all coincide -- one point, or equal points -- has one candidate only and
    needs none)"""
    p, pts, w = case(D, N, kind, man)
    var1 = p.bandwidth[N * D:N * D + D]   # the leaves share one bandwidth vector: original point 1's variances
    xs, vals = M.grid_values(pts, w, var1, man, Ngrid)
    checked = np.array([not full_turn_pair(xs[k], man[k]) for k in range(D)])
    for k in range(D):
        if np.all(xs[k] == xs[k][0]) or not checked[k]:
            continue
        gap = float(M.top_two_gap(vals[k:k + 1])[0])
        assert gap > SEPARATION, (D, N, kind, man, Ngrid, k, gap)
    return xs, vals, M.argmax(xs, vals, man), checked


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_mean_and_range_are_the_model_bit_for_bit_and_the_covariance_to_tolerance(D, N):
    for kind in KINDS:
        for man in manifolds(D):
            man_t = tuple(man)
            p, pts, _ = case(D, N, kind, man_t)
            dp = resident(D, N, kind, man_t)
            assert np.array_equal(kdehip.getKDEMean(dp, manifold=man), M.mean(pts, man)), (kind, man)
            for extend in (0.0, 0.1, 0.3, 1.7):
                got = kdehip.getKDERange(dp, extend, manifold=man)
                assert np.array_equal(got, M.krange(pts, man, extend)), (kind, man, extend)
            mu, S = kdehip.getKDEfit(dp, manifold=man)
            mmu, mS = M.fit(pts, man)
            assert np.array_equal(mu, mmu)
            assert np.max(np.abs(S - mS)) <= COV_TOL * max(float(np.max(np.abs(mS))), 1e-300), (kind, man)
            assert np.array_equal(S, S.T)
            if any(man):
                circ = np.array(man, dtype=bool)
                assert np.all((mu[circ] >= -math.pi) & (mu[circ] < math.pi))
                r = kdehip.getKDERange(dp, 1.7, manifold=man)
                assert np.all((r[circ, 1] - r[circ, 0]) <= 2 * math.pi + 1e-14)
                # the host (numpy) path of the same call
                assert np.array_equal(kdehip.getKDEMean(p, manifold=man), mu)
                assert np.array_equal(kdehip.getKDERange(p, 0.1, manifold=man), kdehip.getKDERange(dp, 0.1, manifold=man))


def test_straddling_heading_belief():
    """the case of the issue: a heading belief around +-pi has its circular mean there and its Euclidean mean near 0"""
    rng = np.random.default_rng(0)
    pts = np.stack([rng.standard_normal(300), rng.standard_normal(300), M.wrap(math.pi + 0.2 * rng.standard_normal(300))])
    dp = kdehip.DeviceDensity(kdehip.kde(pts, [0.3, 0.3, 0.1]))
    dp.manifold = np.array([0, 0, 1], dtype=np.uint8)
    mu = kdehip.getKDEMean(dp, manifold="inherit")
    assert abs(M.wrap(mu[2] - math.pi)) < 0.05
    assert abs(kdehip.getKDEMean(dp)[2]) < 0.5
    mx = kdehip.getKDEMax(dp, manifold=["euclid", "euclid", "circular"])
    assert abs(M.wrap(mx[2] - math.pi)) < 0.2
    assert np.array_equal(dp.getKDEMean(manifold="inherit"), mu) and np.array_equal(dp.getKDEfit(manifold="inherit")[0], mu)


GRID_CASES = [(1, 1), (1, 2), (1, 65), (2, 63), (2, 257), (3, 64), (3, 300), (6, 2), (6, 65), (6, 300)]


@pytest.mark.parametrize("D,N", GRID_CASES)
@pytest.mark.parametrize("Ngrid", GRIDS)
def test_grid_values_and_argmax(D, N, Ngrid):
    for kind in KINDS:
        for man in manifolds(D)[:2]:
            man_t = tuple(man)
            xs, vals, amax, checked = grid_model(D, N, kind, man_t, Ngrid)
            p, _, _ = case(D, N, kind, man_t)
            dp = resident(D, N, kind, man_t)
            m, got = kdehip.getKDEMax(dp, Ngrid, values=True, manifold=man)
            err = np.abs(got.astype(np.longdouble) - vals)
            assert np.all(err <= GRID_TOL * vals), (kind, man, float(np.max(err / vals)))
            assert np.array_equal(m[checked], amax[checked]), (kind, man)
            # the host entry (the density uploaded for the call) gives the same bits
            hm, hv = kdehip.getKDEMax(p, Ngrid, values=True, manifold=man)
            assert np.array_equal(hm, m) and np.array_equal(hv, got)
            if kind == "wide" and N >= 3 and Ngrid == 200:   # the case does exercise the cut to one turn
                circ = np.array(man, dtype=bool)
                assert np.all(np.abs((xs[circ, -1] - xs[circ, 0]) - 2 * math.pi) < 1e-12)


def test_grid_values_with_groups_of_two_chunks():
    """grid_partial_kernel<true> where a group of its own split (256-leaf chunks, at most 256 groups) holds two chunks:
    N = 256 * 256 + 1, 257 chunks, the ring's second buffer and `total += sum` over chunks; the last group is one leaf"""
    D, N, kind, man, Ngrid = 1, 256 * 256 + 1, "straddle", (1,), 3
    assert_chunks_per_group(N, Ngrid, 2, grid=True)
    xs, vals, amax, checked = grid_model(D, N, kind, man, Ngrid)
    p, _, _ = case(D, N, kind, man)
    with kdehip.DeviceDensity(p) as dp:
        m, got = kdehip.getKDEMax(dp, Ngrid, values=True, manifold=list(man))
    err = np.abs(got.astype(np.longdouble) - vals)
    print("largest |value - model| / model:", float(np.max(err / vals)))
    assert np.all(err <= GRID_TOL * vals), float(np.max(err / vals))
    assert np.array_equal(m[checked], amax[checked])
    hm, hv = kdehip.getKDEMax(p, Ngrid, values=True, manifold=list(man))  # the host entry gives the same bits
    assert np.array_equal(hm, m) and np.array_equal(hv, got)


def _summary_all(dp, Ngrid, extend, manifold_bytes):
    """every output of kdehip_density_summary_manifold with the given bytes (None = the entry without a manifold)"""
    D = dp.dims
    bufs = [np.full(s, np.nan) for s in ((2 * D,), (D,), (D * D,), (D,), (D * Ngrid,))]
    ext = C.c_double(extend)
    args = [dp._h, C.byref(ext), Ngrid] + [ptr(b, f64p) for b in bufs]
    if manifold_bytes is None:
        _lib.check(_lib.lib.kdehip_density_summary(*args))
    else:
        _lib.check(_lib.lib.kdehip_density_summary_manifold(*args, ptr(manifold_bytes, u8p)))
    return bufs


@pytest.mark.parametrize("D,N", [(1, 65), (3, 300), (6, 257)])
def test_no_manifold_and_all_euclidean_are_the_existing_entry(D, N):
    man_t = tuple([1] * D)
    dp = resident(D, N, "straddle", man_t)
    p = case(D, N, "straddle", man_t)[0]
    for Ngrid, extend in ((2, 0.1), (257, 0.3)):
        want = _summary_all(dp, Ngrid, extend, None)
        for got in (_summary_all(dp, Ngrid, extend, np.zeros(D, dtype=np.uint8)),):
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes()
    zeros = [0] * D
    assert np.array_equal(kdehip.getKDEMax(dp, 200, manifold=zeros), kdehip.getKDEMax(dp, 200))
    assert np.array_equal(kdehip.getKDEMax(p, 200, manifold=zeros), kdehip.getKDEMax(p, 200))
    assert np.array_equal(kdehip.getKDEMean(dp, manifold=None), kdehip.getKDEMean(dp))
    if D <= 2:
        assert kdehip.intersIntgAppxIS(dp, dp, 50, manifold=zeros) == kdehip.intersIntgAppxIS(dp, dp, 50)
    bad = np.array([2] + [0] * (D - 1), dtype=np.uint8)
    with pytest.raises(kdehip.KdeHipError) as e:
        _summary_all(dp, 10, 0.1, bad)
    assert e.value.code == _lib.ERR_ARG


def test_batch_mixing_euclidean_and_circular_items_equals_the_single_calls():
    import torch
    dev = torch.device("cuda", 0)
    cases = [(1, 65, "straddle", (1,), 0.1, 200), (3, 300, "wide", (1, 0, 1), 0.1, 257), (6, 257, "straddle", (0,) * 6, 0.3, 3),
             (2, 2, "shifted", (1, 1), 0.0, 2), (3, 64, "straddle", (0, 0, 0), 0.1, 200), (6, 300, "shifted", (1,) * 6, 1.7, 200),
             (2, 63, "wide", (0, 1), 0.1, 257)]
    items, outs = [], []
    for D, N, kind, man, extend, Ng in cases:
        o = {"range": torch.full((2 * D,), np.nan, dtype=torch.float64, device=dev),
             "mean": torch.full((D,), np.nan, dtype=torch.float64, device=dev),
             "cov": torch.full((D * D,), np.nan, dtype=torch.float64, device=dev),
             "argmax": torch.full((D,), np.nan, dtype=torch.float64, device=dev),
             "values": torch.full((D * Ng,), np.nan, dtype=torch.float64, device=dev)}
        outs.append(o)
        items.append({"density": resident(D, N, kind, man), "extend": extend, "Ngrid": Ng, **o})
    st = torch.cuda.current_stream(dev)
    kdehip.summary_device_batch(items, stream=st.cuda_stream, manifold=[list(c[3]) for c in cases])
    st.synchronize()
    for (D, N, kind, man, extend, Ng), o in zip(cases, outs):
        mb = np.array(man, dtype=np.uint8)
        single = kdehip.summary._summary(resident(D, N, kind, man), extend=extend, N=Ng, range_=True, mean=True, cov=True,
                                         argmax=True, values=True, man=mb if mb.any() else None)
        for name, t in o.items():
            want = single[name]
            want = want.T.ravel() if name == "range" else want.ravel()  # (device layout: D x 2 column-major)
            assert t.cpu().numpy().tobytes() == want.tobytes(), (D, N, kind, name)
    # one manifold for all items, and an item's own `manifold` key
    D, N, kind, man, extend, Ng = cases[1]
    a = torch.full((D,), np.nan, dtype=torch.float64, device=dev)
    b = torch.full((D,), np.nan, dtype=torch.float64, device=dev)
    kdehip.summary_device_batch([{"density": resident(D, N, kind, man), "mean": a}], stream=st.cuda_stream,
                                manifold=["circular", "euclid", "circular"])
    kdehip.summary_device_batch([{"density": resident(D, N, kind, man), "mean": b, "manifold": list(man)}],
                                stream=st.cuda_stream)
    st.synchronize()
    want = kdehip.getKDEMean(resident(D, N, kind, man), manifold=list(man))
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    # a circular bit at or above the item's dimensions is refused
    arr = (_lib.CSummaryManifoldItem * 1)()
    arr[0].item.density, arr[0].item.Ngrid, arr[0].circular_mask = resident(D, N, kind, man)._h, 10, 1 << D
    with pytest.raises(kdehip.KdeHipError) as e:
        _lib.check(_lib.lib.kdehip_summary_device_batch_manifold(1, arr, None))
    assert e.value.code == _lib.ERR_ARG


@pytest.mark.parametrize("D,Np,Nq,Ngrid,kind", [(1, 65, 300, 201, "straddle"), (1, 300, 63, 257, "shifted"),
                                                (1, 257, 64, 200, "wide"), (2, 64, 257, 64, "straddle"),
                                                (2, 63, 65, 33, "wide")])
def test_inters_on_the_circle(D, Np, Nq, Ngrid, kind):
    for man in manifolds(D)[:2]:
        man_t = tuple(man)
        p, pts, _ = case(D, Np, kind, man_t)
        q, _, _ = case(D, Nq, "straddle", man_t)
        want = M.inters(pts, man, Ngrid, lambda pos: kdehip.evaluateDualTree(p, pos, manifold=man),
                        lambda pos: kdehip.evaluateDualTree(q, pos, manifold=man))
        a = kdehip.intersIntgAppxIS(p, q, Ngrid, manifold=man)
        assert abs(a - want) <= 1e-12 * abs(want), (man, a, want)   # tests/test_gpu_summary.py's tolerance
        b = kdehip.intersIntgAppxIS(resident(D, Np, kind, man_t), resident(D, Nq, "straddle", man_t), Ngrid, manifold=man)
        assert a == b


def _same_density(a, b):
    for k in ARRAYS_BT:
        assert np.array_equal(getattr(a.bt, k), getattr(b.bt, k)), k
    for k in ARRAYS_BD:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_marginal_with_a_circular_tree():
    man = (1, 0, 1)
    p, pts, w = case(3, 300, "straddle", man)
    dp = resident(3, 300, "straddle", man)
    tm = ["circular", "euclid", "circular"]
    for dims in ([0], [1], [2, 0], [1, 2], [0, 2, 1, 0]):
        sub = [tm[d] for d in dims]
        dm = dp.marginal(dims, manifold=tm, tree_manifold=tm)
        hm = kdehip.kde(pts[dims, :], kdehip.getBW(p)[dims, 0], kdehip.getWeights(p), tree_manifold=sub)
        _same_density(dm.download(), hm)
        _same_density(kdehip.marginal(p, dims, tree_manifold=tm), hm)
        want = np.array([1 if s == "circular" else 0 for s in sub], dtype=np.uint8)
        if want.any():
            assert np.array_equal(dm.manifold, want) and np.array_equal(dm.tree_manifold, want)
            # "inherit" picks the record up
            assert np.array_equal(kdehip.getKDEMean(dm, manifold="inherit"), kdehip.getKDEMean(dm, manifold=list(want)))
            again = dm.marginal([0], tree_manifold="inherit")
            _same_density(again.download(), kdehip.marginal(hm, [0], tree_manifold=list(want)))
        else:
            assert dm.manifold is None and dm.tree_manifold is None
    # without the keyword: the existing entry's arrays
    _same_density(dp.marginal([2, 0]).download(), kdehip.marginal(p, [2, 0]))
    with pytest.raises(ValueError):
        dp.marginal([0], tree_manifold=[1, 0])
