"""`marginal`, `getKDERange`, `getKDEMean`, `getKDEfit`, `getKDEMax` and `intersIntgAppxIS` on the GPU (csrc/summary.hip,
include/kdehip.h section 5c).

Resident ranges and means are held bit for bit to the host's numpy (itself held to sequential models in
tests/test_summary_host.py); the covariance to a np.longdouble model.  getKDEMax's grid values to 1e-12 relative of a
np.longdouble model of the marginal density, its argmax to the host composition marginal -> evaluateDualTree on the grid ->
first argmax.  The device marginal to the host marginal in all twelve arrays.  intersIntgAppxIS to a math.fsum model on
evaluateDualTree's values, and to the reference's own statistical bounds (test/runtests.jl:203-224)."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip.summary import grid
from tests.helpers import assert_chunks_per_group

pytestmark = pytest.mark.gpu

ARRAYS_BT = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
ARRAYS_BD = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")


def _density(D, N, seed, weighted=False):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 3.0, size=(D, 1)) + rng.uniform(-2, 2, size=(D, 1))
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    return kdehip.kde(pts, rng.uniform(0.1, 0.7, size=D), w)


def _same_density(a, b):
    for k in ARRAYS_BT:
        assert np.array_equal(getattr(a.bt, k), getattr(b.bt, k)), k
    for k in ARRAYS_BD:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


SHAPES = [(D, N) for D in (1, 2, 3, 6, 8) for N in (1, 2, 100, 2048, 5000)]


@pytest.mark.parametrize("D,N", SHAPES)
def test_resident_range_mean_fit_match_the_host(D, N):
    for weighted in (False, True):
        p = _density(D, N, seed=3 * D + N, weighted=weighted)
        dp = kdehip.DeviceDensity(p)
        for extend in (0.1, 0.0, 0.3, 1.7):
            assert np.array_equal(kdehip.getKDERange(dp, extend), kdehip.getKDERange(p, extend))
        assert np.array_equal(kdehip.getKDEMean(dp), kdehip.getKDEMean(p))
        mu, S = kdehip.getKDEfit(dp)
        assert np.array_equal(mu, kdehip.getKDEMean(p))
        X = kdehip.getPoints(p).astype(np.longdouble)
        Xc = X - X.mean(axis=1, keepdims=True)
        want = (Xc @ Xc.T) / N
        assert np.max(np.abs(S - want)) <= 1e-12 * max(float(np.max(np.abs(want))), 1e-300)


def test_resident_range_of_several_densities():
    ps = [_density(2, N, seed=s) for s, N in ((1, 50), (2, 7), (3, 300))]
    dps = [kdehip.DeviceDensity(p) for p in ps]
    assert np.array_equal(kdehip.getKDERange(dps, 0.25), kdehip.getKDERange(ps, 0.25))


def _marginal_model(p, i, x):
    """the 1-D marginal over [i] at the points x, in np.longdouble: the marginal's own weights and fl(sqrt(v))**2"""
    m = kdehip.marginal(p, [i])
    N = m.bt.num_points
    mu = m.means[N:].astype(np.longdouble)
    w = m.bt.weights[N:].astype(np.longdouble)
    v = np.longdouble(m.bandwidth[N])
    d = np.asarray(x, dtype=np.longdouble)[:, None] - mu[None, :]
    return (np.exp(-d * d / (2 * v)) * w[None, :]).sum(axis=1) / np.sqrt(2 * np.longdouble(np.pi) * v), m


@pytest.mark.parametrize("D,N,weighted", [(1, 100, False), (2, 257, True), (3, 2048, False), (6, 300, True), (8, 40, False)])
@pytest.mark.parametrize("Ngrid", [2, 200, 1000])
def test_kde_max_matches_the_model_and_the_composition(D, N, weighted, Ngrid):
    p = _density(D, N, seed=D * 1000 + N + Ngrid, weighted=weighted)
    m, vals = kdehip.getKDEMax(p, Ngrid, values=True)
    assert m.shape == (D,) and vals.shape == (D, Ngrid)
    for i in range(D):
        mi = kdehip.marginal(p, [i])
        lo, hi = kdehip.getKDERange(mi, 0.1)[0]
        x = grid(lo, hi, Ngrid)
        model, _ = _marginal_model(p, i, x)
        err = np.abs(vals[i].astype(np.longdouble) - model)
        assert np.all(err <= 1e-12 * model), float(np.max(err / model))
        y = kdehip.evaluateDualTree(mi, x[None, :])
        k = int(np.argmax(y))
        got = int(np.flatnonzero(x == m[i])[0])
        if got != k:  # only a near tie of the top two values may pick the other one
            assert abs(y[got] - y[k]) <= 1e-11 * y[k], (i, got, k)
    # the resident entry gives the same bits
    dm, dvals = kdehip.DeviceDensity(p).getKDEMax(Ngrid, values=True)
    assert np.array_equal(dm, m) and np.array_equal(dvals, vals)


# Groups of SEVERAL chunks in grid_partial_kernel (its own ring and split: 256-leaf chunks, at most 256 groups, which a grid of
# up to a few thousand points all gets on the 256 CUs of an MI355X): a group holds more than one chunk only when N > 256 * 256.
#   N = 256 * 256 + 1: 257 chunks, 2 per group, the last group ONE chunk of ONE leaf: the ring's second buffer, total += sum
#   N = 512 * 256 + 1: 513 chunks, 3 per group: a buffer staged a second time
# Small grids (2 points, and 257: a second grid block with one live lane) keep the np.longdouble model at a second or two;
# the model is summed in blocks of grid points, never as an Ngrid x N array.
def _marginal_model_blocked(p, i, x, rows=16):
    """_marginal_model for a large density"""
    m = kdehip.marginal(p, [i])
    N = m.bt.num_points
    mu = m.means[N:].astype(np.longdouble)
    w = m.bt.weights[N:].astype(np.longdouble)
    v = np.longdouble(m.bandwidth[N])
    x = np.asarray(x, dtype=np.longdouble)
    out = np.zeros(len(x), dtype=np.longdouble)
    for r in range(0, len(x), rows):
        d = x[r:r + rows, None] - mu[None, :]
        out[r:r + rows] = (np.exp(-d * d / (2 * v)) * w[None, :]).sum(axis=1)
    return out / np.sqrt(2 * np.longdouble(np.pi) * v)


@pytest.mark.parametrize("D,N,weighted,Ngrid,per_group", [(1, 256 * 256 + 1, True, 2, 2), (1, 256 * 256 + 1, False, 257, 2),
                                                          (1, 512 * 256 + 1, True, 257, 3), (3, 256 * 256 + 1, True, 2, 2)])
def test_kde_max_with_groups_of_several_chunks(D, N, weighted, Ngrid, per_group):
    assert_chunks_per_group(N, Ngrid, per_group, grid=True)
    p = _density(D, N, seed=D * 1000 + N + Ngrid, weighted=weighted)
    m, vals = kdehip.getKDEMax(p, Ngrid, values=True)
    assert m.shape == (D,) and vals.shape == (D, Ngrid)
    for i in range(D):
        lo, hi = kdehip.getKDERange(kdehip.marginal(p, [i]), 0.1)[0]
        x = grid(lo, hi, Ngrid)
        model = _marginal_model_blocked(p, i, x)
        err = np.abs(vals[i].astype(np.longdouble) - model)
        print("dimension", i, "largest |value - model| / model:", float(np.max(err / model)))
        assert np.all(model > 0) and np.all(err <= 1e-12 * model), float(np.max(err / model))
        k = int(np.argmax(model))
        got = int(np.flatnonzero(x == m[i])[0])
        if got != k:  # only a near tie of the top two values may pick the other one
            assert abs(model[got] - model[k]) <= 1e-11 * model[k], (i, got, k)
    dm, dvals = kdehip.DeviceDensity(p).getKDEMax(Ngrid, values=True)  # the resident entry gives the same bits
    assert np.array_equal(dm, m) and np.array_equal(dvals, vals)


def test_kde_max_of_one_point_is_the_point():
    p = _density(3, 1, seed=11)
    m, vals = kdehip.getKDEMax(p, 200, values=True)
    assert np.array_equal(m, kdehip.getPoints(p)[:, 0])
    assert all(np.all(vals[i] == vals[i][0]) for i in range(3))
    assert np.array_equal(kdehip.DeviceDensity(p).getKDEMax(200), m)


def test_summary_batch_items_equal_their_single_calls():
    """mixed D and N, some outputs NULL; the 6 x 50,000 item's leaf sum is split over many groups (196 chunks of 256
    leaves, at most 256 groups): its values are still those of a single call"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [(1, 100, 0.1, 200), (6, 2048, 0.1, 200), (6, 50000, 0.1, 200), (3, 7, 0.3, 1000), (8, 1, 0.0, 2),
             (2, 5000, 1.5, 333)]
    dens = [kdehip.DeviceDensity(_density(D, N, seed=50 + k, weighted=k % 2 == 1)) for k, (D, N, _, _) in enumerate(cases)]
    items, outs = [], []
    for k, ((D, N, extend, Ng), d) in enumerate(zip(cases, dens)):
        o = {"range": torch.full((2 * D,), np.nan, dtype=torch.float64, device=dev),
             "mean": torch.full((D,), np.nan, dtype=torch.float64, device=dev),
             "cov": torch.full((D * D,), np.nan, dtype=torch.float64, device=dev),
             "argmax": torch.full((D,), np.nan, dtype=torch.float64, device=dev),
             "values": torch.full((D * Ng,), np.nan, dtype=torch.float64, device=dev)}
        drop = [("cov", "values"), (), ("range", "mean"), ("argmax",), ("mean", "cov", "range"), ("values", "argmax")][k]
        for name in drop:
            o[name] = None
        outs.append(o)
        items.append({"density": d, "extend": extend, "Ngrid": Ng, **{n: t for n, t in o.items() if t is not None}})
    st = torch.cuda.current_stream(dev)
    kdehip.summary_device_batch(items, stream=st.cuda_stream)
    st.synchronize()
    for (D, N, extend, Ng), d, o in zip(cases, dens, outs):
        single = kdehip.summary._summary(d, extend=extend, N=Ng, range_=True, mean=True, cov=True, argmax=True, values=True)
        for name, t in o.items():
            if t is None:
                continue
            got = t.cpu().numpy()
            want = single[name]
            want = want.T.ravel() if name == "range" else want.ravel()  # (device layout: D x 2 column-major)
            assert np.array_equal(got, want), (D, N, name)


@pytest.mark.parametrize("weighted", [False, True])
def test_resident_marginal_equals_the_host_marginal(weighted):
    p = _density(3, 1000, seed=21, weighted=weighted)
    dp = kdehip.DeviceDensity(p)
    pos = np.random.default_rng(4).standard_normal((2, 77))
    for dims in ([0], [2], [1, 0], [2, 2], [0, 2, 1, 0]):
        hm = kdehip.marginal(p, dims)
        dm = dp.marginal(dims)
        assert dm.dims == len(dims) and dm.num_points == 1000
        _same_density(dm.download(), hm)
        if len(dims) == 2:
            assert np.array_equal(dm.evaluate(pos), kdehip.evaluateDualTree(hm, pos))


def test_resident_marginal_of_one_point_and_of_a_device_built_density():
    p = _density(2, 1, seed=5)
    _same_density(kdehip.DeviceDensity(p).marginal([1]).download(), kdehip.marginal(p, [1]))
    r = kdehip.DeviceDensity(_density(3, 300, seed=6)).resample(200, seed=9)  # built on the device: a host mirror of its own
    _same_density(r.marginal([2, 0]).download(), kdehip.marginal(r.download(), [2, 0]))
    with pytest.raises(ValueError):
        r.marginal([3])


def _inters_model(p, q, N):
    D = p.bt.dims
    rng = kdehip.getKDERange(p, 0.3)
    xs = [grid(rng[d, 0], rng[d, 1], N) for d in range(D)]
    dx = [x[1] - x[0] for x in xs]
    if D == 1:
        pos = xs[0][None, :]
        return math.fsum(kdehip.evaluateDualTree(p, pos) * kdehip.evaluateDualTree(q, pos)) * dx[0]
    pos = np.stack([np.tile(xs[0], N), np.repeat(xs[1], N)])  # row i = (x1_j, x2_i)
    return math.fsum(kdehip.evaluateDualTree(p, pos) * kdehip.evaluateDualTree(q, pos)) * dx[0] * dx[1]


@pytest.mark.parametrize("D,Np,Nq,N", [(1, 100, 150, 201), (1, 300, 40, 1000), (2, 100, 150, 201), (2, 30, 500, 64)])
def test_inters_matches_the_fsum_model_host_and_resident(D, Np, Nq, N):
    p, q = _density(D, Np, seed=Np + D), _density(D, Nq, seed=Nq + 7 * D, weighted=True)
    a = kdehip.intersIntgAppxIS(p, q, N)
    want = _inters_model(p, q, N)
    assert abs(a - want) <= 1e-12 * abs(want)
    b = kdehip.intersIntgAppxIS(kdehip.DeviceDensity(p), kdehip.DeviceDensity(q), N)
    assert a == b


def test_inters_with_a_density_of_several_chunks_per_group():
    """p has 256 * 256 + 1 points and the grid 257: intersIntgAppxIS evaluates both densities on p's grid by the existing
    evaluation, whose split (128-leaf chunks, at most 64 groups) gives a group nine chunks here"""
    Np, N = 256 * 256 + 1, 257
    assert_chunks_per_group(Np, N, 9)
    p, q = _density(1, Np, seed=Np + 1), _density(1, 150, seed=157, weighted=True)
    a = kdehip.intersIntgAppxIS(p, q, N)
    want = _inters_model(p, q, N)
    print("intersIntgAppxIS:", a, "model:", want, "relative difference:", abs(a - want) / abs(want))
    assert abs(a - want) <= 1e-12 * abs(want)
    assert a == kdehip.intersIntgAppxIS(kdehip.DeviceDensity(p), kdehip.DeviceDensity(q), N)


def _offs(seed, offs, N, dim):
    """intgAppxGaussianOffs (test/runtests.jl:203-209) with seeded numpy normals and the automatic bandwidth"""
    rng = np.random.default_rng(seed)
    p = kdehip.kde(rng.standard_normal((dim, 100)))
    pts = rng.standard_normal((dim, 150))
    pts[0, :] += offs
    return kdehip.intersIntgAppxIS(p, kdehip.kde(pts), N)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_inters_reference_statistical_checks(seed):
    assert 0.2 < _offs(seed, 0.0, 201, 1) < 0.35
    assert 0.1 < _offs(seed, 1.0, 1000, 1) < 0.3
    assert 0.01 < _offs(seed, -2.0, 1000, 1) < 0.17
    assert 0.05 < _offs(seed, 0.0, 201, 2) < 0.15


def test_inters_refuses_three_dimensions():
    p, q = _density(3, 20, seed=1), _density(3, 30, seed=2)
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.intersIntgAppxIS(kdehip.DeviceDensity(p), kdehip.DeviceDensity(q))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(kdehip.KdeHipError):
        kdehip.intersIntgAppxIS(p, q)
