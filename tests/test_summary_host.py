"""`marginal` / `getKDERange` / `getKDEMean` / `getKDEfit` without a GPU, and the argument checks the summary entries make
before they touch a device (include/kdehip.h section 5c).  Host ranges and means are held bit for bit to models written
here from getPoints (a plain sequential loop for the mean); the marginal to the reference's composition
kde(getPoints(p)[dims], getBW(p)[dims, 0], getWeights(p)) array for array."""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
ARRAYS_BT = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
ARRAYS_BD = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")


def _density(D=2, N=20, seed=3, weighted=False, per_dim_bw=False):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 3.0, size=(D, 1)) + rng.uniform(-2, 2, size=(D, 1))
    ks = rng.uniform(0.1, 0.7, size=D) if per_dim_bw else [0.3]
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    return kdehip.kde(pts, ks, w)


def _fake_device_density(D=2, N=20):
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    return fake


def _range_model(p, extend):
    pts = kdehip.getPoints(p)
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    dr = extend * (hi - lo)
    return np.stack([lo - dr, hi + dr], axis=1)


def _mean_model(p):
    pts = kdehip.getPoints(p)
    D, N = pts.shape
    out = np.empty(D)
    for d in range(D):
        s = 0.0
        for x in pts[d].tolist():
            s += x
        out[d] = s / N
    return out


SHAPES = [(D, N) for D in (1, 2, 3, 6, 8) for N in (1, 2, 100, 2048, 5000)]


@pytest.mark.parametrize("D,N", SHAPES)
def test_range_is_the_numpy_model_bit_for_bit(D, N):
    for weighted in (False, True):
        p = _density(D, N, seed=10 * D + N, weighted=weighted, per_dim_bw=True)
        for extend in (0.1, 0.0, 0.3, 1.7):
            r = kdehip.getKDERange(p, extend)
            assert r.shape == (D, 2)
            assert np.array_equal(r, _range_model(p, extend))
        assert np.array_equal(kdehip.getKDERange(p), _range_model(p, 0.1))


def test_range_of_several_densities_is_the_elementwise_union():
    ps = [_density(3, N, seed=s) for s, N in ((1, 50), (2, 7), (3, 300))]
    rs = [_range_model(p, 0.2) for p in ps]
    want = np.stack([np.min([r[:, 0] for r in rs], axis=0), np.max([r[:, 1] for r in rs], axis=0)], axis=1)
    assert np.array_equal(kdehip.getKDERange(ps, 0.2), want)
    assert np.array_equal(kdehip.getKDERange(ps[:1], 0.2), rs[0])
    with pytest.raises(ValueError):
        kdehip.getKDERange([ps[0], _density(2, 9)])
    with pytest.raises(ValueError):
        kdehip.getKDERange([])


def test_range_linspace_is_the_stated_grid_and_1d_only():
    p = _density(1, 40, seed=8)
    lo, hi = _range_model(p, 0.1)[0]
    x = kdehip.getKDERangeLinspace(p, N=200)
    h = (hi - lo) / 199.0
    assert x.shape == (200,) and x[0] == lo and x[-1] == hi
    assert all(x[k] == lo + k * h for k in range(199))
    assert np.array_equal(kdehip.getKDERangeLinspace(p, extend=0.3, N=2), np.array(_range_model(p, 0.3)[0]))
    with pytest.raises(ValueError):
        kdehip.getKDERangeLinspace(_density(2, 10))
    with pytest.raises(ValueError):
        kdehip.getKDERangeLinspace(p, N=1)


@pytest.mark.parametrize("D,N", SHAPES)
def test_mean_is_the_sequential_sum_bit_for_bit(D, N):
    p = _density(D, N, seed=7 * D + N, weighted=True)  # (weights play no part: the reference's mean is unweighted)
    m = kdehip.getKDEMean(p)
    assert np.array_equal(m, _mean_model(p))


@pytest.mark.parametrize("D,N", [(1, 1), (2, 100), (3, 2048), (6, 5000), (8, 2)])
def test_fit_mean_is_getKDEMean_and_the_covariance_is_the_mle(D, N):
    p = _density(D, N, seed=D + N)
    mu, S = kdehip.getKDEfit(p)
    assert np.array_equal(mu, kdehip.getKDEMean(p))
    X = kdehip.getPoints(p).astype(np.longdouble)
    Xc = X - X.mean(axis=1, keepdims=True)
    want = (Xc @ Xc.T) / N
    assert S.shape == (D, D) and np.array_equal(S, S.T)
    assert np.max(np.abs(S - want)) <= 1e-12 * max(float(np.max(np.abs(want))), 1e-300)


@pytest.mark.parametrize("dims", [[0], [2], [1, 0], [2, 2], [0, 2, 1, 0]])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_marginal_is_the_reference_composition(dims, weighted):
    p = _density(3, 257, seed=5, weighted=weighted, per_dim_bw=True)
    m = kdehip.marginal(p, dims)
    want = kdehip.kde(kdehip.getPoints(p)[dims], kdehip.getBW(p)[dims, 0], kdehip.getWeights(p))
    for k in ARRAYS_BT:
        assert np.array_equal(getattr(m.bt, k), getattr(want.bt, k)), k
    for k in ARRAYS_BD:
        assert np.array_equal(getattr(m, k), getattr(want, k)), k
    # the variance is fl(sqrt(v))**2, not v
    v = p.bandwidth[p.bt.num_points * 3:].reshape(-1, 3)[np.argmax(p.bt.permutation[p.bt.num_points:] == 1)]
    assert np.array_equal(m.bandwidth[len(dims) * 257:len(dims) * 258], np.sqrt(v[dims]) ** 2)


def test_marginal_of_one_point_and_bad_dims():
    p = _density(2, 1, seed=4)
    m = kdehip.marginal(p, [1])
    want = kdehip.kde(kdehip.getPoints(p)[[1]], kdehip.getBW(p)[[1], 0], kdehip.getWeights(p))
    assert np.array_equal(m.means, want.means) and np.array_equal(m.bandwidth, want.bandwidth)
    q = _density(2, 10)
    for bad in ([2], [-1], [], [0] * 9, [0.5]):
        with pytest.raises(ValueError):
            kdehip.marginal(q, bad)


def test_mixed_density_kinds_are_a_type_error():
    p, fake = _density(), _fake_device_density()
    for fn in (lambda: kdehip.intersIntgAppxIS(p, fake), lambda: kdehip.intersIntgAppxIS(fake, p),
               lambda: kdehip.getKDERange([p, fake]), lambda: kdehip.getKDEMean(np.zeros((2, 3))),
               lambda: kdehip.summary_device_batch([{"density": p}])):
        with pytest.raises(TypeError):
            fn()


def _kde_max(p, Ngrid, out=True, device=NO_SUCH_DEVICE):
    m = np.zeros(max(1, p.bt.dims)) if p is not None else np.zeros(1)
    return _lib.lib.kdehip_kde_max(None if p is None else C.byref(p._cstruct()), int(Ngrid),
                                   _lib.ptr(m, _lib.f64p) if out else None, None, int(device))


def _inters(p, q, Ngrid, out=True, device=NO_SUCH_DEVICE):
    r = C.c_double(0.0)
    return _lib.lib.kdehip_inters_intg_appx_is(None if p is None else C.byref(p._cstruct()),
                                               None if q is None else C.byref(q._cstruct()), int(Ngrid),
                                               C.byref(r) if out else None, int(device))


def test_kde_max_argument_checks_come_before_the_device():
    p = _density()
    assert _kde_max(None, 200) == _lib.ERR_ARG
    assert _kde_max(p, 200, out=False) == _lib.ERR_ARG
    for n in (1, 0, -5):
        assert _kde_max(p, n) == _lib.ERR_ARG
        assert "Ngrid" in _lib.lib.kdehip_last_error().decode()
    assert _kde_max(p, 2 ** 24 + 1) == _lib.ERR_UNSUPPORTED
    assert _kde_max(_density(D=9, N=5), 200) == _lib.ERR_UNSUPPORTED
    # every argument is fine: what fails is the device ordinal
    assert _kde_max(p, 2) != _lib.KDEHIP_OK
    assert "Ngrid" not in _lib.lib.kdehip_last_error().decode()


def test_inters_argument_checks_come_before_the_device():
    p, q = _density(1, 30, seed=1), _density(1, 40, seed=2)
    assert _inters(None, q, 201) == _lib.ERR_ARG
    assert _inters(p, None, 201) == _lib.ERR_ARG
    assert _inters(p, q, 201, out=False) == _lib.ERR_ARG
    assert _inters(p, q, 1) == _lib.ERR_ARG
    assert "Ngrid" in _lib.lib.kdehip_last_error().decode()
    assert _inters(p, _density(2, 10), 201) == _lib.ERR_DIM_MISMATCH
    assert _inters(_density(3, 10), _density(3, 12, seed=9), 201) == _lib.ERR_UNSUPPORTED
    assert _inters(_density(2, 10), _density(2, 12, seed=9), 2 ** 14 + 1) == _lib.ERR_UNSUPPORTED
    r = _density(1, 30, seed=3)
    r.bandwidth[30 + 4] *= 2.0  # leaf 4 gets a bandwidth of its own
    assert _inters(p, r, 201) == _lib.ERR_UNSUPPORTED
    assert "bandwidth" in _lib.lib.kdehip_last_error().decode()
    with pytest.raises(ValueError):
        kdehip.intersIntgAppxIS(p, _density(2, 10))
    with pytest.raises(kdehip.KdeHipError):
        kdehip.intersIntgAppxIS(_density(3, 10), _density(3, 11), device=NO_SUCH_DEVICE)


def test_resident_entries_refuse_null_arguments():
    out = C.c_double(0.0)
    h = C.c_void_p()
    dims = (C.c_int32 * 2)(1, 1)
    assert _lib.lib.kdehip_inters_intg_appx_is_device(None, None, 201, C.byref(out)) == _lib.ERR_ARG
    assert _lib.lib.kdehip_inters_intg_appx_is_device(None, None, 201, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_density_summary(None, None, 200, None, None, None, None, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_density_marginal_device(None, None, 1, dims) == _lib.ERR_ARG
    assert _lib.lib.kdehip_density_marginal_device(C.byref(h), None, 1, dims) == _lib.ERR_ARG
    for nsel in (0, -1, 9):
        assert _lib.lib.kdehip_density_marginal_device(C.byref(h), None, nsel, dims) == _lib.ERR_ARG
        assert "nsel" in _lib.lib.kdehip_last_error().decode()
    assert _lib.lib.kdehip_density_marginal_device(C.byref(h), None, 2, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_summary_device_batch(-1, None, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_summary_device_batch(1, None, None) == _lib.ERR_ARG
    items = (_lib.CSummaryItem * 1)()  # a null handle
    items[0].Ngrid = 200
    assert _lib.lib.kdehip_summary_device_batch(1, items, None) == _lib.ERR_ARG
    assert _lib.lib.kdehip_summary_device_batch(0, None, None) == _lib.KDEHIP_OK  # nothing to do
