"""`sample` / `rand` / `resample` on the GPU (csrc/sample.hip, include/kdehip.h section 2f) against the numpy model

    u, n = philox_streams(seed, sample_offset, Npts, 1, D); C = cumsum(getWeights(p)); C /= C[-1]
    lab = searchsorted(C, u, side="right");  x = getPoints(p)[:, lab] + getBW(p)[:, lab] * n.reshape(Npts, D).T

Labels are compared exactly against that model.  The normals are the one part the host cannot reproduce bit for bit: the
device's log / sin / cos (ocml) and the host libm may round the last bit of a Box-Muller normal differently (the product
tests allow ulps for the same reason).  So the points are compared exactly against the model fed with the DEVICE's own
normals -- read back by sampling a one-point density at the origin with unit variance, where x = 0 + 1 * n = n exactly --
and those normals are compared with the host twin's to a few ulps.  Everything else of a point (gather, sqrt, product,
sum: separate IEEE roundings) is checked bit for bit."""
import math
import threading

import numpy as np
import pytest

import kdehip
from kdehip import _lib

pytestmark = pytest.mark.gpu


def _density(seed, D, N, weighted=False):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-3, 3, size=(D, 1))
    ks = rng.uniform(0.1, 0.6, size=D)  # per-dimension bandwidths
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    return kdehip.kde(pts, ks, w)


_UNIT = {}


def _device_normals(D, seed, offset, Npts):
    """the normals the device draws for samples offset .. offset+Npts-1, (D, Npts)"""
    if D not in _UNIT:
        _UNIT[D] = kdehip.kde(np.zeros((D, 1)), [1.0])
    x, lab = kdehip.sample(_UNIT[D], Npts, seed=seed, sample_offset=offset)
    assert (lab == 1).all()
    return x


def _model_labels(p, Npts, seed, offset):
    u, _ = kdehip.philox_streams(seed, offset, Npts, 1, 1)
    C = np.cumsum(kdehip.getWeights(p))
    C /= C[-1]
    return np.searchsorted(C, u, side="right")


def _model(p, Npts, seed, offset=0, lab=None):
    D = kdehip.Ndim(p)
    if lab is None:
        lab = _model_labels(p, Npts, seed, offset)
    n = _device_normals(D, seed, offset, Npts)
    x = kdehip.getPoints(p)[:, lab] + kdehip.getBW(p)[:, lab] * n
    return x, lab + 1


def _check(p, Npts, seed, offset=0):
    x, ind = kdehip.sample(p, Npts, seed=seed, sample_offset=offset)
    mx, mi = _model(p, Npts, seed, offset)
    assert np.array_equal(ind, mi)
    assert np.array_equal(x, mx)
    return x, ind


@pytest.mark.parametrize("D,N,Npts,weighted", [
    (1, 1, 1000, False), (1, 2, 4096, True), (1, 200, 100000, True), (1, 20000, 1 << 20, False),
    (2, 2, 3000, False), (2, 200, 50000, True), (2, 1000, 70001, False),
    (3, 1, 257, True), (3, 1000, 1 << 16, True), (3, 20000, 300000, True),
    (6, 200, 10000, False), (6, 1000, 1 << 20, False), (6, 20000, 100000, True),
    (8, 2, 999, True), (8, 200, 30000, False), (8, 1000, 1 << 18, True), (8, 20000, 65536, False),
])
def test_labels_and_points_equal_the_model(D, N, Npts, weighted):
    p = _density(1000 * D + N, D, N, weighted)
    _check(p, Npts, seed=77 + D + N)


@pytest.mark.parametrize("D", [1, 3, 8])
def test_device_normals_are_the_host_twins_to_a_few_ulps(D):
    Npts = 200000
    _, n = kdehip.philox_streams(123, 5, Npts, 1, D)
    dev = _device_normals(D, 123, 5, Npts)
    host = n.reshape(Npts, D).T
    assert np.isfinite(dev).all()
    assert np.all(np.abs(dev - host) <= 1e-14 * (1.0 + np.abs(host)))


def test_zero_weight_points_are_never_drawn():
    rng = np.random.default_rng(5)
    N = 300
    w = rng.uniform(0.1, 1.0, size=N)
    zero = rng.choice(N, size=100, replace=False)
    w[zero] = 0.0
    w[0] = w[N - 1] = 0.0  # the first and the last point too
    p = kdehip.kde(rng.standard_normal((2, N)), [0.2], w)
    x, ind = _check(p, 200000, seed=3)
    assert not np.isin(ind - 1, np.concatenate([zero, [0, N - 1]])).any()


def test_a_sample_offset_continues_the_stream():
    p = _density(8, 3, 500, True)
    x, ind = kdehip.sample(p, 10000, seed=9)
    a = kdehip.sample(p, 3333, seed=9)
    b = kdehip.sample(p, 10000 - 3333, seed=9, sample_offset=3333)
    assert np.array_equal(np.concatenate([a[0], b[0]], axis=1), x)
    assert np.array_equal(np.concatenate([a[1], b[1]]), ind)


def test_zero_and_one_sample():
    p = _density(4, 2, 50)
    x, ind = kdehip.sample(p, 0, seed=1)
    assert x.shape == (2, 0) and ind.shape == (0,)
    _check(p, 1, seed=1)
    r = kdehip.rand(p, seed=1)
    assert r.shape == (2, 1) and np.array_equal(r, kdehip.sample(p, 1, seed=1)[0])
    with kdehip.DeviceDensity(p) as dd:
        x, ind = kdehip.sample(dd, 0, seed=1)
        assert x.shape == (2, 0)
        assert np.array_equal(kdehip.sample(dd, 1, seed=1)[0], kdehip.sample(p, 1, seed=1)[0])


def test_given_labels():
    import torch
    p = _density(6, 4, 700, True)
    rng = np.random.default_rng(1)
    Npts = 5000
    lab1 = rng.integers(1, 701, size=Npts)
    x, ind = kdehip.sample(p, Npts, lab1, seed=21, sample_offset=7)
    mx, mi = _model(p, Npts, 21, 7, lab=lab1 - 1)
    assert np.array_equal(ind, lab1) and np.array_equal(mi, lab1)
    assert np.array_equal(x, mx)
    bad = lab1.copy()
    bad[17] = 701
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.sample(p, Npts, bad, seed=21)
    assert e.value.code == _lib.ERR_ARG
    # the device form: an out-of-range label is a NaN point with ind 0, never a read out of bounds
    bad[18], bad[19], bad[20] = 0, -5, 1 << 40
    with kdehip.DeviceDensity(p) as dd:
        dev = torch.device("cuda", 0)
        P = torch.zeros(4 * Npts, dtype=torch.float64, device=dev)
        I = torch.zeros(Npts, dtype=torch.int64, device=dev)
        T = torch.from_numpy(bad).to(dev)
        torch.cuda.synchronize()
        dd.sample_device(P, I, Npts, seed=21, sample_offset=7, ind=T)
        torch.cuda.synchronize()
        gx = P.cpu().numpy().reshape(Npts, 4).T
        gi = I.cpu().numpy()
    badcols = [17, 18, 19, 20]
    assert np.isnan(gx[:, badcols]).all() and (gi[badcols] == 0).all()
    good = np.setdiff1d(np.arange(Npts), badcols)
    assert np.array_equal(gx[:, good], mx[:, good]) and np.array_equal(gi[good], lab1[good])


def _check_handle_equals_host(dd, host, Npts, seed, offset=0):
    a = kdehip.sample(dd, Npts, seed=seed, sample_offset=offset)
    b = kdehip.sample(host, Npts, seed=seed, sample_offset=offset)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def test_resident_handles_equal_the_host_entry():
    host = [_density(30 + j, 2, 200, weighted=(j == 0)) for j in range(3)]
    up = [kdehip.DeviceDensity(h) for h in host]
    for h, d in zip(host, up):
        _check_handle_equals_host(d, h, 20000, seed=4, offset=11)
        _check(h, 2000, seed=4)
    m = kdehip.mul_device(up[:2], seed=99)
    _check_handle_equals_host(m, m.download(), 50000, seed=5)
    mb = kdehip.mul_device_batch([up[:2], up[1:], [up[0], up[2]]], seeds=[1, 2, 3])
    for d in mb:
        _check_handle_equals_host(d, d.download(), 30000, seed=6, offset=3)
    for d in mb + [m] + up:
        d.close()


def test_ragged_mixed_dimension_batch_equals_single_calls():
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(64)
    dens, items, singles = [], [], []
    for k in range(64):
        D = int(rng.integers(1, 9))
        N = int(rng.choice([1, 2, 37, 200, 1500]))
        dens.append(kdehip.DeviceDensity(_density(500 + k, D, N, weighted=bool(k % 2))))
    st = torch.cuda.Stream(device=dev)
    for k in range(64):
        d = dens[k % 40]  # (some densities serve several items)
        Npts = int(rng.choice([0, 1, 200, 255, 257, 3000]))
        seed, off = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 1000))
        it = {"density": d, "Npts": Npts, "seed": seed, "sample_offset": off,
              "d_pts": torch.full((max(1, d.dims * Npts),), -7.0, dtype=torch.float64, device=dev),
              "d_ind": torch.full((max(1, Npts),), -7, dtype=torch.int64, device=dev)}
        if k % 5 == 0 and Npts > 0:
            it["ind"] = torch.from_numpy(rng.integers(1, d.num_points + 1, size=Npts)).to(dev)
        items.append(it)
        P = torch.full_like(it["d_pts"], -7.0)
        I = torch.full_like(it["d_ind"], -7)
        singles.append((P, I))
    torch.cuda.synchronize()
    kdehip.sample_device_batch(items, stream=st.cuda_stream)
    for it, (P, I) in zip(items, singles):
        it["density"].sample_device(P, I, it["Npts"], seed=it["seed"], sample_offset=it["sample_offset"], ind=it.get("ind"),
                                    stream=st.cuda_stream)
    st.synchronize()
    for it, (P, I) in zip(items, singles):
        assert torch.equal(it["d_pts"], P) and torch.equal(it["d_ind"], I)
        if it["Npts"] == 0:
            assert float(P[0]) == -7.0 and int(I[0]) == -7
    # and against the host model
    for it in items[:10]:
        if it["Npts"] == 0 or "ind" in it:
            continue
        d = it["density"]
        x, lab = kdehip.sample(d, it["Npts"], seed=it["seed"], sample_offset=it["sample_offset"])
        assert np.array_equal(it["d_pts"].cpu().numpy().reshape(it["Npts"], d.dims).T, x)
    for d in dens:
        d.close()


def _same_density(a, b):
    for name in ("means", "bandwidth", "bandwidthMin", "bandwidthMax"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation"):
        assert np.array_equal(getattr(a.bt, name), getattr(b.bt, name)), name


@pytest.mark.parametrize("D,N,Np", [(1, 300, None), (2, 200, 500), (6, 1000, 3000)])
def test_resample_device_equals_kde_of_the_sample(D, N, Np):
    p = _density(70 + D, D, N, weighted=True)
    with kdehip.DeviceDensity(p) as dd:
        r = dd.resample(Np, seed=12)
        got = r.download()
        r.close()
    pts, _ = _model(p, N if Np is None else Np, 12)
    _same_density(got, kdehip.kde(pts))
    # the Python front end: a BallTreeDensity gives kde!(sample) on the host arrays
    _same_density(kdehip.resample(p, Np, seed=12), got)
    # :discrete -- labels by weight, the points themselves, p's first kernel size
    q = kdehip.resample(p, Np, "discrete", seed=12)
    lab = _model_labels(p, N if Np is None else Np, 12, 0)
    _same_density(q, kdehip.kde(kdehip.getPoints(p)[:, lab], kdehip.getBW(p)[:, 0]))


def test_resample_needs_two_points():
    p = kdehip.kde(np.zeros((2, 1)), [1.0])
    with kdehip.DeviceDensity(p) as dd:
        with pytest.raises(kdehip.KdeHipError) as e:
            dd.resample(seed=1)
        assert e.value.code == _lib.ERR_ARG


def test_three_component_mixture_statistics():
    mu, w, sig = np.array([-2.0, 0.5, 3.0]), np.array([0.2, 0.5, 0.3]), 0.4
    p = kdehip.kde(mu.reshape(1, 3), [sig], w)
    M = 10 ** 6
    x, ind = kdehip.sample(p, M, seed=2024)
    freq = np.bincount(ind - 1, minlength=3) / M
    assert np.all(np.abs(freq - w) <= 5 * np.sqrt(w * (1 - w) / M)), freq
    xs = np.sort(x[0])
    erf = np.frompyfunc(math.erf, 1, 1)
    F = sum(wi * 0.5 * (1.0 + erf((xs - m) / (sig * math.sqrt(2.0))).astype(np.float64)) for wi, m in zip(w, mu))
    emp_hi = np.arange(1, M + 1) / M
    ks = max(np.max(emp_hi - F), np.max(F - (emp_hi - 1.0 / M)))
    assert ks < 2e-3, ks


def test_concurrent_first_calls_on_one_handle():
    p = _density(99, 3, 20000, True)
    want = kdehip.sample(p, 40000, seed=8)
    dd = kdehip.DeviceDensity(p)
    out, errs = [None, None], []
    barrier = threading.Barrier(2)

    def run(k):
        try:
            barrier.wait()
            out[k] = kdehip.sample(dd, 40000, seed=8)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for o in out:
        assert np.array_equal(o[0], want[0]) and np.array_equal(o[1], want[1])
    dd.close()


def test_resident_handle_with_bad_weights_reports_an_argument_error():
    p = _density(3, 2, 64)
    N = kdehip.Npts(p)
    p.bt.weights[N + 5] = -1.0
    with kdehip.DeviceDensity(p) as dd:
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(kdehip.KdeHipError) as e:
                kdehip.sample(dd, 10, seed=0)
            assert e.value.code == _lib.ERR_ARG
