"""`sample`, `rand` and `resample` with circular dimensions on the GPU (csrc/sample.hip, include/kdehip.h section 5e).

A draw with a manifold is the draw without one with circ_wrap applied to the circular coordinates: labels and Euclidean
coordinates byte-identical, circular ones byte-identical to the model's wrap of the Euclidean call's value, all of them in
[-pi, pi).  The host entry, the resident entry and the batch give the same bytes.  `resample` is that draw followed by
`from_device_points` with the same manifold and tree operators.  Sizes: one point, two, around the 256-sample tile (255, 256,
257, 600: more than one workgroup); D 1, 2, 3, 6; densities of more than 2048 points search C from global memory."""
import math

import numpy as np
import pytest

import kdehip
from tests import summary_circular_model as M

pytestmark = pytest.mark.gpu

ARRAYS_BT = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
ARRAYS_BD = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")


def _density(D, N, seed, man):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * 1.5
    for k in range(D):
        if man[k]:
            pts[k] = M.wrap(math.pi + 0.2 * rng.standard_normal(N)) + (4 * math.pi if k % 2 else 0.0)
    w = rng.uniform(0.05, 1.0, size=N) if N % 2 == 0 else None
    return kdehip.kde(pts, rng.uniform(0.2, 0.9, size=D), w)


def _manifolds(D):
    mixed = [(k + 1) % 2 for k in range(D)]
    return [[1] * D, mixed] if D > 1 else [[1]]


def _check_wrapped(got, plain, man):
    (P, I), (P0, I0) = got, plain
    assert I.tobytes() == I0.tobytes()
    circ = np.array(man, dtype=bool)
    assert P[~circ].tobytes() == P0[~circ].tobytes()
    assert P[circ].tobytes() == M.wrap(P0[circ]).tobytes()
    assert np.all((P[circ] >= -math.pi) & (P[circ] < math.pi))


@pytest.mark.parametrize("D", [1, 2, 3, 6])
@pytest.mark.parametrize("N,Npts", [(1, 5), (2, 255), (65, 256), (300, 257), (3000, 600)])
def test_a_circular_draw_is_the_wrapped_euclidean_draw(D, N, Npts):
    for man in _manifolds(D):
        p = _density(D, N, seed=31 * D + N, man=man)
        dp = kdehip.DeviceDensity(p)
        plain = kdehip.sample(p, Npts, seed=77, sample_offset=3)
        host = kdehip.sample(p, Npts, seed=77, sample_offset=3, manifold=man)
        _check_wrapped(host, plain, man)
        if Npts >= 255:
            assert np.any(host[0] != plain[0])   # the case does wrap something
        res = kdehip.sample(dp, Npts, seed=77, sample_offset=3, manifold=man)
        assert res[0].tobytes() == host[0].tobytes() and res[1].tobytes() == host[1].tobytes()
        # given labels: only the normals are drawn
        lab = plain[1][::-1].copy()
        _check_wrapped(kdehip.sample(dp, Npts, lab, seed=5, manifold=man), kdehip.sample(dp, Npts, lab, seed=5), man)
        # None and all-Euclidean are the call without a manifold
        for none in (None, [0] * D):
            same = kdehip.sample(dp, Npts, seed=77, sample_offset=3, manifold=none)
            assert same[0].tobytes() == plain[0].tobytes() and same[1].tobytes() == plain[1].tobytes()
        assert kdehip.rand(dp, Npts, seed=9, manifold=man).tobytes() == kdehip.sample(dp, Npts, seed=9, manifold=man)[0].tobytes()


def test_the_batch_mixes_euclidean_and_circular_items():
    import torch
    dev = torch.device("cuda", 0)
    cases = [(1, 65, 256, [1]), (3, 300, 257, [1, 0, 1]), (3, 300, 100, None), (6, 2, 600, [1] * 6), (2, 3000, 255, [0, 1]),
             (2, 65, 7, [0, 0])]
    dens = [kdehip.DeviceDensity(_density(D, N, seed=k, man=man or [0] * D)) for k, (D, N, _, man) in enumerate(cases)]
    items = []
    for k, ((D, N, Npts, man), d) in enumerate(zip(cases, dens)):
        items.append({"density": d, "Npts": Npts, "seed": 100 + k, "sample_offset": k,
                      "d_pts": torch.full((D * Npts,), np.nan, dtype=torch.float64, device=dev),
                      "d_ind": torch.zeros(Npts, dtype=torch.int64, device=dev)})
    st = torch.cuda.current_stream(dev)
    kdehip.sample_device_batch(items, stream=st.cuda_stream, manifold=[c[3] for c in cases])
    st.synchronize()
    for k, ((D, N, Npts, man), d, it) in enumerate(zip(cases, dens, items)):
        P, I = kdehip.sample(d, Npts, seed=100 + k, sample_offset=k, manifold=man)
        assert it["d_pts"].cpu().numpy().tobytes() == np.ascontiguousarray(P.T).tobytes(), k
        assert it["d_ind"].cpu().numpy().tobytes() == I.tobytes(), k
    # "inherit" reads the density's record; an item's own key wins over the shared argument
    d = dens[1]
    d.manifold = np.array([1, 0, 1], dtype=np.uint8)
    want = kdehip.sample(d, 50, seed=4, manifold=[1, 0, 1])
    got = kdehip.sample(d, 50, seed=4, manifold="inherit")
    assert got[0].tobytes() == want[0].tobytes()
    one = {"density": d, "Npts": 50, "seed": 4, "manifold": "inherit",
           "d_pts": torch.empty(150, dtype=torch.float64, device=dev), "d_ind": torch.empty(50, dtype=torch.int64, device=dev)}
    kdehip.sample_device_batch([one], stream=st.cuda_stream)
    st.synchronize()
    assert one["d_pts"].cpu().numpy().tobytes() == np.ascontiguousarray(want[0].T).tobytes()
    with pytest.raises(ValueError):
        kdehip.sample(d, 5, seed=1, manifold=[1, 2, 0])


def _same_density(a, b):
    for k in ARRAYS_BT:
        assert np.array_equal(getattr(a.bt, k), getattr(b.bt, k)), k
    for k in ARRAYS_BD:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("D,N,Np,man", [(1, 300, 257, [1]), (3, 300, None, [1, 0, 1]), (2, 65, 64, [1, 1])])
def test_resample_is_the_wrapped_draw_then_kde_on_the_manifold(D, N, Np, man):
    import torch
    dp = kdehip.DeviceDensity(_density(D, N, seed=3 + D, man=man))
    r = dp.resample(Np, seed=42, manifold=man, tree_manifold=man)
    n = N if Np is None else Np
    assert r.num_points == n and r.dims == D
    assert np.array_equal(r.manifold, man) and np.array_equal(r.tree_manifold, man)
    pts, _ = kdehip.sample(dp, n, seed=42, manifold=man)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts.T)).to(torch.device("cuda", 0))
    want = kdehip.DeviceDensity.from_device_points(d_pts, D, n, manifold=man, tree_manifold=man)
    _same_density(r.download(), want.download())
    assert r.bw.tobytes() == want.bw.tobytes() and r.nevals == want.nevals
    # the module-level function and "inherit"
    dp.manifold = dp.tree_manifold = np.array(man, dtype=np.uint8)
    r2 = kdehip.resample(dp, Np, seed=42, manifold="inherit", tree_manifold="inherit")
    _same_density(r2.download(), want.download())
    # without the keywords: the Euclidean resample, whatever the density remembers
    e = dp.resample(Np, seed=42)
    d0 = torch.from_numpy(np.ascontiguousarray(kdehip.sample(dp, n, seed=42)[0].T)).to(torch.device("cuda", 0))
    _same_density(e.download(), kdehip.DeviceDensity.from_device_points(d0, D, n).download())
    assert e.manifold is None and e.tree_manifold is None


def test_mul_device_batch_accepts_a_numpy_bool():
    a = kdehip.DeviceDensity(_density(1, 65, seed=1, man=[0]))
    b = kdehip.DeviceDensity(_density(1, 65, seed=2, man=[0]))
    x = kdehip.mul_device_batch([[a, b]], addEntropy=np.bool_(True), seeds=[5])[0]
    y = kdehip.mul_device_batch([[a, b]], addEntropy=True, seeds=[5])[0]
    _same_density(x.download(), y.download())
