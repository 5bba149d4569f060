"""The exact product of two densities on the GPU (csrc/prodexact.hip, include/kdehip.h section 5p): `prod_exact`,
`product_components`, `log_intersIntg`, `mul_exact` and `prod_exact_device_batch` against tests/prodexact_model.py (fp64,
exactly rounded sums, extended-precision cumulative sums), and against each other bit for bit.

Tolerances, none of them taken from the code under test:
  logz     1e-12 * max(1, |ref|), the bound of tests/test_gpu_logdensity.py; 1e-10 against log(intersIntg) where that is finite
  labels   exact for every draw whose thresholds the MODEL shows to lie at least a relative 1e-9 from a boundary between two
           leaves (section 5p); at most 2 draws of a case may be exempted for that
  points   1e-12 * max(1, |x|), the project's parity tolerance for points (the host's normals may differ from the device's
           in their last bits)
  weights  1e-12 against the enumerated closed form, their sum 1 within 1e-14.
The shapes sit on the kernel's edges: a 128-leaf chunk, a 256-lane block, and more than 64 chunks so that a group holds two."""
import ctypes as C
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import prodexact_model as pm
from tests.test_prodexact_host import _brute

pytestmark = pytest.mark.gpu

SEED = 20261020
# (D, N1, N2, Np, weighted)
SHAPES = [(1, 1, 1, 300, False), (2, 127, 129, 1000, False), (3, 257, 300, 1000, False), (8, 128, 128, 257, False),
          (6, 300, 8320, 600, False), (3, 130, 257, 500, True)]


def _weights(rng, N):
    """non-uniform, with exact zeros"""
    w = rng.uniform(0.05, 1.0, size=N)
    w[::5] = 0.0
    return w


def _density(rng, D, N, weighted=False, shift=0.0, bw=None):
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1)) + shift
    return kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D) if bw is None else bw, _weights(rng, N) if weighted else None)


def _leaf(p):
    """(points (D, N), weights, variances) in leaf order, and the 1-based original index of every leaf"""
    N, D = p.bt.num_points, p.bt.dims
    dens = (p.means[N * D:].reshape(N, D).T.copy(), p.bt.weights[N:].copy(), p.bandwidth[N * D:(N + 1) * D].copy())
    return dens, p.bt.permutation[N:].copy()


def _streams(seed, offset, Np, D):
    u, n = kdehip.philox_streams(seed, offset, Np, 2, D)
    return u.reshape(Np, 2), n.reshape(Np, D)


_CASES = {}


def _case(D, N1, N2, Np, weighted, shift=0.0, fma=False):
    """two densities of one shape, the model's rows and the library's host call: built once, shared, never changed"""
    key = (D, N1, N2, Np, weighted, shift)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * N1 + N2)
        p = _density(rng, D, N1, weighted)
        q = _density(rng, D, N2, weighted, shift=shift)
        (lp, permp), (lq, permq) = _leaf(p), _leaf(q)
        pre = pm.rows(lp, lq, fma)
        pts, ind, logz = kdehip.prod_exact(p, q, Np, seed=SEED, return_logz=True)
        _CASES[key] = dict(p=p, q=q, lp=lp, lq=lq, permp=permp, permq=permq, pre=pre, logz=pm.logz(lp, lq, L=pre[3]),
                           got=(pts, ind, logz))
    return _CASES[key]


def _check_draws(c, pts, ind, Np, D, offset=0):
    U, Nn = _streams(SEED, offset, Np, D)
    want, leaves, gap = pm.draw_labels(c["lp"], c["permp"], c["lq"], c["permq"], U, pre=c["pre"])
    assert pts.shape == (D, Np) and ind.shape == (2, Np) and ind.dtype == np.int64
    firm = gap >= 1e-9
    print("draws exempted for gap < 1e-9:", int((~firm).sum()), " smallest gap:", float(gap.min()))
    assert int((~firm).sum()) <= 2
    assert np.array_equal(ind.T[firm], want[firm]), int((ind.T[firm] != want[firm]).any(axis=1).sum())
    same = (ind.T == want).all(axis=1)
    x = pm.points(c["lp"], c["lq"], leaves, Nn)
    err = np.abs(pts.T[same] - x[same]) / np.maximum(1.0, np.abs(x[same]))
    print("points: max err / bound", float(err.max() / 1e-12))
    assert np.all(np.isfinite(pts)) and np.all(err <= 1e-12)
    # the labels are original indices of points that carry weight
    for k, d in enumerate((c["p"], c["q"])):
        assert ind[k].min() >= 1 and ind[k].max() <= d.bt.num_points
        assert np.all(kdehip.getWeights(d)[ind[k] - 1] > 0.0)


def _close_log(got, want):
    print("logz: |err| / bound", abs(got - want) / (1e-12 * max(1.0, abs(want))))
    assert math.isfinite(got) and abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


# ---- 1. labels, points and logz against the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("D,N1,N2,Np,weighted", SHAPES)
def test_draws_and_logz_equal_the_model(D, N1, N2, Np, weighted):
    c = _case(D, N1, N2, Np, weighted)
    pts, ind, logz = c["got"]
    _check_draws(c, pts, ind, Np, D)
    _close_log(logz, c["logz"])
    direct = kdehip.intersIntg(c["p"], c["q"])
    assert direct > 1e-300  # (no underflow at these shapes)
    assert abs(logz - math.log(direct)) <= 1e-10
    assert kdehip.log_intersIntg(c["p"], c["q"]) == logz


def test_a_sample_offset_continues_an_earlier_call():
    D, N1, N2 = 3, 257, 300
    c = _case(D, N1, N2, 1000, False)
    pts, ind, _ = c["got"]
    tail_pts, tail_ind = kdehip.prod_exact(c["p"], c["q"], 300, seed=SEED, sample_offset=700)
    assert np.array_equal(tail_pts, pts[:, 700:]) and np.array_equal(tail_ind, ind[:, 700:])
    head_pts, head_ind = kdehip.prod_exact(c["p"], c["q"], 10, seed=SEED)
    assert np.array_equal(head_pts, pts[:, :10]) and np.array_equal(head_ind, ind[:, :10])


def test_forty_bandwidths_apart_logz_is_finite():
    """q is moved 40 standard deviations of the summed kernel along every axis: every e_ij is below -745, the integral
    underflows (or nearly), logz and the draws do not"""
    D, N1, N2, Np = 2, 40, 50, 300
    c = _case(D, N1, N2, Np, False, shift=40.0 * math.sqrt(1.2), fma=True)
    assert c["pre"][1].max() < -745.0
    pts, ind, logz = c["got"]
    _close_log(logz, c["logz"])
    assert logz < -700.0 and kdehip.intersIntg(c["p"], c["q"]) < 1e-300
    _check_draws(c, pts, ind, Np, D)


# ---- 2. the call forms agree bit for bit ----------------------------------------------------------------------------------------
def _resident_call(P, Q, Np, D, seed, offset=0):
    import torch
    dev = torch.device("cuda", 0)
    d_pts = torch.full((max(Np, 1), D), 7.0, dtype=torch.float64, device=dev)
    d_ind = torch.full((max(Np, 1), 2), -7, dtype=torch.int64, device=dev)
    d_lz = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    P.prod_exact(Q, d_pts, d_ind, Np=Np, seed=seed, sample_offset=offset, d_logz=d_lz, stream=st.cuda_stream)
    st.synchronize()
    return d_pts.cpu().numpy()[:Np].T, d_ind.cpu().numpy()[:Np].T, float(d_lz.cpu().numpy()[0])


def test_host_resident_and_batched_calls_agree_bit_for_bit():
    import torch
    dev = torch.device("cuda", 0)
    specs = [(2, 127, 129, 1000), (6, 300, 8320, 600), (3, 257, 300, 0), (2, 127, 129, 77)]  # mixed D, sizes, Np; one Np = 0
    cases = [_case(D, N1, N2, Np if Np else 1000, False) for D, N1, N2, Np in specs]
    handles = [(kdehip.DeviceDensity(c["p"]), kdehip.DeviceDensity(c["q"])) for c in cases]
    items, outs = [], []
    for (D, N1, N2, Np), (P, Q) in zip(specs, handles):
        pts = torch.full((max(Np, 1), D), 7.0, dtype=torch.float64, device=dev)
        ind = torch.full((max(Np, 1), 2), -7, dtype=torch.int64, device=dev)
        lz = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
        items.append(dict(p=P, q=Q, Np=Np, pts=pts, ind=ind, logz=lz, seed=SEED))
        outs.append((pts, ind, lz))
    st = torch.cuda.current_stream(dev)
    kdehip.prod_exact_device_batch(items, stream=st.cuda_stream)
    st.synchronize()
    for (D, N1, N2, Np), c, (P, Q), (pts, ind, lz) in zip(specs, cases, handles, outs):
        hp, hi, hl = c["got"] if Np in (600, 1000) else kdehip.prod_exact(c["p"], c["q"], Np, seed=SEED, return_logz=True)
        rp, ri, rl = _resident_call(P, Q, Np, D, SEED)
        bp, bi, bl = pts.cpu().numpy()[:Np].T, ind.cpu().numpy()[:Np].T, float(lz.cpu().numpy()[0])
        assert np.array_equal(hp, rp) and np.array_equal(hi, ri) and hl == rl, (D, N1, N2, Np)
        assert np.array_equal(hp, bp) and np.array_equal(hi, bi) and hl == bl, (D, N1, N2, Np)
        if Np == 0:  # nothing drawn: the arrays keep what they held, logz is still written
            assert (pts.cpu().numpy() == 7.0).all() and (ind.cpu().numpy() == -7).all() and bl == c["got"][2]
        again = kdehip.prod_exact(c["p"], c["q"], Np, seed=SEED, return_logz=True)
        assert np.array_equal(again[0], hp) and np.array_equal(again[1], hi) and again[2] == hl
    kdehip.prod_exact_device_batch([], stream=st.cuda_stream)  # n == 0
    P, Q = handles[0]
    assert _lib.lib.kdehip_prod_exact_device(P._h, Q._h, 0, 1, 0, _lib.addr(outs[0][0]), _lib.addr(outs[0][1]), None,
                                             None) == _lib.KDEHIP_OK  # Np == 0 and no logz: nothing to do
    for P, Q in handles:
        P.close()
        Q.close()


def test_a_captured_call_replays_the_direct_call():
    import torch
    D, N1, N2, Np = 3, 257, 300, 1000
    c = _case(D, N1, N2, Np, False)
    P, Q = kdehip.DeviceDensity(c["p"]), kdehip.DeviceDensity(c["q"])
    dev = torch.device("cuda", 0)
    d_pts = torch.zeros((Np, D), dtype=torch.float64, device=dev)
    d_ind = torch.zeros((Np, 2), dtype=torch.int64, device=dev)
    d_lz = torch.zeros(1, dtype=torch.float64, device=dev)

    def call():
        P.prod_exact(Q, d_pts, d_ind, Np=Np, seed=SEED, d_logz=d_lz, stream=torch.cuda.current_stream().cuda_stream)
    # captured on ONE stream (sequential launches: no parallel branches) and replayed once.  The stream is the test's own,
    # created here and destroyed below, not one of torch's pool: a pool stream stays alive and keeps its hardware queue, and
    # which queue the streams of LATER tests share with the library's preparation stream would depend on this test
    # (tests/test_gpu_stream_order.py holds one stream back and expects a product on another to finish meanwhile)
    hip = C.CDLL(None)  # the HIP runtime the process already has
    raw = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(raw)) == 0
    side = torch.cuda.ExternalStream(raw.value)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        call()
    d_pts.fill_(3.0)
    d_ind.fill_(-3)
    d_lz.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    pts, ind, logz = c["got"]
    assert np.array_equal(d_pts.cpu().numpy().T, pts) and np.array_equal(d_ind.cpu().numpy().T, ind)
    assert float(d_lz.cpu().numpy()[0]) == logz
    del graph, side  # (5h: the captured call's blocks stay in the library's keep list until the next kdehip_clear_cache)
    torch.cuda.synchronize()
    assert hip.hipStreamDestroy(raw) == 0
    P.close()
    Q.close()


# ---- 3. empty sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "p"])
def test_an_empty_set_gives_minus_infinity_zero_labels_and_nan_points(which):
    rng = np.random.default_rng(5)
    p, q = _density(rng, 2, 130), _density(rng, 2, 300)
    empty = q if which == "q" else p
    empty.bt.weights[empty.bt.num_points:] = 0.0  # no leaf carries weight
    pts, ind, logz = kdehip.prod_exact(p, q, 257, seed=SEED, return_logz=True)
    assert logz == -math.inf and not ind.any() and np.isnan(pts).all()
    assert kdehip.log_intersIntg(p, q) == -math.inf
    means, w, sd = kdehip.product_components(p, q)
    assert not w.any() and np.all(np.isfinite(means))


# ---- 4. the mixture itself ---------------------------------------------------------------------------------------------------
def _original(p):
    N, D = p.bt.num_points, p.bt.dims
    return kdehip.getPoints(p), kdehip.getWeights(p), p.bandwidth[N * D:(N + 1) * D].copy()


def test_product_components_equal_the_closed_form():
    rng = np.random.default_rng(43)
    p, q = _density(rng, 2, 4, bw=[0.4, 0.3]), kdehip.kde(rng.standard_normal((2, 3)), [0.5, 0.2], [0.2, 0.5, 0.3])
    means, w, sd = kdehip.product_components(p, q)
    assert means.shape == (2, 12) and w.shape == (12,) and sd.shape == (2,)
    bmeans, bw, blogz = _brute(_original(p), _original(q))
    assert np.all(np.abs(w - bw) <= 1e-12) and np.all(np.abs(means.T - bmeans) <= 1e-12)
    assert abs(math.fsum(w.tolist()) - 1.0) <= 1e-14
    u, v = _original(p)[2], _original(q)[2]
    assert np.all(np.abs(sd - np.sqrt(u * v / (u + v))) <= 1e-15)
    P, Q = kdehip.DeviceDensity(p), kdehip.DeviceDensity(q)
    rm, rw, rs = kdehip.product_components(P, Q)
    assert np.array_equal(rm, means) and np.array_equal(rw, w) and np.array_equal(rs, sd)
    assert abs(kdehip.log_intersIntg(p, q) - blogz) <= 1e-12 * max(1.0, abs(blogz))
    P.close()
    Q.close()


# ---- 5. the fold ---------------------------------------------------------------------------------------------------------------
def test_a_list_of_three_folds_through_the_mixture():
    rng = np.random.default_rng(44)
    p, q, r = _density(rng, 2, 4), _density(rng, 2, 3), _density(rng, 2, 4)
    Np = 500
    pts, ind, logz = kdehip.prod_exact([p, q, r], Np, seed=SEED, return_logz=True)
    means, w, sd = kdehip.product_components(p, q)
    pq = kdehip.kde(means, sd, w)
    pts2, ind2, logz2 = kdehip.prod_exact(pq, r, Np, seed=SEED, return_logz=True)
    assert pts.shape == (2, Np) and ind.shape == (3, Np)
    assert np.array_equal(pts, pts2) and logz == logz2
    for k, n in enumerate((4, 3, 4)):
        assert ind[k].min() >= 1 and ind[k].max() <= n
    assert np.array_equal((ind[0] - 1) * 3 + (ind[1] - 1), ind2[0] - 1) and np.array_equal(ind[2], ind2[1])
    big =_density(rng, 1, 300)
    with pytest.raises(ValueError, match="prodAppxMSGibbsS"):
        kdehip.prod_exact([big, big, big], 10, seed=SEED)


# ---- 6. one statistical check -------------------------------------------------------------------------------------------------
def test_sample_moments_match_the_exact_mixture():
    rng = np.random.default_rng(45)
    p, q = _density(rng, 2, 50), _density(rng, 2, 50, shift=0.5)
    Np = 20000
    pts, ind = kdehip.prod_exact(p, q, Np, seed=SEED)
    mu, va = pm.mixture_moments(_leaf(p)[0], _leaf(q)[0])
    se = np.sqrt(va / Np)
    print("mean: |err| / se", np.abs(pts.mean(axis=1) - mu) / se, " var ratio", pts.var(axis=1) / va)
    assert np.all(np.abs(pts.mean(axis=1) - mu) <= 5.0 * se)
    assert np.all(np.abs(pts.var(axis=1) / va - 1.0) <= 0.05)


# ---- 7. the exact `*` ---------------------------------------------------------------------------------------------------------
def test_mul_exact_builds_a_density_of_the_draws():
    c = _case(2, 127, 129, 1000, False)
    P, Q = kdehip.DeviceDensity(c["p"]), kdehip.DeviceDensity(c["q"])
    out = kdehip.mul_exact(P, Q, Np=200, seed=SEED)
    assert isinstance(out, kdehip.DeviceDensity) and out.num_points == 200 and out.dims == 2
    assert np.array_equal(kdehip.getPoints(out.download()), c["got"][0][:, :200])
    assert out.bw is not None and np.all(np.asarray(out.bw) > 0.0)
    dflt = kdehip.mul_exact(P, Q, seed=SEED)
    assert dflt.num_points == 127
    for d in (out, dflt, P, Q):
        d.close()


# ---- 8. the refusals that read a resident handle ----------------------------------------------------------------------------
def test_resident_refusals():
    import torch
    rng = np.random.default_rng(46)
    p2, p3 = _density(rng, 2, 20), _density(rng, 3, 20)
    var = _density(rng, 2, 20)
    var.bandwidth[(20 + 3) * 2] *= 2.0  # leaf 3 gets a bandwidth of its own
    P2, P3, V = kdehip.DeviceDensity(p2), kdehip.DeviceDensity(p3), kdehip.DeviceDensity(var)
    d = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    di = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    L, a = _lib.lib, _lib.addr

    def err():
        return L.kdehip_last_error().decode()
    assert L.kdehip_prod_exact_device(P2._h, P3._h, 4, 1, 0, a(d), a(di), a(d), None) == _lib.ERR_DIM_MISMATCH
    assert "dimensions of two BallTreeDensities must match" in err()
    for x, y in ((P2, V), (V, P2)):
        assert L.kdehip_prod_exact_device(x._h, y._h, 4, 1, 0, a(d), a(di), a(d), None) == _lib.ERR_UNSUPPORTED and "per-point" in err()
        assert L.kdehip_product_components_device(x._h, y._h, a(d), a(d), a(d), None) == _lib.ERR_UNSUPPORTED and "per-point" in err()
    assert L.kdehip_prod_exact_device(P2._h, P2._h, 4, 1, 0, a(d), None, a(d), None) == _lib.ERR_ARG and "together" in err()
    assert L.kdehip_prod_exact_device(P2._h, P2._h, 4, 1, 0, None, a(di), a(d), None) == _lib.ERR_ARG and "together" in err()
    assert L.kdehip_prod_exact_device(P2._h, P2._h, 4, 1, 0, None, None, None, None) == _lib.ERR_ARG and "null" in err()
    assert L.kdehip_prod_exact_device(P2._h, P2._h, -1, 1, 0, a(d), a(di), a(d), None) == _lib.ERR_ARG and "Np" in err()
    assert L.kdehip_prod_exact_device(P2._h, None, 4, 1, 0, a(d), a(di), a(d), None) == _lib.ERR_ARG and "null density" in err()
    assert L.kdehip_product_components_device(P2._h, P3._h, a(d), a(d), a(d), None) == _lib.ERR_DIM_MISMATCH
    assert L.kdehip_product_components_device(P2._h, P2._h, a(d), None, a(d), None) == _lib.ERR_ARG and "null" in err()
    with pytest.raises(TypeError):
        kdehip.prod_exact(P2, p2)  # host and resident arguments cannot be mixed
    with pytest.raises(TypeError):
        P2.prod_exact(p2, d, di, Np=4, seed=1)
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any() and not di.cpu().numpy().any()  # no refused call wrote anything
    for h in (P2, P3, V):
        h.close()
