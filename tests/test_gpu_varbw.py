"""Densities with per-point bandwidths on the GPU (csrc/varbw.hip, include/kdehip.h section 5o): `kde_varbw` through
`evaluateDualTree`, `evaluate_log`, `evalAvgLogL`, `entropy`, `kld`, the resident entries, `kde_adaptive`, `sample` and one
product.

Reference: the NumPy model tests/varbw_model.py.  Tolerance: |delta| <= 1e-12 * max(1, |ref|) for log p and 1e-12 relative
for p, the project's evaluation tolerance -- against the one-bandwidth path the extra error is a few ulp in the folded
normalisers c_i, lc_i.  Routes (host entry, resident `at` form, resident positions, a second run) are compared bit for bit.

Variances are drawn per point and per dimension as sd_k^2 u^2, u in [0.5, 2].  Sizes are those of
tests/test_gpu_logdensity.py: N in {2, 127, 128, 129, 130, 300} (chunk tail, exact chunk, three one-chunk groups), Nq in
{1, 3, 255, 256, 257} (lane tail, second query block), D in {1, 2, 3, 6, 8}; and N = 128 * 64 + 129 with Nq = 3, where a
group walks two chunks and the carried (m, s) is rescaled (64 = kEvalMaxGroups, csrc/entry_helpers.hpp), and
N = 128 * 128 + 129, where it walks three and pair_sweep_var's ring stages a buffer a second time."""
import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import varbw_model as vm
from tests.helpers import assert_chunks_per_group

pytestmark = pytest.mark.gpu

MAX_GROUPS = 64  # kEvalMaxGroups
BIG = 128 * MAX_GROUPS + 129
BIG3 = 128 * 128 + 129  # three chunks per group
SHAPES = [(1, 2, 1), (2, 127, 255), (3, 128, 256), (6, 129, 257), (2, 300, 257), (6, 2, 255), (8, 130, 3), (3, BIG, 3),
          (3, BIG3, 3)]


def _premise(N, Nq):
    """a large shape is here for the chunks a group walks: asserted from the split restated in tests/helpers.py"""
    if N in (BIG, BIG3):
        assert_chunks_per_group(N, Nq, 2 if N == BIG else 3)


def _pts(rng, D, N):
    return rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))


def _case(seed, D, N, Nq, weighted):
    """points, weights, per-point standard deviations (D, N), queries"""
    rng = np.random.default_rng(seed)
    pts, sd = _pts(rng, D, N), rng.uniform(0.2, 0.6, size=D)
    bw = sd[:, None] * rng.uniform(0.5, 2.0, size=(D, N))
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    return pts, w, bw, _pts(rng, D, Nq)


def _var(p):
    """the variances the library holds for p, (D, N) in original order"""
    return _leaf_rows(p, p.bandwidth)


def _leaf_rows(p, arr):
    N, D = p.bt.num_points, p.bt.dims
    out = np.zeros((D, N))
    out[:, p.bt.permutation[N:] - 1] = np.asarray(arr)[N * D:2 * N * D].reshape(N, D).T
    return out


def _close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.all(np.isfinite(want)), what
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: max |delta| / max(1, |ref|) = {err.max():.3e}")
    assert np.all(err <= 1e-12), (what, float(err.max()))


def _close_rel(got, want, what=""):
    """1e-12 relative, with the project's floor of 1e-300 for values at the edge of the fp64 range
    (tests/test_gpu_circular.py: rtol 1e-12, atol 1e-300)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.all(np.isfinite(want)) and np.all(want >= 0.0), what
    big = want > 1e-280
    if big.any():
        print(f"{what}: max relative error = {(np.abs(got - want)[big] / want[big]).max():.3e}")
    assert np.all(np.abs(got - want) <= 1e-12 * want + 1e-300), what


def _close_ll(got, want, what=""):
    """a log-likelihood: -inf where the model's is, else the tolerance of log p"""
    if np.isneginf(want):
        assert got == want, what
    else:
        _close(got, want, what)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D,N,Nq", SHAPES)
def test_values_equal_the_model(D, N, Nq, weighted):
    _premise(N, Nq)
    pts, w, bw, pos = _case(100 * D + N + Nq + weighted, D, N, Nq, weighted)
    p = kdehip.kde_varbw(pts, bw, w)
    var = _var(p)
    assert np.array_equal(var, bw * bw)
    _close(kdehip.evaluate_log(p, pos), vm.eval_log(pts, w, var, pos), "evaluate_log")
    _close_rel(kdehip.evaluateDualTree(p, pos), vm.eval_direct(pts, w, var, pos), "evaluateDualTree")
    _close_rel(p(pos), vm.eval_direct(pts, w, var, pos), "bd(pos)")
    # leave-one-out (N = 2: one source per query; weighted: 1 - w_q differs per point), in original point order; of the
    # large case the model takes a slice of the rows -- never an N x N array
    rows = slice(None) if N < 1000 else slice(0, N, 97)
    _close(kdehip.evaluate_log(p, lvFlag=True)[rows], vm.eval_log(pts, w, var, loo=True, rows=rows), "log, leave-one-out")
    _close_rel(kdehip.evaluateDualTree(p, lvFlag=True)[rows], vm.eval_direct(pts, w, var, loo=True, rows=rows), "leave-one-out")
    if N < 1000:
        for log_domain in (False, True):
            got = kdehip.evalAvgLogL(p, p, log_domain=log_domain)
            _close_ll(got, vm.eval_avg_logl((pts, w, var), log_domain=log_domain), f"evalAvgLogL(p, p), log_domain={log_domain}")
            assert kdehip.entropy(p, log_domain=log_domain) == -got


@pytest.mark.parametrize("D,N,Nq,weighted", [(1, 127, 256, True), (2, 300, 257, False), (6, 129, 255, True)])
def test_a_uniform_density_through_the_new_entries_agrees_with_the_old_ones(D, N, Nq, weighted):
    """to the tolerance, NOT bit for bit: here the normaliser is folded into every source's term (c_i, lc_i), there it is
    applied once after the sum"""
    import ctypes as C
    pts, w, bw, pos = _case(7 * D + N, D, N, Nq, weighted)
    p = kdehip.kde(pts, bw[:, 0], w)
    cd = p._cstruct()
    flat = np.ascontiguousarray(pos.T).ravel()
    for log, old in ((0, kdehip.evaluateDualTree(p, pos)), (1, kdehip.evaluate_log(p, pos))):
        out = np.zeros(Nq)
        _lib.check(_lib.lib.kdehip_evaluate_varbw(C.byref(cd), _lib.ptr(flat, _lib.f64p), Nq, 0, log, _lib.ptr(out, _lib.f64p), 0, None))
        (_close if log else _close_rel)(out, old, f"uniform density, log={log}")
    for log, old in ((0, kdehip.evaluateDualTree(p, lvFlag=True)), (1, kdehip.evaluate_log(p, lvFlag=True))):
        out = np.zeros(N)
        _lib.check(_lib.lib.kdehip_evaluate_varbw(C.byref(cd), None, 0, 1, log, _lib.ptr(out, _lib.f64p), 0, None))
        (_close if log else _close_rel)(out, old, f"uniform density, leave-one-out, log={log}")
    for log in (0, 1):
        res = C.c_double(0.0)
        _lib.check(_lib.lib.kdehip_eval_avg_logl_varbw(C.byref(cd), C.byref(cd), 1, log, C.byref(res), 0, None))
        _close(res.value, kdehip.evalAvgLogL(p, p, log_domain=bool(log)), f"uniform density, evalAvgLogL, log={log}")
    with kdehip.DeviceDensity(p) as dp:
        assert _lib.lib.kdehip_density_uniform_bandwidth(dp._h) == 1
    with kdehip.DeviceDensity(kdehip.kde_varbw(pts, bw, w)) as dv:
        assert _lib.lib.kdehip_density_uniform_bandwidth(dv._h) == 0


def test_one_circular_dimension_wraps():
    rng = np.random.default_rng(21)
    N, Nq = 130, 257
    pts = np.stack([rng.standard_normal(N), np.pi + rng.uniform(-0.2, 0.2, N)])
    pts[1] = np.where(pts[1] >= np.pi, pts[1] - 2 * np.pi, pts[1])  # within 0.2 of +-pi, on both sides of the cut
    pos = np.stack([rng.standard_normal(Nq), np.pi + rng.uniform(-0.2, 0.2, Nq)])
    pos[1] = np.where(pos[1] >= np.pi, pos[1] - 2 * np.pi, pos[1])
    assert np.any(np.abs(pos[1][:, None] - pts[1][None, :]) > np.pi)  # a wrap must occur
    bw = np.array([[0.4], [0.1]]) * rng.uniform(0.5, 2.0, size=(2, N))
    w = rng.uniform(0.05, 1.0, size=N)
    p = kdehip.kde_varbw(pts, bw, w)
    man = [0, 1]
    want = vm.eval_log(pts, w, bw * bw, pos, manifold=man)
    _close(kdehip.evaluate_log(p, pos, manifold=man), want, "circular, log")
    _close_rel(kdehip.evaluateDualTree(p, pos, manifold=man), vm.eval_direct(pts, w, bw * bw, pos, manifold=man), "circular")
    assert not np.allclose(kdehip.evaluate_log(p, pos), want, rtol=1e-6)  # (the wrap is at work in this data)
    _close(kdehip.evaluate_log(p, lvFlag=True, manifold=man), vm.eval_log(pts, w, bw * bw, loo=True, manifold=man), "circular, loo")
    _close(kdehip.evalAvgLogL(p, p, manifold=man, log_domain=True),
           vm.eval_avg_logl((pts, w, bw * bw), manifold=man, log_domain=True), "circular, evalAvgLogL")


def test_edge_queries_and_weightless_sources():
    rng = np.random.default_rng(31)
    D, N = 2, 140
    pts = rng.standard_normal((D, N)) * 0.5
    bw = 0.3 * rng.uniform(0.5, 2.0, size=(D, N))
    w = rng.uniform(0.2, 1.0, size=N)
    pos = rng.standard_normal((D, 5)) * 0.5
    p = kdehip.kde_varbw(pts, bw, w)
    base = kdehip.evaluate_log(p, pos)
    # a zero-weight source right at query 0, with a tiny bandwidth (the largest a_i + lc_i of all if its weight counted)
    pts2 = np.hstack([pts, pos[:, :1]])
    bw2 = np.hstack([bw, np.full((D, 1), 1e-3)])
    w2 = np.concatenate([w, [0.0]])
    p2 = kdehip.kde_varbw(pts2, bw2, w2)
    lp2 = kdehip.evaluate_log(p2, pos)
    _close(lp2, vm.eval_log(pts2, w2, bw2 * bw2, pos), "weightless source")
    _close(lp2, base, "the weighted sources alone")
    _close_rel(p2(pos), p(pos), "weightless source, direct")
    # a NaN query gives NaN, its neighbours are untouched
    bad = pos.copy()
    bad[1, 2] = np.nan
    for got, ref in ((kdehip.evaluate_log(p, bad), base), (p(bad), p(pos))):
        assert np.isnan(got[2]) and np.array_equal(np.delete(got, 2), np.delete(ref, 2))
    # a query at 50: p underflows to 0, log p stays finite
    far = np.full((D, 3), 50.0)
    assert np.all(p(far) == 0.0)
    lp = kdehip.evaluate_log(p, far)
    assert np.all(np.isfinite(lp))
    _close(lp, vm.eval_log(pts, w, bw * bw, far), "a query at 50")
    # ... and the log-likelihoods there: -inf in the direct domain, finite in the log domain
    q = kdehip.kde(far + rng.standard_normal((D, 3)) * 0.01, [0.3])
    qp = kdehip.getPoints(q)
    assert kdehip.evalAvgLogL(p, q) == -np.inf == vm.eval_avg_logl((pts, w, bw * bw), (qp, None))
    _close(kdehip.evalAvgLogL(p, q, log_domain=True), vm.eval_avg_logl((pts, w, bw * bw), (qp, None), log_domain=True), "far evalAvgLogL")
    # kld between two per-point densities
    pts3, w3, bw3, _ = _case(77, D, 129, 1, True)
    r = kdehip.kde_varbw(pts3, bw3, w3)
    for log_domain in (False, True):
        _close(kdehip.kld(p, r, log_domain=log_domain), vm.kld((pts, w, bw * bw), (pts3, w3, bw3 * bw3), log_domain=log_domain),
               f"kld, log_domain={log_domain}")
        _close(kdehip.minkld(p, r, log_domain=log_domain),
               min(abs(vm.kld((pts, w, bw * bw), (pts3, w3, bw3 * bw3), log_domain=log_domain)),
                   abs(vm.kld((pts3, w3, bw3 * bw3), (pts, w, bw * bw), log_domain=log_domain))), "minkld")
    # a per-point density with no weighted point left for a query: -inf there
    one = kdehip.kde_varbw(np.array([[0.0, 1.0], [0.0, 1.0]]), np.array([[0.3, 0.2], [0.3, 0.2]]), np.array([1.0, 0.0]))
    assert kdehip.evaluate_log(one, lvFlag=True)[0] == -np.inf
    assert kdehip.evalAvgLogL(one, one, log_domain=True) == -np.inf


@pytest.mark.parametrize("D,N,Nq", [(2, 300, 257), (6, 129, 255), (3, BIG, 3), (3, BIG3, 3)])
def test_host_entry_resident_calls_and_a_second_run_agree_bit_for_bit(D, N, Nq):
    _premise(N, Nq)
    import torch
    pts, w, bw, pos = _case(9 * D + N, D, N, Nq, True)
    p = kdehip.kde_varbw(pts, bw, w)
    q = kdehip.kde(pos, [0.3])
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        dev = torch.device("cuda", dp.device)
        for log in (False, True):
            host = kdehip.evaluate_log(p, pos) if log else kdehip.evaluateDualTree(p, pos)
            ev = dp.evaluate_log if log else dp.evaluate
            assert np.array_equal(ev(pos), host)                                    # resident, positions from the host
            assert np.array_equal(ev(torch.from_numpy(pos).to(dev)).cpu().numpy(), host)  # ... positions in HBM
            assert np.array_equal(ev(pos), host)                                    # a second run
            hostq = kdehip.evaluate_log(p, q) if log else kdehip.evaluateDualTree(p, q)
            assert np.array_equal(ev(dq), hostq)                                    # the `at` form, at's original order
            loo = kdehip.evaluate_log(p, lvFlag=True) if log else kdehip.evaluateDualTree(p, lvFlag=True)
            assert np.array_equal(ev(dp), loo) and np.array_equal(ev(lvFlag=True), loo)
            assert np.array_equal(kdehip.evaluate_log(p, lvFlag=True) if log else kdehip.evaluateDualTree(p, lvFlag=True), loo)
            for a, b, da, db in ((p, p, dp, dp), (p, q, dp, dq)):
                hv = kdehip.evalAvgLogL(a, b, log_domain=log)
                assert kdehip.evalAvgLogL(da, db, log_domain=log) == hv == kdehip.evalAvgLogL(a, b, log_domain=log)
        assert kdehip.kld(dp, dq, log_domain=True) == kdehip.kld(p, q, log_domain=True)
        assert kdehip.entropy(dp) == kdehip.entropy(p)


def test_one_capture_into_a_graph_and_one_replay():
    import torch
    pts, w, bw, pos = _case(5, 3, 300, 257, True)
    p = kdehip.kde_varbw(pts, bw, w)
    q = kdehip.kde(pos, [0.3])
    want = kdehip.evaluate_log(p, q)
    dp, dq = kdehip.DeviceDensity(p), kdehip.DeviceDensity(q)
    dev = torch.device("cuda", 0)
    out = torch.zeros(257, dtype=torch.float64, device=dev)

    def call():
        _lib.check(_lib.lib.kdehip_evaluate_varbw_device_at(dp._h, dq._h, 0, 1, _lib.addr(out),
                                                            _lib.addr(torch.cuda.current_stream().cuda_stream), None))
    call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    # captured on ONE stream (sequential launches: no parallel branches) and replayed once
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        call()
    out.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    del graph
    dp.close()
    dq.close()
    kdehip._clib.kdehip_clear_cache()  # (5h: the captured call's blocks are kept until here; the graph is gone)


@pytest.mark.parametrize("method", ["abramson", "knn"])
def test_kde_adaptive_on_the_two_scale_sample(method):
    """2-D, N = 300, seed 2, ks = 0.3: a tight mode and a wide tail.  The leave-one-out log-likelihood of the adaptive
    density exceeds the fixed one's; for Abramson's rule the model's gain is 1.65 nats (-2.43 against -4.08)."""
    pts = vm.two_scale_sample(2, 2)
    N = pts.shape[1]
    v1 = np.array([0.3 ** 2, 0.3 ** 2])
    fixed = kdehip.kde(pts, [0.3])
    lam = kdehip.adaptive_scales(fixed, method=method)
    want = vm.scales_abramson(pts, None, v1) if method == "abramson" else vm.scales_knn(pts, None, v1, 8)
    err = np.abs(lam - want) / want
    print(f"{method}: scales, max relative error = {err.max():.3e}")
    assert lam.shape == (N,) and np.all(err <= 1e-10)
    assert abs(np.sum(np.log(lam)) / N) <= 1e-12  # geometric mean 1
    ad = kdehip.kde_adaptive(pts, [0.3], method=method)
    assert ad.multibandwidth == 1
    assert np.allclose(kdehip.getBW(ad), np.outer([0.3, 0.3], lam), rtol=1e-15, atol=0.0)
    h_ad, h_fixed = kdehip.entropy(ad, log_domain=True), kdehip.entropy(fixed, log_domain=True)
    assert h_ad < h_fixed
    m_fixed = vm.entropy((pts, None, vm._uniform_var(v1, N)), log_domain=True)
    m_ad = vm.entropy((pts, None, np.outer(v1, want ** 2)), log_domain=True)
    print(f"{method}: entropy fixed {h_fixed:.6f} (model {m_fixed:.6f}), adaptive {h_ad:.6f} (model {m_ad:.6f})")
    assert abs((h_fixed - h_ad) - (m_fixed - m_ad)) <= 1e-9
    if method == "abramson":
        assert abs((m_fixed - m_ad) - 1.65) < 0.005
        assert abs(kdehip.entropy(ad) - m_ad) <= 1e-9  # (nothing underflows here: the direct domain agrees)


def test_adaptive_scales_refuse_duplicated_points():
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((2, 40))
    pts[:, 1] = pts[:, 0]
    pts[:, 2] = pts[:, 0]
    pilot = kdehip.kde(pts, [0.3])
    with pytest.raises(ValueError, match="3 points"):
        kdehip.adaptive_scales(pilot, method="knn", k=2)
    assert kdehip.adaptive_scales(pilot, method="knn", k=3).shape == (40,)


def test_sample_draws_with_the_leaf_own_bandwidth():
    """same Philox normals, the leaf's own variance: (x - mean_label) / sd_label agrees with the unit-bandwidth twin"""
    x = np.array([[-1.0, 2.0]])
    sd = np.array([[0.1, 2.0]])
    p = kdehip.kde_varbw(x, sd)
    twin = kdehip.kde(x, [1.0])
    labels = np.random.default_rng(4).integers(1, 3, size=500)
    a, la = kdehip.sample(p, 500, ind=labels, seed=99)
    b, lb = kdehip.sample(twin, 500, ind=labels, seed=99)
    assert np.array_equal(la, labels) and np.array_equal(lb, labels)
    za = (a[0] - x[0, labels - 1]) / sd[0, labels - 1]
    zb = b[0] - x[0, labels - 1]
    assert np.abs(za - zb).max() <= 1e-12
    assert np.abs(zb).max() > 2.0  # (normals were drawn)


def test_one_product_of_two_per_point_densities_equals_the_oracle():
    from oracle import oracle
    rng = np.random.default_rng(12)
    D, N, Np, Niter = 2, 64, 64, 2
    dens, odens = [], []
    for j in range(2):
        pts = rng.standard_normal((D, N)) * 0.7 + rng.uniform(-0.5, 0.5, size=(D, 1))
        bw = 0.25 * rng.uniform(0.5, 2.0, size=(D, N))
        v = kdehip.kde_varbw(pts, bw)
        dens.append(v)
        odens.append(oracle.OracleDensity.from_arrays(D, N, v.means, v.bandwidth, v.bt.weights, v.bt.left_child,
                                                      v.bt.right_child, v.bt.permutation))
    with kdehip.ProductPlan(dens) as plan:
        K, R = plan.randu_per_sample(Niter), plan.randn_per_sample()
        randU, randN = kdehip.philox_streams(20260102, 0, Np, K, R)
        g_pts, g_ind = plan.sample(Np, Niter=Niter, seed=20260102)
    o_pts, o_ind = oracle.gibbs1(odens, Np, Niter, randU, randN)
    assert np.array_equal(g_ind, o_ind)
    err = float(np.abs(g_pts - o_pts).max())
    print(f"product of two per-point densities: max |dx| = {err:.3e}")
    assert err <= 1e-12
