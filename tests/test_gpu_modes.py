"""Gradients and joint modes on the GPU (csrc/modes.hip, include/kdehip.h section 5h): `evaluate_grad`, `meanshift`,
`meanshift_device_batch`, `modes` and `getKDEMode` against tests/modes_model.py (fp64, exactly rounded sums), and against
each other bit for bit.

Tolerances, none of them taken from the code under test:
  log p    1e-12 * max(1, |ref|), the bound of tests/test_gpu_logdensity.py; p within 1e-12 * p
  a signed first moment has the scale of its absolute sum A_k = sum_i w_i e^{a_i - m} |d_ik|:
  grad_k   |got - ref| <= 1e-12 * A_k / (S_0 v_k)      a step   |dx_k - ref| <= 1e-12 * A_k / S_0
Where every exponent is huge (the query far from all data) the model forms a_i with the header's one fma per dimension
(modes_model.moments(fma=True), exactly rounded), so the same bounds hold there.
The one-step check reads the stored point, not the step: the roundings of storing it ride on the step's bound, each counted
where it occurs (see the test).
Section 7 repeats the comparisons at N = 128 * 64 + 1 and 128 * 128 + 1, where a group of the sweep walks two and three chunks
and the carried sums are rescaled: what the smaller sizes never run."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import modes_model as mm
from tests.helpers import assert_chunks_per_group, rescale_premise
from tests.test_gpu_ksum import SHAPES, _arrays, _density, _weights

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CONVERGENCE = [(1, 129), (2, 257), (3, 300), (6, 300), (8, 300), (2, 700)]
TOL = 1e-9


def _close_logp(got, want):
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), \
        float(np.max(np.abs(got - want)))


def _close_scaled(got, want, scale, rel=1e-12):
    assert np.all(np.isfinite(got))
    err = np.abs(got - want)
    assert np.all(err <= rel * scale), (float(np.max(err / np.where(scale > 0, scale, 1.0))), rel)


_CASES = {}


def _case(D, N, Nq):
    """a density of one shape, queries inside its range (widened by one bandwidth) and the model's values: built once, shared,
    never changed"""
    key = (D, N, Nq)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * N + Nq)
        p = _density(rng, D, N)
        A = _arrays(p)
        sd = np.sqrt(A[2])[:, None]  # (one bandwidth beyond the extremes: a one-point density has queries off the point)
        lo, hi = A[0].min(axis=1, keepdims=True) - sd, A[0].max(axis=1, keepdims=True) + sd
        X = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(D, Nq))
        _CASES[key] = dict(p=p, A=A, X=X, log=mm.evaluate_grad(A, X), lin=mm.evaluate_grad(A, X, log=False))
    return _CASES[key]


# ---- 1. evaluate_grad ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq", SHAPES)
def test_evaluate_grad_equals_the_model(D, N, Nq):
    c = _case(D, N, Nq)
    val, grad = kdehip.evaluate_grad(c["p"], c["X"])
    assert val.shape == (Nq,) and grad.shape == (D, Nq)
    want, wgrad, scale = c["log"]
    _close_logp(val, want)
    _close_scaled(grad, wgrad, scale)
    p, pgrad = kdehip.evaluate_grad(c["p"], c["X"], log=False)
    want, wgrad, scale = c["lin"]
    assert np.all(want > 0.0)  # (inside the data's range nothing underflows)
    _close_scaled(p, want, want)
    _close_scaled(pgrad, wgrad, scale)
    # resident: the same bits as the host entry
    with kdehip.DeviceDensity(c["p"]) as d:
        for log, (hv, hg) in ((True, (val, grad)), (False, (p, pgrad))):
            dv, dg = kdehip.evaluate_grad(d, c["X"], log=log)
            assert np.array_equal(dv, hv) and np.array_equal(dg, hg)
        dv, dg = d.evaluate_grad(c["X"])
        assert np.array_equal(dv, val) and np.array_equal(dg, grad)


def test_a_query_far_from_all_data():
    D = 6
    c = _case(D, 129, 257)
    x = c["A"][0].max(axis=1, keepdims=True) + 50.0
    p, pgrad = kdehip.evaluate_grad(c["p"], x, log=False)
    assert p[0] == 0.0 and np.all(pgrad == 0.0)
    val, grad = kdehip.evaluate_grad(c["p"], x)
    # (every exponent is in the tens of thousands here: the model forms a_i as the header words it, one fma per dimension,
    # so that what is compared is the sum and not the rounding of the exponents)
    want, wgrad, scale = mm.evaluate_grad(c["A"], x, fma=True)
    m = mm.moments(c["A"], x[:, 0], fma=True)[0]
    assert m < -745.0 and np.all(np.isfinite(wgrad)) and np.all(np.abs(wgrad) > 50.0)
    _close_logp(val, want)
    _close_scaled(grad, wgrad, scale)
    with kdehip.DeviceDensity(c["p"]) as d:
        dv, dg = kdehip.evaluate_grad(d, x)
        assert np.array_equal(dv, val) and np.array_equal(dg, grad)


def test_a_far_weightless_point_does_not_move_the_gradient():
    rng = np.random.default_rng(77)
    D, N = 3, 130
    pts = rng.standard_normal((D, N))
    w = rng.uniform(0.05, 1.0, size=N)
    ks = np.array([0.3, 0.4, 0.5])
    far = np.hstack([pts, np.full((D, 1), 1e3)])
    p, q = kdehip.kde(pts, ks, w), kdehip.kde(far, ks, np.append(w, 0.0))
    X = rng.standard_normal((D, 40))
    want, wgrad, scale = mm.evaluate_grad(_arrays(p), X)
    for d in (p, q):
        val, grad = kdehip.evaluate_grad(d, X)
        _close_logp(val, want)
        _close_scaled(grad, wgrad, scale)
    # ... nor a near one: it neither sets the maximum nor contributes
    near = np.hstack([pts, X[:, :1]])
    val, grad = kdehip.evaluate_grad(kdehip.kde(near, ks, np.append(w, 0.0)), X)
    _close_logp(val, want)
    _close_scaled(grad, wgrad, scale)


def test_a_density_without_weight_has_no_gradient_and_does_not_move():
    pts = np.array([[0.0, 1.0, 2.0]])
    p = kdehip.kde(pts, [0.3], np.array([1.0, 1.0, 1.0]))
    p.bt.weights[:] = 0.0  # (kde normalises: the weights are cleared afterwards; every leaf is weightless)
    val, grad = kdehip.evaluate_grad(p, np.array([[0.5, 5.0]]))
    assert np.all(val == -math.inf) and np.all(grad == 0.0)
    val, grad = kdehip.evaluate_grad(p, np.array([[0.5, 5.0]]), log=False)
    assert np.all(val == 0.0) and np.all(grad == 0.0)
    x, logp, iters = kdehip.meanshift(p, np.array([[0.5, 5.0]]), maxiter=7)
    assert np.array_equal(x, [[0.5, 5.0]]) and np.all(logp == -math.inf) and iters.tolist() == [0, 0]


# ---- 2. one step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("D,N,Nq", SHAPES)
def test_one_step_equals_the_models(D, N, Nq, circular):
    c = _case(D, N, Nq)
    man = ([0] * (D - 1) + [1]) if circular else None
    x, logp, iters = kdehip.meanshift(c["p"], c["X"], tol=0.0, maxiter=1, manifold=man)
    assert x.shape == (D, Nq) and iters.tolist() == [-1] * Nq  # the step was taken and lies above tol = 0
    circ = np.zeros(D, dtype=bool) if man is None else np.asarray(man, dtype=bool)
    for q in range(Nq):
        xn, dx, scale = mm.step(c["A"], c["X"][:, q], man)
        got = c["X"][:, q] - x[:, q]
        got = np.where(circ, mm.wrap(got), got)
        # What is stored is the point, not the step, so these roundings (u = 2^-53 relative each) ride on the step's bound:
        # the kernel's t = x - dx (u |t|), this test's x - x' (u (|x| + |x'|)), and in a circular dimension the two wraps,
        # w(t) = t - 2 pi n with |2 pi n| <= |t| + pi: the product (u (|t| + pi)) and the difference (u |w(t)|) of each.
        X = np.abs(c["X"][:, q])
        t = X + np.abs(dx)
        store = U * (t + X + np.abs(xn))
        store = store + np.where(circ, U * ((t + math.pi + np.abs(xn)) + (X + np.abs(xn) + math.pi + np.abs(dx))), 0.0)
        assert np.all(np.abs(got - dx) <= 1e-12 * scale + store), (q, got, dx, scale, store)
        assert np.all(~circ | ((x[:, q] >= -math.pi) & (x[:, q] < math.pi)))
        assert abs(logp[q] - mm.log_p(c["A"], x[:, q], man)) <= 1e-12 * max(1.0, abs(logp[q]))
    # maxiter = 0: the starts and their log p
    x0, logp0, iters0 = kdehip.meanshift(c["p"], c["X"], tol=0.0, maxiter=0, manifold=man)
    assert np.array_equal(x0, c["X"]) and iters0.tolist() == [0] * Nq
    if man is None:
        _close_logp(logp0, c["log"][0])


# ---- 3. convergence --------------------------------------------------------------------------------------------------------
_CLUSTERS = {}


def _clusters(D, N, shift=None, man=None, tol=TOL):
    """the convergence data, the library's run from its own points and the model's three modes: built once, shared"""
    key = (D, N, None if shift is None else tuple(shift), None if man is None else tuple(man), tol)
    if key not in _CLUSTERS:
        pts, sd, w = mm.three_clusters(D, N, shift)
        p = kdehip.kde(pts, sd, w)
        A = _arrays(p)
        mx, mlogp, mmass, _ = mm.modes(A, tol, 200, man=man)  # the model's own run from every point of the density
        assert mx.shape == (D, 3)
        start_logp = kdehip.meanshift(p, maxiter=0, manifold=man)[1]
        _CLUSTERS[key] = dict(p=p, A=A, sd=sd, model_modes=mx, model_logp=mlogp, model_mass=mmass, start_logp=start_logp,
                              run=kdehip.meanshift(p, tol=tol, maxiter=200, manifold=man),
                              modes=kdehip.modes(p, tol=tol, maxiter=200, manifold=man))
    return _CLUSTERS[key]


def _nearest(modes, model_modes, sd, man=None):
    """per mode: the index of the model's mode it lies within 1e-6 bandwidths of"""
    circ = np.zeros(len(sd), dtype=bool) if man is None else np.asarray(man, dtype=bool)
    out = []
    for j in range(modes.shape[1]):
        d = modes[:, j:j + 1] - model_modes
        d = np.where(circ[:, None], mm.wrap(d), d)
        far = np.max(np.abs(d) / sd[:, None], axis=0)
        assert far.min() <= 1e-6, far
        out.append(int(np.argmin(far)))
    return out


@pytest.mark.parametrize("D,N", CONVERGENCE)
def test_every_start_converges_to_one_of_three_modes(D, N):
    c = _clusters(D, N)
    x, logp, iters = c["run"]
    A, sd = c["A"], c["sd"]
    assert x.shape == (D, N) and np.all(iters > 0) and iters.max() <= 200
    for q in range(N):  # the model's own step at the returned point is within tol
        _, dx, scale = mm.step(A, x[:, q])
        assert np.all(np.abs(dx) / sd <= TOL + 1e-12 * scale / sd), (q, dx)
    assert np.all(logp >= c["start_logp"] - 1e-12 * np.maximum(1.0, np.abs(logp)))
    modes, mlogp, mass, labels = c["modes"]
    assert modes.shape == (D, 3) and np.all(np.diff(mlogp) <= 0.0) and labels.min() == 0 and labels.max() == 2
    match = _nearest(modes, c["model_modes"], sd)
    assert sorted(match) == [0, 1, 2]
    for j in range(3):  # the masses of the model's own run, mode by mode
        assert abs(mass[j] - c["model_mass"][match[j]]) <= 1e-12, (j, mass, c["model_mass"])
    w = A[1]
    assert abs(math.fsum(mass.tolist()) - math.fsum(w.tolist())) <= 1e-12
    assert np.array_equal(kdehip.getKDEMode(c["p"], tol=TOL, maxiter=200), modes[:, 0])


def test_modes_from_given_starts_and_unconverged_starts():
    c = _clusters(2, 257)
    starts = c["A"][0][:, :40]
    modes, mlogp, mass, labels = kdehip.modes(c["p"], starts, tol=TOL, maxiter=200)
    assert modes.shape[1] == 3 and abs(mass.sum() - 1.0) <= 1e-12  # shares of the starts
    assert np.all(np.abs(mass * 40 - np.bincount(labels, minlength=3)) <= 1e-12)
    modes, mlogp, mass, labels = kdehip.modes(c["p"], starts, tol=TOL, maxiter=2)  # nobody converges in two steps
    assert modes.shape == (2, 0) and mass.shape == (0,) and labels.tolist() == [-1] * 40


# ---- 4. freezing and block skipping ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(1, 129), (2, 257), (6, 300), (2, 700)])
def test_a_longer_run_changes_no_bit(D, N):
    c = _clusters(D, N)
    x, logp, iters = kdehip.meanshift(c["p"], tol=TOL, maxiter=100)
    assert np.array_equal(x, c["run"][0]) and np.array_equal(logp, c["run"][1]) and np.array_equal(iters, c["run"][2])
    # ... nor where the run is cut: after 20 steps some starts are frozen and some are not, 1 is a round of one sweep
    for cap in (1, 20):
        xs, ls, its = kdehip.meanshift(c["p"], tol=TOL, maxiter=cap)
        ref = kdehip.meanshift(c["p"], tol=0.0, maxiter=cap)  # (tol = 0: nobody freezes early, every start takes cap steps)
        done = its > 0
        assert np.array_equal(its[~done], ref[2][~done]) and np.array_equal(xs[:, ~done], ref[0][:, ~done])
        assert np.array_equal(xs[:, done], c["run"][0][:, done]) and np.array_equal(its[done], c["run"][2][done])


def test_a_dead_query_block_is_skipped_and_the_last_lane_still_converges():
    c = _clusters(2, 257)
    modes = c["modes"][0]
    lone = modes[:, :1] + np.array([[2.0], [0.0]])
    starts = np.hstack([np.repeat(modes[:, :1], 256, axis=1), lone])
    x, logp, iters = kdehip.meanshift(c["p"], starts, tol=TOL, maxiter=200)
    alone = kdehip.meanshift(c["p"], modes[:, :1], tol=TOL, maxiter=200)
    assert iters[:256].tolist() == [1] * 256 and alone[2].tolist() == [1]
    # the first query block went dead after its first step: nothing wrote it again
    assert np.array_equal(x[:, :256], np.repeat(alone[0], 256, axis=1)) and np.array_equal(logp[:256], np.repeat(alone[1], 256))
    assert np.max(np.abs(x[:, 0] - modes[:, 0]) / c["sd"]) <= TOL
    assert iters[256] > 1
    _nearest(x[:, 256:], c["model_modes"], c["sd"])
    solo = kdehip.meanshift(c["p"], lone, tol=TOL, maxiter=200)
    assert np.array_equal(solo[0], x[:, 256:]) and solo[2][0] == iters[256] and solo[1][0] == logp[256]


# ---- 5. same bits ----------------------------------------------------------------------------------------------------------
def _mixed_items():
    """densities of mixed D and sizes, Euclidean and circular, from given starts and from their own points"""
    rng = np.random.default_rng(5)
    items = []
    for k, (D, N, K) in enumerate([(1, 300, 2), (6, 129, 257), (2, 257, 300), (8, 2, 127), (3, 700, 128), (2, 128, 700),
                                   (6, 1, 1), (1, 129, None), (2, 300, None)]):
        p = _density(rng, D, N)
        man = None if k % 2 == 0 else ([1] + [0] * (D - 1) if k % 4 == 1 else [0] * (D - 1) + [1])
        starts = None if K is None else rng.standard_normal((D, K))
        items.append(dict(p=p, starts=starts, manifold=man))
    return items


def _batch(devs, tol, niter, stream=None):
    import torch
    out = []
    for it in devs:
        d = it["density"]
        K = d.num_points if it["starts"] is None else it["starts"].shape[1]
        out.append(dict(it, x=torch.full((K, d.dims), np.nan, dtype=torch.float64, device="cuda:0"),
                        logp=torch.full((K,), np.nan, dtype=torch.float64, device="cuda:0"),
                        iters=torch.full((K,), -7, dtype=torch.int32, device="cuda:0"),
                        starts=None if it["starts"] is None else torch.from_numpy(np.ascontiguousarray(it["starts"].T)).to("cuda:0")))
    return out


def _results(items):
    return [(it["x"].cpu().numpy().T, it["logp"].cpu().numpy(), it["iters"].cpu().numpy()) for it in items]


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_host_resident_batch_and_graph_replay_give_the_same_bits():
    import torch
    hosts = _mixed_items()
    niter = 12
    ref = [kdehip.meanshift(it["p"], it["starts"], tol=1e-6, maxiter=niter, manifold=it["manifold"]) for it in hosts]
    assert any(np.any(r[2] > 0) for r in ref) and any(np.any(r[2] < 0) for r in ref)  # frozen and live starts both occur
    devs = [dict(density=kdehip.DeviceDensity(it["p"]), starts=it["starts"], manifold=it["manifold"]) for it in hosts]
    for it, r in zip(devs, ref):  # host entry == single resident call
        assert _same(kdehip.meanshift(it["density"], it["starts"], tol=1e-6, maxiter=niter, manifold=it["manifold"]), r)
    for rep in range(2):  # ... == its place in a mixed batch, twice, on a stream of its own
        items = _batch(devs, 1e-6, niter)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            kdehip.meanshift_device_batch(items, 1e-6, niter, stream=st.cuda_stream)
        st.synchronize()
        for got, r in zip(_results(items), ref):
            assert _same(got, r)
    order = [4, 0, 8, 2, 6, 1, 7, 3, 5]  # another order of the same items: every result keeps its bits
    items = _batch([devs[k] for k in order], 1e-6, niter)
    kdehip.meanshift_device_batch(items, 1e-6, niter)
    torch.cuda.synchronize()
    for got, k in zip(_results(items), order):
        assert _same(got, ref[k])
    # in place: the starts are x itself
    inplace = _batch(devs[:3], 1e-6, niter)
    for it in inplace:
        it["x"].copy_(it["starts"])
        it["starts"] = it["x"]
    kdehip.meanshift_device_batch(inplace, 1e-6, niter)
    torch.cuda.synchronize()
    for got, r in zip(_results(inplace), ref[:3]):
        assert _same(got, r)
    # captured in a graph and replayed (sequential launches on one stream: nothing here needs more hardware queues)
    items = _batch(devs, 1e-6, niter)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        kdehip.meanshift_device_batch(items, 1e-6, niter, stream=torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        for it in items:
            it["x"].fill_(np.nan)
            it["logp"].fill_(np.nan)
            it["iters"].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for got, r in zip(_results(items), ref):
            assert _same(got, r)
    del graph
    for it in devs:
        it["density"].close()


def test_resident_arguments_are_refused_before_the_device_is_used():
    import ctypes as C
    import torch
    rng = np.random.default_rng(32)
    p = _density(rng, 2, 130)
    q = _density(rng, 2, 130)
    q.bandwidth[(130 + 3) * 2] *= 2.0  # leaf 3 gets a bandwidth of its own
    L = _lib.lib
    tol, neg = C.byref(C.c_double(1e-9)), C.byref(C.c_double(-1.0))
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        buf = torch.zeros(4 * 130, dtype=torch.float64, device="cuda:0")
        ibuf = torch.zeros(130, dtype=torch.int32, device="cuda:0")
        a = _lib.addr(buf)
        host = np.zeros(260)
        hp, hi = _lib.ptr(host, _lib.f64p), _lib.ptr(np.zeros(130, dtype=np.int32), _lib.i32p)
        bad = np.array([0, 2], dtype=np.uint8)
        assert L.kdehip_evaluate_grad_device(dp._h, a, 3, 1, None, None, None, None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_grad_device(dp._h, a, -1, 1, a, a, None, None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_grad_device(dp._h, a, 3, 1, a, a, _lib.ptr(bad, _lib.u8p), None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_grad_device(dq._h, a, 3, 1, a, a, None, None) == _lib.ERR_UNSUPPORTED
        assert L.kdehip_meanshift_device(dq._h, a, 3, tol, 5, hp, hp, hi, None) == _lib.ERR_UNSUPPORTED
        assert L.kdehip_meanshift_device(dp._h, None, 3, tol, 5, hp, hp, hi, None) == _lib.ERR_ARG  # own points: nstart == npts
        assert L.kdehip_meanshift_device(dp._h, a, 3, neg, 5, hp, hp, hi, None) == _lib.ERR_ARG
        assert L.kdehip_meanshift_device(dp._h, a, 3, tol, 5, hp, hp, hi, _lib.ptr(bad, _lib.u8p)) == _lib.ERR_ARG
        items = (_lib.CMeanshiftItem * 2)()
        for k in range(2):
            items[k].bd, items[k].d_start, items[k].nstart = dp._h, a, 3
            items[k].d_x, items[k].d_logp, items[k].d_iters = a, a, _lib.addr(ibuf)
        items[1].circular_mask = 1 << 2  # a dimension the density does not have
        assert L.kdehip_meanshift_device_batch(2, items, tol, 5, None) == _lib.ERR_ARG
        assert "circular_mask" in L.kdehip_last_error().decode()
        items[1].circular_mask = 0
        items[1].bd = dq._h
        assert L.kdehip_meanshift_device_batch(2, items, tol, 5, None) == _lib.ERR_UNSUPPORTED
        items[1].bd = dp._h
        items[1].d_logp = None
        assert L.kdehip_meanshift_device_batch(2, items, tol, 5, None) == _lib.ERR_ARG
        with pytest.raises(kdehip.KdeHipError) as e:
            kdehip.modes(dq)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()


# ---- 6. circular -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(2, 257), (3, 300)])
def test_clusters_across_the_cut_of_the_circle(D, N):
    man = [1] + [0] * (D - 1)
    shift = np.zeros(D)
    shift[0] = math.pi  # the cluster at 0 now sits across +-pi in dimension 0, the one at +3 e_1 beyond it
    pts, sd, w = mm.three_clusters(D, N, shift)
    assert pts[0].max() > math.pi
    # tol = 1e-13 here: every start then ends within 1e-13 bandwidths of its fixed point, so whichever start founds a mode
    # (their log p are equal to rounding) two runs agree far below the 1e-12 asked for; with the 1e-9 of the other tests the
    # founders may lie 1e-10 apart.  A step's own rounding is some 1e-15 bandwidths, well below this tol.
    tight = 1e-13
    c = _clusters(D, N, shift, man, tight)
    x, logp, iters = c["run"]
    assert np.all(iters > 0)
    modes = c["modes"][0]
    assert modes.shape == (D, 3) and np.all((modes[0] >= -math.pi) & (modes[0] < math.pi))
    assert np.all((x[0] >= -math.pi) & (x[0] < math.pi))
    assert sorted(_nearest(modes, c["model_modes"], sd, man)) == [0, 1, 2]
    moved = np.zeros(D)
    moved[0] = mm.TWO_PI
    again = kdehip.modes(kdehip.kde(pts + moved[:, None], sd, w), tol=tight, maxiter=200, manifold=man)[0]
    d = again - modes
    d[0] = mm.wrap(d[0])
    assert again.shape == modes.shape and np.all(np.abs(d) <= 1e-12)
    assert np.array_equal(kdehip.getKDEMode(c["p"], tol=tight, maxiter=200, manifold=man), modes[:, 0])


def test_circular_data_that_never_wraps_gives_the_euclidean_bits():
    rng = np.random.default_rng(21)
    pts = np.vstack([rng.standard_normal(150) * 0.3, rng.uniform(-1.0, 1.0, size=150)])
    p = kdehip.kde(pts, [0.1], _weights(rng, 150))
    X = np.vstack([rng.standard_normal(140) * 0.3, rng.uniform(-1.0, 1.0, size=140)])
    man = ["euclid", "circular"]
    for log in (True, False):
        a, b = kdehip.evaluate_grad(p, X, log=log), kdehip.evaluate_grad(p, X, log=log, manifold=man)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _same(kdehip.meanshift(p, X, tol=TOL, maxiter=60), kdehip.meanshift(p, X, tol=TOL, maxiter=60, manifold=man))
    with kdehip.DeviceDensity(p) as d:
        d.manifold = np.array([0, 1], dtype=np.uint8)
        assert _same(kdehip.meanshift(d, tol=TOL, maxiter=60, manifold="inherit"), kdehip.meanshift(p, tol=TOL, maxiter=60))


# ---- 7. groups of several chunks -------------------------------------------------------------------------------------------
# The sizes above give every group of the sweep ONE chunk (split_chunks of csrc/entry_helpers.hpp wants all 64 groups on the
# 256 CUs of an MI355X), so `if (cm > m)` of moments_partial_kernel never met carried sums.  Here a group walks two chunks
# (N = 128 * 64 + 1: 65 chunks, the last group one chunk of one leaf) or three (N = 128 * 128 + 1), with 257 queries: a second
# query block with one live lane.  Two premises are asserted before the library is called, the first from the split restated
# in tests/helpers.py, the second from the model's leaf-order arrays alone (helpers.rescale_premise): for a quarter of the
# queries some group has a later chunk that raises the running maximum by log 2 or more over a non-empty earlier one -- the
# carried s[0..D] are scaled by 1/2 or less -- and a maximum within 30 of the query's overall one, so the group counts.
BIG_NQ = 257
BIG_GRAD = [(1, 128 * 64 + 1, None), (6, 128 * 64 + 1, None), (8, 128 * 128 + 1, None), (3, 128 * 64 + 1, (0, 0, 1))]
_BIG = {}


def _leaf_order(p):
    """(points (D, N), weights (N,)) of a host density in LEAF order: the order the sweep's chunks are cut from"""
    N, D = p.bt.num_points, p.bt.dims
    return np.ascontiguousarray(p.bt.centers[N * D:].reshape(N, D).T), p.bt.weights[N:].copy()


def _big(D, N):
    """a density of one large shape and BIG_NQ queries among its points, a bandwidth or so off them: built once, shared, never
    changed"""
    if (D, N) not in _BIG:
        rng = np.random.default_rng(1000 * D + 10 * N + BIG_NQ)
        p = _density(rng, D, N)
        A = _arrays(p)
        sd = np.sqrt(A[2])[:, None]
        X = A[0][:, rng.integers(0, N, size=BIG_NQ)] + sd * rng.standard_normal((D, BIG_NQ))
        _BIG[(D, N)] = dict(p=p, A=A, X=X, leaf=_leaf_order(p))
    return _BIG[(D, N)]


def _assert_the_rescale_fires_and_matters(c, Nq, per_group, man=None, X=None):
    """the two premises of a large case, from the split restated in tests/helpers.py and from the model's arrays alone"""
    N = c["A"][0].shape[1]
    assert_chunks_per_group(N, Nq, per_group)
    pts, w = c["leaf"]
    hit = rescale_premise(pts, w, c["A"][2], c["X"] if X is None else X, per_group, man)
    print("queries with a rescale by <= 1/2 in a group within 30 of the maximum:", int(hit.sum()), "of", hit.size)
    assert hit.mean() >= 0.25, (int(hit.sum()), hit.size)


@pytest.mark.parametrize("D,N,man", BIG_GRAD)
def test_evaluate_grad_with_groups_of_several_chunks(D, N, man):
    c = _big(D, N)
    man = None if man is None else list(man)
    _assert_the_rescale_fires_and_matters(c, BIG_NQ, 2 if N < 128 * 128 else 3, man)
    want, wgrad, scale = mm.evaluate_grad(c["A"], c["X"], man)
    val, grad = kdehip.evaluate_grad(c["p"], c["X"], manifold=man)
    assert val.shape == (BIG_NQ,) and grad.shape == (D, BIG_NQ)
    print("log p: max |delta| / max(1, |ref|)", float(np.max(np.abs(val - want) / np.maximum(1.0, np.abs(want)))),
          "grad: max |delta| / scale", float(np.max(np.abs(grad - wgrad) / scale)))
    _close_logp(val, want)
    _close_scaled(grad, wgrad, scale)
    pw = np.array([math.exp(v) for v in want])  # mm.evaluate_grad(..., log=False) without summing everything again
    lwant, lgrad, lscale = pw, wgrad * pw, scale * pw
    p, pgrad = kdehip.evaluate_grad(c["p"], c["X"], log=False, manifold=man)
    assert np.all(lwant > 0.0)
    _close_scaled(p, lwant, lwant)
    _close_scaled(pgrad, lgrad, lscale)
    with kdehip.DeviceDensity(c["p"]) as d:  # resident: the same bits as the host entry
        for log, (hv, hg) in ((True, (val, grad)), (False, (p, pgrad))):
            dv, dg = kdehip.evaluate_grad(d, c["X"], log=log, manifold=man)
            assert np.array_equal(dv, hv) and np.array_equal(dg, hg)
        if man is None:
            dv, dg = d.evaluate_grad(c["X"])
            assert np.array_equal(dv, val) and np.array_equal(dg, grad)


@pytest.mark.parametrize("D,N,circular", [(2, 128 * 64 + 1, False), (2, 128 * 64 + 1, True), (6, 128 * 128 + 1, False)])
def test_one_step_with_groups_of_several_chunks(D, N, circular):
    """the one-step bound of section 2, where the step item's group walks two chunks (three at N = 128 * 128 + 1)"""
    c = _big(D, N)
    man = ([0] * (D - 1) + [1]) if circular else None
    Nq = BIG_NQ if D == 2 else 40  # (the model sums 4 D + 2 series of N terms by math.fsum per query)
    Xs = c["X"][:, :Nq]
    _assert_the_rescale_fires_and_matters(c, Nq, 2 if N < 128 * 128 else 3, man, Xs)
    x, logp, iters = kdehip.meanshift(c["p"], Xs, tol=0.0, maxiter=1, manifold=man)
    assert x.shape == (D, Nq) and iters.tolist() == [-1] * Nq
    circ = np.zeros(D, dtype=bool) if man is None else np.asarray(man, dtype=bool)
    worst = 0.0
    for q in range(Nq):
        xn, dx, scale = mm.step(c["A"], Xs[:, q], man)
        got = Xs[:, q] - x[:, q]
        got = np.where(circ, mm.wrap(got), got)
        X = np.abs(Xs[:, q])  # (the roundings of storing the point: see test_one_step_equals_the_models)
        t = X + np.abs(dx)
        store = U * (t + X + np.abs(xn))
        store = store + np.where(circ, U * ((t + math.pi + np.abs(xn)) + (X + np.abs(xn) + math.pi + np.abs(dx))), 0.0)
        worst = max(worst, float(np.max(np.abs(got - dx) / (1e-12 * scale + store))))
        assert np.all(np.abs(got - dx) <= 1e-12 * scale + store), (q, got, dx, scale, store)
        assert np.all(~circ | ((x[:, q] >= -math.pi) & (x[:, q] < math.pi)))
        assert abs(logp[q] - mm.log_p(c["A"], x[:, q], man)) <= 1e-12 * max(1.0, abs(logp[q]))
    print("largest |step - model| / bound:", worst)


_BIG_CLUSTERS = {}


def _big_clusters():
    """mm.three_clusters(2, 128 * 64 + 1), eight starts between and beside the clusters, the model's run from them"""
    if not _BIG_CLUSTERS:
        pts, sd, w = mm.three_clusters(2, 128 * 64 + 1)
        p = kdehip.kde(pts, sd, w)
        A = _arrays(p)
        rng = np.random.default_rng(8)
        starts = np.array([[0.0, 3.0, 0.0, 1.2, 1.9, -0.6, 0.3, 3.5], [0.0, 0.0, -3.0, 0.2, -0.3, -1.2, -1.9, 0.6]])
        starts = starts + 0.05 * rng.standard_normal(starts.shape)
        _BIG_CLUSTERS.update(p=p, A=A, sd=sd, starts=starts, leaf=_leaf_order(p), X=starts,
                             model=mm.meanshift(A, starts, TOL, 200))
    return _BIG_CLUSTERS


def _check_run(c, starts, x, logp, iters, model):
    """the bounds of test_every_start_converges_to_one_of_three_modes for a run from given starts: the model's own step at
    the returned point is within tol, the point lies within 1e-6 bandwidths of where the model's run ends, log p is the
    model's there"""
    A, sd = c["A"], c["sd"]
    mx, mlogp, miters, _ = model
    assert np.all(miters > 0) and np.all(iters > 0) and iters.max() <= 200
    for q in range(x.shape[1]):
        _, dx, scale = mm.step(A, x[:, q])
        assert np.all(np.abs(dx) / sd <= TOL + 1e-12 * scale / sd), (q, dx)
        assert abs(logp[q] - mm.log_p(A, x[:, q])) <= 1e-12 * max(1.0, abs(logp[q]))
    far = np.max(np.abs(x - mx) / sd[:, None], axis=0)
    print("largest distance from the model's end points, in bandwidths:", float(far.max()))
    assert far.max() <= 1e-6, far
    start_logp = np.array([mm.log_p(A, starts[:, q]) for q in range(starts.shape[1])])
    assert np.all(logp >= start_logp - 1e-12 * np.maximum(1.0, np.abs(logp)))


def test_the_iteration_with_groups_of_two_chunks_host_resident_and_batch():
    import torch
    c = _big_clusters()
    starts = c["starts"]
    _assert_the_rescale_fires_and_matters(c, starts.shape[1], 2)
    run = kdehip.meanshift(c["p"], starts, tol=TOL, maxiter=200)
    _check_run(c, starts, *run, c["model"])
    assert len(set(np.round(run[0][0] / 3.0).astype(int).tolist())) >= 2  # the starts end in more than one mode
    # the batch's first item is a small 1-D density from its own points: the large item's launch starts at a block offset
    small = kdehip.kde(np.array([[0.1, 0.4, -0.3, 0.9, 0.5]]), [0.3])
    small_run = kdehip.meanshift(small, tol=TOL, maxiter=200)
    with kdehip.DeviceDensity(c["p"]) as d, kdehip.DeviceDensity(small) as ds:
        assert _same(kdehip.meanshift(d, starts, tol=TOL, maxiter=200), run)
        items = _batch([dict(density=ds, starts=None, manifold=None), dict(density=d, starts=starts, manifold=None)], TOL, 200)
        kdehip.meanshift_device_batch(items, TOL, 200)
        torch.cuda.synchronize()
        got = _results(items)
        assert _same(got[0], small_run) and _same(got[1], run)


def test_a_dead_query_block_beside_a_walking_one_with_groups_of_two_chunks():
    """257 starts: the 256 of the first query block sit on a mode and freeze after their first step, so that block's
    `live[...] == 0` early return runs in every later sweep while the last lane's block walks its two chunks per group"""
    c = _big_clusters()
    assert_chunks_per_group(128 * 64 + 1, 257, 2)
    mode = kdehip.meanshift(c["p"], c["model"][0][:, :1], tol=TOL, maxiter=200)[0]
    lone = mode + np.array([[1.5], [0.0]])
    starts = np.hstack([np.repeat(mode, 256, axis=1), lone])
    model = mm.meanshift(c["A"], lone, TOL, 200)
    assert model[2][0] > 1
    x, logp, iters = kdehip.meanshift(c["p"], starts, tol=TOL, maxiter=200)
    alone = kdehip.meanshift(c["p"], mode, tol=TOL, maxiter=200)
    assert iters[:256].tolist() == [1] * 256 and alone[2].tolist() == [1]
    assert np.array_equal(x[:, :256], np.repeat(alone[0], 256, axis=1)) and np.array_equal(logp[:256], np.repeat(alone[1], 256))
    assert iters[256] > 1
    _check_run(c, lone, x[:, 256:], logp[256:], iters[256:], model)
    solo = kdehip.meanshift(c["p"], lone, tol=TOL, maxiter=200)
    assert np.array_equal(solo[0], x[:, 256:]) and solo[2][0] == iters[256] and solo[1][0] == logp[256]
