"""The curvature of a density on the GPU (csrc/modes.hip, include/kdehip.h section 5k): `evaluate_hess`, `laplace`,
`fit_modes`, `getKDEModeFit` and `evaluate_hess_device_batch` against tests/curvature_model.py (fp64, exactly rounded sums),
and against each other bit for bit.

Tolerances, none of them taken from the code under test (the convention of tests/test_gpu_modes.py: a signed sum is judged
against its absolute sum, A_k = sum t_i |d_ik|, A_kl = sum t_i |d_ik d_il|):
  log p     1e-12 * max(1, |ref|)
  grad_k    1e-12 * A_k / (S_0 v_k)
  hess_kl   1e-12 * ( A_kl / (S_0 v_k v_l) + delta_kl / v_k + (A_k / (S_0 v_k)) (A_l / (S_0 v_l)) )
  cov       against numpy.linalg.inv(-hess) of the Hessian the call returned: max|diff| <= 64 * 2^-53 * kappa_2(H) * max|cov|,
            the c D u kappa form of the Cholesky bound with c D = 64 at D <= 8; kappa_2 <= 1e6 is asserted first.
Section 11 repeats the comparisons where a group of the sweep walks two and three chunks (N = 128 * 64 + 1, 128 * 128 + 1)."""
import importlib.util
import math
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import curvature_model as cm
from tests import modes_model as mm
from tests.helpers import assert_chunks_per_group, rescale_premise
from tests.test_gpu_ksum import SHAPES, _arrays, _density

pytestmark = pytest.mark.gpu

ALL_SHAPES = SHAPES + [(4, 130, 3), (5, 130, 3), (7, 130, 3)]  # every D's triangular indexing is run
OUTS = ("logp", "grad", "hess", "cov", "definite")


def _close_logp(got, want):
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), \
        float(np.max(np.abs(got - want)))


def _close_scaled(got, want, scale, rel=1e-12):
    assert np.all(np.isfinite(got))
    err = np.abs(got - want)
    print("max error / scale:", float(np.max(err / np.where(scale > 0, scale, 1.0))), "allowed", rel)
    assert np.all(err <= rel * scale), (float(np.max(err / np.where(scale > 0, scale, 1.0))), rel)


def _check_cov(hess, cov, v=None):
    """cov of one definite query against numpy's inverse of the returned Hessian; with v, cov - diag(v) is PSD to the bound"""
    kappa, bound = cm.cov_bound(hess, cov)
    assert kappa <= 1e6, kappa
    err = float(np.max(np.abs(cov - np.linalg.inv(-hess))))
    print("cov error", err, "bound", bound, "kappa", kappa)
    assert err <= bound, (err, bound, kappa)
    if v is not None:
        assert np.linalg.eigvalsh(cov - np.diag(v)).min() >= -bound


def _all_outputs(p, X, **kw):
    val, grad, hess = kdehip.evaluate_hess(p, X, **kw)
    cov, definite = kdehip.laplace(p, X, **kw)
    return val, grad, hess, cov, definite


def _same(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


_CASES = {}


def _case(D, N, Nq):
    """a density of one shape, queries inside its range (widened by one bandwidth), the model's values and the host entry's
    results: built once, shared, never changed"""
    key = (D, N, Nq)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * N + Nq)
        p = _density(rng, D, N)
        A = _arrays(p)
        sd = np.sqrt(A[2])[:, None]
        lo, hi = A[0].min(axis=1, keepdims=True) - sd, A[0].max(axis=1, keepdims=True) + sd
        X = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(D, Nq))
        _CASES[key] = dict(p=p, A=A, X=X, model=cm.evaluate_hess(A, X), host=_all_outputs(p, X))
    return _CASES[key]


# ---- 1. the model, symmetry, the same bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq", ALL_SHAPES)
def test_evaluate_hess_equals_the_model(D, N, Nq):
    c = _case(D, N, Nq)
    val, grad, hess, cov, definite = c["host"]
    assert val.shape == (Nq,) and grad.shape == (D, Nq) and hess.shape == (D, D, Nq) and cov.shape == (D, D, Nq)
    assert definite.shape == (Nq,) and definite.dtype == bool
    want, wgrad, gscale, whess, hscale = c["model"]
    _close_logp(val, want)
    _close_scaled(grad, wgrad, gscale)
    _close_scaled(hess, whess, hscale)
    assert np.array_equal(hess, hess.transpose(1, 0, 2))  # symmetric bit for bit
    assert np.array_equal(cov, cov.transpose(1, 0, 2), equal_nan=True)
    assert np.all(np.isnan(cov[:, :, ~definite])) and np.all(np.isfinite(cov[:, :, definite]))
    with kdehip.DeviceDensity(c["p"]) as d:  # resident: the host entry's bits
        assert _same(_all_outputs(d, c["X"]), c["host"])
        assert _same(d.evaluate_hess(c["X"]) + d.laplace(c["X"]), c["host"])
    # the linear domain is formed on the host from the log-domain outputs
    p, pgrad, phess = kdehip.evaluate_hess(c["p"], c["X"], log=False)
    assert np.array_equal(p, np.exp(val)) and np.array_equal(pgrad, np.exp(val) * grad)
    assert np.array_equal(phess, np.exp(val) * (hess + grad[:, None, :] * grad[None, :, :]))


def _batch_items(devs, cases, fill=np.nan):
    import torch
    items = []
    for d, c in zip(devs, cases):
        D, Nq = c["X"].shape
        f64 = dict(dtype=torch.float64, device="cuda:0")
        items.append(dict(density=d, pos=torch.from_numpy(np.ascontiguousarray(c["X"].T)).to("cuda:0"),
                          logp=torch.full((Nq,), fill, **f64), grad=torch.full((Nq, D), fill, **f64),
                          hess=torch.full((Nq, D, D), fill, **f64), cov=torch.full((Nq, D, D), 7.0, **f64),
                          definite=torch.full((Nq,), -7, dtype=torch.int32, device="cuda:0")))
    return items


def _batch_results(it):
    return (it["logp"].cpu().numpy(), it["grad"].cpu().numpy().T, it["hess"].cpu().numpy().transpose(1, 2, 0),
            it["cov"].cpu().numpy().transpose(1, 2, 0), it["definite"].cpu().numpy() != 0)


def test_one_batch_of_all_shapes_and_its_graph_replay_give_the_single_calls_bits():
    import torch
    cases = [_case(*s) for s in ALL_SHAPES]
    devs = [kdehip.DeviceDensity(c["p"]) for c in cases]
    items = _batch_items(devs, cases)
    kdehip.evaluate_hess_device_batch(items)
    torch.cuda.synchronize()
    for it, c in zip(items, cases):
        assert _same(_batch_results(it), c["host"])
    order = list(reversed(range(len(cases))))  # another order, a stream of its own, some outputs left out
    items = _batch_items([devs[k] for k in order], [cases[k] for k in order])
    for j, it in enumerate(items):
        if j % 2:
            it["logp"] = it["cov"] = None
        else:
            it["grad"] = it["hess"] = it["definite"] = None
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        kdehip.evaluate_hess_device_batch(items, stream=st.cuda_stream)
    st.synchronize()
    for j, (it, k) in enumerate(zip(items, order)):
        h = cases[k]["host"]
        if j % 2:
            assert _same((it["grad"].cpu().numpy().T, it["hess"].cpu().numpy().transpose(1, 2, 0),
                          it["definite"].cpu().numpy() != 0), (h[1], h[2], h[4]))
        else:
            assert _same((it["logp"].cpu().numpy(), it["cov"].cpu().numpy().transpose(1, 2, 0)), (h[0], h[3]))
    # captured in a graph on ONE stream and replayed twice (sequential launches: no parallel branches)
    items = _batch_items(devs, cases)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        kdehip.evaluate_hess_device_batch(items, stream=torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        for it in items:
            for name in ("logp", "grad", "hess", "cov"):
                it[name].fill_(3.0)
            it["definite"].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for it, c in zip(items, cases):
            assert _same(_batch_results(it), c["host"])
    del graph
    for d in devs:
        d.close()
    kdehip._clib.kdehip_clear_cache()  # (5h: the captured call's blocks are kept until here; the graph is gone)


# ---- 2. closed forms -----------------------------------------------------------------------------------------------------------
def test_one_point_has_the_kernels_curvature_everywhere():
    pts = np.array([[0.25], [-1.25], [0.5]])
    sd = np.array([0.2, 0.3, 0.5])
    p = kdehip.kde(pts, sd)
    rng = np.random.default_rng(2)
    near = pts + sd[:, None] * rng.uniform(-3.0 / math.sqrt(3.0), 3.0 / math.sqrt(3.0), size=(3, 40))  # inside 3 bandwidths
    far = pts + 50.0 * sd[:, None] * np.array([[1.0, -1.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, -1.0]])
    X = np.hstack([pts, near, far])
    A = _arrays(p)
    v = A[2]
    assert np.all(np.abs(v - sd * sd) <= 4 * 2.0 ** -53 * v)
    _, _, _, _, hscale = cm.evaluate_hess(A, X)
    val, grad, hess, cov, definite = _all_outputs(p, X)
    want = np.repeat(-np.diag(1.0 / v)[:, :, None], X.shape[1], axis=2)
    assert hscale[0, 0, -3] > 2000.0 / v[0]  # 50 bandwidths away the two large terms cancel
    _close_scaled(hess, want, hscale)
    assert definite.all()
    for q in range(41):
        _check_cov(hess[:, :, q], cov[:, :, q])
        # ... and diag(v) itself, within the same bound
        kappa, bound = cm.cov_bound(hess[:, :, q], cov[:, :, q])
        err = float(np.max(np.abs(cov[:, :, q] - np.diag(v))))
        print("cov - diag(v)", err, "bound", bound)
        assert err <= bound, (q, err, bound)


@pytest.mark.parametrize("a,sd,wide", [(1.0, 0.5, False), (0.3, 0.5, True), (2.0, 1.5, False), (1.0, 1.5, True)])
def test_two_points_at_plus_and_minus_a(a, sd, wide):
    v = sd * sd
    p = kdehip.kde(np.array([[-a, a]]), [sd])
    val, grad, hess, cov, definite = _all_outputs(p, np.array([[0.0]]))
    A = _arrays(p)
    _, _, _, whess, hscale = cm.evaluate_hess(A, np.array([[0.0]]))
    assert abs(hess[0, 0, 0] - (a * a / (v * v) - 1.0 / v)) <= 1e-12 * hscale[0, 0, 0] and grad[0, 0] == 0.0
    if wide:  # a^2 < v: one mode, wider than the kernel
        assert a * a < v and definite[0]
        want = 1.0 / (1.0 / v - a * a / (v * v))
        # (cov = -1 / H exactly rounded twice; H itself carries 1e-12 * hscale)
        assert abs(cov[0, 0, 0] - want) <= want * want * 1e-12 * hscale[0, 0, 0] + 4 * 2.0 ** -53 * want
        _check_cov(hess[:, :, 0], cov[:, :, 0], np.array([v]))
    else:     # a^2 > v: the minimum between two modes
        assert a * a > v and not definite[0] and np.isnan(cov[0, 0, 0])


# ---- 4. where p underflows ---------------------------------------------------------------------------------------------------
def test_a_query_far_from_all_data():
    c = _case(6, 129, 257)
    x = c["A"][0].max(axis=1, keepdims=True) + 50.0
    val, grad, hess, cov, definite = _all_outputs(c["p"], x)
    want, wgrad, gscale, whess, hscale = cm.evaluate_hess(c["A"], x, fma=True)
    assert cm.moments2(c["A"], x[:, 0], fma=True)[0] < -745.0 and np.exp(val[0]) == 0.0
    assert np.all(np.isfinite(hess))
    _close_logp(val, want)
    _close_scaled(grad, wgrad, gscale)
    _close_scaled(hess, whess, hscale)
    p, pgrad, phess = kdehip.evaluate_hess(c["p"], x, log=False)
    assert p[0] == 0.0 and np.all(pgrad == 0.0) and np.all(phess == 0.0)


# ---- 5. weights ----------------------------------------------------------------------------------------------------------------
def test_a_weightless_leaf_changes_nothing():
    rng = np.random.default_rng(77)
    D, N = 3, 130
    pts = rng.standard_normal((D, N))
    w = rng.uniform(0.05, 1.0, size=N)
    ks = np.array([0.3, 0.4, 0.5])
    X = rng.standard_normal((D, 40))
    p = kdehip.kde(pts, ks, w)
    want, wgrad, gscale, whess, hscale = cm.evaluate_hess(_arrays(p), X)
    far = kdehip.kde(np.hstack([pts, np.full((D, 1), 1e3)]), ks, np.append(w, 0.0))
    near = kdehip.kde(np.hstack([pts, X[:, :1]]), ks, np.append(w, 0.0))  # it neither sets the maximum nor contributes
    for d in (p, far, near):
        val, grad, hess = kdehip.evaluate_hess(d, X)
        _close_logp(val, want)
        _close_scaled(grad, wgrad, gscale)
        _close_scaled(hess, whess, hscale)


def test_a_density_without_weight_has_no_curvature():
    p = kdehip.kde(np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 0.0]]), [0.3], np.array([1.0, 1.0, 1.0]))
    p.bt.weights[:] = 0.0  # (kde normalises: the weights are cleared afterwards; every leaf is weightless)
    val, grad, hess, cov, definite = _all_outputs(p, np.array([[0.5, 5.0], [0.0, 1.0]]))
    assert np.all(val == -math.inf) and np.all(grad == 0.0) and np.all(hess == 0.0)
    assert not definite.any() and np.all(np.isnan(cov))


# ---- 6. NaN queries ------------------------------------------------------------------------------------------------------------
def test_a_nan_query_is_nan_and_its_block_neighbours_are_untouched():
    c = _case(3, 127, 128)
    rng = np.random.default_rng(6)
    X = np.hstack([c["X"], c["X"] + 0.01 * rng.standard_normal(c["X"].shape)])  # one query block of 256
    ref = _all_outputs(c["p"], X)
    Xn = X.copy()
    Xn[1, 100] = math.nan
    got = _all_outputs(c["p"], Xn)
    keep = np.arange(256) != 100
    for g, r in zip(got, ref):
        assert np.array_equal(g[..., keep], r[..., keep], equal_nan=True)
    val, grad, hess, cov, definite = got
    assert math.isnan(val[100]) and np.all(np.isnan(grad[:, 100])) and np.all(np.isnan(hess[:, :, 100]))
    assert np.all(np.isnan(cov[:, :, 100])) and not definite[100]
    with kdehip.DeviceDensity(c["p"]) as d:
        assert _same(_all_outputs(d, Xn), got)


# ---- 7. circular -----------------------------------------------------------------------------------------------------------------
def test_a_cluster_across_the_cut_of_the_circle():
    rng = np.random.default_rng(8)
    N = 150
    pts = np.vstack([mm.wrap(math.pi + 0.3 * rng.standard_normal(N)), 0.5 * rng.standard_normal(N)])
    assert pts[0].min() < -3.0 and pts[0].max() > 3.0  # both signs occur
    w = rng.uniform(0.05, 1.0, size=N)
    sd = np.array([0.2, 0.3])
    man = [1, 0]
    X = np.vstack([mm.wrap(math.pi + 0.3 * rng.standard_normal(30)), 0.5 * rng.standard_normal(30)])
    p = kdehip.kde(pts, sd, w)
    model = cm.evaluate_hess(_arrays(p), X, man)
    got = kdehip.evaluate_hess(p, X, manifold=man)
    _close_logp(got[0], model[0])
    _close_scaled(got[1], model[1], model[2])
    _close_scaled(got[2], model[3], model[4])
    moved = kdehip.kde(pts + np.array([[mm.TWO_PI], [0.0]]), sd, w)  # the same angles, one turn on
    model2 = cm.evaluate_hess(_arrays(moved), X, man)
    got2 = kdehip.evaluate_hess(moved, X, manifold=man)
    _close_logp(got2[0], model2[0])
    _close_scaled(got2[1], model2[1], model2[2])
    _close_scaled(got2[2], model2[3], model2[4])
    # The two runs agree: c = 3 tolerances -- one for each run against the exact sums of its own data, and one for what the
    # rounding of pts + 2 pi does to those sums (a coordinate moves by at most ulp(3 pi) / 2 = 8.9e-16, some 1e-14 of a
    # difference of a bandwidth's size, which moves every term by a few 1e-14 of its scale: well inside 1e-12 of it).
    c = 3.0
    assert np.all(np.abs(got2[0] - got[0]) <= c * 1e-12 * np.maximum(1.0, np.abs(model[0])))
    assert np.all(np.abs(got2[1] - got[1]) <= c * 1e-12 * model[2])
    print("shifted by 2 pi: max |hess difference| / scale", float(np.max(np.abs(got2[2] - got[2]) / model[4])))
    assert np.all(np.abs(got2[2] - got[2]) <= c * 1e-12 * model[4])
    plain = kdehip.evaluate_hess(p, X)  # on the line the cluster is two, 2 pi apart
    assert np.max(np.abs(plain[2] - got[2]) / model[4]) > 1e-3
    with kdehip.DeviceDensity(p) as d:
        assert _same(kdehip.evaluate_hess(d, X, manifold=man), got)
        d.manifold = np.array(man, dtype=np.uint8)
        assert _same(kdehip.evaluate_hess(d, X, manifold="inherit"), got)
        assert _same(d.laplace(X, manifold="inherit"), kdehip.laplace(p, X, manifold=man))


# ---- 8. the covariance -------------------------------------------------------------------------------------------------------
_MODES = {}


def _cluster_modes(D, N):
    """the convergence data of tests/modes_model.py, the library's modes of it and the curvature there: built once, shared"""
    if (D, N) not in _MODES:
        pts, sd, w = mm.three_clusters(D, N)
        p = kdehip.kde(pts, sd, w)
        modes = kdehip.modes(p, maxiter=200)[0]
        assert modes.shape == (D, 3)
        rng = np.random.default_rng(D)
        X = np.hstack([modes, modes + 0.1 * sd[:, None] * rng.standard_normal((D, 3))])  # the modes, and points beside them
        _MODES[(D, N)] = dict(p=p, v=sd * sd, X=X, out=_all_outputs(p, X))
    return _MODES[(D, N)]


@pytest.mark.parametrize("D,N", [(1, 129), (2, 257), (3, 300), (4, 300), (5, 300), (6, 300), (7, 300), (8, 300)])
def test_covariance_is_the_inverse_and_never_narrower_than_the_kernel(D, N):
    c = _cluster_modes(D, N)
    val, grad, hess, cov, definite = c["out"]
    assert definite.all()
    for q in range(c["X"].shape[1]):
        _check_cov(hess[:, :, q], cov[:, :, q], c["v"])
    model_cov, model_def = cm.laplace(_arrays(c["p"]), c["X"])
    assert model_def.all()


# ---- 9. central differences of the GPU's own gradient ---------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq", [(1, 128, 129), (3, 127, 128), (6, 129, 257), (8, 128, 127), (7, 130, 3)])
def test_hessian_is_the_central_difference_of_evaluate_grad(D, N, Nq):
    c = _case(D, N, Nq)
    hess, hscale = c["host"][2], c["model"][4]
    sd = np.sqrt(c["A"][2])
    for l in range(D):
        e = np.zeros((D, 1))
        e[l] = 1e-5 * sd[l]
        fd = (kdehip.evaluate_grad(c["p"], c["X"] + e)[1] - kdehip.evaluate_grad(c["p"], c["X"] - e)[1]) / (2.0 * e[l])
        _close_scaled(hess[:, l, :], fd, hscale[:, l, :], rel=1e-6)


# ---- 10. a Gaussian per mode ---------------------------------------------------------------------------------------------
def _timing_clusters():
    spec = importlib.util.spec_from_file_location(
        "time_modes", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "time_modes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.clusters


def test_fit_modes_gives_a_gaussian_per_mode():
    pts = _timing_clusters()(np.random.default_rng(7), 3, 300)
    p = kdehip.kde(pts, [0.4])
    modes, logp, mass, labels = kdehip.modes(p)
    means, covs, fmass, flogp, definite = kdehip.fit_modes(p)
    assert means.shape == (3, 3) and covs.shape == (3, 3, 3) and definite.all() and definite.dtype == bool
    assert np.array_equal(means, modes) and np.array_equal(fmass, mass) and np.array_equal(flogp, logp)
    cov, d2 = kdehip.laplace(p, means)
    assert np.array_equal(covs, cov) and np.array_equal(definite, d2)
    for j in range(3):  # a cluster of sd 0.3 under a bandwidth of 0.4: between the kernel's variance and the sum of both
        ev = np.linalg.eigvalsh(covs[:, :, j])
        assert ev.min() >= 0.16 * (1.0 - 1e-12) and ev.max() < 2.0 * (0.09 + 0.16)
    with kdehip.DeviceDensity(p) as d:
        for got in (kdehip.fit_modes(d), d.fit_modes()):
            assert _same(got, (means, covs, fmass, flogp, definite))
    mode, mcov = kdehip.getKDEModeFit(p)
    assert np.array_equal(mode, means[:, 0]) and np.array_equal(mcov, covs[:, :, 0])
    assert np.array_equal(mode, kdehip.getKDEMode(p))


def test_a_batch_refuses_tensors_of_another_type_or_layout():
    import torch
    c = _case(3, 127, 128)
    with kdehip.DeviceDensity(c["p"]) as d:
        def item(**kw):
            it = _batch_items([d], [c])[0]
            it.update(kw)
            return it
        f32 = dict(dtype=torch.float32, device="cuda:0")
        for bad in (item(hess=torch.zeros((128, 3, 3), **f32)), item(cov=torch.zeros((256, 3, 3), **f32)),
                    item(definite=torch.zeros(128, dtype=torch.int64, device="cuda:0")),
                    item(logp=torch.zeros(128, dtype=torch.float64)),            # on the host
                    item(grad=torch.zeros((3, 128), dtype=torch.float64, device="cuda:0").t()),  # not contiguous
                    item(pos=torch.zeros((128, 3), **f32))):
            with pytest.raises(ValueError):
                kdehip.evaluate_hess_device_batch([bad])
        torch.cuda.synchronize()


# ---- the refusals that read a resident handle ------------------------------------------------------------------------------
def test_resident_arguments_are_refused_before_the_device_is_used():
    import torch
    rng = np.random.default_rng(32)
    p = _density(rng, 2, 130)
    q = _density(rng, 2, 130)
    q.bandwidth[(130 + 3) * 2] *= 2.0  # leaf 3 gets a bandwidth of its own
    L = _lib.lib
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        buf = torch.zeros(4 * 130, dtype=torch.float64, device="cuda:0")
        ibuf = torch.zeros(130, dtype=torch.int32, device="cuda:0")
        a, ia = _lib.addr(buf), _lib.addr(ibuf)
        bad = np.array([0, 2], dtype=np.uint8)
        assert L.kdehip_evaluate_hess_device(dp._h, a, 3, None, None, None, None, None, None, None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_hess_device(dp._h, a, -1, a, a, a, a, ia, None, None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_hess_device(dp._h, None, 3, a, a, a, a, ia, None, None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_hess_device(dp._h, a, 3, a, a, a, a, ia, _lib.ptr(bad, _lib.u8p), None) == _lib.ERR_ARG
        assert L.kdehip_evaluate_hess_device(dq._h, a, 3, a, a, a, a, ia, None, None) == _lib.ERR_UNSUPPORTED
        assert L.kdehip_evaluate_hess_device(dp._h, a, 0, a, a, a, a, ia, None, None) == _lib.KDEHIP_OK
        items = (_lib.CHessItem * 2)()
        for k in range(2):
            items[k].bd, items[k].d_pos, items[k].Nq = dp._h, a, 3
            items[k].d_logp, items[k].d_hess, items[k].d_definite = a, a, ia
        items[1].circular_mask = 1 << 2  # a dimension the density does not have
        assert L.kdehip_evaluate_hess_device_batch(2, items, None) == _lib.ERR_ARG
        assert "circular_mask" in L.kdehip_last_error().decode()
        items[1].circular_mask = 0
        items[1].bd = dq._h
        assert L.kdehip_evaluate_hess_device_batch(2, items, None) == _lib.ERR_UNSUPPORTED
        items[1].bd = dp._h
        items[1].Nq = -1
        assert L.kdehip_evaluate_hess_device_batch(2, items, None) == _lib.ERR_ARG
        items[1].Nq = 3
        items[1].d_logp = items[1].d_hess = items[1].d_definite = None  # nothing asked for
        assert L.kdehip_evaluate_hess_device_batch(2, items, None) == _lib.ERR_ARG
        with pytest.raises(kdehip.KdeHipError) as e:
            kdehip.laplace(dq, np.zeros((2, 3)))
        assert e.value.code == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()


# ---- 11. groups of several chunks ------------------------------------------------------------------------------------------
# Every size above gives a group of the sweep ONE chunk, so the rescale of curvature_partial_kernel's 1 + D + D(D+1)/2 carried
# sums (45 at D = 8) by exp_nonpos(m - cm) never met a non-zero sum.  N = 128 * 64 + 1 gives a group two chunks (the last
# group one chunk of one leaf), N = 128 * 128 + 1 three.  The premises are those of tests/test_gpu_modes.py section 7, asserted
# before the library is called: the split restated in tests/helpers.py, and from the model's leaf-order arrays alone that for
# a quarter of the queries a group both rescales its carried sums by 1/2 or less and lies within 30 of the overall maximum.
# Nq is small where D is large: the model sums 2 (1 + D + D(D+1)/2) series per query by math.fsum.
BIG_HESS = [(8, 128 * 64 + 1, 7, None), (3, 128 * 128 + 1, 257, None), (5, 128 * 64 + 1, 7, None),
            (3, 128 * 64 + 1, 7, (0, 0, 1))]


def _leaf_order(p):
    """(points (D, N), weights (N,)) of a host density in LEAF order: the order the sweep's chunks are cut from"""
    N, D = p.bt.num_points, p.bt.dims
    return np.ascontiguousarray(p.bt.centers[N * D:].reshape(N, D).T), p.bt.weights[N:].copy()


@pytest.mark.parametrize("D,N,Nq,man", BIG_HESS)
def test_evaluate_hess_with_groups_of_several_chunks(D, N, Nq, man):
    import torch
    man = None if man is None else list(man)
    rng = np.random.default_rng(1000 * D + 10 * N + Nq)
    p = _density(rng, D, N)
    A = _arrays(p)
    X = A[0][:, rng.integers(0, N, size=Nq)] + np.sqrt(A[2])[:, None] * rng.standard_normal((D, Nq))  # among the points
    per_group = 2 if N < 128 * 128 else 3
    assert_chunks_per_group(N, Nq, per_group)
    pts, w = _leaf_order(p)
    hit = rescale_premise(pts, w, A[2], X, per_group, man)
    print("queries with a rescale by <= 1/2 in a group within 30 of the maximum:", int(hit.sum()), "of", hit.size)
    assert hit.mean() >= 0.25, (int(hit.sum()), hit.size)
    want, wgrad, gscale, whess, hscale = cm.evaluate_hess(A, X, man)
    host = _all_outputs(p, X, manifold=man)
    val, grad, hess, cov, definite = host
    assert val.shape == (Nq,) and grad.shape == (D, Nq) and hess.shape == (D, D, Nq) and cov.shape == (D, D, Nq)
    _close_logp(val, want)
    _close_scaled(grad, wgrad, gscale)
    _close_scaled(hess, whess, hscale)
    assert np.array_equal(hess, hess.transpose(1, 0, 2)) and np.array_equal(cov, cov.transpose(1, 0, 2), equal_nan=True)
    assert np.all(np.isnan(cov[:, :, ~definite])) and np.all(np.isfinite(cov[:, :, definite]))
    for q in range(Nq):  # definite where the model's -H is safely so (its smallest eigenvalue above the Hessian's own bound)
        ev = np.linalg.eigvalsh(-whess[:, :, q])
        margin = D * 1e-12 * float(np.max(hscale[:, :, q]))
        if ev.min() > margin:
            assert definite[q]
            _check_cov(hess[:, :, q], cov[:, :, q], None if man is not None else A[2])
        elif ev.min() < -margin:
            assert not definite[q]
    # host == resident == its place in a batch whose first item is small: the large item's launch starts at a block offset
    small = _case(3, 127, 128)
    with kdehip.DeviceDensity(p) as d, kdehip.DeviceDensity(small["p"]) as ds:
        assert _same(_all_outputs(d, X, manifold=man), host)
        items = _batch_items([ds, d], [small, dict(X=X)])
        items[1]["manifold"] = man
        kdehip.evaluate_hess_device_batch(items)
        torch.cuda.synchronize()
        assert _same(_batch_results(items[0]), small["host"]) and _same(_batch_results(items[1]), host)


def test_a_mode_covariance_with_groups_of_two_chunks():
    """section 8 on mm.three_clusters(2, 128 * 64 + 1): the modes from eight starts, the curvature at them"""
    N = 128 * 64 + 1
    pts, sd, w = mm.three_clusters(2, N)
    p = kdehip.kde(pts, sd, w)
    A = _arrays(p)
    starts = np.array([[0.0, 3.0, 0.0, 1.2, 1.9, -0.6, 0.3, 3.5], [0.0, 0.0, -3.0, 0.2, -0.3, -1.2, -1.9, 0.6]])
    assert_chunks_per_group(N, starts.shape[1], 2)
    assert_chunks_per_group(N, 3, 2)
    modes = kdehip.modes(p, starts, maxiter=200)[0]
    assert modes.shape == (2, 3)
    lpts, lw = _leaf_order(p)
    hit = rescale_premise(lpts, lw, A[2], modes, 2)
    assert hit.any(), hit
    val, grad, hess, cov, definite = _all_outputs(p, modes)
    want, wgrad, gscale, whess, hscale = cm.evaluate_hess(A, modes)
    _close_logp(val, want)
    _close_scaled(grad, wgrad, gscale)
    _close_scaled(hess, whess, hscale)
    assert definite.all()
    for q in range(3):
        _check_cov(hess[:, :, q], cov[:, :, q], sd * sd)
    means, covs, fmass, flogp, fdef = kdehip.fit_modes(p, starts, maxiter=200)
    assert np.array_equal(means, modes) and np.array_equal(covs, cov) and fdef.all()
