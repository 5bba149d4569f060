"""A NaN in a query gives NaN for that query and nothing else; an infinite coordinate gives what the limit demands.

The sweeps cannot see a NaN: csrc/fastexp.hpp's clamp is fmax(x, -800), which returns -800 for a NaN, and the log-domain
kernels' running maximum is an fmax too.  Left to them, `evaluate` answers 0 and the log-domain entries -Inf for a query with
a NaN coordinate -- a confident wrong answer where any fp64 arithmetic gives NaN.  The kernels that finish a query test the
position itself (csrc/pair_sweep.hpp query_has_nan): eval_finish_kernel, eval_finish_log_kernel, moments_init_kernel and
moments_finish_kernel, cond_finish_kernel and cond_weights_kernel.

The rule, for every entry that takes positions from the caller (host, resident and, where there is one, batched):
  * every floating-point output of a query with a NaN coordinate (for the conditionals: a NaN given value) is NaN: value, log
    value, every gradient component, logz, mean, var, the whole weight row, the drawn point; the integer outputs say "nothing
    to report" as they already do elsewhere: ind = 0, and from mean shift iters = 0 with the start returned untouched;
    `condition` refuses (KDEHIP_ERR_ARG), as it refuses a logz of -Inf; `modes` labels the start -1;
  * every OTHER query's outputs are, bit for bit, those of the same call with the NaN replaced by a finite value;
  * host, resident and batch agree bit for bit, NaN included.
+-Inf in a coordinate: `evaluate` 0, `evaluate_log` and logz -Inf, everything else as for a density in which no leaf has a
positive weight (tests/test_gpu_conditional.py test_no_leaf_of_positive_weight, tests/test_gpu_modes.py
test_a_density_without_weight_has_no_gradient_and_does_not_move).

Shapes: N = 700 (six source chunks, the last one partial: several groups), Nq = 257 (two query blocks, the second of one
lane); the NaN query is lane 0 of block 0, the last lane of block 0 or the lone lane of block 1; the NaN sits in the first
coordinate, the last one or all of them."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests.test_gpu_ksum import _density

pytestmark = pytest.mark.gpu

N, NQ = 700, 257
LANES = [0, 255, 256]
WHERE = ["first", "last", "all"]
SEED, OFFSET = 20261019, 1000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """bit for bit, NaN included"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    return np.array_equal(a, b)


def _rows(where, n):
    return [0] if where == "first" else [n - 1] if where == "last" else list(range(n))


def _poison(X, q, where, value=np.nan):
    Y = X.copy()
    Y[_rows(where, X.shape[0]), q] = value
    return Y


def _others(a, q):
    """the array without query q (queries along the last axis)"""
    return np.delete(np.asarray(a), q, axis=-1)


_CASES = {}


def _case(D):
    """one density per D, its queries and the results of every entry at the finite queries: formed once, never changed"""
    if D not in _CASES:
        rng = np.random.default_rng(77 + D)
        p = _density(rng, D, N)
        X = rng.standard_normal((D, NQ))
        c = dict(p=p, X=X, d=kdehip.DeviceDensity(p))
        c["eval"] = kdehip.evaluateDualTree(p, X)
        c["log"] = kdehip.evaluate_log(p, X)
        c["grad"] = {lg: kdehip.evaluate_grad(p, X, log=lg) for lg in (True, False)}
        if D in (2, 6):
            G = [0] if D == 2 else list(range(1, D))
            Y = X[G]
            c.update(G=G, Y=Y, mom=kdehip.conditional_moments(p, G, Y), wts=kdehip.conditional_weights(p, G, Y),
                     draw=kdehip.sample_conditional(p, G, Y, seed=SEED, sample_offset=OFFSET))
        _CASES[D] = c
    return _CASES[D]


# ---- 1. evaluate, evaluate_log -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", LANES)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_evaluate_and_evaluate_log_of_a_nan_query(D, q):
    c = _case(D)
    for where in WHERE[:1] if D == 1 else WHERE:
        Xn = _poison(c["X"], q, where)
        v, lv = kdehip.evaluateDualTree(c["p"], Xn), kdehip.evaluate_log(c["p"], Xn)
        assert math.isnan(v[q]) and math.isnan(lv[q]), (where, v[q], lv[q])
        assert _same(_others(v, q), _others(c["eval"], q)) and _same(_others(lv, q), _others(c["log"], q))
        assert _same(c["d"].evaluate(Xn), v) and _same(c["d"].evaluate_log(Xn), lv)  # resident == host, NaN included


def test_a_nan_in_a_circular_dimension():
    c = _case(3)
    man = [0, 0, 1]
    base, lbase = kdehip.evaluateDualTree(c["p"], c["X"], manifold=man), kdehip.evaluate_log(c["p"], c["X"], manifold=man)
    gbase = kdehip.evaluate_grad(c["p"], c["X"], manifold=man)
    for q in LANES:
        Xn = _poison(c["X"], q, "last")
        v, lv = kdehip.evaluateDualTree(c["p"], Xn, manifold=man), kdehip.evaluate_log(c["p"], Xn, manifold=man)
        val, grad = kdehip.evaluate_grad(c["p"], Xn, manifold=man)
        assert math.isnan(v[q]) and math.isnan(lv[q]) and math.isnan(val[q]) and np.isnan(grad[:, q]).all()
        assert _same(_others(v, q), _others(base, q)) and _same(_others(lv, q), _others(lbase, q))
        assert _same(_others(val, q), _others(gbase[0], q)) and _same(_others(grad, q), _others(gbase[1], q))
        assert _same(c["d"].evaluate(Xn, manifold=man), v) and _same(c["d"].evaluate_log(Xn, manifold=man), lv)
    c2 = _case(2)  # the conditionals: the given dimension is the circular one
    man2 = [1, 0]
    wbase = kdehip.conditional_weights(c2["p"], c2["G"], c2["Y"], manifold=man2)
    dbase = kdehip.sample_conditional(c2["p"], c2["G"], c2["Y"], seed=SEED, sample_offset=OFFSET, manifold=man2)
    Yn = _poison(c2["Y"], 255, "first")
    for dens in (c2["p"], c2["d"]):
        W, lz = kdehip.conditional_weights(dens, c2["G"], Yn, manifold=man2)
        pts, ind = kdehip.sample_conditional(dens, c2["G"], Yn, seed=SEED, sample_offset=OFFSET, manifold=man2)
        assert np.isnan(W[255]).all() and math.isnan(lz[255]) and np.isnan(pts[:, 255]).all() and ind[255] == 0
        assert _same(np.delete(W, 255, axis=0), np.delete(wbase[0], 255, axis=0)) and _same(_others(lz, 255), _others(wbase[1], 255))
        assert _same(_others(pts, 255), _others(dbase[0], 255)) and _same(_others(ind, 255), _others(dbase[1], 255))


# ---- 2. evaluate_grad ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [True, False])
@pytest.mark.parametrize("q", LANES)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_evaluate_grad_of_a_nan_query(D, q, log):
    c = _case(D)
    bval, bgrad = c["grad"][log]
    for where in WHERE[:1] if D == 1 else WHERE:
        Xn = _poison(c["X"], q, where)
        val, grad = kdehip.evaluate_grad(c["p"], Xn, log=log)
        assert math.isnan(val[q]) and np.isnan(grad[:, q]).all(), (where, val[q], grad[:, q])
        assert _same(_others(val, q), _others(bval, q)) and _same(_others(grad, q), _others(bgrad, q))
        rval, rgrad = kdehip.evaluate_grad(c["d"], Xn, log=log)
        assert _same(rval, val) and _same(rgrad, grad)


# ---- 3. mean shift and modes ---------------------------------------------------------------------------------------------------
def _shift_batch(d, starts, tol, niter):
    import torch
    K = starts.shape[1]
    it = dict(density=d, starts=torch.from_numpy(np.ascontiguousarray(starts.T)).to("cuda:0"),
              x=torch.full((K, d.dims), 7.0, dtype=torch.float64, device="cuda:0"),
              logp=torch.full((K,), 7.0, dtype=torch.float64, device="cuda:0"),
              iters=torch.full((K,), -7, dtype=torch.int32, device="cuda:0"))
    kdehip.meanshift_device_batch([it], tol, niter)
    torch.cuda.synchronize()
    return it["x"].cpu().numpy().T, it["logp"].cpu().numpy(), it["iters"].cpu().numpy()


@pytest.mark.parametrize("q", LANES)
@pytest.mark.parametrize("D", [1, 3])
def test_meanshift_from_a_nan_start(D, q):
    c = _case(D)
    tol, niter = 1e-3, 40  # (some starts freeze within the steps given, others are still moving)
    base = kdehip.meanshift(c["p"], c["X"], tol=tol, maxiter=niter)
    for where in WHERE[:1] if D == 1 else WHERE:
        Xn = _poison(c["X"], q, where)
        x, logp, iters = kdehip.meanshift(c["p"], Xn, tol=tol, maxiter=niter)
        assert _same(x[:, q], Xn[:, q]) and math.isnan(logp[q]) and iters[q] == 0, (where, x[:, q], logp[q], iters[q])
        for got, want in zip((x, logp, iters), base):
            assert _same(_others(got, q), _others(want, q))
        assert all(_same(g, w) for g, w in zip(kdehip.meanshift(c["d"], Xn, tol=tol, maxiter=niter), (x, logp, iters)))
        assert all(_same(g, w) for g, w in zip(_shift_batch(c["d"], Xn, tol, niter), (x, logp, iters)))
    # modes: the NaN start belongs to no mode, and the others give what they give without it
    Xn = _poison(c["X"], q, "first")
    m, lp, mass, labels = kdehip.modes(c["p"], Xn, tol=1e-9, maxiter=500)
    m0, lp0, mass0, labels0 = kdehip.modes(c["p"], np.delete(c["X"], q, axis=1), tol=1e-9, maxiter=500)
    assert labels[q] == -1 and np.isfinite(m).all() and np.isfinite(lp).all()
    assert _same(m, m0) and _same(lp, lp0) and np.array_equal(np.delete(labels, q), labels0)
    assert np.array_equal(np.rint(mass * NQ), np.rint(mass0 * (NQ - 1)))


def test_meanshift_with_a_whole_query_block_of_nan_starts():
    """257 starts, all of block 0 NaN: that block is dead from the outset (its live count is 0 and its sweep blocks return at
    once); the one finite start runs to the mode it reaches alone, in the steps it takes alone."""
    c = _case(3)
    Xn = c["X"].copy()
    Xn[:, :256] = np.nan
    alone = kdehip.meanshift(c["p"], c["X"][:, 256:], tol=1e-6, maxiter=5000)
    assert alone[2][0] > 0  # it converges
    for dens in (c["p"], c["d"]):
        x, logp, iters = kdehip.meanshift(dens, Xn, tol=1e-6, maxiter=5000)
        assert np.isnan(x[:, :256]).all() and np.isnan(logp[:256]).all() and not iters[:256].any()
        assert _same(x[:, 256:], alone[0]) and _same(logp[256:], alone[1]) and _same(iters[256:], alone[2])
    got = _shift_batch(c["d"], Xn, 1e-6, int(alone[2][0]) + 3)
    assert all(_same(g, w) for g, w in zip(got, (x, logp, iters)))


# ---- 4. the conditionals -------------------------------------------------------------------------------------------------------
def _cond_batch(d, G, Y, moments):
    import torch
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    Nq, nf = Y.shape[1], d.dims - len(G)
    it = dict(density=d, dims=G, given=torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev), seed=SEED, sample_offset=OFFSET,
              logz=torch.full((Nq,), 7.0, **f64), pts=torch.full((Nq, nf), 7.0, **f64),
              ind=torch.full((Nq,), 7, dtype=torch.int64, device=dev))
    if moments:
        it.update(mean=torch.full((Nq, nf), 7.0, **f64), var=torch.full((Nq, nf), 7.0, **f64))
    kdehip.conditional_device_batch([it])
    torch.cuda.synchronize(dev)
    return {k: it[k].cpu().numpy().T for k in ("logz", "mean", "var", "pts", "ind") if k in it}


@pytest.mark.parametrize("q", LANES)
@pytest.mark.parametrize("D", [2, 6])
def test_the_conditionals_of_a_nan_query(D, q):
    c = _case(D)
    G, ng = c["G"], len(c["G"])  # (ascending: the batch's column order is the caller's)
    for where in WHERE[:1] if ng == 1 else WHERE:
        Yn = _poison(c["Y"], q, where)
        lz, mean, var = kdehip.conditional_moments(c["p"], G, Yn)
        assert math.isnan(lz[q]) and np.isnan(mean[:, q]).all() and np.isnan(var[:, q]).all(), (where, lz[q])
        for got, want in zip((lz, mean, var), c["mom"]):
            assert _same(_others(got, q), _others(want, q))
        W, lz2 = kdehip.conditional_weights(c["p"], G, Yn)
        assert np.isnan(W[q]).all() and _same(lz2, lz)
        assert _same(np.delete(W, q, axis=0), np.delete(c["wts"][0], q, axis=0))
        pts, ind = kdehip.sample_conditional(c["p"], G, Yn, seed=SEED, sample_offset=OFFSET)
        assert np.isnan(pts[:, q]).all() and ind[q] == 0
        assert _same(_others(pts, q), _others(c["draw"][0], q)) and _same(_others(ind, q), _others(c["draw"][1], q))
        assert np.all(_others(ind, q) >= 1)
        # resident and batch
        assert all(_same(g, w) for g, w in zip(kdehip.conditional_moments(c["d"], G, Yn), (lz, mean, var)))
        assert all(_same(g, w) for g, w in zip(kdehip.conditional_weights(c["d"], G, Yn), (W, lz2)))
        assert all(_same(g, w) for g, w in zip(kdehip.sample_conditional(c["d"], G, Yn, seed=SEED, sample_offset=OFFSET), (pts, ind)))
        b = _cond_batch(c["d"], G, Yn, True)
        assert _same(b["logz"], lz) and _same(b["mean"], mean) and _same(b["var"], var) and _same(b["pts"], pts) and _same(b["ind"], ind)
        b = _cond_batch(c["d"], G, Yn, False)  # (an item without moments runs the other branch of the sweep)
        assert _same(b["logz"], lz) and _same(b["pts"], pts) and _same(b["ind"], ind)
        # condition refuses
        for dens in (c["p"], c["d"]):
            with pytest.raises(kdehip.KdeHipError) as e:
                kdehip.condition(dens, G, Yn[:, q])
            assert e.value.code == _lib.ERR_ARG


# ---- 5. +-Inf ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inf", [math.inf, -math.inf])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_an_infinite_coordinate_is_infinitely_far_away(D, inf):
    c = _case(D)
    for q, where in zip(LANES, WHERE):
        if D == 1:
            where = "first"
        Xi = _poison(c["X"], q, where, inf)
        for dens in (c["p"], c["d"]):
            v = dens(Xi) if dens is c["d"] else kdehip.evaluateDualTree(dens, Xi)
            lv = dens.evaluate_log(Xi) if dens is c["d"] else kdehip.evaluate_log(dens, Xi)
            assert v[q] == 0.0 and not np.signbit(v[q]) and lv[q] == -math.inf
            assert _same(_others(v, q), _others(c["eval"], q)) and _same(_others(lv, q), _others(c["log"], q))
            for lg in (True, False):
                val, grad = kdehip.evaluate_grad(dens, Xi, log=lg)
                assert val[q] == (-math.inf if lg else 0.0) and np.all(grad[:, q] == 0.0)
                assert _same(_others(val, q), _others(c["grad"][lg][0], q)) and _same(_others(grad, q), _others(c["grad"][lg][1], q))
            x, logp, iters = kdehip.meanshift(dens, Xi[:, q:q + 1], maxiter=7)
            assert _same(x, Xi[:, q:q + 1]) and logp[0] == -math.inf and iters[0] == 0
    if D == 3:  # a circular dimension: the wrapped difference of an infinite coordinate is NaN, which the sweep drops -- the same answers
        man = [0, 0, 1]
        Xi = _poison(c["X"], 255, "last", inf)
        assert kdehip.evaluateDualTree(c["p"], Xi, manifold=man)[255] == 0.0
        assert kdehip.evaluate_log(c["p"], Xi, manifold=man)[255] == -math.inf
        assert c["d"].evaluate(Xi, manifold=man)[255] == 0.0 and c["d"].evaluate_log(Xi, manifold=man)[255] == -math.inf


@pytest.mark.parametrize("inf", [math.inf, -math.inf])
@pytest.mark.parametrize("D", [2, 6])
def test_the_conditionals_of_an_infinite_query(D, inf):
    """as for a density without a leaf of positive weight: logz = -Inf, mean and var NaN, the point NaN and ind = 0, the
    weight row all 0 (it was 0 / 0 = NaN before the row's S_0 was looked at), and `condition` refuses"""
    c = _case(D)
    G, ng = c["G"], len(c["G"])
    for q, where in zip(LANES, WHERE):
        Yi = _poison(c["Y"], q, where if ng > 1 else "first", inf)
        for dens in (c["p"], c["d"]):
            lz, mean, var = kdehip.conditional_moments(dens, G, Yi)
            assert lz[q] == -math.inf and np.isnan(mean[:, q]).all() and np.isnan(var[:, q]).all()
            for got, want in zip((lz, mean, var), c["mom"]):
                assert _same(_others(got, q), _others(want, q))
            W, lz2 = kdehip.conditional_weights(dens, G, Yi)
            assert not W[q].any() and _same(lz2, lz) and _same(np.delete(W, q, axis=0), np.delete(c["wts"][0], q, axis=0))
            pts, ind = kdehip.sample_conditional(dens, G, Yi, seed=SEED, sample_offset=OFFSET)
            assert np.isnan(pts[:, q]).all() and ind[q] == 0
            assert _same(_others(pts, q), _others(c["draw"][0], q)) and _same(_others(ind, q), _others(c["draw"][1], q))
            with pytest.raises(kdehip.KdeHipError) as e:
                kdehip.condition(dens, G, Yi[:, q])
            assert e.value.code == _lib.ERR_ARG
