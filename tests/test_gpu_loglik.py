"""`evalAvgLogL` / `entropy` / `kld` / `minkld` and the evaluation of resident densities on the GPU (csrc/evaluate.hip,
include/kdehip.h section 5b).

Device evaluation is checked bit for bit against `kdehip_evaluate` on the same host arrays.  The log-likelihoods are
checked against the model  np.dot(W, log(L))  with the reference's zero rule (src/DualTree01.jl:450-470), L from the oracle's
direct evaluation, to |delta| <= 1e-12 * sum_q W_q |log L_q|; the composites, batches and entries against each other bit
for bit."""
import numpy as np
import pytest

import kdehip
from oracle import oracle
from tests import circular_model as cm

pytestmark = pytest.mark.gpu

SHAPES = [(1, 100, 33, False), (2, 257, 300, True), (6, 2048, 2048, False), (8, 50, 7, True), (1, 2, 1, False)]


def _pts(rng, D, N):
    return rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))


def _pair(seed, D, N, Nq, weighted):
    """(host density, OracleDensity of the same inputs, query points, a second density on the query points + its oracle)"""
    rng = np.random.default_rng(seed)
    pts, ks = _pts(rng, D, N), rng.uniform(0.2, 0.6, size=D)
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    pos = _pts(rng, D, Nq)
    wq = rng.uniform(0.05, 1.0, size=Nq) if weighted else None
    ksq = rng.uniform(0.2, 0.6, size=D)
    return (kdehip.kde(pts, ks, w), oracle.OracleDensity(pts, ks, w), pos, kdehip.kde(pos, ksq, wq))


def _model(L, W):
    """evalAvgLogL's arithmetic on L and W (src/DualTree01.jl:456-466) and the tolerance scale sum W |log L|"""
    zero = L == 0.0
    if np.any(W[zero] != 0.0):
        return -np.inf, 0.0
    Ls = np.where(zero, 1.0, L)
    return float(np.dot(np.log(Ls), W)), float(np.dot(np.abs(np.log(Ls)), np.abs(W)))


def _close(got, want, scale):
    if np.isinf(want):
        assert got == want
    else:
        assert abs(got - want) <= 1e-12 * scale + 1e-300, (got, want, scale)


@pytest.mark.parametrize("D,N,Nq,weighted", SHAPES)
def test_device_evaluation_equals_kdehip_evaluate(D, N, Nq, weighted):
    import torch
    p, _, pos, q = _pair(10 * D + N, D, N, Nq, weighted)
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        host = kdehip.evaluateDualTree(p, pos)
        assert np.array_equal(dp.evaluate(pos), host)
        assert np.array_equal(dp(pos), host)
        t = dp.evaluate(torch.from_numpy(pos).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), host)
        loo = kdehip.evaluateDualTree(p, lvFlag=True)
        assert np.array_equal(dp.evaluate(dp), loo)
        assert np.array_equal(dp.evaluate(pos, lvFlag=True), loo)
        # at another density's points: values in ITS original order (getPoints)
        assert np.array_equal(dp.evaluate(dq), kdehip.evaluateDualTree(p, kdehip.getPoints(q)))
        with pytest.raises(ValueError):
            dp.evaluate(np.zeros((D + 1, 3)))


def test_device_evaluation_of_densities_built_on_the_device():
    """a density from from_device_points and the densities of a mul_device_batch block, against their download()"""
    import torch
    rng = np.random.default_rng(4)
    D, N = 2, 300
    pts = _pts(rng, D, N)
    pos = _pts(rng, D, 123)
    flat = torch.from_numpy(np.ascontiguousarray(pts.T).ravel()).to("cuda:0")
    with kdehip.DeviceDensity.from_device_points(flat, D, N) as dd:
        h = dd.download()
        assert np.array_equal(dd.evaluate(pos), kdehip.evaluateDualTree(h, pos))
        assert np.array_equal(dd.evaluate(dd), kdehip.evaluateDualTree(h, lvFlag=True))
        assert kdehip.entropy(dd) == kdehip.entropy(h)
    ins = [kdehip.DeviceDensity(kdehip.kde(_pts(rng, D, 200), [0.3])) for _ in range(3)]
    outs = kdehip.mul_device_batch([[ins[0], ins[1]], [ins[1], ins[2]], [ins[2], ins[0]]], seeds=[1, 2, 3])
    hs = [o.download() for o in outs]
    for k, (o, h) in enumerate(zip(outs, hs)):
        assert np.array_equal(o.evaluate(pos), kdehip.evaluateDualTree(h, pos))
        assert np.array_equal(o.evaluate(o), kdehip.evaluateDualTree(h, lvFlag=True))
        j = (k + 1) % 3  # (another density of the same block)
        assert np.array_equal(o.evaluate(outs[j]), kdehip.evaluateDualTree(h, kdehip.getPoints(hs[j])))
    assert kdehip.kld(outs[0], outs[1]) == kdehip.kld(hs[0], hs[1])
    for d in ins + outs:
        d.close()


@pytest.mark.parametrize("D,N,Nq,weighted", SHAPES)
def test_evalAvgLogL_against_the_model(D, N, Nq, weighted):
    p, o, pos, q = _pair(20 * D + N, D, N, Nq, weighted)
    # at another density's points
    want, scale = _model(oracle.eval_direct(o, kdehip.getPoints(q)), kdehip.getWeights(q))
    got = kdehip.evalAvgLogL(p, q)
    _close(got, want, scale)
    # leave-one-out: the same object
    want_loo, scale_loo = _model(oracle.eval_direct(o, loo=True), kdehip.getWeights(p))
    _close(kdehip.evalAvgLogL(p, p), want_loo, scale_loo)
    # an equal copy is NOT the same object: no leave-one-out
    copy = _pair(20 * D + N, D, N, Nq, weighted)[0]
    want_cp, scale_cp = _model(oracle.eval_direct(o, kdehip.getPoints(p)), kdehip.getWeights(p))
    _close(kdehip.evalAvgLogL(p, copy), want_cp, scale_cp)
    if N > 1:
        assert kdehip.evalAvgLogL(p, copy) != kdehip.evalAvgLogL(p, p)
    # the device entry gives the same bits as the host entry
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert kdehip.evalAvgLogL(dp, dq) == got
        assert kdehip.evalAvgLogL(dp, dp) == kdehip.evalAvgLogL(p, p)
    with pytest.raises(ValueError):
        kdehip.evalAvgLogL(p, kdehip.kde(np.zeros((D + 1, 4)) + np.arange(4), [0.3]))


def test_zero_likelihood_with_weight_is_minus_infinity():
    rng = np.random.default_rng(8)
    p = kdehip.kde(rng.standard_normal((2, 40)) * 0.01, [1e-3])  # exponents near -1e8 at distance 100
    far = kdehip.kde(rng.standard_normal((2, 30)) + 100.0, [0.1])
    assert kdehip.evalAvgLogL(p, far) == -np.inf
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(far) as dfar:
        assert kdehip.evalAvgLogL(dp, dfar) == -np.inf
        assert kdehip.kld(dfar, dp) == np.inf  # evalAvgLogL(far, far) - (-inf)


def test_zero_likelihood_without_weight_counts_as_zero():
    """one `at` point far away with weight 0 (L == 0 exactly: exponent ~ -2e6), every other L > 0: finite, = the model"""
    rng = np.random.default_rng(9)
    src = rng.standard_normal((2, 60))
    p = kdehip.kde(src, [0.5])
    o = oracle.OracleDensity(src, np.array([0.5]))
    at_pts = np.hstack([src[:, :25] + 0.1, np.array([[1000.0], [1000.0]])])
    w = np.ones(26)
    w[-1] = 0.0
    at = kdehip.kde(at_pts, [0.3], w)
    L = oracle.eval_direct(o, kdehip.getPoints(at))
    W = kdehip.getWeights(at)
    assert np.sum(L == 0.0) == 1 and W[L == 0.0][0] == 0.0
    want, scale = _model(L, W)
    got = kdehip.evalAvgLogL(p, at)
    assert np.isfinite(got)
    _close(got, want, scale)
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(at) as dat:
        assert kdehip.evalAvgLogL(dp, dat) == got


@pytest.mark.parametrize("host", [True, False])
def test_composites_are_the_primitive(host):
    p, o, _, q = _pair(31, 3, 400, 250, True)
    if not host:
        p, q = kdehip.DeviceDensity(p), kdehip.DeviceDensity(q)
    e = kdehip.evalAvgLogL
    assert kdehip.entropy(p) == -e(p, p)
    assert kdehip.kld(p, q) == e(p, p) - e(q, p)
    assert kdehip.kld(q, p) == e(q, q) - e(p, q)
    assert kdehip.minkld(p, q) == min(abs(kdehip.kld(p, q)), abs(kdehip.kld(q, p)))
    # identity decides leave-one-out in BOTH terms (src/DualTree01.jl:333, 483): kld(p, p) is the same term twice, 0; against
    # an equal copy the first term is leave-one-out and the second is not -- not 0
    assert kdehip.kld(p, p) == 0.0
    ref = _pair(31, 3, 400, 250, True)[0]
    copy = ref if host else kdehip.DeviceDensity(ref)
    want_loo, s1 = _model(oracle.eval_direct(o, loo=True), kdehip.getWeights(ref))
    want_all, s2 = _model(oracle.eval_direct(o, kdehip.getPoints(ref)), kdehip.getWeights(ref))
    kcp = kdehip.kld(p, copy)
    assert kcp == e(p, p) - e(copy, p)
    assert kcp != 0.0 and (want_loo - want_all) != 0.0
    assert abs(kcp - (want_loo - want_all)) <= 1e-12 * (s1 + s2)


def _batch_pairs(n):
    rng = np.random.default_rng(77)
    pairs = []
    for k in range(n):
        D = 1 + k % 8
        Np, Nq = int(rng.integers(2, 700)), int(rng.integers(2, 700))
        w = rng.uniform(0.1, 1.0, size=Np) if k % 3 == 0 else None
        p = kdehip.kde(_pts(rng, D, Np), rng.uniform(0.2, 0.6, size=D), w)
        q = kdehip.kde(_pts(rng, D, Nq), rng.uniform(0.2, 0.6, size=D))
        pairs.append((p, q))
    return pairs


def test_kld_batch_equals_single_calls_and_is_deterministic():
    import torch
    hosts = _batch_pairs(72)
    devs = [(kdehip.DeviceDensity(p), kdehip.DeviceDensity(q)) for p, q in hosts]
    got = kdehip.kld_batch(devs)
    assert got.shape == (72,)
    singles = np.array([kdehip.kld(p, q) for p, q in devs])
    assert np.array_equal(got, singles)
    assert np.array_equal(kdehip.kld_batch(devs), got)                          # run to run
    assert np.array_equal(np.array([kdehip.kld(p, q) for p, q in hosts]), got)  # host entry == device entry
    assert np.all(np.isfinite(got))
    # the enqueue-only batch on a stream of its own, values after a synchronize
    items = [(p, q) for p, q in devs] + [(p, p) for p, _ in devs]
    out = torch.full((len(items),), np.nan, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        kdehip.eval_avg_logl_device_batch(items, out, stream=st.cuda_stream)
    st.synchronize()
    want = np.array([kdehip.evalAvgLogL(a, b) for a, b in items])
    assert np.array_equal(out.cpu().numpy(), want)
    for p, q in devs:
        p.close()
        q.close()


# Shapes at which a block walks MORE than one source chunk, the only part of the all-pairs sweep (csrc/pair_sweep.hpp) that
# really double-buffers.  split_chunks (csrc/entry_helpers.hpp) deals the ceil(N / 128) chunks to at most 64 groups
# (kEvalMaxGroups), and on the 256 CUs of an MI355X it wants all 64 for any query count up to a few thousand: a group holds
# more than one chunk only when N > 128 * 64.
#   N = 128 * 64 + 1:  65 chunks, 2 per group, 33 groups; the last group is ONE chunk of ONE point, every other group prefetches
#   N = 128 * 128 + 1: 129 chunks, 3 per group: both buffer parities inside a group; the last chunk holds one point
# 257 queries: a second query block with one live lane.  One case has a circular dimension.
SWEEP_NQ = 257
SWEEP_CASES = [(1, 128 * 64 + 1, None), (6, 128 * 64 + 1, None), (1, 128 * 128 + 1, None), (6, 128 * 128 + 1, None),
               (6, 128 * 64 + 1, [0, 0, 1, 0, 0, 0])]


def _sweep_case(D, N, man):
    """points, weights (with exact zeros), standard deviations and SWEEP_NQ queries"""
    if man is None:
        rng = np.random.default_rng(3 * N + D)
        pts, w, sd, pos = _pts(rng, D, N), rng.uniform(0.05, 1.0, size=N), rng.uniform(0.2, 0.6, size=D), _pts(rng, D, SWEEP_NQ)
    else:
        pts, w, sd, pos = cm.circular_case(3 * N + D, D, N, SWEEP_NQ, man, True)
    w[::5] = 0.0
    return pts, w, sd, pos


def _var(p):
    """the variances the library holds for p (its first leaf's)"""
    N, D = p.bt.num_points, p.bt.dims
    return np.array(p.bandwidth[N * D:N * D + D])


@pytest.mark.parametrize("D,N,man", SWEEP_CASES)
def test_groups_of_several_chunks_against_the_model(D, N, man):
    import torch
    pts, w, sd, pos = _sweep_case(D, N, man)
    p, q = kdehip.kde(pts, sd, w), kdehip.kde(pos, [0.3])
    want = cm.eval_direct(pts, w, _var(p), pos, man)
    assert np.all(want > 0.0)
    host = kdehip.evaluateDualTree(p, pos, manifold=man)
    print("evaluate: max relative error", np.max(np.abs(host - want) / want))
    assert np.allclose(host, want, rtol=1e-12, atol=1e-300)
    want_ll, scale = cm.avg_logl(want, np.full(SWEEP_NQ, 1.0 / SWEEP_NQ))  # (q's weights are uniform; a sum has no order)
    e = kdehip.evalAvgLogL(p, q, manifold=man)
    print("evalAvgLogL", e, want_ll, abs(e - want_ll), 1e-12 * scale)
    _close(e, want_ll, scale)
    # host entry == resident entry == a batch whose first item is a small 1-D Euclidean one: the launch of a 6-D or circular
    # item then starts at a block offset (first[0] != 0), and a Euclidean 1-D item is the second of its launch
    small = kdehip.kde(np.array([[0.1, 0.4, -0.3, 0.9, 0.5]]), [0.3])
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq, kdehip.DeviceDensity(small) as ds:
        assert np.array_equal(dp.evaluate(pos, manifold=man), host)
        assert np.array_equal(dp.evaluate(dq, manifold=man), kdehip.evaluateDualTree(p, kdehip.getPoints(q), manifold=man))
        assert kdehip.evalAvgLogL(dp, dq, manifold=man) == e
        out = torch.full((2,), np.nan, dtype=torch.float64, device="cuda:0")
        kdehip.eval_avg_logl_device_batch([(ds, ds), (dp, dq)], out, manifolds=[None, man])
        torch.cuda.synchronize()
        assert out[1].item() == e and out[0].item() == kdehip.evalAvgLogL(small, small)


def test_leave_one_out_with_the_self_term_in_a_groups_second_chunk():
    """N = Nq = 128 * 64 + 1 in 1-D: 33 query blocks, 33 groups of 2 chunks; for half the queries the self term is a point of
    the second chunk its block walks.  The model is evaluated in row blocks (never an N x N array)."""
    N = 128 * 64 + 1
    rng = np.random.default_rng(N)
    pts, w, sd = _pts(rng, 1, N), rng.uniform(0.05, 1.0, size=N), rng.uniform(0.2, 0.6, size=1)
    w[::5] = 0.0
    p = kdehip.kde(pts, sd, w)
    want = np.concatenate([cm.eval_direct(pts, w, _var(p), loo=True, rows=slice(r, r + 1024)) for r in range(0, N, 1024)])
    assert want.shape == (N,) and np.all(want > 0.0)
    loo = kdehip.evaluateDualTree(p, lvFlag=True)
    print("leave-one-out: max relative error", np.max(np.abs(loo - want) / want))
    assert np.allclose(loo, want, rtol=1e-12, atol=1e-300)
    want_ll, scale = cm.avg_logl(want, cm.normalise(w, N))
    e = kdehip.evalAvgLogL(p, p)
    print("evalAvgLogL(p, p)", e, want_ll, abs(e - want_ll), 1e-12 * scale)
    _close(e, want_ll, scale)
    with kdehip.DeviceDensity(p) as dp:
        assert kdehip.evalAvgLogL(dp, dp) == e
        assert np.array_equal(dp.evaluate(dp), loo)
