"""Log-domain evaluation on the GPU (csrc/evaluate.hip eval_partial_log_kernel / eval_finish_log_kernel, include/kdehip.h
section 5f): `evaluate_log`, and `evalAvgLogL` / `kld` with `log_domain=True`.

Reference: the NumPy model tests/logdensity_model.py (pinned against the oracle in tests/test_logdensity_host.py).
Tolerance: |delta| <= 1e-12 * max(1, |ref|), the project's evaluation tolerance carried to the log -- the exponent a_i is a
handful of fmas on inputs both sides share, a few ulp of |a_i|, and log p is m plus a term of order 1.  Routes (host entry,
resident call, `at` form, batch, a second run) are compared bit for bit.

Sizes: N in {2, 127, 128, 129, 300} (chunk tail, exact chunk, three one-chunk groups), Nq in {1, 255, 256, 257} (lane tail,
second query block), D in {1, 2, 3, 6}; and N = 128 * 64 + 129 with Nq = 3, where a group walks two chunks and the carried
(m, s) is rescaled (64 = kEvalMaxGroups, csrc/entry_helpers.hpp)."""
import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import circular_model as cm
from tests import logdensity_model as lm

pytestmark = pytest.mark.gpu

MAX_GROUPS = 64  # kEvalMaxGroups
SHAPES = [(1, 2, 1, False), (2, 127, 255, True), (3, 128, 256, False), (6, 129, 257, True), (2, 300, 257, False),
          (1, 300, 1, True), (6, 2, 255, True), (3, 128 * MAX_GROUPS + 129, 3, True)]


def _pts(rng, D, N):
    return rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))


def _var(p):
    """the variances the library holds for p (its first leaf's)"""
    N, D = p.bt.num_points, p.bt.dims
    return np.array(p.bandwidth[N * D:N * D + D])


def _case(seed, D, N, Nq, weighted):
    rng = np.random.default_rng(seed)
    pts, sd = _pts(rng, D, N), rng.uniform(0.2, 0.6, size=D)
    w = rng.uniform(0.05, 1.0, size=N) if weighted else None
    return pts, w, sd, _pts(rng, D, Nq)


def _close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.all(np.isfinite(want)), what
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: max |delta| / max(1, |ref|) = {err.max():.3e}")
    assert np.all(err <= 1e-12), (what, float(err.max()))


@pytest.mark.parametrize("D,N,Nq,weighted", SHAPES)
def test_evaluate_log_equals_the_model(D, N, Nq, weighted):
    pts, w, sd, pos = _case(100 * D + N + Nq, D, N, Nq, weighted)
    p = kdehip.kde(pts, sd, w)
    var = _var(p)
    _close(kdehip.evaluate_log(p, pos), lm.eval_log(pts, w, var, pos), "evaluate_log")
    # leave-one-out (N = 2: one source per query; weighted: log(1 - w_q) differs per point), original point order
    _close(kdehip.evaluate_log(p, lvFlag=True), lm.eval_log(pts, w, var, loo=True), "leave-one-out")
    got = kdehip.evalAvgLogL(p, p, log_domain=True)
    want, _ = lm.eval_avg_logl_log((pts, w, var))
    _close(got, want, "evalAvgLogL(p, p)")
    assert kdehip.entropy(p, log_domain=True) == -got


def _far_clusters():
    """p around the origin with sd 0.05; q2 the same shape 100 sd away (a ~ -5000), q1 200 sd away"""
    rng = np.random.default_rng(5)
    D, N = 2, 130
    base = rng.standard_normal((D, N)) * 0.05
    sd = np.array([0.05, 0.05])
    shift = np.array([[5.0], [0.0]])
    mk = lambda x: kdehip.kde(x, sd)
    return (base, mk(base)), (base + 2 * shift, mk(base + 2 * shift)), (base + shift, mk(base + shift)), sd ** 2


def test_underflow_is_the_point():
    (ppts, p), (q1pts, q1), (q2pts, q2), _ = _far_clusters()
    var = _var(p)
    assert np.all(p(q2pts) == 0.0) and np.all(p(q1pts) == 0.0)  # the direct sum underflows: the case means something
    for at in (q2pts, q1pts):
        lp = kdehip.evaluate_log(p, at)
        assert np.all(np.isfinite(lp)) and np.all(lp < -4000.0)
        _close(lp, lm.eval_log(ppts, None, var, at), "evaluate_log, 100+ sd away")
    assert kdehip.evalAvgLogL(p, q2) == -np.inf
    got = kdehip.evalAvgLogL(p, q2, log_domain=True)
    want, _ = lm.eval_avg_logl_log((ppts, None, var), (q2pts, None, None))
    assert np.isfinite(got)
    _close(got, want, "evalAvgLogL(p, q2), log domain")
    assert not np.isfinite(kdehip.kld(p, q2))
    k1, k2 = kdehip.kld(p, q1, log_domain=True), kdehip.kld(p, q2, log_domain=True)
    assert np.isfinite(k1) and np.isfinite(k2)
    assert k1 > k2  # q1 is the farther copy
    _close(k2, lm.kld_log((ppts, None, var), (q2pts, None, _var(q2))), "kld(p, q2)")
    _close(k1, lm.kld_log((ppts, None, var), (q1pts, None, _var(q1))), "kld(p, q1)")
    assert kdehip.minkld(p, q1, log_domain=True) > kdehip.minkld(p, q2, log_domain=True)
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q1) as d1, kdehip.DeviceDensity(q2) as d2:
        assert kdehip.kld(dp, d1, log_domain=True) == k1 and kdehip.kld(dp, d2, log_domain=True) == k2
        assert np.array_equal(kdehip.kld_batch([(dp, d1), (dp, d2)], log_domain=True), np.array([k1, k2]))


@pytest.mark.parametrize("D,N,Nq,weighted", [(1, 127, 256, True), (2, 300, 257, False), (6, 129, 255, True)])
def test_agreement_with_the_direct_entries_where_nothing_underflows(D, N, Nq, weighted):
    pts, w, sd, pos = _case(7 * D + N, D, N, Nq, weighted)
    p = kdehip.kde(pts, sd, w)
    direct = kdehip.evaluateDualTree(p, pos)
    assert np.all(direct > 1e-200)
    _close(kdehip.evaluate_log(p, pos), np.log(direct), "evaluate_log against log(evaluate)")
    q = kdehip.kde(pos, [0.3])
    for a, b, lp in ((p, q, np.log(direct)), (p, p, np.log(kdehip.evaluateDualTree(p, lvFlag=True)))):
        old, new = kdehip.evalAvgLogL(a, b), kdehip.evalAvgLogL(a, b, log_domain=True)
        print(f"evalAvgLogL: |log domain - direct| = {abs(new - old):.3e}, scale {np.abs(lp).max():.3e}")
        assert abs(new - old) <= 1e-12 * np.abs(lp).max()  # (the weights sum to 1)


def test_weightless_sources_take_no_part_in_the_maximum():
    """the sources nearest the queries carry weight 0 and the weighted ones are 60 sd away: a maximum over all sources would
    shift every real term into underflow and return -Inf"""
    rng = np.random.default_rng(11)
    D, sd = 2, np.array([0.05, 0.05])
    near = rng.standard_normal((D, 140)) * 0.05                                # two chunks of weightless points ...
    far = rng.standard_normal((D, 60)) * 0.05 + np.array([[3.0], [0.0]])      # ... and the density proper, 60 sd away
    pts = np.hstack([near, far])
    w = np.concatenate([np.zeros(140), rng.uniform(0.2, 1.0, 60)])
    pos = rng.standard_normal((D, 257)) * 0.05
    p = kdehip.kde(pts, sd, w)
    assert np.all(p(pos) == 0.0)
    lp = kdehip.evaluate_log(p, pos)
    assert np.all(np.isfinite(lp))
    _close(lp, lm.eval_log(pts, w, _var(p), pos), "weightless near points")
    _close(lp, lm.eval_log(far, w[140:], _var(p), pos), "the weighted points alone")
    # leave-one-out: finite at every point, weightless ones included (their weight keeps them out of evalAvgLogL)
    _close(kdehip.evaluate_log(p, lvFlag=True), lm.eval_log(pts, w, _var(p), loo=True), "leave-one-out")
    _close(kdehip.evalAvgLogL(p, p, log_domain=True), lm.eval_avg_logl_log((pts, w, _var(p)))[0], "evalAvgLogL(p, p)")
    # a density with no weighted point left for a query: -Inf there, and only a weighted query carries it into the sum
    one = kdehip.kde(np.array([[0.0, 1.0], [0.0, 1.0]]), sd, np.array([1.0, 0.0]))
    got = kdehip.evaluate_log(one, lvFlag=True)
    assert got[0] == -np.inf
    _close(got[1:], lm.eval_log(np.array([[0.0, 1.0], [0.0, 1.0]]), [1.0, 0.0], _var(one), loo=True)[1:], "the weightless point")
    assert kdehip.evalAvgLogL(one, one, log_domain=True) == -np.inf


@pytest.mark.parametrize("D,man,weighted", [(1, [1], False), (2, [1, 0], True), (3, [0, 1, 1], False)])
def test_circular_dimensions(D, man, weighted):
    """data on both sides of +-pi, queries over (-2 pi, 2 pi), unwrapped: the model's wrap, and not the Euclidean call"""
    N, Nq = 129, 257
    pts, w, sd, pos = cm.circular_case(40 + D, D, N, Nq, man, weighted)
    p = kdehip.kde(pts, sd, w)
    var = _var(p)
    got = kdehip.evaluate_log(p, pos, manifold=man)
    _close(got, lm.eval_log(pts, w, var, pos, man), "circular evaluate_log")
    eucl = kdehip.evaluate_log(p, pos)
    _close(eucl, lm.eval_log(pts, w, var, pos), "the Euclidean call on the same data")
    assert np.max(np.abs(got - eucl)) > 1.0
    _close(kdehip.evaluate_log(p, lvFlag=True, manifold=man), lm.eval_log(pts, w, var, manifold=man, loo=True), "circular loo")
    q = kdehip.kde(pos, [0.3])
    _close(kdehip.evalAvgLogL(p, q, manifold=man, log_domain=True),
           lm.eval_avg_logl_log((pts, w, var), (pos, None, None), man)[0], "circular evalAvgLogL")
    with kdehip.DeviceDensity(p) as dp:
        assert np.array_equal(dp.evaluate_log(pos, manifold=man), got)


def test_routes_return_the_same_bits():
    import torch
    hosts, devs, mans = [], [], []
    for k, (D, N, Nq, man) in enumerate([(2, 300, 257, None), (3, 129, 255, None), (2, 127, 256, [1, 0]), (3, 300, 129, [0, 1, 1])]):
        if man is None:
            pts, w, sd, pos = _case(50 + k, D, N, Nq, k % 2 == 0)
        else:
            pts, w, sd, pos = cm.circular_case(50 + k, D, N, Nq, man, k % 2 == 0)
        p, q = kdehip.kde(pts, sd, w), kdehip.kde(pos, [0.3])
        hosts.append((p, q, pos))
        devs.append((kdehip.DeviceDensity(p), kdehip.DeviceDensity(q)))
        mans.append(man)
    singles = []
    for (p, q, pos), (dp, dq), man in zip(hosts, devs, mans):
        host = kdehip.evaluate_log(p, pos, manifold=man)
        assert np.array_equal(kdehip.evaluate_log(p, pos, manifold=man), host)           # a second run
        assert np.array_equal(dp.evaluate_log(pos, manifold=man), host)                   # resident, host points
        t = dp.evaluate_log(torch.from_numpy(pos).to("cuda:0"), manifold=man)              # resident, device points
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), host)
        # the `at` form: values at q's points in ITS original order, through its permutation
        assert np.array_equal(dp.evaluate_log(dq, manifold=man), kdehip.evaluate_log(p, kdehip.getPoints(q), manifold=man))
        loo = kdehip.evaluate_log(p, lvFlag=True, manifold=man)
        assert np.array_equal(dp.evaluate_log(dp, manifold=man), loo)
        assert np.array_equal(dp.evaluate_log(lvFlag=True, manifold=man), loo)
        e = kdehip.evalAvgLogL(p, q, manifold=man, log_domain=True)
        assert kdehip.evalAvgLogL(dp, dq, manifold=man, log_domain=True) == e
        assert kdehip.evalAvgLogL(dp, dp, manifold=man, log_domain=True) == kdehip.evalAvgLogL(p, p, manifold=man, log_domain=True)
        assert kdehip.kld(dp, dq, manifold=man, log_domain=True) == kdehip.kld(p, q, manifold=man, log_domain=True)
        singles.append(kdehip.kld(dp, dq, manifold=man, log_domain=True))
    # one batch that mixes D = 2 and D = 3, Euclidean and circular items
    got = kdehip.kld_batch(devs, manifolds=mans, log_domain=True)
    assert np.array_equal(got, np.array(singles))
    assert np.array_equal(kdehip.kld_batch(devs, manifolds=mans, log_domain=True), got)  # run to run
    items = [(dp, dq) for dp, dq in devs] + [(dp, dp) for dp, _ in devs]
    out = torch.full((len(items),), np.nan, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        kdehip.eval_avg_logl_device_batch(items, out, stream=st.cuda_stream, manifolds=mans + mans, log_domain=True)
    st.synchronize()
    want = np.array([kdehip.evalAvgLogL(a, b, manifold=m, log_domain=True) for (a, b), m in zip(items, mans + mans)])
    assert np.array_equal(out.cpu().numpy(), want)
    # the direct entries next to them keep their own results (another launch, other kernels)
    assert kdehip.kld(devs[0][0], devs[0][1]) == kdehip.kld(hosts[0][0], hosts[0][1])
    for dp, dq in devs:
        dp.close()
        dq.close()


def test_a_batch_mask_bit_beyond_ndims_is_refused():
    import torch
    rng = np.random.default_rng(3)
    with kdehip.DeviceDensity(kdehip.kde(_pts(rng, 2, 64), [0.3])) as dq:
        arr = (_lib.CLoglManifoldItem * 1)()
        arr[0].bd, arr[0].at, arr[0].leave_one_out, arr[0].circular_mask = dq._h, dq._h, 1, 1 << 2
        out = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        assert _lib.lib.kdehip_eval_avg_logl_log_device_batch(1, arr, out.data_ptr(), None) == _lib.ERR_ARG
        assert "circular_mask" in _lib.lib.kdehip_last_error().decode()
        arr[0].circular_mask = 1 << 1
        _lib.check(_lib.lib.kdehip_eval_avg_logl_log_device_batch(1, arr, out.data_ptr(), None))
        torch.cuda.synchronize()
        assert out.item() == kdehip.evalAvgLogL(dq, dq, manifold=[0, 1], log_domain=True)


# Groups of SEVERAL chunks (the shape in SHAPES has 3 queries): the double-buffered walk of csrc/pair_sweep.hpp with the
# carried (m, s) rescaled inside a group.  On the 256 CUs of an MI355X split_chunks wants all MAX_GROUPS groups for any query
# count up to a few thousand, so a group holds more than one chunk only when N > 128 * MAX_GROUPS.
#   N = 128 * 64 + 1:  65 chunks, 2 per group, 33 groups; the last group is ONE chunk of ONE point, every other group prefetches
#   N = 128 * 128 + 1: 129 chunks, 3 per group: both buffer parities inside a group; the last chunk holds one point
# 257 queries: a second query block with one live lane.  One case has a circular dimension.
SWEEP_NQ = 257
SWEEP_CASES = [(1, 128 * MAX_GROUPS + 1, None), (6, 128 * MAX_GROUPS + 1, None), (1, 256 * MAX_GROUPS + 1, None),
               (6, 256 * MAX_GROUPS + 1, None), (6, 128 * MAX_GROUPS + 1, [0, 0, 1, 0, 0, 0])]


def _sweep_case(D, N, man):
    """points, weights (with exact zeros), standard deviations and SWEEP_NQ queries"""
    if man is None:
        pts, w, sd, pos = _case(5 * N + D, D, N, SWEEP_NQ, True)
    else:
        pts, w, sd, pos = cm.circular_case(5 * N + D, D, N, SWEEP_NQ, man, True)
    w[::5] = 0.0
    return pts, w, sd, pos


@pytest.mark.parametrize("D,N,man", SWEEP_CASES)
def test_groups_of_several_chunks_against_the_model(D, N, man):
    import torch
    pts, w, sd, pos = _sweep_case(D, N, man)
    p, q = kdehip.kde(pts, sd, w), kdehip.kde(pos, [0.3])
    want = lm.eval_log(pts, w, _var(p), pos, man)
    host = kdehip.evaluate_log(p, pos, manifold=man)
    _close(host, want, "evaluate_log")
    want_ll, _ = lm.avg_logl_log(want, np.full(SWEEP_NQ, 1.0 / SWEEP_NQ))  # (q's weights are uniform; a sum has no order)
    e = kdehip.evalAvgLogL(p, q, manifold=man, log_domain=True)
    _close(e, want_ll, "evalAvgLogL")
    # host entry == resident entry == a batch whose first item is a small 1-D Euclidean one: the launch of a 6-D or circular
    # item then starts at a block offset (first[0] != 0), and a Euclidean 1-D item is the second of its launch
    small = kdehip.kde(np.array([[0.1, 0.4, -0.3, 0.9, 0.5]]), [0.3])
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq, kdehip.DeviceDensity(small) as ds:
        assert np.array_equal(dp.evaluate_log(pos, manifold=man), host)
        assert np.array_equal(dp.evaluate_log(dq, manifold=man), kdehip.evaluate_log(p, kdehip.getPoints(q), manifold=man))
        assert kdehip.evalAvgLogL(dp, dq, manifold=man, log_domain=True) == e
        out = torch.full((2,), np.nan, dtype=torch.float64, device="cuda:0")
        kdehip.eval_avg_logl_device_batch([(ds, ds), (dp, dq)], out, manifolds=[None, man], log_domain=True)
        torch.cuda.synchronize()
        assert out[1].item() == e and out[0].item() == kdehip.evalAvgLogL(small, small, log_domain=True)


def test_leave_one_out_with_the_self_term_in_a_groups_second_chunk():
    """N = Nq = 128 * 64 + 1 in 1-D: 33 query blocks, 33 groups of 2 chunks; for half the queries the self term is a point of
    the second chunk its block walks.  The model is evaluated in row blocks (never an N x N array)."""
    N = 128 * MAX_GROUPS + 1
    pts, w, sd, _ = _case(N, 1, N, 1, True)
    w[::5] = 0.0
    p = kdehip.kde(pts, sd, w)
    want = np.concatenate([lm.eval_log(pts, w, _var(p), loo=True, rows=slice(r, r + 1024)) for r in range(0, N, 1024)])
    assert want.shape == (N,)
    loo = kdehip.evaluate_log(p, lvFlag=True)
    _close(loo, want, "leave-one-out")
    want_ll, _ = lm.avg_logl_log(want, cm.normalise(w, N))
    e = kdehip.evalAvgLogL(p, p, log_domain=True)
    _close(e, want_ll, "evalAvgLogL(p, p)")
    with kdehip.DeviceDensity(p) as dp:
        assert kdehip.evalAvgLogL(dp, dp, log_domain=True) == e
        assert np.array_equal(dp.evaluate_log(dp), loo)
