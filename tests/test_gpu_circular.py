"""Circular dimensions in evaluation, log-likelihoods and the bandwidth search on the GPU (include/kdehip.h section 5d;
CIRC instantiations of the kernels in csrc/evaluate.hip), against the NumPy model of tests/circular_model.py (pinned to the
oracle in tests/test_circular_host.py).  Tolerances are the project's own for the same comparisons in Euclidean form:
rtol 1e-12 for density and leave-one-out values, rtol 1e-9 with equal evaluation counts for bandwidths,
1e-12 * sum |W log L| for log-likelihoods."""
import math

import numpy as np
import pytest

import kdehip
from tests import circular_model as cm

pytestmark = pytest.mark.gpu

# N and Nq are no multiples of 64, 128 or 256; D = 6 is the SE(3)-like eeeccc
SHAPES = [(1, 100, 33, [1], False), (2, 257, 300, [0, 1], True), (3, 1000, 129, [1, 0, 1], False),
          (6, 321, 450, [0, 0, 0, 1, 1, 1], True), (6, 65, 70, [0, 0, 0, 1, 1, 1], False), (2, 130, 77, [1, 1], True)]


def _close_ll(got, want, scale):
    if np.isinf(want):
        assert got == want
    else:
        print("logl", got, want, abs(got - want), 1e-12 * scale)
        assert abs(got - want) <= 1e-12 * scale + 1e-300, (got, want, scale)


@pytest.mark.parametrize("D,N,Nq,man,weighted", SHAPES)
def test_evaluation_and_loglikelihood_against_the_model(D, N, Nq, man, weighted):
    pts, w, bw, pos = cm.circular_case(10 * D + N, D, N, Nq, man, weighted)
    p = kdehip.kde(pts, bw, w)
    assert any(np.any(np.abs(pts[k]) > math.pi) for k in range(D) if man[k])  # inputs outside [-pi, pi)
    want = cm.eval_direct(pts, w, bw ** 2, pos, man)
    got = kdehip.evaluateDualTree(p, pos, manifold=man)
    print("eval max rel", np.max(np.abs(got - want) / np.maximum(want, 1e-300)))
    assert np.allclose(got, want, rtol=1e-12, atol=1e-300)
    assert np.array_equal(p(pos, manifold=man), got)
    assert not np.allclose(got, kdehip.evaluateDualTree(p, pos), rtol=1e-6)  # (the wrap is at work in this data)
    want_loo = cm.eval_direct(pts, w, bw ** 2, manifold=man, loo=True)
    got_loo = kdehip.evaluateDualTree(p, lvFlag=True, manifold=man)
    assert np.allclose(got_loo, want_loo, rtol=1e-12)
    assert np.array_equal(kdehip.evaluateDualTree(p, p, manifold=man), got_loo)
    # log-likelihoods: at another density's points, and leave-one-out
    wq = np.random.default_rng(N).uniform(0.1, 1.0, Nq) if weighted else None
    q = kdehip.kde(pos, [0.3], wq)
    ll, scale = cm.eval_avg_logl((pts, w, bw ** 2), (pos, wq, None), man)
    _close_ll(kdehip.evalAvgLogL(p, q, manifold=man), ll, scale)
    ll0, scale0 = cm.eval_avg_logl((pts, w, bw ** 2), None, man)
    _close_ll(kdehip.evalAvgLogL(p, p, manifold=man), ll0, scale0)
    assert kdehip.entropy(p, manifold=man) == -kdehip.evalAvgLogL(p, p, manifold=man)
    e = kdehip.evalAvgLogL
    assert kdehip.kld(p, q, manifold=man) == e(p, p, manifold=man) - e(q, p, manifold=man)
    assert kdehip.minkld(p, q, manifold=man) == min(abs(kdehip.kld(p, q, manifold=man)), abs(kdehip.kld(q, p, manifold=man)))
    # resident densities: the same bits
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert np.array_equal(dp.evaluate(pos, manifold=man), got)
        assert np.array_equal(dp(pos, manifold=man), got)
        assert np.array_equal(dp.evaluate(dp, manifold=man), got_loo)
        assert np.array_equal(dp.evaluate(dq, manifold=man), kdehip.evaluateDualTree(p, kdehip.getPoints(q), manifold=man))
        assert e(dp, dq, manifold=man) == e(p, q, manifold=man)
        assert e(dp, dp, manifold=man) == e(p, p, manifold=man)


@pytest.mark.parametrize("D,N,man", cm.BANDWIDTH_CASES)
def test_bandwidth_search_against_the_model(D, N, man):
    """(N = 65 and 129: the infinity padding of the pair kernels' last tile must contribute 0 and no NaN)"""
    pts = cm.bandwidth_case(D, N, man)
    want, wnev, _ = cm.auto_bandwidth(pts, man)
    got, nev = kdehip.auto_bandwidth(pts, return_evals=True, manifold=man)
    print("bw", got, want, nev, wnev)
    assert np.all(np.isfinite(got))
    assert np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
    assert nev == wnev
    eu = kdehip.auto_bandwidth(pts)
    assert not np.allclose(got, eu, rtol=1e-6)  # (and the circular search differs from the Euclidean one on this data)
    # kde_auto / kde(points, manifold=...) carry that bandwidth
    d = kdehip.kde(pts, manifold=man)
    assert np.array_equal(kdehip.getBW(d)[:, 0], got)
    assert np.array_equal(kdehip.getBW(kdehip.kde_auto(pts, overlap=False, manifold=man))[:, 0], got)


_TWO_LAUNCH_SCRIPT = """
import json, numpy as np, kdehip
from tests import circular_model as cm
out = []
for D, N, man in cm.BANDWIDTH_CASES:
    bw, nev = kdehip.auto_bandwidth(cm.bandwidth_case(D, N, man), return_evals=True, manifold=man)
    out.append([list(bw), nev])
print("RESULT " + json.dumps(out))
"""


def test_two_launch_rounds_agree_with_the_one_launch_rounds():
    """KDEHIP_LOOCV_TWO_LAUNCH=1 takes loo_round_partial_kernel (what marginals above 4096 points run) and KDEHIP_LOOCV_SPEC=0
    the plain pair rounds: the same searches as the library's own choice"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    for extra in ({}, {"KDEHIP_LOOCV_SPEC": "0"}, {"KDEHIP_LOOCV_TWO_LAUNCH": "1"}):
        env = dict(os.environ, PYTHONPATH=root, **extra)
        out = subprocess.run([sys.executable, "-c", _TWO_LAUNCH_SCRIPT], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
        res.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    for other in res[1:]:
        for (b0, n0), (b1, n1) in zip(res[0], other):
            assert n0 == n1
            assert np.allclose(b0, b1, rtol=1e-9, atol=0.0), (b0, b1)
    for (D, N, man), (b, n) in zip(cm.BANDWIDTH_CASES, res[2]):
        want, wnev, _ = cm.auto_bandwidth(cm.bandwidth_case(D, N, man), man)
        assert np.allclose(b, want, rtol=1e-9, atol=0) and n == wnev


def test_no_wrap_same_bits():
    """all coordinates in (-pi/2, pi/2): no pair difference leaves [-pi, pi), circ_wrap is the identity, and every new
    entry returns exactly the bytes of its Euclidean counterpart; NULL and all-zero manifolds likewise"""
    import torch
    rng = np.random.default_rng(11)
    for D, N, Nq in [(1, 129, 65), (3, 300, 257), (6, 1000, 130)]:
        pts, pos = rng.uniform(-1.5, 1.5, (D, N)), rng.uniform(-1.5, 1.5, (D, Nq))
        w = rng.uniform(0.2, 1.0, N)
        p, q = kdehip.kde(pts, rng.uniform(0.2, 0.5, D), w), kdehip.kde(pos, [0.3])
        bw_e, n_e = kdehip.auto_bandwidth(pts, return_evals=True)
        flat = torch.from_numpy(np.ascontiguousarray(pts.T).ravel()).to("cuda:0")
        for man in ([1] * D, [0] * D, None, ["circular"] * D):
            assert np.array_equal(kdehip.evaluateDualTree(p, pos, manifold=man), kdehip.evaluateDualTree(p, pos))
            assert np.array_equal(kdehip.evaluateDualTree(p, lvFlag=True, manifold=man), kdehip.evaluateDualTree(p, lvFlag=True))
            assert kdehip.evalAvgLogL(p, q, manifold=man) == kdehip.evalAvgLogL(p, q)
            assert kdehip.evalAvgLogL(p, p, manifold=man) == kdehip.evalAvgLogL(p, p)
            assert kdehip.kld(p, q, manifold=man) == kdehip.kld(p, q)
            bw_c, n_c = kdehip.auto_bandwidth(pts, return_evals=True, manifold=man)
            assert np.array_equal(bw_c, bw_e) and n_c == n_e
            assert np.array_equal(kdehip.kde(pts, manifold=man).bandwidth, kdehip.kde(pts).bandwidth)
            with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
                assert np.array_equal(dp.evaluate(pos, manifold=man), dp.evaluate(pos))
                assert np.array_equal(dp.evaluate(dq, manifold=man), dp.evaluate(dq))
                assert np.array_equal(dp.evaluate(dp, manifold=man), dp.evaluate(dp))
                assert kdehip.evalAvgLogL(dp, dq, manifold=man) == kdehip.evalAvgLogL(dp, dq)
                assert np.array_equal(kdehip.kld_batch([(dp, dq), (dq, dp)], manifold=man), kdehip.kld_batch([(dp, dq), (dq, dp)]))
            with kdehip.DeviceDensity.from_device_points(flat, D, N, manifold=man) as dd:
                assert np.array_equal(dd.bw, bw_e) and dd.nevals == n_e


def test_one_arithmetic_everywhere():
    """a circular pair: host entry, device entry, _device_at and a batch that mixes circular and Euclidean items of
    different D give the same bits"""
    import torch
    man = [0, 1, 1]
    pts, w, bw, pos = cm.circular_case(77, 3, 333, 205, man, True)
    p, q = kdehip.kde(pts, bw, w), kdehip.kde(pos, [0.4])
    rng = np.random.default_rng(2)
    others = [(kdehip.kde(rng.standard_normal((D, 150 + 7 * D)) * 2.5, [0.3]), kdehip.kde(rng.standard_normal((D, 90 + D)) * 2.5, [0.3]),
               ([k % 2 for k in range(D)] if D % 2 else None)) for D in (1, 2, 3, 6, 3)]
    host = kdehip.evalAvgLogL(p, q, manifold=man)
    host_loo = kdehip.evalAvgLogL(p, p, manifold=man)
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert kdehip.evalAvgLogL(dp, dq, manifold=man) == host
        assert kdehip.evalAvgLogL(dp, dp, manifold=man) == host_loo
        assert np.array_equal(dp.evaluate(dq, manifold=man), kdehip.evaluateDualTree(p, kdehip.getPoints(q), manifold=man))
        devs = [(kdehip.DeviceDensity(a), kdehip.DeviceDensity(b), m) for a, b, m in others]
        items = [(dp, dq), (dp, dp)] + [(a, b) for a, b, _ in devs] + [(dp, dq)]
        mans = [man, man] + [m for _, _, m in devs] + [None]
        out = torch.full((len(items),), np.nan, dtype=torch.float64, device="cuda:0")
        kdehip.eval_avg_logl_device_batch(items, out, manifolds=mans)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[0] == host and got[1] == host_loo
        for k, (a, b, m) in enumerate(others):
            assert got[2 + k] == kdehip.evalAvgLogL(a, b, manifold=m)
        assert got[-1] == kdehip.evalAvgLogL(p, q) and got[-1] != host
        # kld_batch: one manifold for all pairs, one per pair
        assert np.array_equal(kdehip.kld_batch([(dp, dq), (dq, dp)], manifold=man),
                              [kdehip.kld(p, q, manifold=man), kdehip.kld(q, p, manifold=man)])
        assert np.array_equal(kdehip.kld_batch([(dp, dq), (dq, dp)], manifolds=[man, None]),
                              [kdehip.kld(p, q, manifold=man), kdehip.kld(q, p)])
        for a, b, _ in devs:
            a.close()
            b.close()
    with pytest.raises(kdehip.KdeHipError):  # a mask bit beyond the item's dimensions
        with kdehip.DeviceDensity(q) as dq:
            from kdehip import _lib
            arr = (_lib.CLoglManifoldItem * 1)()
            arr[0].bd, arr[0].at, arr[0].leave_one_out, arr[0].circular_mask = dq._h, dq._h, 1, 8
            out = torch.zeros(1, dtype=torch.float64, device="cuda:0")
            _lib.check(_lib.lib.kdehip_eval_avg_logl_device_batch_manifold(1, arr, out.data_ptr(), None))


def test_it_matters_a_cluster_on_the_cut():
    """a symmetric 1-D cluster centred on the cut, evaluated at the cut: the Euclidean sum sees half of it"""
    rng = np.random.default_rng(5)
    a = math.pi + 0.3 * rng.standard_normal(400)
    a = np.concatenate([a, 2.0 * math.pi - a])
    pts = np.where(a >= math.pi, a - 2.0 * math.pi, a).reshape(1, -1)
    at = np.array([[-math.pi]])
    p = kdehip.kde(pts, [0.2])
    circ, eucl = kdehip.evaluateDualTree(p, at, manifold=[1])[0], kdehip.evaluateDualTree(p, at)[0]
    assert np.isclose(circ, cm.eval_direct(pts, None, [0.04], at, [1])[0], rtol=1e-12)
    assert np.isclose(eucl, cm.eval_direct(pts, None, [0.04], at, [0])[0], rtol=1e-12)
    assert 1.9 < circ / eucl < 2.1


def test_zero_likelihood_with_weight_is_minus_infinity_on_the_circle():
    rng = np.random.default_rng(8)
    pts = np.vstack([rng.standard_normal(40) * 0.01, 3.1 + rng.standard_normal(40) * 0.001])
    p = kdehip.kde(pts, [0.05])
    far = np.vstack([rng.standard_normal(30) + 100.0, rng.uniform(-3, 3, 30)])
    q = kdehip.kde(far, [0.1])
    assert kdehip.evalAvgLogL(p, q, manifold=[0, 1]) == -np.inf
    assert cm.eval_avg_logl((pts, None, np.array([0.0025, 0.0025])), (far, None, None), [0, 1])[0] == -np.inf
    # the circular dimension alone cannot be that far away: finite where the Euclidean form is -Inf
    near = np.vstack([rng.standard_normal(30) * 0.01, -3.1 + 2.0 * math.pi * 3 + rng.standard_normal(30) * 0.001])
    qn = kdehip.kde(near, [0.1])
    assert np.isfinite(kdehip.evalAvgLogL(p, qn, manifold=[0, 1]))
    assert kdehip.evalAvgLogL(p, qn) == -np.inf
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert kdehip.evalAvgLogL(dp, dq, manifold=[0, 1]) == -np.inf


@pytest.mark.parametrize("D,N,man", [(2, 300, [0, 1]), (6, 129, [0, 0, 0, 1, 1, 1]), (1, 65, [1])])
def test_resident_bandwidth_equals_the_host_entry(D, N, man):
    import torch
    pts = cm.bandwidth_case(D, N, man)
    bw, nev = kdehip.auto_bandwidth(pts, return_evals=True, manifold=man)
    flat = torch.from_numpy(np.ascontiguousarray(pts.T).ravel()).to("cuda:0")
    with kdehip.DeviceDensity.from_device_points(flat, D, N, manifold=man) as dd:
        assert np.array_equal(dd.bw, bw) and dd.nevals == nev
        h = dd.download()
        ref = kdehip.kde(pts, manifold=man)
        assert np.array_equal(h.bandwidth, ref.bandwidth) and np.array_equal(h.means, ref.means)
