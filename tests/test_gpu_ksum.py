"""Exact overlap measures on the GPU (csrc/ksum.hip, include/kdehip.h section 5g): `kernel_sum`, `intersIntg`, `ise`, `mmd`
and their batches against tests/ksum_model.py (an exactly rounded double sum), against the existing evaluation entry,
against sums written out by hand, and against each other bit for bit.

Tolerance: every term of S is positive, so the value itself is the scale: |got - want| <= 1e-12 * want, the bound the
evaluation and log-likelihood tests use against their oracle."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import circular_model as cm
from tests import ksum_model as km

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * math.pi
# (D, N, M) with N, M from {1, 2, 127, 128, 129, 257, 300, 700}: the chunk edge at 128, the query-block edge at 256, dead
# lanes, more than one source group (N > 128) and more than one query block (M > 256)
SHAPES = [(1, 1, 1), (2, 2, 1), (3, 127, 128), (1, 128, 129), (6, 129, 257), (2, 257, 300), (8, 300, 700), (6, 700, 2),
          (3, 700, 700), (1, 1, 700), (8, 128, 127), (6, 257, 257)]


def _weights(rng, N):
    """non-uniform, with exact zeros"""
    w = rng.uniform(0.05, 1.0, size=N)
    if N > 2:
        w[::5] = 0.0
    return w


def _density(rng, D, N, shift=0.0):
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1)) + shift
    return kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D), _weights(rng, N))


def _arrays(p):
    """(points, weights, leaf variances) of a host density, as the model takes them"""
    N, D = p.bt.num_points, p.bt.dims
    return kdehip.getPoints(p), kdehip.getWeights(p), p.bandwidth[N * D:(N + 1) * D].copy()


def _close(got, want, scale=None):
    scale = abs(want) if scale is None else scale
    assert math.isfinite(got) and abs(got - want) <= 1e-12 * scale, (got, want, scale)


_CASES = {}


def _case(D, N, M):
    """the pair of one shape, its explicit variances and the model's values: built once, shared, never changed"""
    key = (D, N, M)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * N + M)
        a, b = _density(rng, D, N), _density(rng, D, M, shift=0.4)
        sd = rng.uniform(0.3, 0.9, size=D)
        v = sd * sd
        A, B = _arrays(a), _arrays(b)
        _CASES[key] = dict(a=a, b=b, sd=sd, v=v, A=A, B=B,
                           want_v=km.kernel_sum(A, B, v), want_sum=km.kernel_sum(A, B, None, True))
    return _CASES[key]


@pytest.mark.parametrize("D,N,M", SHAPES)
def test_kernel_sum_equals_the_model(D, N, M):
    c = _case(D, N, M)
    assert c["want_v"] > 0.0 and c["want_sum"] > 0.0
    # explicit variances, not normalised and normalised; NULL = the summed leaf variances
    got = kdehip.kernel_sum(c["a"], c["b"], c["v"])
    _close(got, c["want_v"])
    _close(kdehip.kernel_sum(c["a"], c["b"], c["v"], normalize=True), c["want_v"] / km.norm(c["v"]))
    _close(kdehip.intersIntg(c["a"], c["b"]), c["want_sum"])
    # resident: the same bits as the host entry
    with kdehip.DeviceDensity(c["a"]) as da, kdehip.DeviceDensity(c["b"]) as db:
        assert kdehip.kernel_sum(da, db, c["v"]) == got
        assert kdehip.intersIntg(da, db) == kdehip.intersIntg(c["a"], c["b"])


@pytest.mark.parametrize("D,N,M", [(1, 128, 129), (2, 257, 300), (6, 129, 257), (8, 300, 700), (3, 700, 700)])
def test_kernel_sum_equals_the_weighted_sum_of_the_existing_evaluation(D, N, M):
    """S(a, b; v) normalised = sum_j b_j p(y_j) with p = kde(a's points, sqrt(v), a's weights), by evaluateDualTree"""
    c = _case(D, N, M)
    pa, wa, _ = c["A"]
    pb, wb, _ = c["B"]
    p = kdehip.kde(pa, c["sd"], wa)  # its variances are sd * sd == v, bit for bit
    want = math.fsum((wb * kdehip.evaluateDualTree(p, pb)).tolist())
    _close(kdehip.kernel_sum(c["a"], c["b"], c["v"], normalize=True), want)


@pytest.mark.parametrize("D", [1, 6])
def test_intersIntg_of_two_point_densities_is_the_sum_of_four_normal_densities(D):
    rng = np.random.default_rng(40 + D)
    xa, xb = rng.standard_normal((D, 2)), rng.standard_normal((D, 2)) + 0.5
    sa, sb = rng.uniform(0.3, 0.8, size=D), rng.uniform(0.3, 0.8, size=D)
    wa, wb = np.array([0.25, 0.75]), np.array([0.6, 0.4])
    a, b = kdehip.kde(xa, sa, wa), kdehip.kde(xb, sb, wb)
    want = math.fsum(wa[i] * wb[j] * math.prod(km.normal_pdf(xa[k, i] - xb[k, j], sa[k] * sa[k] + sb[k] * sb[k]) for k in range(D))
                     for i in range(2) for j in range(2))
    _close(kdehip.intersIntg(a, b), want)
    with kdehip.DeviceDensity(a) as da, kdehip.DeviceDensity(b) as db:
        _close(kdehip.intersIntg(da, db), want)


def _mixed_items():
    """pairs of mixed D and sizes, Euclidean and circular, explicit and summed variances, normalised or not"""
    rng = np.random.default_rng(5)
    items = []
    for k, (D, N, M) in enumerate([(1, 300, 2), (6, 129, 257), (2, 257, 300), (8, 2, 127), (3, 700, 128), (2, 128, 700),
                                   (6, 1, 1), (1, 129, 129), (2, 300, 257)]):
        a, b = _density(rng, D, N), _density(rng, D, M, shift=0.2)
        man = None if k % 2 == 0 else ([1] + [0] * (D - 1) if k % 4 == 1 else [0] * (D - 1) + [1])
        var = None if k % 3 == 0 else rng.uniform(0.2, 1.5, size=D)
        items.append(dict(a=a, b=b, var=var, normalize=k % 2 == 1, manifold=man))
    return items


def test_host_single_and_batch_give_the_same_bits_run_after_run():
    import torch
    hosts = _mixed_items()
    host_vals = np.array([kdehip.kernel_sum(it["a"], it["b"], it["var"], normalize=it["normalize"], manifold=it["manifold"])
                          for it in hosts])
    assert np.all(np.isfinite(host_vals)) and np.all(host_vals > 0.0)
    devs = [dict(it, a=kdehip.DeviceDensity(it["a"]), b=kdehip.DeviceDensity(it["b"])) for it in hosts]
    singles = np.array([kdehip.kernel_sum(it["a"], it["b"], it["var"], normalize=it["normalize"], manifold=it["manifold"])
                        for it in devs])
    assert np.array_equal(singles, host_vals)  # host entry == single resident call
    for rep in range(2):  # ... == its place in a mixed batch, twice, on a stream of its own
        out = torch.full((len(devs),), np.nan, dtype=torch.float64, device="cuda:0")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            kdehip.kernel_sum_device_batch(devs, out, stream=st.cuda_stream)
        st.synchronize()
        assert np.array_equal(out.cpu().numpy(), singles)
    order = [4, 0, 8, 2, 6, 1, 7, 3, 5]  # another order of the same items: every value keeps its bits
    out = torch.full((len(devs),), np.nan, dtype=torch.float64, device="cuda:0")
    kdehip.kernel_sum_device_batch([devs[k] for k in order], out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), singles[order])
    for it in devs:
        it["a"].close()
        it["b"].close()


@pytest.mark.parametrize("host", [True, False])
def test_self_terms_cancel_exactly(host):
    rng = np.random.default_rng(9)
    D, N = 3, 300
    pts, ks, w = rng.standard_normal((D, N)), rng.uniform(0.2, 0.5, size=D), _weights(rng, N)
    p, copy, q = kdehip.kde(pts, ks, w), kdehip.kde(pts, ks, w), _density(rng, D, 257)
    if not host:
        p, copy, q = kdehip.DeviceDensity(p), kdehip.DeviceDensity(copy), kdehip.DeviceDensity(q)
    assert kdehip.ise(p, p) == 0.0
    assert kdehip.mmd(p, p, 0.4) == 0.0
    assert kdehip.mmd(p, p, [0.4, 0.2, 0.9], manifold=[0, 1, 0]) == 0.0
    # the full square is summed whatever the identity of the arguments
    assert kdehip.intersIntg(p, p) == kdehip.intersIntg(p, copy) == kdehip.intersIntg(copy, p)
    assert kdehip.kernel_sum(p, p, [0.3]) == kdehip.kernel_sum(p, copy, [0.3, 0.3, 0.3])
    assert kdehip.ise(p, copy) == 0.0
    # the compositions are the primitive
    i = kdehip.intersIntg
    assert kdehip.ise(p, q) == i(p, p) - 2.0 * i(p, q) + i(q, q)
    sd = np.array([0.4, 0.2, 0.9])
    s = lambda a, b: kdehip.kernel_sum(a, b, sd * sd)  # noqa: E731
    assert kdehip.mmd(p, q, sd) == s(p, p) - 2.0 * s(p, q) + s(q, q)
    assert kdehip.ise(p, q) > 0.0 and kdehip.mmd(p, q, sd) > 0.0
    if not host:
        for d in (p, copy, q):
            d.close()


def test_ise_batch_and_mmd_batch_equal_the_single_functions():
    rng = np.random.default_rng(12)
    pairs, mans = [], []
    for k in range(10):
        D = 1 + k % 8
        p = kdehip.DeviceDensity(_density(rng, D, int(rng.integers(2, 400))))
        q = p if k == 3 else kdehip.DeviceDensity(_density(rng, D, int(rng.integers(2, 400)), shift=0.3))
        pairs.append((p, q))
        mans.append(None if k % 3 else [1] + [0] * (D - 1))
    pairs.append((pairs[0][1], pairs[0][0]))  # shares its three items with pair 0
    mans.append(mans[0])
    got = kdehip.ise_batch(pairs, manifolds=mans)
    assert got.shape == (11,)
    assert np.array_equal(got, np.array([kdehip.ise(p, q, manifold=m) for (p, q), m in zip(pairs, mans)]))
    assert got[3] == 0.0 and np.all(got[np.arange(11) != 3] > 0.0)
    assert np.array_equal(kdehip.ise_batch(pairs, manifolds=mans), got)  # run to run
    same_d = [pq for pq in pairs if pq[0].dims == 2]
    assert np.array_equal(kdehip.ise_batch(same_d, manifold=[0, 1]), np.array([kdehip.ise(p, q, manifold=[0, 1]) for p, q in same_d]))
    got = kdehip.mmd_batch(pairs, 0.5, manifolds=mans)
    assert np.array_equal(got, np.array([kdehip.mmd(p, q, 0.5, manifold=m) for (p, q), m in zip(pairs, mans)]))
    assert got[3] == 0.0
    assert kdehip.ise_batch([]).shape == (0,)
    for p, q in pairs[:10]:
        p.close()
        if q is not p:
            q.close()


@pytest.mark.parametrize("D,N,M", [(2, 257, 300), (6, 129, 257), (3, 700, 700)])
def test_symmetry_and_non_negativity(D, N, M):
    c = _case(D, N, M)
    a, b = c["a"], c["b"]
    ab, ba = kdehip.kernel_sum(a, b, c["v"]), kdehip.kernel_sum(b, a, c["v"])
    _close(ab, ba)                # two summation orders of the same terms
    _close(ab, c["want_v"])
    _close(kdehip.intersIntg(b, a), c["want_sum"])
    i = kdehip.intersIntg
    e = kdehip.ise(a, b)
    assert e >= -1e-12 * (i(a, a) + 2.0 * i(a, b) + i(b, b))
    _close(e, kdehip.ise(b, a), i(a, a) + 2.0 * i(a, b) + i(b, b))
    want, mag = km.mmd(c["A"], c["B"], c["sd"])
    m = kdehip.mmd(a, b, c["sd"])
    assert m >= -1e-12 * mag
    _close(m, want, mag)
    _close(m, kdehip.mmd(b, a, c["sd"]), mag)


def _circular_pair(lo_a, hi_a, lo_b, hi_b, N=150, M=140, seed=21):
    """2-D, dimension 1 an angle: a's angles in [lo_a, hi_a], b's in [lo_b, hi_b]; bandwidth 0.1"""
    rng = np.random.default_rng(seed)
    pa = np.vstack([rng.standard_normal(N) * 0.3, rng.uniform(lo_a, hi_a, size=N)])
    pb = np.vstack([rng.standard_normal(M) * 0.3, rng.uniform(lo_b, hi_b, size=M)])
    return kdehip.kde(pa, [0.1], _weights(rng, N)), kdehip.kde(pb, [0.1], _weights(rng, M))


MAN = ["euclid", "circular"]


def test_circular_neighbours_across_the_cut():
    a, b = _circular_pair(3.0, 3.14, -3.14, -3.0)
    want = km.inters_intg(_arrays(a), _arrays(b), [0, 1])
    got = kdehip.intersIntg(a, b, manifold=MAN)
    _close(got, want)
    assert got >= 10.0 * kdehip.intersIntg(a, b)  # across the cut they are neighbours; on the line, 6 apart
    with kdehip.DeviceDensity(a) as da, kdehip.DeviceDensity(b) as db:
        assert kdehip.intersIntg(da, db, manifold=MAN) == got
        da.manifold = np.array([0, 1], dtype=np.uint8)
        assert kdehip.intersIntg(da, db, manifold="inherit") == got
    v = np.array([0.05, 0.03])
    _close(kdehip.kernel_sum(a, b, v, manifold=MAN), km.kernel_sum(_arrays(a), _arrays(b), v, False, [0, 1]))
    e, mag = km.ise(_arrays(a), _arrays(b), [0, 1])
    _close(kdehip.ise(a, b, manifold=MAN), e, mag)


def test_circular_data_that_never_wraps_gives_the_euclidean_bits():
    a, b = _circular_pair(-1.0, 1.0, -1.0, 1.0)
    assert kdehip.intersIntg(a, b, manifold=MAN) == kdehip.intersIntg(a, b)
    assert kdehip.kernel_sum(a, b, [0.2, 0.1], manifold=MAN) == kdehip.kernel_sum(a, b, [0.2, 0.1])
    assert kdehip.ise(a, b, manifold=MAN) == kdehip.ise(a, b)
    with kdehip.DeviceDensity(a) as da, kdehip.DeviceDensity(b) as db:
        assert kdehip.mmd(da, db, 0.3, manifold=MAN) == kdehip.mmd(da, db, 0.3) == kdehip.mmd(a, b, 0.3)


def test_circular_inputs_outside_the_principal_interval():
    a, b = _circular_pair(3.0 + TWO_PI, 3.14 + TWO_PI, -3.14 - TWO_PI, -3.0 - TWO_PI)
    want = km.inters_intg(_arrays(a), _arrays(b), [0, 1])
    assert want > 1e-3
    _close(kdehip.intersIntg(a, b, manifold=MAN), want)
    e, mag = km.ise(_arrays(a), _arrays(b), [0, 1])
    _close(kdehip.ise(a, b, manifold=MAN), e, mag)


def test_densities_far_apart_give_an_exact_zero():
    rng = np.random.default_rng(30)
    D, h = 2, 0.05
    pts = rng.standard_normal((D, 140)) * 0.02
    far = pts[:, :131] + np.array([[1e3 * h], [0.0]])  # 1e3 bandwidths away
    p, q = kdehip.kde(pts, [h], _weights(rng, 140)), kdehip.kde(far, [h], _weights(rng, 131))
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        for a, b in ((p, q), (dp, dq)):
            assert kdehip.intersIntg(a, b) == 0.0  # (== fails on a NaN)
            assert kdehip.kernel_sum(a, b, [h * h]) == 0.0
            pp, qq = kdehip.kernel_sum(a, a, [h * h]), kdehip.kernel_sum(b, b, [h * h])
            assert pp > 0.0 and qq > 0.0 and math.isfinite(pp + qq)
            assert kdehip.mmd(a, b, h) == pp + qq
            assert kdehip.ise(a, b) == kdehip.intersIntg(a, a) + kdehip.intersIntg(b, b)


def test_per_point_bandwidths_need_explicit_variances():
    rng = np.random.default_rng(31)
    D, N = 2, 130
    p, q = _density(rng, D, N), _density(rng, D, 40)
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    v = np.array([0.2, 0.35])
    want = km.kernel_sum(_arrays(p), _arrays(q), v, True)
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        for a, b in ((p, q), (q, p), (dp, dq), (dq, dp)):
            with pytest.raises(kdehip.KdeHipError) as e:
                kdehip.intersIntg(a, b)
            assert e.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(kdehip.KdeHipError) as e:
            kdehip.ise_batch([(dp, dq)])
        assert e.value.code == _lib.ERR_UNSUPPORTED
        got = kdehip.kernel_sum(p, q, v, normalize=True)
        _close(got, want)
        assert kdehip.kernel_sum(dp, dq, v, normalize=True) == got


def test_resident_arguments_are_refused_before_the_device_is_used():
    import ctypes as C
    rng = np.random.default_rng(32)
    with kdehip.DeviceDensity(_density(rng, 2, 20)) as p2, kdehip.DeviceDensity(_density(rng, 3, 20)) as p3:
        res = C.c_double(0.0)
        L = _lib.lib
        assert L.kdehip_kernel_sum_device(p2._h, p3._h, None, 1, C.byref(res), None) == _lib.ERR_DIM_MISMATCH
        assert L.kdehip_kernel_sum_device(p2._h, p2._h, None, 1, None, None) == _lib.ERR_ARG
        bad = np.array([0, 2], dtype=np.uint8)
        assert L.kdehip_kernel_sum_device(p2._h, p2._h, None, 1, C.byref(res), _lib.ptr(bad, _lib.u8p)) == _lib.ERR_ARG
        for var in ([1.0, 0.0], [np.nan, 1.0], [1.0, -np.inf]):
            v = np.array(var)
            assert L.kdehip_kernel_sum_device(p2._h, p2._h, _lib.ptr(v, _lib.f64p), 0, C.byref(res), None) == _lib.ERR_ARG
        items = (_lib.CKsumItem * 2)()
        for k in range(2):
            items[k].a, items[k].b, items[k].normalize = p2._h, p2._h, 1
        items[1].circular_mask = 1 << 2  # a dimension the densities do not have
        assert L.kdehip_kernel_sum_device_batch(2, items, C.c_void_p(256), None) == _lib.ERR_ARG
        assert "circular_mask" in L.kdehip_last_error().decode()
        items[1].circular_mask = 0
        items[1].b = p3._h
        assert L.kdehip_kernel_sum_device_batch(2, items, C.c_void_p(256), None) == _lib.ERR_DIM_MISMATCH
        with pytest.raises(ValueError):
            kdehip.ise(p2, p3)


# Groups of SEVERAL source chunks, the only part of the all-pairs sweep (csrc/pair_sweep.hpp) that really double-buffers.
# split_chunks (csrc/entry_helpers.hpp) deals the ceil(N / 128) chunks to at most 64 groups (kEvalMaxGroups), and on the
# 256 CUs of an MI355X it wants all 64 for any M up to a few thousand: a group holds more than one chunk only when
# N > 128 * 64.
#   N = 128 * 64 + 1:  65 chunks, 2 per group, 33 groups; the last group is ONE chunk of ONE point, every other group prefetches
#   N = 128 * 128 + 1: 129 chunks, 3 per group: both buffer parities inside a group; the last chunk holds one point
# M = 257: a second query block with one live lane.  One case has a circular dimension.
SWEEP_M = 257
SWEEP_CASES = [(1, 128 * 64 + 1, None), (6, 128 * 64 + 1, None), (1, 128 * 128 + 1, None), (6, 128 * 128 + 1, None),
               (6, 128 * 64 + 1, [0, 0, 1, 0, 0, 0])]


@pytest.mark.parametrize("D,N,man", SWEEP_CASES)
def test_groups_of_several_chunks_against_the_model(D, N, man):
    import torch
    rng = np.random.default_rng(7 * N + D)
    if man is None:
        a, b = _density(rng, D, N), _density(rng, D, SWEEP_M, shift=0.4)
    else:
        pa, _, ks, pb = cm.circular_case(7 * N + D, D, N, SWEEP_M, man, False)
        a, b = kdehip.kde(pa, ks, _weights(rng, N)), kdehip.kde(pb, ks[::-1].copy(), _weights(rng, SWEEP_M))
    sd = rng.uniform(0.3, 0.9, size=D)
    v = sd * sd
    A, B = _arrays(a), _arrays(b)
    got_v = kdehip.kernel_sum(a, b, v, manifold=man)
    _close(got_v, km.kernel_sum(A, B, v, False, man))            # explicit variances
    got_sum = kdehip.kernel_sum(a, b, manifold=man)
    _close(got_sum, km.kernel_sum(A, B, None, False, man))       # the summed leaf variances
    # normalised = sum_j b_j p(y_j) with p = kde(a's points, sqrt(v), a's weights), by evaluateDualTree
    p = kdehip.kde(A[0], sd, A[1])  # its variances are sd * sd == v, bit for bit
    want = math.fsum((B[1] * kdehip.evaluateDualTree(p, B[0], manifold=man)).tolist())
    _close(kdehip.kernel_sum(a, b, v, normalize=True, manifold=man), want)
    # host entry == resident entry == a batch whose first item is a small 1-D Euclidean one: the launch of a 6-D or circular
    # item then starts at a block offset (first[0] != 0), and a Euclidean 1-D item is the second of its launch
    small = kdehip.kde(np.array([[0.1, 0.4, -0.3]]), [0.3])
    with kdehip.DeviceDensity(a) as da, kdehip.DeviceDensity(b) as db, kdehip.DeviceDensity(small) as ds:
        assert kdehip.kernel_sum(da, db, v, manifold=man) == got_v
        assert kdehip.kernel_sum(da, db, manifold=man) == got_sum
        out = torch.full((3,), np.nan, dtype=torch.float64, device="cuda:0")
        kdehip.kernel_sum_device_batch([dict(a=ds, b=ds), dict(a=da, b=db, var=v, manifold=man),
                                        dict(a=da, b=db, manifold=man)], out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tolist() == [kdehip.kernel_sum(small, small), got_v, got_sum]
