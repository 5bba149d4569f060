"""Compression by kernel herding on the GPU (csrc/compress.hip, include/kdehip.h section 5t): `compress`, `herding_order` and
`compress_batch` against tests/compress_model.py (NumPy fp64), and the routes, the host and resident entries and the batch
against each other bit for bit.

Tolerances, none of them taken from the code under test:
  idx           equal at every step.  PRECONDITION, asserted and never skipped: the model's margin (best score minus second
                best) at every step is at least 1e-9 * max_j z_j -- far above the 1e-12 the two sides' scores may differ by
  zpick, rpick, self_sum   1e-12 relative to their own value: every term is positive (the bound and the argument
                tests/test_gpu_ksum.py holds kernel_sum to); rpick of the first pick is exactly 0 on both sides
  the curve     1e-12 times the sum of the magnitudes of the three terms, as tests/test_gpu_ksum.py bounds mmd
The sizes: 129 and 257 leave a second chunk / a second query block with one leaf, every fifth weight is 0,
KDEHIP_COMPRESS_ONE_BLOCK_MAX + 1 is the first size the default sends to route B, and (3, 8193, 16) is where a group of the z
pass walks two chunks.  The seeds are fixed so that every step of every shape meets the precondition (the smallest relative
margins lie between 4.6e-6 and 4.7e-4 at the five shapes).  Each case runs in well under a second on the device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import compress_model as cm
from tests.helpers import chunks_per_group

pytestmark = pytest.mark.gpu

SHAPES = [(1, 129, 16), (2, 257, 32), (3, 300, 30), (6, 513, 64), (8, 130, 13)]
SEEDS = {(1, 129): 1}   # (the default seed of the 1-D shape leaves a margin of 9.5e-9)
KS = 0.4
LIMIT = int(re.search(r"#define KDEHIP_COMPRESS_ONE_BLOCK_MAX (\d+)",
                      open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kdehip.h")).read()).group(1))
_CASES = {}


def _leaf_var(p):
    N, D = p.bt.num_points, p.bt.dims
    return np.array(p.bandwidth[N * D:N * D + D])


def _case(D, N):
    """a weighted density of one shape and the model's view of it (its own points and weights, by original point): built
    once, shared, never changed; the model's answers are kept by their arguments"""
    if (D, N) not in _CASES:
        pts, w = cm.two_clusters(D, N, seed=SEEDS.get((D, N)))
        p = kdehip.kde(pts, [KS], w)
        _CASES[(D, N)] = dict(p=p, pts=kdehip.getPoints(p), w=kdehip.getWeights(p), var=2.0 * _leaf_var(p), model={}, dev=None)
    return _CASES[(D, N)]


def _model(c, M, var=None, man=None):
    v = c["var"] if var is None else np.asarray(var, dtype=np.float64)
    key = (M, v.tobytes(), None if man is None else tuple(man))
    if key not in c["model"]:
        c["model"][key] = cm.herd(c["pts"], c["w"], v, M, man)
    return c["model"][key]


def _resident(c):
    if c["dev"] is None:
        c["dev"] = kdehip.DeviceDensity(c["p"])
    return c["dev"]


def _rel12(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    print(f"{name}: max relative difference {np.max(diff / np.maximum(np.abs(want), 1e-300)):.3e}")
    assert np.all(np.isfinite(got)) and np.all(diff <= 1e-12 * np.abs(want)), (name, float(diff.max()))


def _check_model(info, want):
    big = float(want["z"].max())
    print(f"smallest relative margin {want['margin'].min() / big:.3e}")
    assert np.all(want["margin"] >= 1e-9 * big), "the precondition: a step of the model is too close to a tie"
    assert np.array_equal(info["idx"], want["idx"])
    _rel12("zpick", info["zpick"], want["zpick"])
    _rel12("rpick", info["rpick"], want["rpick"])
    _rel12("self_sum", info["self_sum"], want["self_sum"])
    assert info["rpick"][0] == 0.0


def _same_bits(a, b):
    assert np.array_equal(a["idx"], b["idx"])
    for name in ("zpick", "rpick", "mmd2"):
        assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name
    assert a["self_sum"] == b["self_sum"]


# ---- G1: against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g1_picks_and_traces_equal_the_model(D, N, M):
    c = _case(D, N)
    idx, info = c["p"].herding_order(M)
    assert idx is info["idx"] and idx.dtype == np.int64 and len(idx) == M
    _check_model(info, _model(c, M))
    assert len(set(idx.tolist())) == M and idx.min() >= 1 and idx.max() <= N


# ---- G2: the routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g2_stepwise_route_gives_the_same_bits(D, N, M):
    c = _case(D, N)
    assert N <= LIMIT
    _same_bits(c["p"].herding_order(M, stepwise=True)[1], c["p"].herding_order(M)[1])


def test_g2_just_above_the_limit_the_default_is_stepwise():
    c = _case(2, LIMIT + 1)
    info = c["p"].herding_order(16)[1]
    _check_model(info, _model(c, 16))
    _same_bits(c["p"].herding_order(16, stepwise=True)[1], info)


def test_g2_a_group_of_the_z_pass_walks_two_chunks():
    assert chunks_per_group(8193, 8193) == 2
    c = _case(3, 8193)
    _check_model(c["p"].herding_order(16)[1], _model(c, 16))


# ---- G3: anytime ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepwise", [False, True])
@pytest.mark.parametrize("D,N,M", [(2, 257, 32), (6, 513, 64)])
def test_g3_a_shorter_run_is_a_prefix(D, N, M, stepwise):
    c = _case(D, N)
    full = c["p"].herding_order(M, stepwise=stepwise)[1]
    for m in (1, M // 2, M - 1):
        short = c["p"].herding_order(m, stepwise=stepwise)[1]
        assert np.array_equal(short["idx"], full["idx"][:m])
        for name in ("zpick", "rpick", "mmd2"):
            assert short[name].tobytes() == full[name][:m].tobytes(), (m, name)
        assert short["self_sum"] == full["self_sum"]


# ---- G4: ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepwise", [False, True])
def test_g4_equal_points_are_picked_in_index_order(stepwise):
    p = kdehip.kde(np.tile(np.array([[0.3], [-1.2]]), (1, 300)), [KS])
    idx, info = p.herding_order(40, stepwise=stepwise)
    assert idx.tolist() == list(range(1, 41))
    assert np.array_equal(info["rpick"], np.arange(40.0)) and np.all(info["zpick"] == info["zpick"][0])


@pytest.mark.parametrize("stepwise", [False, True])
def test_g4_the_lower_copy_of_a_doubled_point_goes_first(stepwise):
    base, w = cm.two_clusters(3, 150, seed=77)
    p = kdehip.kde(np.hstack([base, base]), [KS], np.concatenate([w, w]))
    idx = p.herding_order(200, stepwise=stepwise)[0]
    seen = set()
    uppers = 0
    for i in idx.tolist():
        if i > 150:
            assert i - 150 in seen, i
            uppers += 1
        seen.add(i)
    assert uppers > 0   # (200 picks of 150 distinct points: some copy is taken)


# ---- G5: the ends --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepwise", [False, True])
def test_g5_all_points_one_point_and_a_single_point_density(stepwise):
    c = _case(8, 130)
    idx = c["p"].herding_order(130, stepwise=stepwise)[0]
    assert sorted(idx.tolist()) == list(range(1, 131))
    z = _model(c, 13)["z"]
    top = np.sort(z)[-2:]
    assert top[1] - top[0] >= 1e-9 * top[1]
    one, info = c["p"].herding_order(1, stepwise=stepwise)
    assert one.tolist() == [int(np.argmax(z)) + 1] and info["rpick"][0] == 0.0
    single = kdehip.kde(np.array([[0.5], [1.5]]), [KS])
    idx, info = single.herding_order(1, stepwise=stepwise)
    assert idx.tolist() == [1] and info["zpick"][0] == 1.0 and info["self_sum"] == 1.0 and info["mmd2"][0] == 0.0
    q = single.compress(1)
    assert q.bt.num_points == 1 and np.array_equal(kdehip.getPoints(q), kdehip.getPoints(single))


# ---- G6: the curve -------------------------------------------------------------------------------------------------------------
BW = 0.55


def _three_terms(p, q, bw):
    v = np.full(p.bt.dims, bw * bw)
    return kdehip.kernel_sum(p, p, v), kdehip.kernel_sum(p, q, v), kdehip.kernel_sum(q, q, v)


@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g6_the_curve_ends_at_the_mmd_of_the_result(D, N, M):
    c = _case(D, N)
    q, info = c["p"].compress(M, bw=BW, return_info=True)
    assert q.bt.num_points == M and info["M"] == M and info["reached"] and len(info["mmd2"]) == M
    pp, pq, qq = _three_terms(c["p"], q, BW)
    mag = pp + 2.0 * pq + qq
    got = kdehip.mmd(c["p"], q, BW)
    print(f"mmd2 {info['mmd2'][-1]:.6e} against {got:.6e}")
    assert abs(info["mmd2"][-1] - got) <= 1e-12 * mag
    assert abs(info["self_sum"] - pp) <= 1e-12 * pp
    own = kdehip.kernel_sum(c["p"], c["p"], c["var"])                            # the default kernel: twice the leaf variance
    assert abs(c["p"].herding_order(M)[1]["self_sum"] - own) <= 1e-12 * own


def test_g6_mmd_tol_returns_the_shortest_prefix_that_reaches_it():
    c = _case(3, 300)
    full = c["p"].herding_order(60, bw=BW)[1]
    curve = full["mmd2"]
    tol = math.sqrt(curve[20]) * (1.0 + 1e-12)                                      # reached after 21 picks at the latest
    first = int(np.nonzero(curve <= tol ** 2)[0][0]) + 1
    assert 1 < first <= 21
    q, info = c["p"].compress(60, mmd_tol=tol, bw=BW, return_info=True)
    assert info["reached"] and info["M"] == first and q.bt.num_points == first
    assert np.all(curve[:first - 1] > tol ** 2) and curve[first - 1] <= tol ** 2
    assert np.array_equal(info["idx"], full["idx"]) and len(info["mmd2"]) == 60      # the whole run is reported
    want = kdehip.kde(c["pts"][:, full["idx"][:first] - 1], [KS], np.full(first, 1.0 / first))
    assert np.array_equal(q.means, want.means) and np.array_equal(q.bt.weights, want.bt.weights)
    q, info = c["p"].compress(10, mmd_tol=1e-9, bw=BW, return_info=True)              # out of reach in 10 picks
    assert not info["reached"] and info["M"] == 10 and q.bt.num_points == 10
    q = c["p"].compress(mmd_tol=tol, bw=BW)                                            # M defaults to N
    assert q.bt.num_points == first


# ---- G7: quality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,M", [(2, 300, 30), (6, 513, 64)])
def test_g7_herding_beats_random_subsets(D, N, M):
    c = _case(D, N)
    bw = math.sqrt(2.0) * KS
    herded = kdehip.mmd(c["p"], c["p"].compress(M), bw)
    rng = np.random.default_rng(5)
    rnd = []
    for _ in range(20):
        sub = rng.choice(N, size=M, replace=False, p=c["w"])
        rnd.append(kdehip.mmd(c["p"], kdehip.kde(c["pts"][:, sub], [KS]), bw))
    print(f"herded {herded:.4e}, random mean {np.mean(rnd):.4e}, best {np.min(rnd):.4e}")
    assert herded < np.mean(rnd)


# ---- G8: resident, host and batch --------------------------------------------------------------------------------------------
def _arrays_equal(a, b):
    for name in ("means", "bandwidth", "bandwidthMin", "bandwidthMax"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation"):
        assert np.array_equal(getattr(a.bt, name), getattr(b.bt, name)), name


@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g8_resident_equals_host(D, N, M):
    c = _case(D, N)
    d = _resident(c)
    host = c["p"].herding_order(M)[1]
    _same_bits(d.herding_order(M)[1], host)
    _same_bits(d.herding_order(M, stepwise=True)[1], host)
    ks = np.linspace(0.3, 0.5, D)
    with d.compress(M, ks=ks) as q:
        assert q.num_points == M and q.dims == D
        _arrays_equal(q.download(), kdehip.kde(c["pts"][:, host["idx"] - 1], ks, np.full(M, 1.0 / M)))
    with d.compress(M) as q:                                                     # ks = None: the bandwidth stays
        _arrays_equal(q.download(), c["p"].compress(M))
    q, info = d.compress(M, return_info=True)
    with q:
        _same_bits(info, host)


def _circular_case():
    if "circ" not in _CASES:
        pts, w = cm.cut_pair()
        p = kdehip.kde(pts, [0.5, 0.35], w)
        _CASES["circ"] = dict(p=p, pts=kdehip.getPoints(p), w=kdehip.getWeights(p), var=2.0 * _leaf_var(p), model={}, dev=None)
    return _CASES["circ"]


MAN = ["euclid", "circular"]


def test_g8_a_batch_equals_the_single_calls():
    import torch
    cases = [(_case(D, N), M, None, False) for D, N, M in SHAPES]
    cases.append((_circular_case(), 20, MAN, False))
    cases.append((_case(2, 257), 32, None, True))                                  # one item on route B
    items = [dict(density=_resident(c), M=M, manifold=man, stepwise=sw) for c, M, man, sw in cases]
    out = kdehip.DeviceDensity.compress_batch(items, None, return_info=True)
    assert len(out) == len(cases)
    for (c, M, man, sw), (q, info) in zip(cases, out):
        with q:
            single = _resident(c).herding_order(M, manifold=man)[1]
            _same_bits(info, single)
            _arrays_equal(q.download(), c["p"].compress(M, manifold=man))
    # d_points of the entry itself: the gathered leaves, in pick order
    c = _case(3, 300)
    d = _resident(c)
    dev = torch.device("cuda", d.device)
    d_idx = torch.empty(30, dtype=torch.int64, device=dev)
    d_pts = torch.empty((30, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(_lib.lib.kdehip_compress_device(d._h, 30, None, 0, _lib.addr(d_idx), _lib.addr(d_pts), None, None, None, None))
    idx = d_idx.cpu().numpy()
    assert np.array_equal(idx, c["p"].herding_order(30)[0])
    assert np.array_equal(d_pts.cpu().numpy().T, c["pts"][:, idx - 1])
    plain = kdehip.DeviceDensity.compress_batch([_resident(c)], 30)
    with plain[0] as q:
        _arrays_equal(q.download(), c["p"].compress(30))


# ---- G9: circular ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepwise", [False, True])
def test_g9_differences_wrap_across_the_cut(stepwise):
    c = _circular_case()
    want = _model(c, 20, man=[0, 1])
    info = c["p"].herding_order(20, manifold=MAN, stepwise=stepwise)[1]
    _check_model(info, want)
    line = c["p"].herding_order(20)[1]
    assert info["self_sum"] > 1.2 * line["self_sum"]      # (on the line the two sides of the cut do not see each other)
    _same_bits(_resident(c).herding_order(20, manifold=MAN)[1], info)


# ---- G10: scale and translation -------------------------------------------------------------------------------------------------
def _bits(info):
    return info["idx"].tobytes(), info["zpick"].tobytes(), info["rpick"].tobytes(), np.float64(info["self_sum"]).tobytes()


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("k", [-80, -30, 30, 80])
def test_g10_rescaling_by_a_power_of_two_changes_no_bit(k, explicit):
    """points, bandwidth and bw times 2^k exactly: every difference, its square and -0.5 / v scale exactly, the exponent keeps
    its bits and with it z, r, the scores and the picks"""
    pts, w = cm.two_clusters(3, 300)
    bw = [0.5, 0.6, 0.7] if explicit else None
    base = kdehip.kde(pts, [KS], w).herding_order(30, bw=bw)[1]
    got = kdehip.kde(np.ldexp(pts, k), [math.ldexp(KS, k)], w).herding_order(30, bw=None if bw is None else np.ldexp(bw, k))[1]
    assert _bits(got) == _bits(base)


@pytest.mark.parametrize("stepwise", [False, True])
def test_g10_an_exact_translation_changes_no_bit(stepwise):
    """coordinates on the 2^-10 grid below 2^4, moved by 2^10 (x + t is exact): every difference is the untranslated one"""
    pts, w = cm.two_clusters(3, 300, grid=2.0 ** -10)
    assert np.abs(pts).max() < 16.0
    t = np.array([[2.0 ** 10], [-(2.0 ** 10)], [2.0 ** 10]])
    assert np.array_equal((pts + t) - t, pts)
    base = kdehip.kde(pts, [KS], w).herding_order(30, stepwise=stepwise)[1]
    got = kdehip.kde(pts + t, [KS], w).herding_order(30, stepwise=stepwise)[1]
    assert _bits(got) == _bits(base)


# ---- G11: refusals that need a real handle ----------------------------------------------------------------------------------------
def test_g11_refusals_of_resident_densities():
    import torch
    c = _case(2, 257)
    d = _resident(c)
    sd = np.full((2, 257), KS)
    sd[0, 3] *= 2.0
    with kdehip.DeviceDensity(kdehip.kde_varbw(c["pts"], sd, c["w"])) as v:
        with pytest.raises(kdehip.KdeHipError) as e:
            v.herding_order(8)
        assert e.value.code == _lib.ERR_UNSUPPORTED and "per-point" in str(e.value)
        with pytest.raises(kdehip.KdeHipError) as e:
            v.compress(8, bw=0.5)                      # the kernel is given, the result's bandwidth is not
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert len(v.herding_order(8, bw=0.5)[0]) == 8   # with variances it runs
    dev = torch.device("cuda", d.device)
    d_idx = torch.empty(8, dtype=torch.int64, device=dev)
    items = (_lib.CCompressItem * 1)()
    items[0].p, items[0].M, items[0].d_idx, items[0].circular_mask = d._h, 8, d_idx.data_ptr(), 1 << 2   # a bit at ndims
    assert _lib.lib.kdehip_compress_device_batch(1, items) == _lib.ERR_ARG
    assert "circular_mask" in _lib.lib.kdehip_last_error().decode()
    h = C.c_void_p()
    for M in (0, 258):
        assert _lib.lib.kdehip_density_compress_device(C.byref(h), d._h, M, None, None, None, None) == _lib.ERR_ARG and not h.value
    three = np.array([0, 0, 1], dtype=np.uint8)   # a manifold of another dimension count is the front end's to refuse
    with pytest.raises(ValueError):
        d.herding_order(8, manifold=three)
    with pytest.raises(ValueError):
        d.compress(8, bw=[0.5, 0.5, 0.5])
