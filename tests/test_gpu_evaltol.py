"""Evaluation within a tolerance on the GPU (csrc/evaltol.hip, include/kdehip.h section 5m): `evaluate_tol`,
`DeviceDensity.evaluate_tol` and the switch `setForceEvalDirect` against the direct evaluation, which stays as it is.

Bounds, none of them taken from the code under test:
  no tolerance  rel_tol = abs_tol = 0 visits every tile: bit for bit `evaluateDualTree`.
  the bound     direct (1 - rel_tol) - abs_tol - 1e-12 direct <= got <= direct (1 + 1e-12): section 5m's guarantee, with 1e-12
                the project's tolerance for sums of positive terms (tests/test_gpu_ksum.py) for "up to rounding".
  pruning       four clusters 40 apart, bandwidth 0.3: a chunk of another cluster is more than 100 bandwidths away, exp(a_min)
                underflows to 0 while tau_q > 0, so a query block of one cluster visits that cluster's two chunks of the eight:
                at most a quarter of the tiles (tests/evaltol_model.py gives exactly a quarter)."""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import evaltol_model as em
from tests.helpers import assert_chunks_per_group
from tests.test_evaltol_host import SHAPES, leaf_arrays, queries
from tests.test_gpu_mass import _density

pytestmark = pytest.mark.gpu

TOLS = [(1e-2, 0.0), (1e-2, 1e-30), (1e-6, 0.0), (1e-6, 1e-30)]
_CASES = {}


def _case(D, N, Nq, circular):
    """a density of one shape, its queries (as columns and as a density of their own), the direct values and every
    tolerance's values from the host entry: built once, shared, never changed"""
    key = (D, N, Nq, circular)
    if key not in _CASES:
        rng = np.random.default_rng(3000 * D + 10 * N + Nq)
        p = _density(rng, D, N)
        pos = queries(rng, p, Nq)
        at = kdehip.kde(pos, [1.0])
        man = ([0] * (D - 1) + [1]) if circular else None
        c = dict(p=p, pos=pos, at=at, man=man,
                 direct=kdehip.evaluateDualTree(p, pos, manifold=man),
                 direct_loo=kdehip.evaluateDualTree(p, lvFlag=True, manifold=man))
        for rel, ab in TOLS:
            c[(rel, ab)] = kdehip.evaluate_tol(p, at, rel, ab, manifold=man, return_stats=True)
            c[(rel, ab, "loo")] = kdehip.evaluate_tol(p, None, rel, ab, lvFlag=True, manifold=man, return_stats=True)
        _CASES[key] = c
    return _CASES[key]


def _bounded(got, direct, rel, ab):
    assert got.shape == direct.shape and np.all(np.isfinite(got))
    lower = direct * (1.0 - rel) - ab - 1e-12 * direct
    with np.errstate(divide="ignore", invalid="ignore"):
        print("rel_tol", rel, "abs_tol", ab, "largest loss (direct - got) / direct:",
              float(np.nanmax(np.where(direct > 0, (direct - got) / direct, 0.0))),
              "largest excess:", float(np.nanmax(np.where(direct > 0, (got - direct) / direct, 0.0))))
    assert np.all(got <= direct * (1.0 + 1e-12))
    assert np.all(got >= lower)


CASES = [(D, N, Nq, circular) for D, N, Nq in SHAPES for circular in (False, True)]
# N = 128 * 129 + 1: 130 chunks, so tol_plan_kernel stages a second tile of boxes (128 to a tile) and a row of flags has three
# words; a group of the sweep walks three chunks (asserted where the case is used, from the split restated in tests/helpers.py)
BIG = (2, 128 * 129 + 1, 300, False)


def _premise(D, N, Nq):
    if N == BIG[1]:
        assert_chunks_per_group(N, Nq, 3)
        assert_chunks_per_group(N, N, 5)  # leave-one-out: 65 query blocks, 32 groups


# ---- 1. no tolerance: the direct evaluation's bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq,circular", CASES + [BIG])
def test_no_tolerance_is_the_direct_evaluation_bit_for_bit(D, N, Nq, circular):
    _premise(D, N, Nq)
    c = _case(D, N, Nq, circular)
    p, man = c["p"], c["man"]
    total = ((Nq + 255) // 256) * ((N + 127) // 128)
    for order in ("tree", "given"):
        got, stats = kdehip.evaluate_tol(p, c["pos"], 0.0, 0.0, order=order, manifold=man, return_stats=True)
        assert np.array_equal(got, c["direct"]), order
        assert stats == (total, total)
    assert np.array_equal(kdehip.evaluate_tol(p, c["at"], 0.0, 0.0, manifold=man), c["direct"])
    got, stats = kdehip.evaluate_tol(p, None, 0.0, 0.0, lvFlag=True, manifold=man, return_stats=True)
    assert np.array_equal(got, c["direct_loo"])
    assert stats[0] == stats[1] == ((N + 255) // 256) * ((N + 127) // 128)
    assert np.array_equal(kdehip.evaluate_tol(p, p, 0.0, 0.0, manifold=man), c["direct_loo"])  # pos is bd: leave-one-out
    with kdehip.DeviceDensity(p) as d, kdehip.DeviceDensity(c["at"]) as a:
        assert np.array_equal(d.evaluate_tol(a, 0.0, 0.0, manifold=man), c["direct"])
        assert np.array_equal(d.evaluate_tol(None, 0.0, 0.0, manifold=man), c["direct_loo"])
        assert np.array_equal(kdehip.evaluate_tol(d, d, 0.0, 0.0, manifold=man), c["direct_loo"])


# ---- 2. the bound ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq,circular", CASES + [BIG])
def test_every_value_lies_within_the_tolerance_below_the_direct_one(D, N, Nq, circular):
    _premise(D, N, Nq)
    c = _case(D, N, Nq, circular)
    assert np.all(c["direct"] > 0.0) and np.all(c["direct_loo"] >= 0.0)
    for rel, ab in TOLS:
        got, stats = c[(rel, ab)]
        assert 0 < stats[0] <= stats[1] == ((Nq + 255) // 256) * ((N + 127) // 128)
        _bounded(got, c["direct"], rel, ab)
        got, stats = c[(rel, ab, "loo")]
        assert 0 < stats[0] <= stats[1]
        _bounded(got, c["direct_loo"], rel, ab)
        got = kdehip.evaluate_tol(c["p"], c["pos"], rel, ab, order="given", manifold=c["man"])
        _bounded(got, c["direct"], rel, ab)


@pytest.mark.parametrize("D,N,Nq,circular", [(2, 129, 257, False), (3, 300, 7, True), (2, 8200, 300, False)])
def test_a_nan_query_gets_nan_and_the_others_keep_the_bound(D, N, Nq, circular):
    c = _case(D, N, Nq, circular)
    pos = c["pos"].copy()
    pos[D - 1, 1] = np.nan
    for order in ("tree", "given"):
        got = kdehip.evaluate_tol(c["p"], pos, 1e-2, 0.0, order=order, manifold=c["man"])
        assert np.isnan(got[1]) and not np.isnan(np.delete(got, 1)).any()
        _bounded(np.delete(got, 1), np.delete(c["direct"], 1), 1e-2, 0.0)


@pytest.mark.parametrize("D,N,Nq,circular", [(1, 5, 3, False), (2, 129, 257, False), (6, 257, 5, False), (2, 8200, 300, False),
                                              BIG])
def test_queries_far_outside_the_data_get_the_direct_values(D, N, Nq, circular):
    """50 bandwidths beyond the data in every dimension: L_q underflows to 0, tau_q is 0, every chunk is needed"""
    if N == BIG[1]:
        assert_chunks_per_group(N, 5, 3)
    c = _case(D, N, Nq, circular)
    pts, _, v, _ = leaf_arrays(c["p"])
    far = (pts.max(axis=0) + 50.0 * np.sqrt(v))[:, None] + np.arange(3.0)[None, :]
    pos = np.concatenate([far, c["pos"][:, :2]], axis=1)
    direct = kdehip.evaluateDualTree(c["p"], pos)
    assert np.all(direct[:3] == 0.0) and np.all(direct[3:] > 0.0)
    for rel in (1e-2, 1e-6):
        for order in ("tree", "given"):
            got = kdehip.evaluate_tol(c["p"], pos, rel, 0.0, order=order)
            assert np.array_equal(got[:3], direct[:3])
            _bounded(got, direct, rel, 0.0)


# ---- 3. pruning happens ------------------------------------------------------------------------------------------------------
def test_separated_clusters_visit_at_most_a_quarter_of_the_tiles():
    rng = np.random.default_rng(2024)
    centres = np.array([[-20.0, -20.0], [-20.0, 20.0], [20.0, -20.0], [20.0, 20.0]])
    pts = np.concatenate([c[:, None] + rng.standard_normal((2, 256)) for c in centres], axis=1)
    pts = pts[:, rng.permutation(1024)]
    p = kdehip.kde(pts, [0.3])
    leaves, _, _, _ = leaf_arrays(p)
    # the premise: every aligned 128-leaf run of the density lies in one cluster
    which = (leaves[:, 0] > 0).astype(int) * 2 + (leaves[:, 1] > 0).astype(int)
    assert np.all(np.abs(np.abs(leaves) - 20.0) < 8.0)
    runs = which.reshape(8, 128)
    assert np.all(runs == runs[:, :1]) and sorted(runs[:, 0].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3]
    direct = kdehip.evaluateDualTree(p, lvFlag=True)
    got, stats = kdehip.evaluate_tol(p, None, 1e-3, lvFlag=True, return_stats=True)
    print("tiles visited / total:", stats)
    assert stats[1] == 32 and stats[0] > 0
    assert stats[0] * 4 <= stats[1]
    _bounded(got, direct, 1e-3, 0.0)
    with kdehip.DeviceDensity(p) as d:
        got_d, stats_d = d.evaluate_tol(None, 1e-3, return_stats=True)
    assert stats_d == stats and np.array_equal(got_d, got)


def test_separated_clusters_in_a_second_tile_of_boxes():
    """N = Nq = 128 * 129 + 1 in tree order, built like the test above: four clusters of 4128 points (one of 4129) 40 apart,
    bandwidth 0.3.  The tree splits at the median of the widest dimension, so the clusters are runs of leaves; the last run
    covers chunks 128 and 129, which the first tile of 128 boxes does not reach: the plan's second tile decides those flags.  The tiles visited are the model's (tests/evaltol_model.py) to the count."""
    N = 128 * 129 + 1
    assert_chunks_per_group(N, N, 5)  # (65 query blocks: 32 groups)
    rng = np.random.default_rng(2025)
    centres = np.array([[-20.0, -20.0], [-20.0, 20.0], [20.0, -20.0], [20.0, 20.0]])
    sizes = [N // 4 + (1 if j < N % 4 else 0) for j in range(4)]
    pts = np.concatenate([c[:, None] + rng.standard_normal((2, n)) for c, n in zip(centres, sizes)], axis=1)
    pts = pts[:, rng.permutation(N)]
    p = kdehip.kde(pts, [0.3])
    leaves, w, v, _ = leaf_arrays(p)
    # the premises, on the leaves and the model alone: some cluster lies wholly in chunks 128 and beyond, none of the chunks
    # below 120 holds a leaf of it, and pruning happens
    which = (leaves[:, 0] > 0).astype(int) * 2 + (leaves[:, 1] > 0).astype(int)
    assert np.all(np.abs(np.abs(leaves) - 20.0) < 8.0)
    tail = which[128 * 128:]
    assert np.all(tail == tail[0]) and not np.any(which[:128 * 96] == tail[0])
    pl = em.plan(leaves, w, v, leaves, 1e-3, 0.0, loo=True)
    want = (int(pl["visited"].sum()), int(pl["visited"].size))
    print("the model's tiles visited / total:", want)
    assert want[1] == ((N + 255) // 256) * 130 and 0 < want[0] * 3 <= want[1]
    assert pl["visited"][:, 128:].any() and not pl["visited"][:, 128:].all()
    direct = kdehip.evaluateDualTree(p, lvFlag=True)
    got, stats = kdehip.evaluate_tol(p, None, 1e-3, lvFlag=True, return_stats=True)
    print("tiles visited / total:", stats)
    assert stats == want
    _bounded(got, direct, 1e-3, 0.0)
    with kdehip.DeviceDensity(p) as d:
        got_d, stats_d = d.evaluate_tol(None, 1e-3, return_stats=True)
    assert stats_d == stats and np.array_equal(got_d, got)


# ---- 4. the entries agree, run after run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq,circular", CASES)
def test_the_resident_entry_returns_the_host_entrys_bits(D, N, Nq, circular):
    c = _case(D, N, Nq, circular)
    with kdehip.DeviceDensity(c["p"]) as d, kdehip.DeviceDensity(c["at"]) as a:
        for rel, ab in TOLS:
            host, hstats = c[(rel, ab)]
            got, stats = d.evaluate_tol(a, rel, ab, manifold=c["man"], return_stats=True)
            assert np.array_equal(got, host) and stats == hstats
            host, hstats = c[(rel, ab, "loo")]
            got, stats = d.evaluate_tol(None, rel, ab, manifold=c["man"], return_stats=True)
            assert np.array_equal(got, host) and stats == hstats
    rel, ab = TOLS[0]
    again, stats = kdehip.evaluate_tol(c["p"], c["at"], rel, ab, manifold=c["man"], return_stats=True)
    assert np.array_equal(again, c[(rel, ab)][0]) and stats == c[(rel, ab)][1]


# ---- 5. capture --------------------------------------------------------------------------------------------------------------
def test_the_resident_entry_replays_from_a_graph():
    import torch
    c = _case(2, 8200, 300, False)
    rel, ab = 1e-2, 0.0
    want, wstats = c[(rel, ab, "loo")]
    d = kdehip.DeviceDensity(c["p"])
    dev = torch.device("cuda", 0)
    out = torch.zeros(8200, dtype=torch.float64, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    rt, at = C.c_double(rel), C.c_double(ab)

    def call():
        _lib.check(_lib.lib.kdehip_evaluate_device_at_tol(d._h, d._h, C.byref(rt), C.byref(at), _lib.addr(out), _lib.addr(stats),
                                                          _lib.addr(torch.cuda.current_stream().cuda_stream), None))
    call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and tuple(stats.cpu().tolist()) == wstats
    # captured on ONE stream (sequential launches: no parallel branches) and replayed once
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        call()
    out.fill_(3.0)
    stats.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and tuple(stats.cpu().tolist()) == wstats
    del graph
    d.close()
    kdehip._clib.kdehip_clear_cache()  # (5h: the captured call's blocks are kept until here; the graph is gone)


# ---- 6. the switch -----------------------------------------------------------------------------------------------------------
def test_the_switch_routes_the_references_calls_to_the_tolerance():
    c = _case(2, 8200, 300, False)
    p, pos = c["p"], c["pos"]
    want = kdehip.evaluate_tol(p, pos, rel_tol=1e-2)
    assert np.array_equal(p(pos, False, 1e-2), c["direct"])  # the default: direct, errTol unread
    try:
        kdehip.setForceEvalDirect(False)
        assert np.array_equal(p(pos, False, 1e-2), want)
        assert np.array_equal(kdehip.evaluateDualTree(p, pos, False, 1e-2), want)
        assert np.array_equal(kdehip.evaluateDualTree(p, None, True, 1e-2), c[(1e-2, 0.0, "loo")][0])
    finally:
        kdehip.setForceEvalDirect(True)
    assert np.array_equal(p(pos, False, 1e-2), c["direct"])
