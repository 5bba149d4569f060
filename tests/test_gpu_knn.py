"""Nearest neighbours on the GPU (csrc/knn.hip, include/kdehip.h section 5n): `knn`, `DeviceDensity.knn`, `entropy_knn` and
`kld_knn` against tests/knn_model.py, which tests/test_knn_host.py checks against closed forms.

Nothing here has a tolerance but the estimators: the search is exact, so indices are compared with `==`, squared distances
with np.array_equal (the contract's distance is a chain of correctly rounded operations, which the model restates to the bit),
and the tile counts with the model's plan.  The estimators are sums of N logarithms: 1e-12, the project's tolerance for sums
(tests/test_gpu_ksum.py).  Section 8 has the sizes at which a row of flags has more than one word and the boxes more than one tile
(N = 128 * 64 + 1, 128 * 129 + 1); the model runs its leave-one-out there in row blocks."""
import ctypes as C
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import knn_model as km
from tests.helpers import assert_chunks_per_group
from tests.test_gpu_evaltol import leaf_arrays

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 3), (3, 129, 257), (2, 300, 64), (8, 384, 100)]  # (D, N, Nq)
VARIANTS = ["euclid", "scale", "circular"]
_CASES = {}


def _column(rng, n, circular):
    """n values of one dimension: two clusters, or -- circular -- angles straddling +-pi"""
    if circular:
        return km.wrap(math.pi + 0.4 * rng.standard_normal(n))
    x = rng.standard_normal(n)
    x[n // 2:] += 3.0
    return x


def _case(D, N, Nq, variant):
    """a density of one shape, its queries, the model's distance matrices (queries and leave-one-out): built once, shared,
    never changed"""
    key = (D, N, Nq, variant)
    if key not in _CASES:
        rng = np.random.default_rng(5000 * D + 10 * N + Nq)
        circular = variant == "circular"
        pts = np.stack([_column(rng, N, circular and j == D - 1) for j in range(D)])
        pos = np.stack([_column(rng, Nq, circular and j == D - 1) for j in range(D)])
        if circular:  # query 0 just inside -pi, point 2 just inside +pi and otherwise on top of it
            pos[D - 1, 0] = -math.pi + 1e-3
            pts[:, 2] = pos[:, 0]
            pts[D - 1, 2] = math.pi - 1e-3
        p = kdehip.kde(pts, [0.5])
        leaves, _, _, where = leaf_arrays(p)
        scale = rng.uniform(0.3, 3.0, size=D) if variant == "scale" else None
        circ = (D - 1,) if circular else ()
        _CASES[key] = dict(p=p, pts=pts, pos=pos, leaves=leaves, where=where, orig=where + 1, scale=scale, circ=circ,
                           man=([0] * (D - 1) + [1]) if circular else None,
                           metric="euclid" if scale is None else scale,
                           d2=km.all_dist2(leaves, np.ascontiguousarray(pos.T), scale, circ),
                           d2_loo=km.all_dist2(leaves, leaves, scale, circ))
    return _CASES[key]


def _expected(c, k, loo):
    """the model's (d2 (k, Nq), idx (k, Nq)) in the caller's order and its tile counts for the given processing order"""
    qry = c["leaves"] if loo else np.ascontiguousarray(c["pos"].T)
    kw = dict(loo=loo, scale=c["scale"], circ=c["circ"], d2=c["d2_loo"] if loo else c["d2"])
    d2, idx = km.knn(c["leaves"], c["orig"], qry, k, **kw)
    stats = km.plan(c["leaves"], c["orig"], qry, k, **kw)["stats"]
    if loo:  # leaf q is original point where[q]
        back = np.argsort(c["where"])
        d2, idx = d2[back], idx[back]
    return d2.T, idx.T, stats


def _same(got, want):
    d2, idx, stats = got
    wd2, widx, wstats = want
    assert idx.shape == widx.shape and d2.shape == wd2.shape
    assert np.array_equal(idx, widx)
    assert np.array_equal(d2, wd2, equal_nan=True)
    assert stats == wstats


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D,N,Nq", SHAPES)
def test_the_search_is_brute_force_bit_for_bit(D, N, Nq, variant):
    c = _case(D, N, Nq, variant)
    kw = dict(metric=c["metric"], manifold=c["man"], squared=True, return_stats=True)
    for k in sorted({k for k in (1, 8, 32, N if N == 5 else 1) if k <= N}):
        _same(kdehip.knn(c["p"], c["pos"], k=k, order="given", **kw), _expected(c, k, False))
    for k in sorted({k for k in (1, 8, 32, N - 1 if N == 5 else 1) if k <= N - 1}):
        _same(kdehip.knn(c["p"], k=k, lvFlag=True, **kw), _expected(c, k, True))
    if variant == "circular":  # the query just inside -pi finds the point just inside +pi
        d2, idx = kdehip.knn(c["p"], c["pos"], k=1, manifold=c["man"], squared=True)
        assert idx[0, 0] == 3 and abs(d2[0, 0] - 4e-6) < 1e-9
    dist, idx = kdehip.knn(c["p"], c["pos"], k=1, metric=c["metric"], manifold=c["man"])  # the default: distances
    assert np.array_equal(dist, np.sqrt(_expected(c, 1, False)[0]))


def test_metric_bandwidth_is_the_scale_of_the_variances():
    c = _case(2, 300, 64, "euclid")
    got = kdehip.knn(c["p"], c["pos"], k=8, metric="bandwidth", squared=True)
    want = kdehip.knn(c["p"], c["pos"], k=8, metric=1.0 / np.full(2, 0.25), squared=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    d2, idx = km.knn(c["leaves"], c["orig"], np.ascontiguousarray(c["pos"].T), 8, scale=np.full(2, 4.0))
    assert np.array_equal(got[0], d2.T) and np.array_equal(got[1], idx.T)


# ---- 2. the nearest chunk is too small ---------------------------------------------------------------------------------------
def test_a_nearest_chunk_with_fewer_than_k_leaves_visits_everything():
    rng = np.random.default_rng(130)
    pts = rng.standard_normal((2, 130))
    pts[:, 5] = [100.0, 0.3]  # two outliers: the two leaves of the last chunk
    pts[:, 77] = [100.5, -0.2]
    p = kdehip.kde(pts, [0.5])
    leaves, _, _, where = leaf_arrays(p)
    assert sorted(where[128:].tolist()) == [5, 77]
    pos = leaves[128:].mean(axis=0)[:, None]
    pl = km.plan(leaves, where + 1, np.ascontiguousarray(pos.T), 8)
    assert pl["cstar"][0] == 1 and pl["r"][0] == np.inf and pl["stats"] == (2, 2)  # the premise, on the model alone
    d2, idx, stats = kdehip.knn(p, pos, k=8, squared=True, return_stats=True)
    wd2, widx = km.knn(leaves, where + 1, np.ascontiguousarray(pos.T), 8)
    assert stats == (2, 2)
    assert np.array_equal(idx, widx.T) and np.array_equal(d2, wd2.T)
    assert sorted(idx[:2, 0].tolist()) == [6, 78]


# ---- 3. ties -----------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_original_index():
    rng = np.random.default_rng(4)
    base = rng.standard_normal((2, 64))
    pts = np.concatenate([base] * 4, axis=1)[:, rng.permutation(256)]  # every point four times
    p = kdehip.kde(pts, [0.5])
    leaves, _, _, where = leaf_arrays(p)
    pos = base[:, :40]  # queries ON data points
    for order in ("given", "tree"):
        d2, idx = kdehip.knn(p, pos, k=8, order=order, squared=True)
        wd2, widx = km.knn(leaves, where + 1, np.ascontiguousarray(pos.T), 8)
        assert np.array_equal(idx, widx.T) and np.array_equal(d2, wd2.T)
        assert np.all(d2[:4] == 0.0) and np.all(np.diff(idx[:4], axis=0) > 0)  # the four copies, ascending index
    # leave-one-out is by index: the other three copies stay, at distance 0
    d2, idx = kdehip.knn(p, k=3, lvFlag=True, squared=True)
    assert np.all(d2 == 0.0)
    for i in range(256):
        copies = np.nonzero((pts == pts[:, i:i + 1]).all(axis=0))[0] + 1
        assert idx[:, i].tolist() == [j for j in copies.tolist() if j != i + 1]


# ---- 4. non-finite queries ---------------------------------------------------------------------------------------------------
def test_a_non_finite_query_gets_nan_and_index_zero():
    c = _case(3, 129, 257, "euclid")
    pos = c["pos"].copy()
    pos[2, 1] = np.nan
    pos[0, 200] = np.inf
    clean = kdehip.knn(c["p"], c["pos"], k=8, order="given", squared=True)
    for order in ("tree", "given"):
        d2, idx = kdehip.knn(c["p"], pos, k=8, order=order, squared=True)
        for q in (1, 200):
            assert np.isnan(d2[:, q]).all() and np.all(idx[:, q] == 0)
        keep = np.delete(np.arange(257), [1, 200])
        assert np.array_equal(d2[:, keep], clean[0][:, keep]) and np.array_equal(idx[:, keep], clean[1][:, keep])
    wd2, widx = km.knn(c["leaves"], c["orig"], np.ascontiguousarray(pos.T), 8)
    assert np.array_equal(d2, wd2.T, equal_nan=True) and np.array_equal(idx, widx.T)


# ---- 5. pruning happens ------------------------------------------------------------------------------------------------------
def test_separated_clusters_visit_a_quarter_of_the_tiles():
    """the construction of tests/test_gpu_evaltol.py: four clusters 40 apart, 256 points each, N = Nq = 1024 in tree order"""
    rng = np.random.default_rng(2024)
    centres = np.array([[-20.0, -20.0], [-20.0, 20.0], [20.0, -20.0], [20.0, 20.0]])
    pts = np.concatenate([c[:, None] + rng.standard_normal((2, 256)) for c in centres], axis=1)
    pts = pts[:, rng.permutation(1024)]
    p = kdehip.kde(pts, [0.3])
    leaves, _, _, where = leaf_arrays(p)
    pl = km.plan(leaves, where + 1, leaves, 8, loo=True)
    print("the model's tiles visited / total:", pl["stats"])
    assert pl["stats"][1] == 32 and 0 < pl["stats"][0] * 4 <= pl["stats"][1]  # the cap, on the model alone
    d2, idx, stats = kdehip.knn(p, k=8, lvFlag=True, squared=True, return_stats=True)
    print("tiles visited / total:", stats)
    assert stats == pl["stats"]
    wd2, widx = km.knn(leaves, where + 1, leaves, 8, loo=True)
    back = np.argsort(where)
    assert np.array_equal(idx, widx[back].T) and np.array_equal(d2, wd2[back].T)


# ---- 6. the entries agree, run after run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D,N,Nq", SHAPES[1:])
def test_the_orders_and_the_resident_entry_return_the_same_arrays(D, N, Nq, variant):
    c = _case(D, N, Nq, variant)
    kw = dict(k=8, metric=c["metric"], manifold=c["man"], squared=True)
    given = kdehip.knn(c["p"], c["pos"], order="given", **kw)
    tree = kdehip.knn(c["p"], c["pos"], order="tree", **kw)
    assert np.array_equal(given[0], tree[0]) and np.array_equal(given[1], tree[1])
    at = kdehip.kde(c["pos"], [1.0])
    as_density = kdehip.knn(c["p"], at, **kw)
    assert np.array_equal(given[0], as_density[0]) and np.array_equal(given[1], as_density[1])
    loo = kdehip.knn(c["p"], lvFlag=True, return_stats=True, **kw)
    is_bd = kdehip.knn(c["p"], c["p"], **kw)  # pos is bd: leave-one-out
    assert np.array_equal(loo[0], is_bd[0]) and np.array_equal(loo[1], is_bd[1])
    with kdehip.DeviceDensity(c["p"]) as d, kdehip.DeviceDensity(at) as a:
        host = kdehip.knn(c["p"], at, return_stats=True, **kw)  # (processed in at's leaf order, as the resident entry does)
        got = d.knn(a, return_stats=True, **kw)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]) and got[2] == host[2]
        for got in (d.knn(None, return_stats=True, **kw), d.knn(d, return_stats=True, **kw),
                    kdehip.knn(d, lvFlag=True, return_stats=True, **kw)):
            assert np.array_equal(got[0], loo[0]) and np.array_equal(got[1], loo[1]) and got[2] == loo[2]


def test_the_resident_entry_replays_from_a_graph():
    import torch
    c = _case(2, 300, 64, "euclid")
    k = 8
    want = kdehip.knn(c["p"], k=k, lvFlag=True, squared=True, return_stats=True)
    d = kdehip.DeviceDensity(c["p"])
    dev = torch.device("cuda", 0)
    d2 = torch.zeros(300 * k, dtype=torch.float64, device=dev)
    idx = torch.zeros(300 * k, dtype=torch.int64, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)

    def call():
        _lib.check(_lib.lib.kdehip_knn_device_at(d._h, d._h, k, None, _lib.addr(d2), _lib.addr(idx), _lib.addr(stats),
                                                 _lib.addr(torch.cuda.current_stream().cuda_stream), None))

    def check():
        torch.cuda.synchronize()
        assert np.array_equal(d2.cpu().numpy().reshape(300, k).T, want[0])
        assert np.array_equal(idx.cpu().numpy().reshape(300, k).T, want[1])
        assert tuple(stats.cpu().tolist()) == want[2]
    call()
    check()
    # captured on ONE stream (sequential launches: no parallel branches) and replayed twice
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        call()
    for fill in (3, 5):
        d2.fill_(float(fill))
        idx.fill_(-fill)
        stats.fill_(-1)
        graph.replay()
        check()
    del graph
    d.close()
    kdehip._clib.kdehip_clear_cache()  # (5h: the captured call's block is kept until here; the graph is gone)


# ---- 7. the estimators -------------------------------------------------------------------------------------------------------
def test_the_estimators_are_the_models_formulas_of_the_models_distances():
    rng = np.random.default_rng(77)
    D, n, m, k = 3, 600, 500, 4
    P, Q = rng.standard_normal((D, n)), 0.5 + 1.3 * rng.standard_normal((D, m))
    p, q = kdehip.kde(P, [0.4]), kdehip.kde(Q, [0.4])
    # the model's distances in original point order (the sums do not depend on it: math.fsum)
    rho = np.sqrt(np.sort(km.dist2(P.T, P.T) + np.diag(np.full(n, np.inf)), axis=1)[:, k - 1])
    nu = np.sqrt(np.sort(km.dist2(Q.T, P.T), axis=1)[:, k - 1])
    want_h, want_d = km.entropy_kl(rho, D, k), km.kld_wkv(rho, nu, D, m)
    print("entropy_knn:", kdehip.entropy_knn(p, k), "model:", want_h, "| kld_knn:", kdehip.kld_knn(p, q, k), "model:", want_d)
    assert abs(kdehip.entropy_knn(p, k) - want_h) <= 1e-12
    assert abs(kdehip.kld_knn(p, q, k) - want_d) <= 1e-12
    assert kdehip.kld_knn(p, p, k) == 0.0
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert abs(kdehip.entropy_knn(dp, k) - want_h) <= 1e-12
        assert abs(kdehip.kld_knn(dp, dq, k) - want_d) <= 1e-12
        assert kdehip.kld_knn(dp, dp, k) == 0.0
        with pytest.raises(TypeError):
            kdehip.kld_knn(p, dq, k)
    dup = kdehip.kde(np.concatenate([P[:, :50]] * 5, axis=1), [0.4])  # every point has k = 4 duplicates: -inf
    assert kdehip.entropy_knn(dup, k) == -np.inf


# ---- 8. more than one flag word, more than one box tile ----------------------------------------------------------------------
# A row of the plan's flags has one 64-bit word per 64 chunks and the boxes are staged in tiles of 128 chunks, so with the
# sizes above (at most 8 chunks) the second word, `next()` crossing a word, the second tile (`c0 > 0`) and a group of the sweep
# that walks more than one chunk never ran.
#   N = 128 * 64 + 1   65 chunks: two flag words, the second holding one chunk of one leaf; a group of the sweep walks 2 chunks
#   N = 128 * 129 + 1  130 chunks: a second box tile of two boxes, three flag words, a last chunk of one leaf; 3 chunks a group
# (N - 1) % 128 == 0 in both: in leave-one-out the last leaf is alone in its chunk, at 16513 in the second tile.
# The points are the module's clustered columns with the first 256 and the last 128 moved 40 away along dimension 0, so that
# tree order separates them.  Queries 0 .. 127 lie beside the first 128 leaves and queries 128 .. 255 beside some of the last 120 but
# the lone last one:
# the first query block needs chunks at both ends of the row and nothing in between, and `next()` jumps over the words
# between them; the other 44 queries are clustered columns again.
BIG_SHAPES = {8193: (2, 300, ("euclid", "circular"), (1, 8, 32)), 16513: (3, 300, ("euclid", "scale"), (1, 8))}
_BIG = {}


def _big_case(N, variant):
    if (N, variant) not in _BIG:
        D, Nq, _, _ = BIG_SHAPES[N]
        rng = np.random.default_rng(5000 * D + 10 * N + Nq)
        circular = variant == "circular"
        pts = np.stack([_column(rng, N, circular and j == D - 1) for j in range(D)])
        pts[0, :256] -= 40.0   # the tree splits at the median of the widest dimension, the lower values to the left: these
        pts[0, -128:] += 40.0  # become the first 256 leaves or so (chunks 0, 1) and the last 128 (what the plan makes of it is
        #                        asserted on the model where it is used)
        p = kdehip.kde(pts, [0.5])
        leaves, _, _, where = leaf_arrays(p)
        pos = np.stack([_column(rng, Nq, circular and j == D - 1) for j in range(D)])
        pos[:, :128] = leaves[:128].T + 0.01 * rng.standard_normal((D, 128))
        pos[:, 128:256] = leaves[rng.integers(N - 120, N - 1, size=128)].T + 0.01 * rng.standard_normal((D, 128))
        pos[:, 256] = leaves[-1] + 0.001 * rng.standard_normal(D)  # beside the lone last leaf: the second block needs its chunk
        scale = rng.uniform(0.3, 3.0, size=D) if variant == "scale" else None
        circ = (D - 1,) if circular else ()
        qry = np.ascontiguousarray(pos.T)
        _BIG[(N, variant)] = dict(p=p, pos=pos, qry=qry, leaves=leaves, where=where, orig=where + 1, scale=scale, circ=circ,
                                  man=([0] * (D - 1) + [1]) if circular else None,
                                  metric="euclid" if scale is None else scale, d2=km.all_dist2(leaves, qry, scale, circ))
    return _BIG[(N, variant)]


def _gap(row):
    """the longest unvisited stretch between two visited chunks of one query block that lie in different flag words"""
    at = np.nonzero(row)[0]
    return max([b - a - 1 for a, b in zip(at[:-1], at[1:]) if a // 64 != b // 64], default=0)


@pytest.mark.parametrize("N,variant", [(N, v) for N, (_, _, vs, _) in BIG_SHAPES.items() for v in vs])
def test_the_search_with_several_flag_words_and_box_tiles(N, variant):
    D, Nq, _, ks = BIG_SHAPES[N]
    assert_chunks_per_group(N, Nq, 2 if N == 8193 else 3)
    c = _big_case(N, variant)
    kw = dict(scale=c["scale"], circ=c["circ"], d2=c["d2"])
    nc = (N + 127) // 128
    for k in ks:
        pl = km.plan(c["leaves"], c["orig"], c["qry"], k, **kw)
        # the premises, on the model alone
        assert pl["stats"][0] < pl["stats"][1] == 2 * nc  # pruning happens: a flag in the wrong word changes what is scanned
        assert (pl["cstar"] < 64).any() and (pl["cstar"] >= (128 if N == 16513 else 63)).any(), np.unique(pl["cstar"])
        if N == 16513:  # a block visits chunks of two flag words and none of the 64 or more between them
            assert max(_gap(row) for row in pl["visited"]) >= 64, [_gap(row) for row in pl["visited"]]
        else:  # (65 chunks: the second word is chunk 64 alone) a block visits it, and a block leaves most of the first word out
            assert pl["visited"][:, 64].any() and any(0 < row[:64].sum() < 32 for row in pl["visited"])
        d2, idx = km.knn(c["leaves"], c["orig"], c["qry"], k, **kw)
        got = kdehip.knn(c["p"], c["pos"], k=k, order="given", metric=c["metric"], manifold=c["man"], squared=True,
                         return_stats=True)
        print("N", N, variant, "k", k, "tiles visited / total:", got[2], "model:", pl["stats"])
        _same(got, (d2.T, idx.T, pl["stats"]))
    with kdehip.DeviceDensity(c["p"]) as d, kdehip.DeviceDensity(kdehip.kde(c["pos"], [1.0])) as a:  # resident == host
        kw = dict(k=8, metric=c["metric"], manifold=c["man"], squared=True, return_stats=True)
        host = kdehip.knn(c["p"], kdehip.kde(c["pos"], [1.0]), **kw)
        got = d.knn(a, **kw)
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]) and got[2] == host[2]


_BIG_LOO = {}


def _big_loo(N, variant, k=8):
    """the model's leave-one-out search of a large density in row blocks of 1024 leaves (never an N x N array): (d2 (k, N),
    idx (k, N)) in the caller's order, the summed stats and every leaf's nearest chunk"""
    if (N, variant) not in _BIG_LOO:
        c = _big_case(N, variant)
        d2s, idxs, cstar, visited, total = [], [], [], 0, 0
        for r in range(0, N, 1024):
            rows = slice(r, min(N, r + 1024))
            qry = c["leaves"][rows]
            kw = dict(loo=True, scale=c["scale"], circ=c["circ"], d2=km.all_dist2(c["leaves"], qry, c["scale"], c["circ"]),
                      rows=rows)
            d2, idx = km.knn(c["leaves"], c["orig"], qry, k, **kw)
            pl = km.plan(c["leaves"], c["orig"], qry, k, **kw)
            d2s.append(d2)
            idxs.append(idx)
            cstar.append(pl["cstar"])
            visited, total = visited + pl["stats"][0], total + pl["stats"][1]
        back = np.argsort(c["where"])  # leaf q is original point where[q]
        _BIG_LOO[(N, variant)] = dict(d2=np.concatenate(d2s)[back].T, idx=np.concatenate(idxs)[back].T,
                                      stats=(visited, total), cstar=np.concatenate(cstar))
    return _BIG_LOO[(N, variant)]


@pytest.mark.parametrize("N,variant", [(8193, "euclid"), (8193, "circular"), (16513, "euclid")])
def test_leave_one_out_with_the_last_leaf_alone_in_its_chunk(N, variant):
    assert (N - 1) % 128 == 0
    assert_chunks_per_group(N, N, 2 if N == 8193 else 5)  # (N = Nq = 16513: 65 query blocks, 32 groups)
    c = _big_case(N, variant)
    m = _big_loo(N, variant)
    nc = (N + 127) // 128
    # the premises, on the model alone: the lone leaf's own chunk does not count for it, pruning happens, both ends occur
    assert m["cstar"][N - 1] != nc - 1 and m["cstar"][N - 2] < nc - 1
    assert m["stats"][0] < m["stats"][1] == ((N + 255) // 256) * nc
    assert (m["cstar"] < 64).any() and (m["cstar"] >= (128 if N == 16513 else 63)).any()
    got = kdehip.knn(c["p"], k=8, lvFlag=True, metric=c["metric"], manifold=c["man"], squared=True, return_stats=True)
    print("N", N, variant, "tiles visited / total:", got[2], "model:", m["stats"])
    _same(got, (m["d2"], m["idx"], m["stats"]))
    with kdehip.DeviceDensity(c["p"]) as d:
        again = d.knn(None, k=8, metric=c["metric"], manifold=c["man"], squared=True, return_stats=True)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2] == got[2]


def test_entropy_knn_with_two_flag_words():
    N, k = 8193, 4
    c = _big_case(N, "euclid")
    eps = np.sqrt(_big_loo(N, "euclid")["d2"][k - 1])  # the model's 4th leave-one-out neighbour of every point
    want = km.entropy_kl(eps, 2, k)
    got = kdehip.entropy_knn(c["p"], k)
    print("entropy_knn:", got, "model:", want, "difference:", abs(got - want))
    assert abs(got - want) <= 1e-12
    with kdehip.DeviceDensity(c["p"]) as d:
        assert abs(kdehip.entropy_knn(d, k) - want) <= 1e-12
