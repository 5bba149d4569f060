"""The probability mass of a density on the GPU (csrc/mass.hip, include/kdehip.h section 5l): `box_mass`, `cdf`, `quantile`,
`median`, `interval`, `grid_mass` and the two batches against tests/mass_model.py (the contract's factor with math.erfc, one
fsum per value), and against each other bit for bit.

Tolerances, none of them taken from the code under test:
  mass      |got - want| <= 1e-12 * want, the project's tolerance for sums of positive terms (tests/test_gpu_ksum.py).  It holds
            because every test box is at least half a bandwidth wide in every bounded dimension, or infinite there: a factor's
            two erfc values then differ by a factor of at least 1.6, the cancellation stays below about 10, and 8 dimensions
            x 10 x 16 ulp is 1.4e-13.  Narrower boxes are tested for 0 <= mass only, empty ones for mass == 0.
  erfc      the device library's erfc against math.erfc over [0, 26]: at most 16 ulp, the OpenCL bound (the device library
            documents none tighter).  Measured on one MI355X: 4.0 ulp, at x = 16.005.
  quantile  |F_model(x) - alpha| <= tol + 1e-12 and |resid - (F_model(x) - alpha)| <= 1e-12: tol is the caller's, 1e-12 what
            the device's F may differ from the model's by."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import mass_model as mm
from tests.helpers import assert_chunks_per_group
from tests.test_gpu_ksum import _arrays

pytestmark = pytest.mark.gpu

# (D, dims, N, Nq): the smallest case; two chunks and groups with Nq across a block; gathered dimensions; 6-D; 8-D; 65 chunks
# (two chunks per group: the ring's second buffer); 129 chunks (three per group: a buffer staged a second time)
SHAPES = [(1, [0], 5, 3), (2, [0, 1], 129, 257), (3, [0, 2], 300, 7), (6, None, 257, 5), (8, None, 130, 3), (2, [1], 8200, 3),
          (2, [1], 16500, 3)]
LEVELS = np.array([1e-9, 0.025, 0.5, 0.975, 1.0 - 1e-9])


def _density(rng, D, N):
    """two clusters, non-uniform weights with ONE exact zero"""
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))
    pts[:, N // 2:] += 3.0
    w = rng.uniform(0.05, 1.0, size=N)
    if N > 1:
        w[N // 3] = 0.0
    return kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D), w)


def _boxes(rng, A, dims, Nq):
    """Nq boxes over `dims`, centred inside the data, between half a bandwidth and four wide; a fifth of the lower and a
    fifth of the upper bounds infinite (the first box: one of each)"""
    pts, _, v = A
    P, sd = pts[dims, :], np.sqrt(v[dims])[:, None]
    c = P.min(axis=1, keepdims=True) + (P.max(axis=1, keepdims=True) - P.min(axis=1, keepdims=True)) * rng.uniform(0, 1, size=(len(dims), Nq))
    half = 0.5 * sd * rng.uniform(0.5, 4.0, size=(len(dims), Nq))
    lo, hi = c - half, c + half
    assert np.all(hi - lo >= 0.5 * sd * (1.0 - 1e-12))
    lo[rng.uniform(size=lo.shape) < 0.2] = -math.inf
    hi[rng.uniform(size=hi.shape) < 0.2] = math.inf
    lo[0, 0], hi[-1, 0] = -math.inf, math.inf
    return lo, hi


_CASES = {}


def _case(D, dims, N, Nq):
    """a density of one shape, its boxes, the model's masses and the host entry's: built once, shared, never changed"""
    key = (D, None if dims is None else tuple(dims), N, Nq)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * N + Nq)
        p = _density(rng, D, N)
        A = _arrays(p)
        dl = list(range(D)) if dims is None else dims
        lo, hi = _boxes(rng, A, dl, Nq)
        _CASES[key] = dict(p=p, A=A, dims=dims, dl=dl, lo=lo, hi=hi, model=mm.box_mass(A, lo, hi, dl),
                           host=kdehip.box_mass(p, lo, hi, dims))
    return _CASES[key]


def _close(got, want):
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = np.abs(got - want)
    print("max relative error:", float(np.max(err / want)), "allowed 1e-12")
    assert np.all(err <= 1e-12 * want), float(np.max(err / want))


# ---- 1. the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dims,N,Nq", SHAPES)
def test_box_mass_equals_the_model(D, dims, N, Nq):
    if N > 8192:  # a large shape is here for the chunks a group walks: asserted from the split restated in tests/helpers.py
        assert_chunks_per_group(N, Nq, 2 if N == 8200 else 3)
    c = _case(D, dims, N, Nq)
    assert np.all(c["model"] > 0.0) and int(np.sum(c["A"][1] == 0.0)) == (1 if N > 1 else 0)
    assert np.isinf(c["lo"]).any() and np.isinf(c["hi"]).any()
    _close(c["host"], c["model"])
    with kdehip.DeviceDensity(c["p"]) as d:  # resident: the host entry's bits
        assert np.array_equal(kdehip.box_mass(d, c["lo"], c["hi"], dims), c["host"])
        assert np.array_equal(d.box_mass(c["lo"], c["hi"], dims), c["host"])


def test_dims_in_any_order_name_the_same_boxes():
    c = _case(3, [0, 2], 300, 7)
    assert np.array_equal(kdehip.box_mass(c["p"], c["lo"][::-1], c["hi"][::-1], [2, 0]), c["host"])


# ---- 2. special bounds -------------------------------------------------------------------------------------------------------
def test_a_nan_bound_is_nan_for_that_box_only():
    c = _case(2, [0, 1], 129, 257)
    lo, hi = c["lo"].copy(), c["hi"].copy()
    lo[1, 100] = math.nan
    hi[0, 256] = math.nan
    got = kdehip.box_mass(c["p"], lo, hi)
    keep = np.ones(257, dtype=bool)
    keep[[100, 256]] = False
    assert math.isnan(got[100]) and math.isnan(got[256]) and np.array_equal(got[keep], c["host"][keep])
    with kdehip.DeviceDensity(c["p"]) as d:
        assert np.array_equal(d.box_mass(lo, hi), got, equal_nan=True)


def test_empty_and_narrow_boxes():
    c = _case(3, [0, 2], 300, 7)
    lo, hi = c["lo"].copy(), c["hi"].copy()
    lo[:, 1], hi[:, 1] = [0.5, -math.inf], [0.5, math.inf]      # degenerate in one dimension
    lo[:, 2], hi[:, 2] = [0.7, -1.0], [0.5, 1.0]                # reversed
    lo[:, 3], hi[:, 3] = [math.inf, -1.0], [math.inf, 1.0]
    lo[:, 4], hi[:, 4] = [-math.inf, -1.0], [-math.inf, 1.0]
    lo[:, 5], hi[:, 5] = [0.5, 0.5], [0.5 + 1e-9, 0.5 + 1e-13]  # far narrower than a bandwidth
    got = kdehip.box_mass(c["p"], lo, hi, c["dims"])
    assert np.all(got[1:5] == 0.0) and got[5] >= 0.0 and math.isfinite(got[5])
    assert got[0] == c["host"][0] and got[6] == c["host"][6]


@pytest.mark.parametrize("D,dims,N,Nq", SHAPES)
def test_all_bounds_infinite_give_one(D, dims, N, Nq):
    c = _case(D, dims, N, Nq)
    nb = len(c["dl"])
    got = kdehip.box_mass(c["p"], np.full((nb, 1), -math.inf), np.full((nb, 1), math.inf), dims)
    assert abs(got[0] - 1.0) <= 1e-12


# ---- 3. the device library's erfc, measured -------------------------------------------------------------------------------
def test_device_erfc_is_within_16_ulp():
    """a 1-D one-point density with c = 0, v = 0.5 (s = 1) and w = 1: cdf(x) = erfc(-x) / 2 exactly for x <= 0"""
    p = kdehip.kde(np.array([[0.0]]), [1.0])
    p.bandwidth[:] = 0.5  # (exactly: the square of fl(sqrt(0.5)) is not)
    assert _arrays(p)[1][0] == 1.0 and _arrays(p)[2][0] == 0.5 and 1.0 / math.sqrt(2.0 * 0.5) == 1.0
    rng = np.random.default_rng(5)
    x = -np.concatenate([rng.uniform(0.0, 26.0, size=100000), np.linspace(0.0, 26.0, 2601), 2.0 ** -np.arange(1.0, 60.0)])
    got = 2.0 * kdehip.cdf(p, x, 0)
    want = np.array([math.erfc(-t) for t in x])
    ulp = np.array([math.ulp(t) for t in want])
    err = np.abs(got - want) / ulp
    k = int(np.argmax(err))
    print("device erfc: max error", float(err[k]), "ulp at x =", float(-x[k]), "over", x.size, "points in [0, 26]")
    assert np.all(np.isfinite(got)) and err[k] <= 16.0


# ---- 4. cross-checks ---------------------------------------------------------------------------------------------------------
def test_a_grid_with_infinite_outer_edges_sums_to_one():
    c = _case(2, [0, 1], 129, 257)
    pts = c["A"][0]
    edges = [np.concatenate([[-math.inf], np.linspace(pts[k].min(), pts[k].max(), 4), [math.inf]]) for k in range(2)]
    cells = kdehip.grid_mass(c["p"], edges)
    assert cells.shape == (5, 5) and np.all(cells >= 0.0)
    assert abs(math.fsum(cells.reshape(-1)) - 1.0) <= 1e-12
    # a cell is the box between its edges (both calls are one query block over two chunks: the same group split)
    assert cells[1, 3] == kdehip.box_mass(c["p"], [[edges[0][1]], [edges[1][3]]], [[edges[0][2]], [edges[1][4]]])[0]
    one = kdehip.grid_mass(c["p"], [edges[1]], [1])  # the other dimension free: the row sums
    assert one.shape == (5,) and np.all(np.abs(one - cells.sum(axis=0)) <= 1e-12 * one)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_bounded_dimension_is_the_box_mass_of_the_marginal(k):
    c = _case(3, [0, 2], 300, 7)
    rng = np.random.default_rng(k)
    lo, hi = _boxes(rng, c["A"], [k], 40)
    got = kdehip.box_mass(c["p"], lo, hi, [k])
    want = kdehip.box_mass(kdehip.marginal(c["p"], [k]), lo, hi)
    assert np.all(want > 0.0) and np.all(np.abs(got - want) <= 1e-12 * want), float(np.max(np.abs(got - want) / want))
    assert np.array_equal(kdehip.cdf(c["p"], hi[0], k), kdehip.box_mass(c["p"], -math.inf, hi, [k]))


# ---- 5. the same bits --------------------------------------------------------------------------------------------------------
def _batch_items(devs, cases, fill=math.nan):
    import torch
    items = []
    for d, c in zip(devs, cases):
        f64 = dict(dtype=torch.float64, device="cuda:0")
        order = np.argsort(c["dl"])
        items.append(dict(density=d, dims=c["dims"], lo=torch.from_numpy(np.ascontiguousarray(c["lo"][order].T)).to("cuda:0"),
                          hi=torch.from_numpy(np.ascontiguousarray(c["hi"][order].T)).to("cuda:0"),
                          mass=torch.full((c["lo"].shape[1],), fill, **f64)))
    return items


def test_host_resident_and_batch_give_the_same_bits_run_after_run():
    import torch
    cases = [_case(*s) for s in SHAPES]  # mixed D, N, Nq and masks
    for c in cases:
        assert np.array_equal(kdehip.box_mass(c["p"], c["lo"], c["hi"], c["dims"]), c["host"])  # run after run
    devs = [kdehip.DeviceDensity(c["p"]) for c in cases]
    items = _batch_items(devs, cases)
    kdehip.box_mass_device_batch(items)
    torch.cuda.synchronize()
    for it, c in zip(items, cases):
        assert np.array_equal(it["mass"].cpu().numpy(), c["host"])
    order = list(reversed(range(len(cases))))  # another order, a stream of its own
    items = _batch_items([devs[k] for k in order], [cases[k] for k in order])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        kdehip.box_mass_device_batch(items, stream=st.cuda_stream)
    st.synchronize()
    for it, k in zip(items, order):
        assert np.array_equal(it["mass"].cpu().numpy(), cases[k]["host"])
    # captured in a graph on ONE stream and replayed twice (sequential launches: no parallel branches)
    items = _batch_items(devs, cases)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        kdehip.box_mass_device_batch(items, stream=torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        for it in items:
            it["mass"].fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        for it, c in zip(items, cases):
            assert np.array_equal(it["mass"].cpu().numpy(), c["host"])
    del graph
    for d in devs:
        d.close()
    kdehip._clib.kdehip_clear_cache()  # (5h: the captured call's blocks are kept until here; the graph is gone)


# ---- 6. quantiles ------------------------------------------------------------------------------------------------------------
_QUANT = {}


def _qcase(N):
    """a 2-D density of N points and the quantiles of its dimension 1 at LEVELS (full outputs, host entry): built once"""
    if N not in _QUANT:
        rng = np.random.default_rng(50 + N)
        p = _density(rng, 2, N)
        _QUANT[N] = dict(p=p, A=_arrays(p), out=kdehip.quantile(p, LEVELS, 1, full=True))
    return _QUANT[N]


def _check_quantiles(A, dim, levels, out, tol, max_iter=100):
    x, resid, iters, conv = out
    assert x.shape == levels.shape and conv.dtype == bool and conv.all() and np.all(np.isfinite(x))
    assert np.all(iters >= 1) and np.all(iters <= max_iter)
    assert np.all(np.diff(x) >= 0.0)  # non-decreasing in alpha
    for xq, a, r in zip(x, levels, resid):
        want = mm.cdf(A, xq, dim) - a
        print("alpha", a, "x", xq, "model residual", want, "device residual", r)
        assert abs(want) <= tol + 1e-12 and abs(r - want) <= 1e-12 and abs(r) <= tol


@pytest.mark.parametrize("N", [1, 5, 257, 8200])
def test_quantiles_solve_the_models_cdf(N):
    c = _qcase(N)
    _check_quantiles(c["A"], 1, LEVELS, c["out"], 1e-12)
    assert np.array_equal(kdehip.quantile(c["p"], LEVELS, 1), c["out"][0])
    assert kdehip.median(c["p"], 1) == c["out"][0][2]
    with kdehip.DeviceDensity(c["p"]) as d:  # resident: the host entry's bits
        for got in (kdehip.quantile(d, LEVELS, 1, full=True), d.quantile(LEVELS, 1, full=True)):
            assert all(np.array_equal(u, v) for u, v in zip(got, c["out"]))
    if N == 257:  # a tighter and a looser tolerance
        for tol in (1e-14, 1e-6):
            _check_quantiles(c["A"], 1, LEVELS, kdehip.quantile(c["p"], LEVELS, 1, tol=tol, full=True), tol)


@pytest.mark.parametrize("w_left", [0.5, 0.4])
def test_two_distant_clusters_and_the_plateau_between_them(w_left):
    """clusters at -50 and +50 under a bandwidth of 0.05: with equal weights alpha = 0.5 falls on the plateau, where the pdf
    is 0; with 0.4 on the left the root lies inside the right cluster, across the plateau from the first iterate"""
    off = np.array([-0.1, 0.0, 0.1])
    pts = np.concatenate([-50.0 + off, 50.0 + off])[None, :]
    w = np.concatenate([np.full(3, w_left / 3.0), np.full(3, (1.0 - w_left) / 3.0)])
    p = kdehip.kde(pts, [0.05], w)
    A = _arrays(p)
    levels = np.array([0.1, 0.5, 0.9])
    out = kdehip.quantile(p, levels, 0, full=True)
    _check_quantiles(A, 0, levels, out, 1e-12)
    assert out[0][0] < -49.0 and out[0][2] > 49.0


def test_one_evaluation_returns_the_midpoint_unconverged():
    c = _qcase(257)
    x, resid, iters, conv = kdehip.quantile(c["p"], LEVELS, 1, max_iter=1, full=True)
    pts, w, v = c["A"]
    live = pts[1, w > 0.0]
    sigma = math.sqrt(v[1])
    mid = 0.5 * ((live.min() - 39.0 * sigma) + (live.max() + 39.0 * sigma))
    assert np.all(x == mid) and np.all(iters == 1) and np.all(np.isfinite(resid))
    assert not conv[[0, 1, 3, 4]].any()  # (the midpoint lies between the clusters: far from these four levels)
    for a, r in zip(LEVELS, resid):
        assert abs(r - (mm.cdf(c["A"], mid, 1) - a)) <= 1e-12


def test_a_level_outside_zero_to_one_is_nan_for_that_level_only():
    c = _qcase(257)
    levels = np.array([LEVELS[0], 0.0, LEVELS[1], 1.0, LEVELS[2], math.nan, LEVELS[3], -0.5, LEVELS[4], 1.5])
    x, resid, iters, conv = kdehip.quantile(c["p"], levels, 1, full=True)
    assert np.all(np.isnan(x[1::2])) and np.all(np.isnan(resid[1::2])) and np.all(iters[1::2] == 0) and not conv[1::2].any()
    for got, ref in zip((x, resid, iters, conv), c["out"]):
        assert np.array_equal(got[0::2], ref)


def test_an_interval_holds_its_level():
    c = _qcase(257)
    lo, hi = kdehip.interval(c["p"], 1, 0.9)
    assert lo < hi
    got = kdehip.box_mass(c["p"], lo, hi, [1])[0]
    assert abs(got - 0.9) <= 2 * 1e-12 + 1e-12
    with kdehip.DeviceDensity(c["p"]) as d:
        assert d.interval(1, 0.9) == (lo, hi)
    assert kdehip.interval(c["p"], 1) == tuple(kdehip.quantile(c["p"], [(1.0 - 0.95) / 2.0, (1.0 + 0.95) / 2.0], 1))


def test_a_quantile_batch_gives_the_single_calls_bits():
    import torch
    Ns = [1, 5, 257, 8200]
    cases = [_qcase(N) for N in Ns]
    devs = [kdehip.DeviceDensity(c["p"]) for c in cases]
    dev = dict(device="cuda:0")
    alpha = torch.from_numpy(LEVELS).to("cuda:0")

    def items(full):
        out = []
        for j, d in enumerate(devs):
            it = dict(density=d, dim=1, alpha=alpha, x=torch.full((5,), math.nan, dtype=torch.float64, **dev))
            if full or j % 2:
                it.update(resid=torch.full((5,), math.nan, dtype=torch.float64, **dev),
                          iters=torch.full((5,), -7, dtype=torch.int32, **dev), converged=torch.full((5,), -7, dtype=torch.int32, **dev))
            out.append(it)
        return out

    for full in (True, False):
        its = items(full)
        kdehip.quantile_device_batch(its)
        torch.cuda.synchronize()
        for it, c in zip(its, cases):
            assert np.array_equal(it["x"].cpu().numpy(), c["out"][0])
            if "resid" in it:
                assert np.array_equal(it["resid"].cpu().numpy(), c["out"][1])
                assert np.array_equal(it["iters"].cpu().numpy(), c["out"][2])
                assert np.array_equal(it["converged"].cpu().numpy() != 0, c["out"][3])
    # another dimension and tolerance for all items of a batch
    its = items(True)
    for it in its:
        it["dim"] = 0
    kdehip.quantile_device_batch(its, tol=1e-9, max_iter=50)
    torch.cuda.synchronize()
    for it, c in zip(its, cases):
        single = kdehip.quantile(c["p"], LEVELS, 0, tol=1e-9, max_iter=50, full=True)
        assert np.array_equal(it["x"].cpu().numpy(), single[0]) and np.array_equal(it["iters"].cpu().numpy(), single[2])
    for d in devs:
        d.close()


# ---- 7. the refusals that read a resident handle ---------------------------------------------------------------------------
def test_resident_arguments_are_refused_before_the_device_is_used():
    import ctypes as C

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
        circ0 = np.array([1, 0], dtype=np.uint8)
        u8 = lambda m: _lib.ptr(m, _lib.u8p)  # noqa: E731
        for mask in (0, 1 << 2, 0b110):  # no dimension; a bit at or above D
            assert L.kdehip_box_mass_device(dp._h, mask, a, a, 3, a, None, None) == _lib.ERR_ARG
        assert L.kdehip_box_mass_device(dp._h, 1, a, a, -1, a, None, None) == _lib.ERR_ARG
        assert L.kdehip_box_mass_device(dp._h, 1, None, a, 3, a, None, None) == _lib.ERR_ARG
        assert L.kdehip_box_mass_device(dp._h, 1, a, a, 3, None, None, None) == _lib.ERR_ARG
        assert L.kdehip_box_mass_device(dp._h, 1, a, a, 3, a, u8(bad), None) == _lib.ERR_ARG
        assert L.kdehip_box_mass_device(dp._h, 0b01, a, a, 3, a, u8(circ0), None) == _lib.ERR_UNSUPPORTED  # a bounded circle
        assert L.kdehip_box_mass_device(dq._h, 1, a, a, 3, a, None, None) == _lib.ERR_UNSUPPORTED          # per-point bandwidths
        assert L.kdehip_box_mass_device(dp._h, 1, a, a, 0, a, None, None) == _lib.KDEHIP_OK
        for dim in (-1, 2):
            assert L.kdehip_quantile_device(dp._h, dim, a, 3, None, 0, a, a, ia, ia, None, None) == _lib.ERR_ARG
        assert L.kdehip_quantile_device(dp._h, 0, a, 3, C.byref(C.c_double(1e-15)), 0, a, a, ia, ia, None, None) == _lib.ERR_ARG
        assert L.kdehip_quantile_device(dp._h, 0, a, 3, None, -1, a, a, ia, ia, None, None) == _lib.ERR_ARG
        assert L.kdehip_quantile_device(dp._h, 0, a, 3, None, 0, None, a, ia, ia, None, None) == _lib.ERR_ARG
        assert L.kdehip_quantile_device(dp._h, 0, a, 3, None, 0, a, a, ia, ia, u8(circ0), None) == _lib.ERR_UNSUPPORTED
        assert L.kdehip_quantile_device(dq._h, 0, a, 3, None, 0, a, a, ia, ia, None, None) == _lib.ERR_UNSUPPORTED
        assert L.kdehip_quantile_device(dp._h, 0, a, 0, None, 0, a, a, ia, ia, None, None) == _lib.KDEHIP_OK
        items = (_lib.CBoxMassItem * 2)()
        for k in range(2):
            items[k].bd, items[k].d_lo, items[k].d_hi, items[k].Nq, items[k].d_mass, items[k].dim_mask = dp._h, a, a, 3, a, 1
        items[1].dim_mask = 1 << 2  # a dimension the density does not have
        assert L.kdehip_box_mass_device_batch(2, items, None) == _lib.ERR_ARG and "dim_mask" in L.kdehip_last_error().decode()
        items[1].dim_mask = 1
        items[1].circular_mask = 1 << 2
        assert L.kdehip_box_mass_device_batch(2, items, None) == _lib.ERR_ARG and "circular_mask" in L.kdehip_last_error().decode()
        items[1].circular_mask = 1  # the bounded dimension
        assert L.kdehip_box_mass_device_batch(2, items, None) == _lib.ERR_UNSUPPORTED
        items[1].circular_mask = 0
        items[1].bd = dq._h
        assert L.kdehip_box_mass_device_batch(2, items, None) == _lib.ERR_UNSUPPORTED
        items[1].bd = dp._h
        items[1].Nq = -1
        assert L.kdehip_box_mass_device_batch(2, items, None) == _lib.ERR_ARG
        qitems = (_lib.CQuantileItem * 2)()
        for k in range(2):
            qitems[k].bd, qitems[k].d_alpha, qitems[k].Nq, qitems[k].d_x = dp._h, a, 3, a
        qitems[1].dim = 2
        assert L.kdehip_quantile_device_batch(2, qitems, None, 0, None) == _lib.ERR_ARG
        qitems[1].dim = 1
        qitems[1].circular_mask = 0b10
        assert L.kdehip_quantile_device_batch(2, qitems, None, 0, None) == _lib.ERR_UNSUPPORTED
        qitems[1].circular_mask = 0
        qitems[1].bd = dq._h
        assert L.kdehip_quantile_device_batch(2, qitems, None, 0, None) == _lib.ERR_UNSUPPORTED
        qitems[1].bd = dp._h
        qitems[1].d_x = None
        assert L.kdehip_quantile_device_batch(2, qitems, None, 0, None) == _lib.ERR_ARG
        if kdehip.device_count() >= 2:  # densities on different devices within one batch
            with kdehip.DeviceDensity(p, device=1) as d1:
                items[1].Nq, items[1].bd = 3, d1._h
                assert L.kdehip_box_mass_device_batch(2, items, None) == _lib.ERR_ARG and "devices" in L.kdehip_last_error().decode()
                qitems[1].d_x, qitems[1].bd = a, d1._h
                assert L.kdehip_quantile_device_batch(2, qitems, None, 0, None) == _lib.ERR_ARG
        with pytest.raises(kdehip.KdeHipError) as e:
            kdehip.box_mass(dq, 0.0, 1.0, [0])
        assert e.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(kdehip.KdeHipError) as e:
            kdehip.quantile(dp, 0.5, 0, manifold=[1, 0])
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert kdehip.box_mass(dp, 0.0, 1.0, [1], manifold=[1, 0])[0] > 0.0  # an unbounded circle is fine
        torch.cuda.synchronize()
