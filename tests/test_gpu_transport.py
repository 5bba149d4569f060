"""Entropic optimal transport on the GPU (csrc/sinkhorn.hip, include/kdehip.h section 5s): `sinkhorn`, `sinkhorn_divergence`,
`transport_map`, `transport_to`, `equalize` and `sinkhorn_batch` against tests/transport_model.py (fp64, log-sum-exp with the
maximum taken out, exactly rounded sums over the points), and against each other bit for bit.

Tolerances, none of them taken from the code under test:
  potentials   1e-9 * max(1, max |phi|) against the model, per iterate
  scalars      1e-9 * max(1, |.|): value, transport_cost, err, mass; the map likewise per entry
  plan         column sums within 1e-12 of b (the last half-step of a cross item IS the column normalisation)
  mean         |sum a T - sum b y|_inf <= err * max |T| + 1e-12 * max |y|: the row error is all that moves the mean
The sizes: 129 and 257 leave a second chunk / a second query block with one leaf, every fifth weight is 0 on both sides
(weightless sources and queries), and (2, 8193, 300) is where a group of the second half-step walks two chunks and the
carried sum is rescaled; G10 does the same to the first half-step, the map pass and a self item, G11 empties whole chunks
and groups of sources, G12 takes the scale from the caller, G13 stops on the boundaries of the rounds of eight iterations,
G14 moves a tree built with circular operators without leaving the device.  Every case runs in well under a second on the
device; the model is computed once per case (the row-blocked one of G10's self item takes a few seconds)."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import refit_model as rm
from tests import transport_model as tm
from tests.helpers import chunks_per_group

pytestmark = pytest.mark.gpu

SHAPES = [(1, 129, 257), (2, 257, 129), (3, 300, 257), (6, 300, 130), (8, 130, 129)]
REG, TOL = 4.0, 1e-6   # G3 .. G5
_CASES = {}


def _views(p):
    """the model's view of a density: its own points and weights, in the order of getPoints"""
    return kdehip.getPoints(p), kdehip.getWeights(p)


def _variances(p):
    return kdehip.getBW(p)[:, 0] ** 2


def _case(D, N, M):
    """a weighted pair of one shape at Silverman-style bandwidths, and the model's view of it: built once, shared, never
    changed; the model's answers are kept by their arguments"""
    if (D, N, M) not in _CASES:
        (x, a), (y, b) = tm.two_clusters_pair(D, N, M)
        p, q = kdehip.kde(x, tm.silverman(x), a), kdehip.kde(y, tm.silverman(y), b)
        _CASES[(D, N, M)] = dict(p=p, q=q, vp=_views(p), vq=_views(q), s=tm.default_scale(_variances(p), _variances(q)),
                                 s_self=tm.default_scale(_variances(p), _variances(p)), model={})
    return _CASES[(D, N, M)]


def _model(c, self_item, reg, tol, maxiter):
    key = (self_item, reg, tol, maxiter)
    if key not in c["model"]:
        # the default scale of the call: sqrt(v_p + v_q), for a self item sqrt(2 v_p)
        c["model"][key] = tm.iterate(c["vp"], None if self_item else c["vq"], c["s_self" if self_item else "s"], reg, tol, maxiter)
    return c["model"][key]


def _close(name, got, want, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = 1e-9 * (np.maximum(1.0, np.abs(want)) if scale is None else scale)
    diff = np.abs(got - want)
    print(f"{name}: max difference {diff.max():.3e} (bound {np.min(bound):.3e})")
    assert np.all(np.isfinite(got)) and np.all(diff <= bound), (name, float(diff.max()))


def _check_item(info, want):
    big = max(1.0, float(np.abs(want["phi"]).max()), float(np.abs(want["gamma"]).max()))
    _close("phi", info["phi"], want["phi"], big)
    _close("gamma", info["gamma"], want["gamma"], big)
    for name in ("value", "transport_cost", "err", "mass"):
        _close(name, info[name], want[name])


# ---- G1: iterates against the model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_item", [False, True])
@pytest.mark.parametrize("maxiter", [0, 1, 5])
@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g1_iterates_equal_the_model(D, N, M, maxiter, self_item):
    c = _case(D, N, M)
    p, q = c["p"], (c["p"] if self_item else c["q"])
    want = _model(c, self_item, 1.0, 0.0, maxiter)
    value, info = p.sinkhorn(q, reg=1.0, tol=0.0, maxiter=maxiter, return_info=True)
    assert value == info["value"]
    assert want["iters"] == -maxiter and info["iters"] == -maxiter
    _check_item(info, want)
    if self_item:
        assert np.array_equal(info["gamma"], info["phi"])
    if maxiter == 0:
        assert not info["phi"].any() and not info["gamma"].any()


# ---- G2: several chunks a group ------------------------------------------------------------------------------------------
def test_g2_several_chunks_a_group():
    """(2, 8193, 300): in the second half-step q's 300 points are the queries and p's 65 chunks go to 33 groups of two (one of
    one), so the carried sum is rescaled between chunks; one step, so that gamma -- which that half-step makes -- is compared"""
    assert chunks_per_group(8193, 300) == 2
    c = _case(2, 8193, 300)
    want = _model(c, False, 1.0, 0.0, 1)
    info = c["p"].sinkhorn(c["q"], reg=1.0, tol=0.0, maxiter=1, return_info=True)[1]
    assert info["iters"] == -1
    _check_item(info, want)
    _close("map", info["map"], want["map"])


# ---- G3: convergence -----------------------------------------------------------------------------------------------------
def _converged(D, N, M, self_item):
    c = _case(D, N, M)
    key = ("run", self_item)
    if key not in c:
        c[key] = c["p"].sinkhorn(c["p"] if self_item else c["q"], reg=REG, tol=TOL, return_info=True)[1]
    return c, c[key], _model(c, self_item, REG, TOL, 1000)


@pytest.mark.parametrize("self_item", [False, True])
@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g3_the_iteration_stops_where_the_model_stops(D, N, M, self_item):
    """reg = 4, tol = 1e-6, the default scale.  The model on the CPU takes 13, 12, 23,
    24, 40 cross and 13, 15, 16, 17, 16 self steps at these shapes, and its err at the stop and at the step before differ from
    tol by at least 6 % (cross) and 7 % (self) -- checked on the CPU for these inputs, and asserted at 1 % below --, so the
    equality of the step counts is no rounding accident."""
    c, info, want = _converged(D, N, M, self_item)
    errs = want["errs"]
    assert min(abs(errs[-1] - TOL), abs(errs[-2] - TOL)) > 0.01 * TOL
    print(f"{'self' if self_item else 'cross'}: {info['iters']} steps (model {want['iters']}), err {info['err']:.3e}")
    assert want["iters"] > 0 and info["iters"] == want["iters"]
    assert info["err"] <= TOL
    _check_item(info, want)


# ---- G4: plan properties, from the returned potentials alone -----------------------------------------------------------------
@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g4_plan_properties(D, N, M):
    c, info, _ = _converged(D, N, M, False)
    (x, a), (y, b) = c["vp"], c["vq"]
    P = tm.plan(c["vp"], c["vq"], c["s"], REG, info["phi"], info["gamma"])
    cols = np.abs(P.sum(axis=0) - b).max()
    print(f"column sums: max |sum_i pi_ij - b_j| = {cols:.3e}")
    assert cols <= 1e-12
    T = info["map"]
    drift = np.abs((T * a[None, :]).sum(axis=1) - (y * b[None, :]).sum(axis=1)).max()
    bound = info["err"] * np.abs(T).max() + 1e-12 * np.abs(y).max()
    print(f"mean: |sum a T - sum b y| = {drift:.3e} (bound {bound:.3e})")
    assert drift <= bound
    if D == 1:
        W = tm.unregularised_1d_weighted(x, a, y, b, c["s"][0])
        indep = float((tm.cost(x, y, c["s"]) * a[:, None] * b[None, :]).sum())
        print(f"W {W:.6f} <= <pi, c> {info['transport_cost']:.6f} <= value {info['value']:.6f} <= <a x b, c> {indep:.6f}")
        assert W <= info["transport_cost"] <= info["value"] <= indep


# ---- G5: map and moved density ---------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("D,N,M", SHAPES)
def test_g5_the_map_and_the_moved_density(D, N, M):
    """`T - x` of the issue is the displacement the call returns (in floating point (x + m) - x is not m): the moved density
    equals movePoints(delta) in all twelve arrays, and its points ARE the map, bit for bit"""
    c, _, want = _converged(D, N, M, False)
    p, q = c["p"], c["q"]
    T, info = p.transport_map(q, reg=REG, tol=TOL, return_info=True)
    _close("map", T, want["map"])
    _close("delta", info["delta"], want["delta"], np.maximum(1.0, np.abs(want["map"])))
    moved = p.transport_to(q, reg=REG, tol=TOL)
    rm.same_bits(moved, p.movePoints(info["delta"]), "transport_to")
    assert np.array_equal(kdehip.getPoints(moved), T) and np.array_equal(kdehip.getWeights(moved), c["vp"][1])


def test_g5_a_resident_density_moves_without_leaving_the_device():
    import torch
    D, N, M = 3, 300, 257
    (x, a), (y, b) = tm.two_clusters_pair(D, N, M)
    dx, dy = _dev(x.T), _dev(y.T)  # column-major D x N
    torch.cuda.synchronize()
    with kdehip.DeviceDensity.from_device_points(dx, D, N) as p0, kdehip.DeviceDensity.from_device_points(dy, D, M) as q0, \
            p0.changeWeights(a) as dp, q0.changeWeights(b) as dq:
        hp, hq = dp.download(), dq.download()
        host = hp.transport_to(hq, reg=REG)
        moved, info = dp.transport_to(dq, reg=REG, return_info=True)
        assert isinstance(moved, kdehip.DeviceDensity) and isinstance(info["map"], torch.Tensor) and info["map"].is_cuda
        rm.same_bits(moved.download(), host, "the resident route")
        T = dp.transport_map(dq, reg=REG)
        assert T.is_cuda and tuple(T.shape) == (D, N)
        assert np.array_equal(T.cpu().numpy(), hp.transport_map(hq, reg=REG))
        assert np.array_equal(kdehip.getPoints(host), T.cpu().numpy())
        moved.close()


# ---- G6: bit equality across routes ------------------------------------------------------------------------------------------
_SCALARS = ("value", "transport_cost", "err", "mass", "iters")


def _same_item(got, want, what):
    for k in _SCALARS:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (what, k, got[k], want[k])
    for k in ("phi", "gamma", "map", "delta_leaf"):
        if k in want and k in got:
            assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), (what, k)


def test_g6_host_resident_and_batches_give_the_same_bits():
    kw = dict(reg=2.0, tol=1e-5, maxiter=60)
    ca, cb, cc = _case(3, 300, 257), _case(1, 129, 257), _case(6, 300, 130)
    (ax, aa), (ay, ab) = tm.angle_pair()
    ap, aq = kdehip.kde(ax, [0.3, 0.2], aa), kdehip.kde(ay, [0.3, 0.2], ab)
    man = ["euclid", "circular"]
    host = [(ca["p"], ca["q"], None), (cb["p"], cb["p"], None), (cc["p"], cc["q"], None), (ap, aq, man), (ca["q"], ca["q"], None)]
    dens = {}
    try:
        for p, q, _ in host:
            for d in (p, q):
                if id(d) not in dens:
                    dens[id(d)] = kdehip.DeviceDensity(d)
        items = [dict(p=dens[id(p)], q=dens[id(q)], manifold=m) for p, q, m in host]
        single = [it["p"].sinkhorn(it["q"], manifold=it["manifold"], return_info=True, **kw)[1] for it in items]
        assert len({s["iters"] for s in single}) > 1   # items that stop at different steps share the launches
        for (p, q, m), s in zip(host, single):
            h = p.sinkhorn(q, manifold=m, return_info=True, **kw)[1]
            for k in _SCALARS:
                assert np.float64(h[k]).tobytes() == np.float64(s[k]).tobytes(), k
            leaf = p.bt.permutation[p.bt.num_points:] - 1
            assert np.array_equal(h["phi"], s["phi"].cpu().numpy()) and np.array_equal(h["gamma"], s["gamma"].cpu().numpy())
            assert np.array_equal(h["map"], s["map"].cpu().numpy())
            assert np.array_equal(h["delta"][:, leaf], s["delta_leaf"].cpu().numpy())
        batch = kdehip.DeviceDensity.sinkhorn_batch(items, vectors=True, **kw)
        back = kdehip.DeviceDensity.sinkhorn_batch(items[::-1], vectors=True, **kw)[::-1]
        assert len(batch) == len(back) == 5
        for k, s in enumerate(single):
            _same_item(batch[k], s, f"batch item {k}")
            _same_item(back[k], s, f"reversed batch item {k}")
        again = items[0]["p"].sinkhorn(items[0]["q"], return_info=True, **kw)[1]
        _same_item(again, single[0], "run after run")
    finally:
        for d in dens.values():
            d.close()


# ---- G7: divergence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,M", [(2, 257, 129), (6, 300, 130)])
def test_g7_the_sinkhorn_divergence(D, N, M):
    c = _case(D, N, M)
    p, q = c["p"], c["q"]
    want, (pq, pp, qq) = tm.divergence(c["vp"], c["vq"], c["s"], REG, TOL, 1000)
    S, info = p.sinkhorn_divergence(q, reg=REG, tol=TOL, return_info=True)
    print(f"S = {S!r} (model {want!r}), steps {info['iters']} (model {(pq['iters'], pp['iters'], qq['iters'])})")
    assert abs(S - want) <= 1e-9 * max(1.0, abs(pq["value"]))
    assert S > 0.0
    assert p.sinkhorn_divergence(p, reg=REG, tol=TOL) == 0.0
    # a copy is another object: three items run, the cross one by the alternating updates
    twin = kdehip.kde(*[c["vp"][0], kdehip.getBW(p)[:, 0], c["vp"][1]])
    s2 = tm.default_scale(_variances(p), _variances(p))
    want2, (tw, _, _) = tm.divergence(c["vp"], c["vp"], s2, REG, TOL, 1000)
    got2 = p.sinkhorn_divergence(twin, reg=REG, tol=TOL)
    print(f"S(p, copy of p) = {got2!r} (model {want2!r})")
    assert abs(got2 - want2) <= 1e-9 * max(1.0, abs(tw["value"]))
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        assert dp.sinkhorn_divergence(dq, reg=REG, tol=TOL) == S
        assert dp.sinkhorn_divergence(dp, reg=REG) == 0.0


# ---- G8: circular ------------------------------------------------------------------------------------------------------------
def test_g8_a_pair_clustered_across_the_cut_of_the_circle():
    man = ["euclid", "circular"]
    (x, a), (y, b) = tm.angle_pair()
    p, q = kdehip.kde(x, [0.3, 0.2], a), kdehip.kde(y, [0.3, 0.2], b)
    vp, vq = _views(p), _views(q)
    s = tm.default_scale(_variances(p), _variances(q))
    assert np.abs(tm.diffs(vp[0], vq[0])[1]).max() > math.pi   # the premise: the plain difference is the long way round
    want = tm.iterate(vp, vq, s, 1.0, TOL, 1000, [0, 1])
    T, info = p.transport_map(q, reg=1.0, tol=TOL, manifold=man, return_info=True)
    assert info["iters"] == want["iters"] > 0
    _check_item(info, want)
    _close("map", T, want["map"])
    assert np.all(T[1] >= -math.pi) and np.all(T[1] < math.pi)
    line = p.sinkhorn(q, reg=1.0, tol=TOL)
    print(f"value {info['value']:.6f} on the circle, {line:.6f} on the line")
    assert line > 2.0 * info["value"]


def test_g8_circular_data_in_which_nothing_wraps_gives_the_euclidean_bits():
    c = _case(2, 257, 129)
    big = max(np.abs(c["vp"][0]).max(), np.abs(c["vq"][0]).max())
    x, y = c["vp"][0] / big * 0.99, c["vq"][0] / big * 0.99          # |angle| < 1: every difference inside [-pi, pi)
    p, q = kdehip.kde(x, tm.silverman(x), c["vp"][1]), kdehip.kde(y, tm.silverman(y), c["vq"][1])
    e = p.transport_map(q, reg=1.0, maxiter=40, return_info=True)[1]
    for man in ([1, 1], [0, 1]):
        m = p.transport_map(q, reg=1.0, maxiter=40, manifold=man, return_info=True)[1]
        for k in _SCALARS:
            assert np.float64(m[k]).tobytes() == np.float64(e[k]).tobytes(), k
        for k in ("phi", "gamma", "delta", "map"):
            assert np.array_equal(m[k], e[k]), k


# ---- G9: equalize ------------------------------------------------------------------------------------------------------------
def test_g9_equalize_is_the_ensemble_transform():
    import torch
    D, N = 2, 257
    (x, _), _ = tm.two_clusters_pair(D, N, 129)
    dx = _dev(x.T)
    torch.cuda.synchronize()
    logl = -0.5 * ((x - (x.mean(axis=1, keepdims=True) + 0.3)) ** 2).sum(axis=0) / 0.5 ** 2   # a Gaussian likelihood off the mean
    with kdehip.DeviceDensity.from_device_points(dx, D, N) as d0:
        dw, _, ess = d0.bayes_update(logl)
        with dw:
            assert ess < N / 2
            hw = dw.download()
            out, info = hw.equalize(reg=1.0, return_info=True)
            w = kdehip.getWeights(out)
            assert np.array_equal(w, np.full(N, 1.0 / N))
            for name in ("left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation"):
                assert np.array_equal(getattr(out.bt, name), getattr(hw.bt, name)), name
            assert info["iters"] > 0 and info["err"] <= 1e-6
            X, a = _views(hw)
            T = kdehip.getPoints(out)
            drift = np.abs(T.mean(axis=1) - (X * a[None, :]).sum(axis=1)).max()
            bound = info["err"] * np.abs(T).max() + 1e-12 * np.abs(X).max()
            print(f"ess {ess:.1f} of {N}; {info['iters']} steps; mean drift {drift:.3e} (bound {bound:.3e})")
            assert drift <= bound
            with dw.equalize(reg=1.0) as dout:
                rm.same_bits(dout.download(), out, "the resident route")


# ---- G10: several chunks a group on side 0 and in the map pass ----------------------------------------------------------------
def _check_all(info, want):
    """every output of an item: potentials and scalars (`_check_item`), the map, and the displacement at the map's size (G5)"""
    _check_item(info, want)
    _close("map", info["map"], want["map"])
    _close("delta", info["delta"], want["delta"], np.maximum(1.0, np.abs(want["map"])))


@pytest.mark.parametrize("D,N,M", [(3, 130, 8193), (6, 130, 8321)])
def test_g10_several_chunks_a_group_on_side_0_and_in_the_map_pass(D, N, M):
    """q is the large side: its 65 (66) chunks are the SOURCES of the first half-step and of the map pass and go to groups of
    two, so `total` of ot_partial_kernel<SIDE = 0> and the D + 2 carried sums of ot_map_kernel are rescaled between the chunks
    of a group; p's two chunks on side 1 stay one a group.  8193 leaves a last group of one chunk of one point, 8321 a last
    group whose second chunk is partial.  Two steps: the second one's first half reads the gamma the first one made."""
    assert chunks_per_group(M, N) == 2 and chunks_per_group(N, M) == 1
    c = _case(D, N, M)
    want = _model(c, False, 1.0, 0.0, 2)
    info = c["p"].sinkhorn(c["q"], reg=1.0, tol=0.0, maxiter=2, return_info=True)[1]
    assert info["iters"] == -2
    _check_all(info, want)


def test_g10_a_self_item_with_two_chunks_a_group():
    """(1, 8193) against itself: 65 chunks in groups of two on the only side there is.  The model is the row-blocked one (the
    dense one would hold several GB), which tests/test_transport_host.py holds to the dense one; one step keeps it short."""
    assert chunks_per_group(8193, 8193) == 2
    (x, a), _ = tm.two_clusters_pair(1, 8193, 129)
    p = kdehip.kde(x, tm.silverman(x), a)
    vp = _views(p)
    want = tm.iterate_blocked(vp, None, tm.default_scale(_variances(p), _variances(p)), 1.0, 0.0, 1)
    info = p.sinkhorn(p, reg=1.0, tol=0.0, maxiter=1, return_info=True)[1]
    assert info["iters"] == want["iters"] == -1
    _check_all(info, want)
    assert np.array_equal(info["gamma"], info["phi"])


# ---- G11: whole chunks and whole groups of weightless sources ----------------------------------------------------------------
def _weightless(p, runs):
    """p with the leaf positions [lo, hi) of every run made weightless (through the permutation, as tests/test_gpu_refit.py's
    `_runs_of_zeros`), the rest renormalised: the same tree"""
    N = p.bt.num_points
    w = kdehip.getWeights(p).copy()
    for lo, hi in runs:
        w[p.bt.permutation[N + lo:N + hi] - 1] = 0.0
    out = p.changeWeights(w / w.sum())
    assert np.array_equal(out.bt.permutation, p.bt.permutation)
    for lo, hi in runs:
        assert not out.bt.weights[N + lo:N + hi].any()
    return out


@pytest.mark.parametrize("D,N,M,side,runs", [(2, 130, 300, "q", [(128, 256)]), (2, 300, 130, "p", [(128, 256)]),
                                             (3, 130, 8193, "q", [(0, 128), (256, 512)])])
def test_g11_weightless_chunks_and_groups(D, N, M, side, runs):
    """300 sources are three chunks in three groups: positions 128..255 weightless empty group 1 -- of side 0 and the map pass
    when they are q's, of side 1 when they are p's -- which leaves (-Inf, 0) and is skipped by `mg > -INFINITY`.  8193 sources
    go two chunks a group: positions 0..127 empty the FIRST chunk of group 0 (m stays -Inf, and the rescale of the still zero
    sums by exp_nonpos(-Inf) must give 0 and no NaN), positions 256..511 all of group 1.  The model leaves weightless leaves
    out by their value; p's weightless leaves still move (section 5s)."""
    big = max(N, M)
    assert chunks_per_group(big, min(N, M)) == (2 if big > 8192 else 1)
    c = _case(D, N, M)
    p, q = (_weightless(c["p"], runs), c["q"]) if side == "p" else (c["p"], _weightless(c["q"], runs))
    vp, vq = _views(p), _views(q)
    leaves = (p if side == "p" else q).bt.permutation[(N if side == "p" else M):] - 1
    for lo, hi in runs:
        assert not (vp if side == "p" else vq)[1][leaves[lo:hi]].any()
    want = tm.iterate(vp, vq, c["s"], 1.0, 0.0, 2)
    info = p.sinkhorn(q, reg=1.0, tol=0.0, maxiter=2, return_info=True)[1]
    assert info["iters"] == -2
    for k in ("phi", "gamma", "map", "delta"):
        assert np.all(np.isfinite(info[k])), k
    _check_all(info, want)


# ---- G12: a scale from the caller ----------------------------------------------------------------------------------------------
def test_g12_an_explicit_scale():
    """`write_scale`: the model at the caller's scale; host, resident and batch give the same bits, the batch with two items
    on the SAME pair at different scales (and one at the default); a per-point-bandwidth q, which must have a scale"""
    D, N, M = 3, 300, 257
    c = _case(D, N, M)
    p, q = c["p"], c["q"]
    s1, s2 = np.array([0.7, 1.3, 2.1]), np.array([2.1, 0.7, 1.3])
    kw = dict(reg=1.0, tol=0.0, maxiter=5)
    h1 = p.sinkhorn(q, scale=s1, return_info=True, **kw)[1]
    h2 = p.sinkhorn(q, scale=s2, return_info=True, **kw)[1]
    h0 = p.sinkhorn(q, return_info=True, **kw)[1]
    _check_all(h1, tm.iterate(c["vp"], c["vq"], s1, 1.0, 0.0, 5))
    _check_all(h2, tm.iterate(c["vp"], c["vq"], s2, 1.0, 0.0, 5))
    assert h1["value"] != h2["value"] != h0["value"]
    leaf = p.bt.permutation[N:] - 1
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(q) as dq:
        items = [dict(p=dp, q=dq, scale=s1), dict(p=dp, q=dq, scale=s2), dict(p=dp, q=dq), dict(p=dp, q=dp, scale=s1)]
        single = [it["p"].sinkhorn(it["q"], scale=it.get("scale"), return_info=True, **kw)[1] for it in items]
        batch = kdehip.DeviceDensity.sinkhorn_batch(items, vectors=True, **kw)
        for k, (one, b) in enumerate(zip(single, batch)):
            _same_item(b, one, f"batch item {k}")
        for h, one in ((h1, single[0]), (h2, single[1]), (h0, single[2]), (p.sinkhorn(p, scale=s1, return_info=True, **kw)[1], single[3])):
            for k in _SCALARS:
                assert np.float64(h[k]).tobytes() == np.float64(one[k]).tobytes(), k
            for k in ("phi", "gamma", "map"):
                assert np.array_equal(h[k], one[k].cpu().numpy()), k
            assert np.array_equal(h["delta"][:, leaf], one["delta_leaf"].cpu().numpy())
    rng = np.random.default_rng(12)
    y, b = c["vq"]
    qv = kdehip.kde_varbw(y, tm.silverman(y)[:, None] * rng.uniform(0.5, 2.0, size=(D, M)), b)
    assert qv.multibandwidth == 1
    want = tm.iterate(c["vp"], _views(qv), s1, 1.0, 0.0, 5)   # (the model never reads a bandwidth)
    hv = p.sinkhorn(qv, scale=s1, return_info=True, **kw)[1]
    _check_all(hv, want)
    with kdehip.DeviceDensity(p) as dp, kdehip.DeviceDensity(qv) as dv:
        rv = dp.sinkhorn(dv, scale=s1, return_info=True, **kw)[1]
        for k in _SCALARS:
            assert np.float64(hv[k]).tobytes() == np.float64(rv[k]).tobytes(), k
        assert np.array_equal(hv["phi"], rv["phi"].cpu().numpy()) and np.array_equal(hv["map"], rv["map"].cpu().numpy())


# ---- G13: maxiter on the boundaries of the rounds ------------------------------------------------------------------------------
ROUND_EDGES = [7, 8, 9, 16]   # rounds() runs maxiter + 1 iterations in rounds of 8: the last of a round, the first and the
# second of the next one, and the first of the third


@pytest.mark.parametrize("self_item", [False, True])
@pytest.mark.parametrize("maxiter", ROUND_EDGES)
def test_g13_stopping_by_maxiter_on_a_round_boundary(maxiter, self_item):
    c = _case(2, 257, 129)
    p, q = c["p"], (c["p"] if self_item else c["q"])
    want = _model(c, self_item, 1.0, 0.0, maxiter)
    info = p.sinkhorn(q, reg=1.0, tol=0.0, maxiter=maxiter, return_info=True)[1]
    assert want["iters"] == -maxiter and info["iters"] == -maxiter
    _check_all(info, want)


def test_g13_a_batch_of_items_that_stop_in_different_rounds():
    c = _case(2, 257, 129)
    with kdehip.DeviceDensity(c["p"]) as dp, kdehip.DeviceDensity(c["q"]) as dq:
        items = [dict(p=dp, q=dq, maxiter=m) for m in ROUND_EDGES]
        batch = kdehip.DeviceDensity.sinkhorn_batch(items, reg=1.0, tol=0.0, vectors=True)
        for it, b in zip(items, batch):
            one = dp.sinkhorn(dq, reg=1.0, tol=0.0, maxiter=it["maxiter"], return_info=True)[1]
            assert b["iters"] == -it["maxiter"]
            _same_item(b, one, f"maxiter {it['maxiter']}")
            host = c["p"].sinkhorn(c["q"], reg=1.0, tol=0.0, maxiter=it["maxiter"], return_info=True)[1]
            assert np.array_equal(host["phi"], one["phi"].cpu().numpy()) and host["value"] == one["value"]


# ---- G14: a tree built with circular operators, resident ----------------------------------------------------------------------
def test_g14_a_circular_tree_moves_on_the_device_as_on_the_host():
    """both densities are built on the device with circular operators in dimension 1 (a moved density can be downloaded only
    if its source was built by the library); the host route runs on their downloaded arrays"""
    import torch
    man = ["euclid", "circular"]
    (x, a), (y, b) = tm.angle_pair()
    dx, dy = _dev(x.T), _dev(y.T)
    torch.cuda.synchronize()
    kw = dict(reg=1.0, tol=TOL, manifold=man)
    with kdehip.DeviceDensity.from_device_points(dx, 2, x.shape[1], tree_manifold=man) as dp, \
            kdehip.DeviceDensity.from_device_points(dy, 2, y.shape[1], tree_manifold=man) as dq:
        p, q = dp.download(), dq.download()
        assert list(p.tree_manifold) == [0, 1] and list(dp.tree_manifold) == [0, 1]
        T, info = p.transport_map(q, return_info=True, **kw)
        assert info["iters"] > 0
        moved = p.transport_to(q, **kw)
        assert np.array_equal(moved.tree_manifold, p.tree_manifold)
        rm.same_bits(moved, p.movePoints(info["delta"]), "transport_to is movePoints(delta) with the tree's operators")
        pts = kdehip.getPoints(moved)
        assert np.array_equal(pts, T)
        assert np.all(pts[1] >= -math.pi) and np.all(pts[1] < math.pi)
        assert (np.abs(_views(p)[0][1] + info["delta"][1]) > math.pi).any()   # the premise: some sums left [-pi, pi) and were wrapped
        even = p.equalize(**kw)
        assert np.array_equal(kdehip.getWeights(even), np.full(len(a), 1.0 / len(a)))
        th = kdehip.getPoints(even)[1]
        assert np.all(th >= -math.pi) and np.all(th < math.pi)
        with dp.transport_to(dq, **kw) as dm:
            assert np.array_equal(dm.tree_manifold, dp.tree_manifold)
            rm.same_bits(dm.download(), moved, "transport_to, the resident route")
        assert np.array_equal(dp.transport_map(dq, **kw).cpu().numpy(), T)
        with dp.equalize(**kw) as de:
            rm.same_bits(de.download(), even, "equalize, the resident route")


# ---- the refusals that read a handle ----------------------------------------------------------------------------------------
def test_resident_arguments_are_refused():
    import ctypes as C
    rng = np.random.default_rng(5)
    p2, p3 = kdehip.kde(rng.standard_normal((2, 130)), [0.3]), kdehip.kde(rng.standard_normal((3, 130)), [0.3])
    none = kdehip.kde(rng.standard_normal((2, 130)), [0.3]).changeWeights(np.zeros(130))
    var = kdehip.kde(rng.standard_normal((2, 130)), [0.3])
    var.bandwidth[(130 + 3) * 2] *= 2.0  # leaf 3 gets a bandwidth of its own
    L = _lib.lib
    vals, it = np.zeros(4), np.zeros(1, dtype=np.int32)
    o = [C.cast(vals[k:].ctypes.data, _lib.f64p) for k in range(4)] + [_lib.ptr(it, _lib.i32p)]
    bad = np.array([0, 2], dtype=np.uint8)
    one = np.ones(2)
    with kdehip.DeviceDensity(p2) as d2, kdehip.DeviceDensity(p3) as d3, kdehip.DeviceDensity(none) as d0, \
            kdehip.DeviceDensity(var) as dv:
        def call(p, q, scale=None, reg=1.0, tol=1e-6, maxiter=5, man=None):
            return L.kdehip_sinkhorn_device(p._h, q._h, _lib.optr(scale, _lib.f64p), C.byref(C.c_double(reg)), C.byref(C.c_double(tol)),
                                            maxiter, *o, None, None, None, None, man)
        assert call(d2, d3) == _lib.ERR_ARG and "ndims" in L.kdehip_last_error().decode()
        assert call(d2, d2, man=_lib.ptr(bad, _lib.u8p)) == _lib.ERR_ARG
        assert call(d2, dv) == _lib.ERR_ARG and "per-point" in L.kdehip_last_error().decode()
        assert call(d2, dv, scale=one) == _lib.KDEHIP_OK
        assert call(d2, d0) == _lib.ERR_ARG and "positive weight" in L.kdehip_last_error().decode()
        assert call(d0, d2) == _lib.ERR_ARG and "positive weight" in L.kdehip_last_error().decode()
        items = (_lib.CSinkhornItem * 2)()
        for k in range(2):
            items[k].p, items[k].q, items[k].reg, items[k].tol, items[k].maxiter = d2._h, d2._h, 1.0, 1e-6, 5
            items[k].value, items[k].transport_cost, items[k].err, items[k].mass, items[k].iters = o
        assert L.kdehip_sinkhorn_device_batch(2, items) == _lib.KDEHIP_OK
        items[1].circular_mask = 1 << 2
        assert L.kdehip_sinkhorn_device_batch(2, items) == _lib.ERR_ARG and "circular_mask" in L.kdehip_last_error().decode()
        items[1].circular_mask = 0
        items[1].reg = 0.0
        assert L.kdehip_sinkhorn_device_batch(2, items) == _lib.ERR_ARG
