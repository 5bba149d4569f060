"""Conditioning a density on some of its dimensions on the GPU (csrc/conditional.hip, include/kdehip.h section 5i):
`conditional_moments`, `conditional_weights`, `sample_conditional`, `condition` and `conditional_device_batch` against
tests/conditional_model.py (fp64, exactly rounded sums), and against each other bit for bit.

Tolerances, none of them taken from the code under test:
  logz     1e-12 * max(1, |ref|), the bound of tests/test_gpu_logdensity.py
  mean_k   1e-12 * (R_k + |ref|), var_k  1e-12 * (R_k^2 + v_k): 1e-12 is the project's bound for these sums, the scales are
           the largest term of each sum (R_k = the data's range in dimension k)
  omega    1e-12 * ref + 1e-300 (the absolute part: where t_i is subnormal)
  labels   exact, after the MODEL has shown that no draw's u S_0 lies within 1e-9 S_0 of a boundary between two leaves
           (three orders above the 1e-12 the sums are held to); points bit for bit from the device's own normals.
Where every exponent is huge (the query far from all data) the model forms a_i with the header's one fma per dimension."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import conditional_model as cm
from tests.test_gpu_ksum import SHAPES, _density

pytestmark = pytest.mark.gpu

CASES = [s + (which,) for s in [t for t in SHAPES if t[0] >= 2] + [(2, 8300, 3)] for which in ("first", "last")]
SEED = 20261018


def _gdims(D, which):
    """ng = 1: the first dimension; ng = D - 1: the LAST D - 1 dimensions"""
    return [0] if which == "first" else list(range(1, D))


def _leaf(p):
    """(points (D, N), weights, variances) in leaf order, and the 1-based original index of every leaf"""
    N, D = p.bt.num_points, p.bt.dims
    dens = (p.means[N * D:].reshape(N, D).T.copy(), p.bt.weights[N:].copy(), p.bandwidth[N * D:(N + 1) * D].copy())
    return dens, p.bt.permutation[N:].copy()


def _uniforms(seed, offset, n):
    u = np.zeros(max(n, 1))
    _lib.lib.kdehip_philox_fill_uniform(_lib.u64(seed), int(offset), int(n), 1, _lib.ptr(u, _lib.f64p))
    return u[:n]


_UNIT = {}


def _device_normals(nf, seed, offset, n):
    """the normals the device draws for indices offset .. offset + n - 1 of an nf-dimensional density, (nf, n): a one-point
    density at the origin with unit variance returns x = 0 + 1 * n = n exactly (the device of tests/test_gpu_sample.py)"""
    if nf not in _UNIT:
        _UNIT[nf] = kdehip.kde(np.zeros((nf, 1)), [1.0])
    x, lab = kdehip.sample(_UNIT[nf], n, seed=seed, sample_offset=offset)
    assert (lab == 1).all()
    return x


_CASES = {}


def _case(D, N, Nq, which):
    """a density of one shape, queries inside its range in the given dimensions and the model's values: built once, shared,
    never changed"""
    key = (D, N, Nq, which)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + 10 * N + Nq)
        p = _density(rng, D, N)
        dens, perm = _leaf(p)
        G = _gdims(D, which)
        F = cm.free_dims(D, G)
        lo, hi = dens[0][G].min(axis=1, keepdims=True), dens[0][G].max(axis=1, keepdims=True)
        Y = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(len(G), Nq))
        mom = [cm.moments(dens, G, Y[:, q]) for q in range(Nq)]
        _CASES[key] = dict(p=p, dens=dens, perm=perm, G=G, F=F, Y=Y, logz=np.array([m[0] for m in mom]),
                           mean=np.array([m[1] for m in mom]).T.reshape(len(F), Nq),
                           var=np.array([m[2] for m in mom]).T.reshape(len(F), Nq),
                           R=(dens[0].max(axis=1) - dens[0].min(axis=1)))
    return _CASES[key]


def _close_log(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), \
        float(np.max(np.abs(got - want)))


# ---- 1. logz -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq,which", CASES)
def test_logz_equals_the_model_and_the_marginal(D, N, Nq, which):
    c = _case(D, N, Nq, which)
    logz, mean, var = kdehip.conditional_moments(c["p"], c["G"], c["Y"])
    assert logz.shape == (Nq,) and mean.shape == var.shape == (len(c["F"]), Nq)
    print("logz: max |err| / bound", float(np.max(np.abs(logz - c["logz"]) / (1e-12 * np.maximum(1.0, np.abs(c["logz"]))))))
    _close_log(logz, c["logz"])
    _close_log(logz, kdehip.evaluate_log(kdehip.marginal(c["p"], c["G"]), c["Y"]))


@pytest.mark.parametrize("which", ["first", "last"])
def test_logz_far_outside_the_data(which):
    c = _case(6, 129, 257, which)
    y = c["dens"][0][c["G"]].max(axis=1) + 50.0
    logz, mean, var = kdehip.conditional_moments(c["p"], c["G"], y)
    want = cm.logz(c["dens"], c["G"], y, fma=True)
    assert cm.terms(c["dens"], c["G"], y, fma=True)[0] < -745.0 and math.isfinite(want)  # the marginal itself underflows
    _close_log(logz, [want])
    assert np.all(np.isfinite(mean)) and np.all(var >= c["dens"][2][c["F"]][:, None])


# ---- 2. moments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq,which", CASES)
def test_moments_equal_the_model(D, N, Nq, which):
    c = _case(D, N, Nq, which)
    _, mean, var = kdehip.conditional_moments(c["p"], c["G"], c["Y"])
    R, v = c["R"][c["F"]][:, None], c["dens"][2][c["F"]][:, None]
    em, ev = np.abs(mean - c["mean"]), np.abs(var - c["var"])
    print("mean: max err / bound", float(np.max(em / (1e-12 * (R + np.abs(c["mean"]))))),
          "var:", float(np.max(ev / (1e-12 * (R * R + v)))))
    assert np.all(np.isfinite(mean)) and np.all(em <= 1e-12 * (R + np.abs(c["mean"])))
    assert np.all(np.isfinite(var)) and np.all(ev <= 1e-12 * (R * R + v))
    assert np.all(var >= v)  # exactly: the excess is clamped at 0


# ---- 3. weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,Nq,which", CASES)
def test_weights_equal_the_model(D, N, Nq, which):
    c = _case(D, N, Nq, which)
    W, logz = kdehip.conditional_weights(c["p"], c["G"], c["Y"])
    assert W.shape == (Nq, N)
    _close_log(logz, c["logz"])
    o = c["perm"] - 1
    zero = c["dens"][1] == 0.0
    for q in range(Nq):
        ref = cm.weights(c["dens"], c["G"], c["Y"][:, q])
        got = W[q, o]  # leaf order
        assert np.all(np.abs(got - ref) <= 1e-12 * ref + 1e-300), (q, float(np.max(np.abs(got - ref))))
        assert abs(math.fsum(got.tolist()) - 1.0) <= 1e-12
        assert not got[zero].any()  # exactly 0


@pytest.mark.parametrize("D,N,Nq,which", [(2, 257, 300, "last"), (6, 129, 257, "first"), (8, 300, 700, "last"), (2, 8300, 3, "first")])
def test_chain_rule_through_condition(D, N, Nq, which):
    """log p([y; x]) = logz(y) + log p(x | y) with p(. | y) the density `condition` returns"""
    c = _case(D, N, Nq, which)
    rng = np.random.default_rng(D + N)
    for q in (0, Nq // 2):
        y = c["Y"][:, q]
        pc = kdehip.condition(c["p"], c["G"], y)
        assert pc.bt.dims == len(c["F"]) and pc.bt.num_points == N
        z = np.zeros((D, 3))
        z[c["G"]] = y[:, None]
        z[c["F"]] = c["mean"][:, q][:, None] + np.sqrt(c["var"][:, q])[:, None] * rng.standard_normal((len(c["F"]), 3))
        joint = kdehip.evaluate_log(c["p"], z)
        cond = kdehip.evaluate_log(pc, z[c["F"]])
        logz = kdehip.conditional_moments(c["p"], c["G"], y)[0][0]
        bound = 1e-12 * max(1.0, abs(logz)) + 1e-12 * np.maximum(1.0, np.abs(cond))
        assert np.all(np.isfinite(joint)) and np.all(np.abs(joint - (logz + cond)) <= bound), (joint, logz, cond)


# ---- 4. draws ------------------------------------------------------------------------------------------------------------
def _model_draws(c, seed, offset=0, man=None):
    Nq = c["Y"].shape[1]
    u = _uniforms(seed, offset, Nq)
    got = [cm.draw_label(c["dens"], c["perm"], c["G"], c["Y"][:, q], u[q], man) for q in range(Nq)]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got]), min(g[2] for g in got)


@pytest.mark.parametrize("D,N,Nq,which", CASES)
def test_draws_equal_the_model(D, N, Nq, which):
    c = _case(D, N, Nq, which)
    ind, leaf, gap = _model_draws(c, SEED)
    print("smallest gap between u S_0 and a boundary, relative to S_0:", gap)
    assert gap >= 1e-9  # no draw of this seed is near a boundary: none is excused below
    pts, got = kdehip.sample_conditional(c["p"], c["G"], c["Y"], seed=SEED)
    assert pts.shape == (len(c["F"]), Nq) and got.dtype == np.int64
    assert np.array_equal(got, ind)
    n = _device_normals(len(c["F"]), SEED, 0, Nq)
    want = c["dens"][0][c["F"]][:, leaf] + np.sqrt(c["dens"][2][c["F"]])[:, None] * n  # (numpy rounds the two separately)
    assert np.array_equal(pts, want)
    if Nq >= 2:  # sample_offset continues a stream: two half calls are the whole call
        h = Nq // 2
        a = kdehip.sample_conditional(c["p"], c["G"], c["Y"][:, :h], seed=SEED)
        b = kdehip.sample_conditional(c["p"], c["G"], c["Y"][:, h:], seed=SEED, sample_offset=h)
        assert np.array_equal(np.hstack([a[0], b[0]]), pts) and np.array_equal(np.concatenate([a[1], b[1]]), got)


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------
def _full(p, G, Y, seed=SEED, offset=0, manifold=None):
    """(logz, mean, var, pts, ind) of the public functions: two calls of the same entry"""
    lz, mean, var = kdehip.conditional_moments(p, G, Y, manifold=manifold)
    pts, ind = kdehip.sample_conditional(p, G, Y, seed=seed, sample_offset=offset, manifold=manifold)
    return lz, mean, var, pts, ind


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _mixed_items():
    """9 items of mixed D, N, Nq, masks and circularity: (host density, given dims, Y, manifold or None, asks moments)"""
    rng = np.random.default_rng(6)
    spec = [(2, 300, 40, [0], None), (2, 300, 300, [1], [1, 0]), (3, 700, 257, [0, 2], None), (3, 127, 5, [1], [0, 1, 0]),
            (6, 257, 129, [3, 4, 5], None), (6, 129, 64, [0], None), (8, 300, 33, [1, 2, 3, 4, 5, 6, 7], None),
            (2, 8300, 3, [0], None), (3, 700, 600, [2], [0, 0, 1])]
    out = []
    for D, N, Nq, G, man in spec:
        p = _density(rng, D, N)
        pts = _leaf(p)[0][0]
        Y = pts[G][:, rng.integers(0, N, size=Nq)] + 0.1 * rng.standard_normal((len(G), Nq))
        free_circ = man is not None and any(man[k] for k in range(D) if k not in G)
        out.append((p, G, Y, man, not free_circ))
    return out


def test_host_resident_and_batch_give_the_same_bits_run_after_run():
    import torch
    hosts = _mixed_items()
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    singles, items, devs = [], [], []
    for k, (p, G, Y, man, mom) in enumerate(hosts):
        D, Nq, nf = p.bt.dims, Y.shape[1], p.bt.dims - len(G)
        d = kdehip.DeviceDensity(p)
        devs.append(d)
        pts, ind = kdehip.sample_conditional(p, G, Y, seed=SEED + k, sample_offset=7 * k, manifold=man)
        rpts, rind = kdehip.sample_conditional(d, G, Y, seed=SEED + k, sample_offset=7 * k, manifold=man)
        assert np.array_equal(pts, rpts, equal_nan=True) and np.array_equal(ind, rind)
        if mom:
            lz, mean, var = kdehip.conditional_moments(p, G, Y, manifold=man)
            assert _same((lz, mean, var), kdehip.conditional_moments(d, G, Y, manifold=man))
            assert _same((lz, mean, var), d.conditional_moments(G, Y, manifold=man))
        else:
            with pytest.raises(kdehip.KdeHipError):
                kdehip.conditional_moments(p, G, Y, manifold=man)
            lz, mean, var = kdehip.conditional_weights(p, G, Y, manifold=man)[1], None, None
        # a call that asks only for logz returns the logz bits of the full call
        assert np.array_equal(kdehip.conditional_weights(d, G, Y, manifold=man)[1], lz)
        singles.append((lz, mean, var, pts, ind))
        order = np.argsort(G)
        it = dict(density=d, dims=G, given=torch.from_numpy(np.ascontiguousarray(Y[order].T)).to(dev), manifold=man,
                  seed=SEED + k, sample_offset=7 * k, logz=torch.zeros(Nq, **f64), pts=torch.zeros((Nq, nf), **f64),
                  ind=torch.zeros(Nq, dtype=torch.int64, device=dev))
        if mom:
            it.update(mean=torch.zeros((Nq, nf), **f64), var=torch.zeros((Nq, nf), **f64))
        items.append(it)

    def read(it):
        return (it["logz"].cpu().numpy(), it["mean"].cpu().numpy().T if "mean" in it else None,
                it["var"].cpu().numpy().T if "var" in it else None, it["pts"].cpu().numpy().T, it["ind"].cpu().numpy())

    def check():
        for it, want in zip(items, singles):
            got = read(it)
            for g, w in zip(got, want):
                assert (g is None and w is None) or np.array_equal(g, w, equal_nan=True)

    def clear():
        for it in items:
            for name in ("logz", "mean", "var", "pts", "ind"):
                if name in it:
                    it[name].zero_()

    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(dev)
    for order in (range(9), range(9), [4, 8, 0, 7, 2, 6, 1, 5, 3]):
        clear()
        torch.cuda.synchronize(dev)
        kdehip.conditional_device_batch([items[k] for k in order], stream=st.cuda_stream)
        st.synchronize()
        check()
    for d in devs:
        d.close()


@pytest.mark.parametrize("D,N,Nq,which", [(3, 127, 128, "first"), (6, 257, 257, "last"), (2, 8300, 3, "last")])
def test_condition_host_and_resident_build_the_same_density(D, N, Nq, which):
    c = _case(D, N, Nq, which)
    y = c["Y"][:, 0]
    host = kdehip.condition(c["p"], c["G"], y)
    with kdehip.DeviceDensity(c["p"]) as d, d.condition(c["G"], y) as dc:
        assert isinstance(dc, kdehip.DeviceDensity) and dc.dims == len(c["F"]) and dc.num_points == N
        got = dc.download()
    for name in ("means", "bandwidth", "bandwidthMin", "bandwidthMax"):
        assert np.array_equal(getattr(got, name), getattr(host, name)), name
    for name in ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation"):
        assert np.array_equal(getattr(got.bt, name), getattr(host.bt, name)), name
    W = kdehip.conditional_weights(c["p"], c["G"], y)[0][0]
    # (the builder divides by its own sum of the N weights: two orders of summing N positive terms differ by N ulps at most)
    assert np.allclose(kdehip.getWeights(host), W / W.sum(), rtol=N * 2.0 ** -52, atol=0.0)
    assert np.array_equal(kdehip.getPoints(host), kdehip.getPoints(c["p"])[c["F"]])
    assert np.array_equal(kdehip.getBW(host)[:, 0], kdehip.getBW(c["p"])[c["F"], 0])


# ---- 6. circular ---------------------------------------------------------------------------------------------------------
def _heading_density(shift=0.0, N=300, seed=31):
    """3-D (x, heading, z): two clusters, the heading of cluster A straddles +-pi, that of cluster B sits at 0.5"""
    rng = np.random.default_rng(seed)
    a = np.arange(N) % 2 == 0
    ang = np.where(a, cm.wrap(math.pi + 0.05 * rng.standard_normal(N)), 0.5 + 0.05 * rng.standard_normal(N))
    pts = np.vstack([np.where(a, -2.0, 2.0) + 0.2 * rng.standard_normal(N), ang + shift, 0.3 * rng.standard_normal(N)])
    w = rng.uniform(0.05, 1.0, size=N)
    w[::7] = 0.0
    return kdehip.kde(pts, [0.2, 0.05, 0.2], w), a


def test_a_given_heading_across_the_cut():
    man = [0, 1, 0]
    p, a = _heading_density()
    assert kdehip.getPoints(p)[1, a].min() < -3.0 and kdehip.getPoints(p)[1, a].max() > 3.0
    Y = np.array([[math.pi - 0.01, -math.pi + 0.01]])
    W, _ = kdehip.conditional_weights(p, [1], Y, manifold=man)
    assert np.all(W[:, a].sum(axis=1) > 1.0 - 1e-12)  # both queries weight the cluster at the cut
    line = kdehip.conditional_weights(p, [1], Y)[0]  # on the line each query sees only its own side of the cut
    pos = kdehip.getPoints(p)[1] > 0
    assert line[0, a & ~pos].max() < 1e-300 and line[1, a & pos].max() < 1e-300
    dens, perm = _leaf(p)
    for q in range(2):
        ref = cm.weights(dens, [1], Y[:, q], man)
        assert np.all(np.abs(W[q, perm - 1] - ref) <= 1e-12 * ref + 1e-300)
    # the data shifted by 2 pi: the same labels, the points in the Euclidean free dimensions bit for bit
    Yq = cm.wrap(math.pi + 0.05 * np.random.default_rng(3).standard_normal((1, 200)))
    c = dict(dens=dens, perm=perm, G=[1], Y=Yq)
    ind, _, gap = _model_draws(c, SEED, man=man)
    assert gap >= 1e-9
    pts, got = kdehip.sample_conditional(p, [1], Yq, seed=SEED, manifold=man)
    p2, _ = _heading_density(shift=2.0 * math.pi)
    dens2, perm2 = _leaf(p2)
    assert np.array_equal(perm2, perm)  # (the same tree: the labels of the two densities can be compared)
    pts2, got2 = kdehip.sample_conditional(p2, [1], Yq, seed=SEED, manifold=man)
    assert np.array_equal(got, ind) and np.array_equal(got2, ind) and np.array_equal(pts2, pts)
    assert a[got - 1].all()


def test_circular_data_that_never_wraps_gives_the_euclidean_bits():
    c = _case(3, 700, 700, "last")
    scale = 1.0 / (1.0 + np.abs(c["dens"][0]).max())  # every coordinate and query inside (-1, 1): no difference wraps
    pts = kdehip.getPoints(c["p"]) * scale
    p = kdehip.kde(pts, [0.05, 0.04, 0.06], kdehip.getWeights(c["p"]))
    Y = c["Y"] * scale
    plain = _full(p, c["G"], Y) + tuple(kdehip.conditional_weights(p, c["G"], Y))
    circ = _full(p, c["G"], Y, manifold=[0, 1, 1]) + tuple(kdehip.conditional_weights(p, c["G"], Y, manifold=[0, 1, 1]))
    assert _same(plain, circ)


def test_draws_in_a_circular_free_dimension_are_wrapped_and_its_moments_refused():
    p, a = _heading_density()
    man = [0, 1, 0]
    Y = np.full((1, 300), -2.0)  # x of the cluster whose heading straddles the cut
    pts, ind = kdehip.sample_conditional(p, [0], Y, seed=SEED, manifold=man)
    assert np.all(pts[0] >= -math.pi) and np.all(pts[0] < math.pi) and a[ind - 1].all()
    flat, ind2 = kdehip.sample_conditional(p, [0], Y, seed=SEED)
    assert np.array_equal(ind, ind2) and np.array_equal(pts[1], flat[1]) and np.array_equal(pts[0], cm.wrap(flat[0]))
    assert (flat[0] >= math.pi).any() or (flat[0] < -math.pi).any()  # some draw did leave the interval
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.conditional_moments(p, [0], Y, manifold=man)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with kdehip.DeviceDensity(p) as d:
        with pytest.raises(kdehip.KdeHipError) as e:
            d.conditional_moments([0, 2], Y[:, :2].repeat(2, axis=0), manifold=man)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert np.array_equal(d.sample_conditional([0], Y, seed=SEED, manifold=man)[0], pts)


# ---- 7. block skipping ---------------------------------------------------------------------------------------------------
def test_a_query_block_that_chose_one_group_skips_the_others():
    """257 queries: the first 256 (one query block) share a y next to ONE leaf, so their draws fall into few groups and the
    select sweep skips that block's other groups; the last query is elsewhere.  The results are those of the separate calls."""
    rng = np.random.default_rng(70)
    w = rng.uniform(0.05, 1.0, size=700)
    w[::5] = 0.0
    p = kdehip.kde(rng.standard_normal((3, 700)), [0.01], w)  # (the points are many bandwidths apart)
    (dens, perm), G = _leaf(p), [1, 2]
    assert p.bt.num_points > 4 * 128  # several groups
    leaf, other = (int(i) for i in np.flatnonzero(dens[1] > 0.0)[[350, 20]])
    y0 = dens[0][G, leaf] + 1e-3
    Y = np.hstack([np.repeat(y0[:, None], 256, axis=1), dens[0][G, other][:, None] - 2e-3])
    assert cm.weights(dens, G, y0)[leaf] > 0.5  # the shared query is close to that one leaf
    whole = _full(p, G, Y)
    first = _full(p, G, Y[:, :256])
    last = _full(p, G, Y[:, 256:], offset=256)
    for w, f, l in zip(whole, first, last):
        assert np.array_equal(w, np.concatenate([f, l], axis=-1))
    ind, _, gap = _model_draws(dict(dens=dens, perm=perm, G=G, Y=Y), SEED)
    assert gap >= 1e-9 and np.array_equal(whole[4], ind)
    assert np.count_nonzero(ind[:256] == perm[leaf]) > 128 and ind[256] == perm[other]


# ---- 8. refusals that need real handles -------------------------------------------------------------------------------------
def test_resident_refusals():
    import ctypes as C

    import torch
    c = _case(3, 127, 128, "first")
    dev = torch.device("cuda", 0)
    y = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    out = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    a = _lib.addr
    L = _lib.lib
    with kdehip.DeviceDensity(c["p"]) as d:
        for mask in (8, 9, 0, 7):  # a bit at or above D, none, all
            assert L.kdehip_conditional_device(d._h, mask, a(y), 4, 1, 0, a(out), None, None, None, None, None, None) == _lib.ERR_ARG
            assert L.kdehip_condition_weights_device(d._h, mask, a(y), 4, a(out), None, None, None) == _lib.ERR_ARG
            h = C.c_void_p()
            yy = np.zeros(3)
            assert L.kdehip_density_condition_device(C.byref(h), d._h, mask, _lib.ptr(yy, _lib.f64p), None, None) == _lib.ERR_ARG
        assert L.kdehip_conditional_device(d._h, 1, a(y), 4, 1, 0, None, None, None, a(out), None, None, None) == _lib.ERR_ARG
        assert L.kdehip_conditional_device(d._h, 1, a(y), 4, 1, 0, None, None, None, None, a(idx), None, None) == _lib.ERR_ARG
        assert L.kdehip_conditional_device(d._h, 1, a(y), 4, 1, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
        assert L.kdehip_conditional_device(d._h, 1, None, 4, 1, 0, a(out), None, None, None, None, None, None) == _lib.ERR_ARG
        assert L.kdehip_conditional_device(d._h, 1, a(y), -1, 1, 0, a(out), None, None, None, None, None, None) == _lib.ERR_ARG
        items = (_lib.CConditionalItem * 1)()
        items[0].bd, items[0].d_given, items[0].Nq, items[0].d_logz = d._h, a(y), 4, a(out)
        items[0].given_mask, items[0].circular_mask = 1, 8  # a circular bit at or above D
        assert L.kdehip_conditional_device_batch(1, items, None) == _lib.ERR_ARG
        with pytest.raises(kdehip.KdeHipError) as e:  # logz = -Inf: nothing to build a density from
            d.condition([0], [np.inf])
        assert e.value.code == _lib.ERR_ARG
    q = _density(np.random.default_rng(9), 3, 40)
    N, D = q.bt.num_points, q.bt.dims
    q.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    with kdehip.DeviceDensity(q) as d:
        assert L.kdehip_conditional_device(d._h, 1, a(y), 4, 1, 0, a(out), None, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
        assert L.kdehip_condition_weights_device(d._h, 1, a(y), 4, a(out), None, None, None) == _lib.ERR_UNSUPPORTED
        h = C.c_void_p()
        yy = np.zeros(3)
        assert L.kdehip_density_condition_device(C.byref(h), d._h, 1, _lib.ptr(yy, _lib.f64p), None, None) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize(dev)


def test_no_leaf_of_positive_weight():
    """S empty: logz = -Inf, mean and var NaN, ind = 0 and the point NaN"""
    rng = np.random.default_rng(1)
    p = kdehip.kde(rng.standard_normal((2, 130)), [0.3])
    p.bt.weights[:] = 0.0  # (the builder normalises: the zeros are written afterwards)
    Y = rng.standard_normal((1, 5))
    for q in (p, kdehip.DeviceDensity(p)):
        lz, mean, var = kdehip.conditional_moments(q, [0], Y)
        pts, ind = kdehip.sample_conditional(q, [0], Y, seed=1)
        assert np.all(lz == -np.inf) and np.isnan(mean).all() and np.isnan(var).all()
        assert np.isnan(pts).all() and not ind.any()
        W, lz2 = kdehip.conditional_weights(q, [0], Y)
        assert not W.any() and np.all(lz2 == -np.inf)
