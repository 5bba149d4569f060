"""Circular dimensions on RESIDENT densities (include/kdehip.h sections 2c-2e): `prodAppxMSGibbsS_device`,
`prodAppxMSGibbsS_resident`, `mul_device` and `mul_device_batch` with `manifold=`, which run the general sampler's circular
fast mode (csrc/gibbs_kernel.hip, kModeFastCirc), against the CPU oracle's enumerated manifold (oracle/kde_oracle.c
okde_gibbs1_manifold) on the host twin of the device Philox streams.

Comparison rule: labels identical; Euclidean dimensions within atol = 1e-12 (the project's bound for fast against generic
arithmetic, tests/test_gpu_manifold.py); circular dimensions on the circle, |wrap(gpu - oracle)| <= 1e-12 (a value within
rounding of +-pi may land on either side of the cut).  A label can flip only where a uniform falls within rounding (~1e-16
per draw) of a CDF boundary: the cap is zero flips.  The oracle alone is deterministic on these sizes (two runs on the same
streams return the same bits), so the cap compares one fixed set of labels.
The data are `_trees` of tests/test_gpu_manifold.py: clouds centred at the cut, so that wrapping happens."""
import numpy as np
import pytest

import kdehip
from oracle import oracle

pytestmark = pytest.mark.gpu

ARRAYS = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
DARRAYS = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")
ATOL = 1e-12


def _wrap(t):
    return t - 2.0 * np.pi * np.floor((t + np.pi) / (2.0 * np.pi))


def _trees(seed, D, Ns, circ):
    rng = np.random.default_rng(seed)
    g, o = [], []
    for n in Ns:
        p = rng.standard_normal((D, n)) * 0.7
        for d in range(D):
            if circ[d]:
                p[d] = _wrap(np.pi + 1.0 * rng.standard_normal(n))   # a cloud centred AT the cut
        ks = rng.uniform(0.15, 0.5, D)
        w = rng.uniform(0.3, 1.0, n)
        g.append(kdehip.kde(p, ks, w))
        o.append(oracle.OracleDensity(p, ks, w))
    return rng, g, o


def _device_product(dd, Np, Niter, seed, *, addEntropy=True, mask=None, manifold=None, sample_offset=0, precision=64,
                    nlev=None):
    """prodAppxMSGibbsS_device into torch arrays; returns (points[D, Np], indices[M, Np], labels[Np, M, L] or None)"""
    import torch
    D, M = dd[0].dims, len(dd)
    P = torch.zeros(D * Np, dtype=torch.float64, device="cuda:0")
    I = torch.zeros(M * Np, dtype=torch.int64, device="cuda:0")
    Lb = torch.zeros(Np * M * nlev, dtype=torch.int32, device="cuda:0") if nlev else None
    torch.cuda.synchronize()
    kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=Niter, seed=seed, sample_offset=sample_offset, addEntropy=addEntropy,
                                   partialDimMask=mask, manifold=manifold, precision=precision, d_labels=Lb)
    torch.cuda.synchronize()
    return (P.cpu().numpy().reshape(Np, D).T.copy(), I.cpu().numpy().reshape(Np, M).T.copy(),
            None if Lb is None else Lb.cpu().numpy().reshape(Np, M, nlev))


def _assert_points(gp, op, circ, why):
    for d in range(gp.shape[0]):
        diff = gp[d] - op[d]
        if circ[d]:
            diff = _wrap(diff)
        err = float(np.abs(diff).max())
        print(f"{why}: dimension {d} ({'circular' if circ[d] else 'euclid'}) max error {err:.3e}")
        assert err <= ATOL, (why, d, err)


def _against_oracle(g, o, Ns, D, Np, Niter, circ, mask, seed, why, check_differs=True):
    M = len(Ns)
    K, R, _, _ = oracle.rng_sizes(M, D, Np, Niter, Ns)
    randU, randN = kdehip.philox_streams(seed, 0, Np, K, R)
    L = oracle.nlevels(max(Ns))
    dd = [kdehip.DeviceDensity(t) for t in g]
    try:
        for addEntropy in (True, False):
            op, oi, ol = oracle.gibbs1(o, Np, Niter, randU, randN, addEntropy=addEntropy, partialDimMask=mask, manifold=circ,
                                       want_labels=True)
            gp, gi, gl = _device_product(dd, Np, Niter, seed, addEntropy=addEntropy, mask=mask, manifold=circ, nlev=L)
            flips = int((gi != oi).sum())
            print(f"{why}: addEntropy={addEntropy} label flips {flips}")
            assert flips == 0, why
            if Niter > 0:   # (the reference records a level's labels inside sampleIndex only)
                assert np.array_equal(gl, ol), why
            _assert_points(gp, op, circ, why)
            if addEntropy:
                for d in range(D):
                    if circ[d]:
                        assert np.all(gp[d] >= -np.pi) and np.all(gp[d] < np.pi), why
        if check_differs:
            cp, ci, _ = _device_product(dd, Np, Niter, seed, mask=mask, manifold=circ)
            ep, ei, _ = _device_product(dd, Np, Niter, seed, mask=mask)
            assert not (np.array_equal(ci, ei) and np.allclose(cp, ep)), why
    finally:
        for d in dd:
            d.close()


CASES = [
    (1, [6, 6], 64, 0, [1], None, "diffop (:290) and addop (:456) alone"),
    (1, [9, 5, 7], 64, 3, [1], None, "getMu / getLambda (:183-184)"),
    (2, [40, 55], 100, 2, [0, 1], None, "a Euclidean and a circular dimension"),
    (2, [120, 120, 120], 96, 2, [1, 1], [[1, 0], [1, 1], [0, 1]], "the reference angle under a mask"),
    (6, [1000, 700, 1000, 513], 130, 3, [0, 0, 0, 1, 1, 1], None, "streamed levels, a frontier that is no power of two"),
    (3, [5000, 3000], 70, 1, [0, 0, 1], None, "chunked tiles"),
]


@pytest.mark.parametrize("D,Ns,Np,Niter,circ,mask,why", CASES)
def test_resident_circular_product_equals_the_oracle(D, Ns, Np, Niter, circ, mask, why):
    _, g, o = _trees(23 * D + len(Ns) + Np, D, Ns, circ)
    _against_oracle(g, o, Ns, D, Np, Niter, circ, mask, 4000 + D * 10 + len(Ns), why)


def test_uniform_and_per_node_bandwidth_evaluators():
    """Which evaluator a level takes is the level's shared-bandwidth flag: a frontier of leaves of a `kde(points, ks)` density
    shares one bandwidth vector (EvalUniform), internal nodes carry their own moment-matched variances (EvalFast).  Two
    densities of N = 2 points have leaf levels ONLY (levels 1 and 2 are the two leaves), so with Niter = 0 every draw of the run
    goes through EvalUniform; the deep run (N = 40 / 55) draws on internal levels first (EvalFast) and on the leaves last.
    Both must equal the oracle, and both must differ from the Euclidean product."""
    pa = np.array([[0.1, -0.2], [3.0, -3.1]])
    pb = np.array([[-0.1, 0.3], [-3.0, 3.1]])
    ks = [0.4, 0.3]
    g = [kdehip.kde(pa, ks), kdehip.kde(pb, ks)]
    o = [oracle.OracleDensity(pa, ks), oracle.OracleDensity(pb, ks)]
    _against_oracle(g, o, [2, 2], 2, 64, 0, [0, 1], None, 91, "leaf levels only: the uniform-bandwidth evaluator")
    _, g2, o2 = _trees(23 * 2 + 2 + 100, 2, [40, 55], [0, 1])
    _against_oracle(g2, o2, [40, 55], 2, 100, 2, [0, 1], None, 92, "internal levels: the per-node evaluator, then the leaves")


def test_fallback_to_the_generic_circular_arithmetic():
    """One variance of 1e-320 (a denormal) takes the density set out of the fast forms' domain: the resident entry then runs
    the generic circular arithmetic, and the labels are still the oracle's."""
    rng = np.random.default_rng(77)
    D, Ns, Np, Niter, circ = 2, [24, 31], 64, 2, [0, 1]
    g, o = [], []
    for k, n in enumerate(Ns):
        p = rng.standard_normal((D, n)) * 0.7
        p[1] = _wrap(np.pi + rng.standard_normal(n))
        ks = rng.uniform(0.15, 0.5, D)
        t = kdehip.kde(p, ks)
        if k == 0:
            t.bandwidth[0] = 1e-320   # (flat [node * D + d]: dimension 0 of node 0, the root -- read at level 0 only)
        g.append(t)
        o.append(oracle.OracleDensity.from_arrays(D, n, t.means, t.bandwidth, t.bt.weights, t.bt.left_child, t.bt.right_child,
                                                  t.bt.permutation))
    M = len(Ns)
    K, R, _, _ = oracle.rng_sizes(M, D, Np, Niter, Ns)
    randU, randN = kdehip.philox_streams(5, 0, Np, K, R)
    op, oi = oracle.gibbs1(o, Np, Niter, randU, randN, manifold=circ)
    dd = [kdehip.DeviceDensity(t) for t in g]
    gp, gi, _ = _device_product(dd, Np, Niter, 5, manifold=circ)
    assert np.array_equal(gi, oi)
    _assert_points(gp, op, circ, "generic fallback")


def test_resident_entries_agree_and_zero_manifold_is_euclidean():
    D, Ns, Np, Niter, circ = 2, [40, 55], 100, 2, [0, 1]
    _, g, _ = _trees(11, D, Ns, circ)
    dd = [kdehip.DeviceDensity(t) for t in g]
    cp, ci, _ = _device_product(dd, Np, Niter, 9, manifold=circ)
    rp, ri = kdehip.prodAppxMSGibbsS_resident(dd, Np=Np, Niter=Niter, seed=9, manifold=circ)
    assert np.array_equal(rp, cp) and np.array_equal(ri, ci)
    ep, ei, _ = _device_product(dd, Np, Niter, 9)
    for man in ([0] * D, None):
        zp, zi, _ = _device_product(dd, Np, Niter, 9, manifold=man)
        assert np.array_equal(zp, ep) and np.array_equal(zi, ei)
        yp, yi = kdehip.prodAppxMSGibbsS_resident(dd, Np=Np, Niter=Niter, seed=9, manifold=man)
        assert np.array_equal(yp, ep) and np.array_equal(yi, ei)
    assert not (np.array_equal(ci, ei) and np.allclose(cp, ep))
    # sample_offset splits a run exactly
    h = Np // 2
    ap, ai, _ = _device_product(dd, h, Niter, 9, manifold=circ)
    bp, bi, _ = _device_product(dd, Np - h, Niter, 9, manifold=circ, sample_offset=h)
    assert np.array_equal(np.concatenate([ap, bp], axis=1), cp) and np.array_equal(np.concatenate([ai, bi], axis=1), ci)


def _same_density(a, b, what=""):
    assert a.bt.dims == b.bt.dims and a.bt.num_points == b.bt.num_points, what
    for name in ARRAYS:
        assert np.array_equal(getattr(a.bt, name), getattr(b.bt, name)), (what, name)
    for name in DARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


def _mul_by_hand(dd, seed, circ, addEntropy=True):
    """prodAppxMSGibbsS_device(manifold=, Niter=5, Np=round(mean N)) then from_device_points(manifold=) on the device matrix"""
    import torch
    D, M = dd[0].dims, len(dd)
    Np = int(round(float(np.mean([d.num_points for d in dd]))))
    P = torch.zeros(D * Np, dtype=torch.float64, device="cuda:0")
    I = torch.zeros(M * Np, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=5, seed=seed, addEntropy=addEntropy, manifold=circ)
    torch.cuda.synchronize()
    return kdehip.DeviceDensity.from_device_points(P, D, Np, manifold=circ)


@pytest.fixture(scope="module")
def shape_2d_3x200():
    """config 2's shape (2-D, 3 x 200 points) with the second dimension an angle; seven such density sets"""
    sets = []
    for k in range(7):
        _, g, _ = _trees(300 + k, 2, [200, 200, 200], [0, 1])
        sets.append([kdehip.DeviceDensity(t) for t in g])
    yield sets
    for s in sets:
        for d in s:
            d.close()


def test_mul_device_manifold_is_product_then_kde(shape_2d_3x200):
    dd, circ = shape_2d_3x200[0], [0, 1]
    got = kdehip.mul_device(dd, seed=31, manifold=circ)
    ref = _mul_by_hand(dd, 31, circ)
    _same_density(got.download(), ref.download(), "mul_device(manifold=)")
    assert np.array_equal(got.bw, ref.bw) and got.nevals == ref.nevals
    assert list(got.manifold) == circ
    euc = kdehip.mul_device(dd, seed=31)
    assert euc.manifold is None
    assert got.bw[1] != euc.bw[1]   # cut-centred data: the circular search and product see another spread
    # all zeros is the Euclidean `*`
    zer = kdehip.mul_device(dd, seed=31, manifold=[0, 0])
    _same_density(zer.download(), euc.download(), "manifold of zeros")


def test_mul_device_batch_manifold_equals_the_single_calls(shape_2d_3x200):
    sets, circ = shape_2d_3x200, [0, 1]
    products = [sets[0], sets[1], sets[2], sets[3], sets[4], [sets[5][0]]]
    mans = [circ, None, circ, [0, 0], circ, circ]
    flags = [True, True, True, True, False, False]   # (the last item: one density, no entropy = the shortcut)
    seeds = [501, 502, 503, 504, 505, 506]
    outs = kdehip.mul_device_batch(products, addEntropy=flags, seeds=seeds, manifold=mans)
    for k, out in enumerate(outs):
        one = kdehip.mul_device(products[k], addEntropy=flags[k], seed=seeds[k], manifold=mans[k])
        _same_density(out.download(), one.download(), f"item {k}")
        assert np.array_equal(out.bw, one.bw) and out.nevals == one.nevals, k
    # the Euclidean items are today's batch outputs
    today = kdehip.mul_device_batch([products[1], products[3]], addEntropy=True, seeds=[502, 504])
    _same_density(outs[1].download(), today[0].download(), "Euclidean item 1")
    _same_density(outs[3].download(), today[1].download(), "Euclidean item 3")
    # one manifold for all products
    shared = kdehip.mul_device_batch([sets[0], sets[2]], seeds=[501, 503], manifold=circ)
    _same_density(shared[0].download(), outs[0].download(), "shared manifold 0")
    _same_density(shared[1].download(), outs[2].download(), "shared manifold 2")


def test_argument_errors():
    import torch
    rng = np.random.default_rng(0)
    g2 = [kdehip.DeviceDensity(kdehip.kde(rng.standard_normal((2, 20)), [0.3])) for _ in range(2)]
    g3 = kdehip.DeviceDensity(kdehip.kde(rng.standard_normal((3, 20)), [0.3]))
    P = torch.zeros(3 * 8, dtype=torch.float64, device="cuda:0")
    I = torch.zeros(2 * 8, dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):
        kdehip.prodAppxMSGibbsS_device(g2, P, I, Np=8, seed=1, manifold=[1])          # one entry per dimension
    with pytest.raises(ValueError):
        kdehip.mul_device(g2, seed=1, manifold=[1, 0, 0])
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.prodAppxMSGibbsS_device(g2, P, I, Np=8, seed=1, manifold=[0, 2])       # not a member of the enum
    assert e.value.code == kdehip._lib.ERR_ARG
    with pytest.raises(kdehip.KdeHipError):
        kdehip.prodAppxMSGibbsS_resident(g2, Np=8, seed=1, manifold=[0, 2])
    with pytest.raises(kdehip.KdeHipError):
        kdehip.mul_device(g2, seed=1, manifold=[2, 0])
    with pytest.raises(kdehip.KdeHipError):
        kdehip.mul_device_batch([g2], seeds=[1], manifold=[[0, 2]])
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.prodAppxMSGibbsS_device(g2, P, I, Np=8, seed=1, manifold=[0, 1], precision=32)
    assert e.value.code == kdehip._lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):                                                   # densities of different dimension
        kdehip.prodAppxMSGibbsS_device([g2[0], g3], P, I, Np=8, seed=1, manifold=[0, 1])
    with pytest.raises(ValueError):
        kdehip.mul_device([g2[0], g3], seed=1, manifold=[0, 1])
