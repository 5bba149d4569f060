"""Tree construction on a manifold (include/kdehip.h sections 4, 2d, 5d) on the GPU: the device builder
(csrc/treebuild.hip, tree_build_kernel<true>) against the host builder, which tests/test_tree_manifold_host.py holds to the
reference's buildBall! chain with operators; the batched build; `kde!(points, addop, diffop)`; the resident chain
(`from_device_points`, `mul_device`, `mul_device_batch` with `tree_manifold=`); and a circular tree under the sampler.
Everything is compared bit for bit except the sampler's points (1e-12, the contract of the resident entries)."""
import numpy as np
import pytest

import kdehip
from kdehip import _lib
from oracle import oracle
from tests import manifold_tree_model as tm

pytestmark = pytest.mark.gpu


def _same(a, b, what=""):
    assert a.bt.dims == b.bt.dims and a.bt.num_points == b.bt.num_points, what
    assert tm.differing(tm.density_arrays(a), tm.density_arrays(b)) == [], what


# (D, N, manifold, kind, weighted): the one-lane replay (<= 32 leaves), the wavefront tape (> 32), ranges that end one past
# a multiple of 64, mixed and alternating masks, the deepest LDS carve-up
BUILDER_CASES = [
    (1, 2, [1], "straddle", False), (1, 3, [1], "outside", False), (2, 5, [1, 1], "uniform", True),
    (2, 33, [0, 1], "straddle", False), (2, 64, [1, 1], "outside", False), (2, 65, [1, 0], "straddle", True),
    (3, 257, [1, 0, 1], "uniform", False), (6, 1000, [0, 0, 0, 1, 1, 1], "straddle", False),
    (8, 300, [0, 1, 0, 1, 0, 1, 0, 1], "outside", True), (2, 500, [1, 1], "ties", False),
    (3, 200, [1, 1, 0], "constant", False), (1, 1000, [1], "ties", True), (2, 4096, [0, 1], "straddle", False),
]


@pytest.mark.parametrize("D,N,man,kind,weighted", BUILDER_CASES)
def test_gpu_builder_is_the_host_builder(D, N, man, kind, weighted):
    assert _lib.lib.kdehip_make_density_device_supported(D, N) == 1
    pts, ks, w = tm.tree_case(kind, 77 * D + N, D, N, man, weighted, nks=D if N % 2 else 1)
    host = kdehip.kde(pts, ks, w, tree_manifold=man)
    dev = kdehip.kde(pts, ks, w, device=0, tree_manifold=man)
    _same(dev, host, f"{kind} D={D} N={N}")
    assert list(dev.tree_manifold) == man


def test_gpu_builder_with_an_all_zero_mask_is_the_euclidean_kernel():
    pts, ks, w = tm.tree_case("straddle", 3, 2, 300, [1, 1], True)
    _same(kdehip.kde(pts, ks, w, device=0, tree_manifold=[0, 0]), kdehip.kde(pts, ks, w, device=0), "zeros")
    _same(kdehip.kde(pts, ks, w, device=0), kdehip.kde(pts, ks, w), "euclid")
    unit = tm.tree_case("unit", 4, 2, 300, [1, 1], True)
    _same(kdehip.kde(*unit, device=0, tree_manifold=[1, 1]), kdehip.kde(*unit, device=0), "data inside [-1, 1]")


def test_kde_batch_with_one_tree_manifold():
    man, D = [0, 1], 2
    Ns = [1, 2, 7, 31, 32, 33, 63, 64, 65, 100, 129, 200, 257, 500, 1025, 20000]  # 1 and 20000: the host builder's
    assert _lib.lib.kdehip_make_density_device_supported(D, 20000) == 0
    kinds = ["straddle", "uniform", "outside", "ties"]
    cases = [tm.tree_case(kinds[k % 4], 500 + n, D, n, man, weighted=k % 2 == 0) for k, n in enumerate(Ns)]
    got = kdehip.kde_batch(cases, device=0, tree_manifold=man)
    assert len(got) == len(Ns)
    for n, g, (pts, ks, w) in zip(Ns, got, cases):
        _same(g, kdehip.kde(pts, ks, w, tree_manifold=man), f"N={n}")
        assert list(g.tree_manifold) == man


@pytest.mark.parametrize("D,N,man", [(1, 150, [1]), (2, 300, [0, 1]), (3, 2500, [1, 0, 1])])
def test_kde_with_both_manifolds_is_search_then_build(D, N, man):
    """kde!(points, addop, diffop): the search is kde(pts, manifold=m)'s, the tree kde(pts, bw, tree_manifold=m)'s"""
    pts, _, _ = tm.tree_case("straddle", 900 + N, D, N, man)
    both = kdehip.kde(pts, manifold=man, tree_manifold=man)
    search_only = kdehip.kde(pts, manifold=man)
    assert np.array_equal(both.bandwidth[N * D:], search_only.bandwidth[N * D:])
    bw = kdehip.auto_bandwidth(pts, manifold=man)
    _same(both, kdehip.kde(pts, bw, tree_manifold=man), "search, then build")
    _same(both, kdehip.kde_auto(pts, overlap=False, manifold=man, tree_manifold=man), "one after the other")
    assert not np.array_equal(both.bt.permutation, search_only.bt.permutation)
    assert list(both.tree_manifold) == man and search_only.tree_manifold is None


def _sets(count, D, Ns, man, seed):
    out = []
    for k in range(count):
        trees = [kdehip.kde(*tm.tree_case("straddle", seed + 10 * k + j, D, n, man, weighted=True, nks=D), tree_manifold=man)
                 for j, n in enumerate(Ns)]
        out.append([kdehip.DeviceDensity(t) for t in trees])
    return out


@pytest.fixture(scope="module")
def resident_sets():
    sets = _sets(6, 2, [200, 200, 200], [0, 1], 3000)
    yield sets
    for s in sets:
        for d in s:
            d.close()


def _product_matrix(dd, seed, man, addEntropy=True):
    import torch
    D, M = dd[0].dims, len(dd)
    Np = int(round(float(np.mean([d.num_points for d in dd]))))
    P = torch.zeros(D * Np, dtype=torch.float64, device="cuda:0")
    I = torch.zeros(M * Np, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=5, seed=seed, addEntropy=addEntropy, manifold=man)
    torch.cuda.synchronize()
    return P, D, Np


def test_from_device_points_with_a_tree_manifold_is_the_host_route(resident_sets):
    man = [0, 1]
    P, D, Np = _product_matrix(resident_sets[0], 61, man)
    pts = P.cpu().numpy().reshape(Np, D).T.copy()
    got = kdehip.DeviceDensity.from_device_points(P, D, Np, manifold=man, tree_manifold=man)
    _same(got.download(), kdehip.kde(pts, manifold=man, tree_manifold=man), "from_device_points(tree_manifold=)")
    assert list(got.tree_manifold) == man and list(got.manifold) == man
    plain = kdehip.DeviceDensity.from_device_points(P, D, Np, manifold=man)
    assert plain.tree_manifold is None
    _same(plain.download(), kdehip.kde(pts, manifold=man), "the tree stays Euclidean without the keyword")
    assert not np.array_equal(got.download().bt.permutation, plain.download().bt.permutation)
    zer = kdehip.DeviceDensity.from_device_points(P, D, Np, manifold=man, tree_manifold=[0, 0])
    _same(zer.download(), plain.download(), "tree_manifold of zeros")


def test_mul_device_with_a_tree_manifold_is_product_then_kde(resident_sets):
    dd, man = resident_sets[0], [0, 1]
    got = kdehip.mul_device(dd, seed=31, manifold=man, tree_manifold=man)
    P, D, Np = _product_matrix(dd, 31, man)
    ref = kdehip.DeviceDensity.from_device_points(P, D, Np, manifold=man, tree_manifold=man)
    _same(got.download(), ref.download(), "mul_device(tree_manifold=)")
    assert np.array_equal(got.bw, ref.bw) and got.nevals == ref.nevals
    assert list(got.tree_manifold) == man
    old = kdehip.mul_device(dd, seed=31, manifold=man)
    assert old.tree_manifold is None and np.array_equal(old.bw, got.bw)
    assert not np.array_equal(old.download().bt.permutation, got.download().bt.permutation)
    # the one-density shortcut: kde! of its own points, with both manifolds
    one = kdehip.mul_device([dd[0]], addEntropy=False, seed=1, manifold=man, tree_manifold=man)
    pts, _, _ = tm.tree_case("straddle", 3000, 2, 200, man, weighted=True, nks=2)  # (the points dd[0] was built from)
    _same(one.download(), kdehip.kde(pts, manifold=man, tree_manifold=man), "shortcut")


def test_mul_device_batch_with_tree_manifolds_equals_the_single_calls(resident_sets):
    sets, man = resident_sets, [0, 1]
    products = [sets[0], sets[1], sets[2], sets[3], sets[4], [sets[5][0]]]
    mans = [man, None, man, man, man, man]
    tmans = [man, None, None, [0, 0], man, man]   # circular and Euclidean trees mixed
    flags = [True, True, True, True, False, False]  # (the last item: one density, no entropy = the shortcut)
    seeds = [701, 702, 703, 704, 705, 706]
    outs = kdehip.mul_device_batch(products, addEntropy=flags, seeds=seeds, manifold=mans, tree_manifold=tmans)
    for k, out in enumerate(outs):
        one = kdehip.mul_device(products[k], addEntropy=flags[k], seed=seeds[k], manifold=mans[k], tree_manifold=tmans[k])
        _same(out.download(), one.download(), f"item {k}")
        assert np.array_equal(out.bw, one.bw) and out.nevals == one.nevals, k
    assert list(outs[0].tree_manifold) == man and outs[1].tree_manifold is None
    # the items without a circular tree are the _manifold batch's
    before = kdehip.mul_device_batch(products[1:4], seeds=seeds[1:4], manifold=mans[1:4])
    for k in range(3):
        _same(outs[1 + k].download(), before[k].download(), f"Euclidean-tree item {1 + k}")
    # one tree_manifold for all products
    shared = kdehip.mul_device_batch([sets[0], sets[4]], addEntropy=[True, False], seeds=[701, 705], manifold=man, tree_manifold=man)
    _same(shared[0].download(), outs[0].download(), "shared 0")
    _same(shared[1].download(), outs[4].download(), "shared 4")
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.mul_device_batch([sets[0]], seeds=[1], tree_manifold=[[0, 2]])
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        kdehip.mul_device(sets[0], seed=1, tree_manifold=[1])


def _wrap(t):
    return t - 2.0 * np.pi * np.floor((t + np.pi) / (2.0 * np.pi))


def test_a_circular_tree_flows_through_the_sampler():
    """The sampler reads means, variances, weights, children and the permutation of whatever tree it is given: two densities
    concentrated at the cut, built with the circular operators, sampled on the circle, against the oracle's enumerated
    manifold on the same arrays and the host twin of the Philox streams."""
    man, D, N, Np, Niter, seed = [0, 1], 2, 200, 128, 3, 4242
    cases = [tm.tree_case("straddle", 800 + j, D, N, man, weighted=True, nks=D) for j in range(2)]
    circ = [kdehip.kde(*c, tree_manifold=man) for c in cases]
    eucl = [kdehip.kde(*c) for c in cases]
    K, R, _, _ = oracle.rng_sizes(2, D, Np, Niter, [N, N])
    randU, randN = kdehip.philox_streams(seed, 0, Np, K, R)
    labels = {}
    for name, trees in (("circular", circ), ("euclid", eucl)):
        o = [oracle.OracleDensity.from_arrays(D, N, t.means, t.bandwidth, t.bt.weights, t.bt.left_child, t.bt.right_child,
                                              t.bt.permutation) for t in trees]
        op, oi = oracle.gibbs1(o, Np, Niter, randU, randN, manifold=man)
        dd = [kdehip.DeviceDensity(t) for t in trees]
        try:
            gp, gi = kdehip.prodAppxMSGibbsS_resident(dd, Np=Np, Niter=Niter, seed=seed, manifold=man)
        finally:
            for d in dd:
                d.close()
        assert np.array_equal(gi, oi), name
        err = [float(np.abs(gp[0] - op[0]).max()), float(np.abs(_wrap(gp[1] - op[1])).max())]
        print(f"{name} trees: max point error {err}")
        assert max(err) <= 1e-12, name
        labels[name] = gi
    assert not np.array_equal(labels["circular"], labels["euclid"])
