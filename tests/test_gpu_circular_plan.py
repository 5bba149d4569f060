"""Circular dimensions on RESIDENT PLANS (include/kdehip.h section 2: kdehip_product_create_manifold): `ProductPlan(manifold=)`
sampled with device Philox must return byte for byte what the one-shot resident entry (`prodAppxMSGibbsS_resident(manifold=)`,
kdehip_prod_philox_device_manifold) returns, and both must match the CPU oracle's enumerated manifold (okde_gibbs1_manifold)
on the host twin of the Philox streams: labels identical (zero flips), points within 1e-12, circular dimensions compared on
the circle.  The data straddle the cut (tests/circular_plan_cases.py)."""
import numpy as np
import pytest

import kdehip
from oracle import oracle
from tests.circular_plan_cases import assert_points, cut_trees, oracle_run, refused_trees

pytestmark = pytest.mark.gpu

SHAPES = {
    "d2": (2, [50, 60], 40, 2, [0, 1], [[1, 1], [1, 0]]),
    "d3": (3, [70, 70, 70], 37, 2, [1, 0, 1], [[1, 1, 1], [0, 1, 1], [1, 1, 0]]),
    "d6": (6, [130, 130, 130, 130], 64, 3, [0, 0, 0, 1, 1, 1],
           [[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 0, 1]]),
}
_cache = {}


def _shape(name):
    """the densities of a shape: host, oracle and resident copies, built once for the module"""
    if name not in _cache:
        D, Ns, Np, Niter, circ, mask = SHAPES[name]
        g, o = cut_trees(100 + D, D, Ns, circ)
        _cache[name] = (g, o, [kdehip.DeviceDensity(t) for t in g])
    return _cache[name]


@pytest.mark.parametrize("variant", ["plain", "no_entropy", "masked", "labels"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_equals_the_one_shot_entry_and_the_oracle(name, variant):
    D, Ns, Np, Niter, circ, mask = SHAPES[name]
    g, o, dd = _shape(name)
    seed = 7000 + D
    addEntropy = variant != "no_entropy"
    m = mask if variant == "masked" else None
    why = f"{name}/{variant}"
    with kdehip.ProductPlan(g, partialDimMask=m, manifold=circ) as plan:
        assert list(plan.manifold) == circ
        assert plan.fast_math_path
        out = plan.sample(Np, Niter=Niter, seed=seed, addEntropy=addEntropy, want_labels=(variant == "labels"))
    rp, ri = kdehip.prodAppxMSGibbsS_resident(dd, Np=Np, Niter=Niter, seed=seed, addEntropy=addEntropy, partialDimMask=m,
                                              manifold=circ)
    assert np.array_equal(out[0], rp) and np.array_equal(out[1], ri), why
    op, oi, ol = oracle_run(o, Ns, D, Np, Niter, circ, seed, addEntropy=addEntropy, mask=m)
    flips = int((out[1] != oi).sum())
    print(f"{why}: label flips {flips}")
    assert flips == 0, why
    assert_points(out[0], op, circ, why)
    if variant == "labels":
        assert np.array_equal(out[2], ol), why   # the label kept at the end of every level
    if addEntropy and m is None:
        for d in range(D):
            if circ[d]:
                assert np.all(out[0][d] >= -np.pi) and np.all(out[0][d] < np.pi), why
    # the circular operators were applied: the Euclidean plan on the same densities gives other numbers
    with kdehip.ProductPlan(g, partialDimMask=m) as euc:
        ep, ei = euc.sample(Np, Niter=Niter, seed=seed, addEntropy=addEntropy)
    assert not (np.array_equal(ei, out[1]) and np.allclose(ep, out[0])), why


def test_sample_offset_splits_a_run():
    D, Ns, Np, Niter, circ, _ = SHAPES["d2"]
    g, _, _ = _shape("d2")
    with kdehip.ProductPlan(g, manifold=circ) as plan:
        wp, wi = plan.sample(40, Niter=Niter, seed=3)
        ap, ai = plan.sample(20, Niter=Niter, seed=3, sample_offset=0)
        bp, bi = plan.sample(20, Niter=Niter, seed=3, sample_offset=20)
    assert np.array_equal(np.concatenate([ap, bp], axis=1), wp)
    assert np.array_equal(np.concatenate([ai, bi], axis=1), wi)


def test_caller_streams_on_a_circular_plan():
    import torch
    D, Ns, Np, Niter, circ, _ = SHAPES["d3"]
    g, _, _ = _shape("d3")
    M = len(Ns)
    K, R, nU, nN = oracle.rng_sizes(M, D, Np, Niter, Ns)
    rng = np.random.default_rng(5)
    randU, randN = rng.random(nU), rng.standard_normal(nN)
    glbs = kdehip.makeEmptyGbGlb(recordChoosen=True)
    rp = np.zeros(D * Np)
    ri = np.ones((M, Np), dtype=np.int64)
    kdehip.gibbs1(M, g, Np, Niter, rp, ri, randU, randN, glbs=glbs, manifold=circ)   # the generic arithmetic
    dev = torch.device("cuda", 0)
    with kdehip.ProductPlan(g, manifold=circ) as plan:
        L = plan.nlevels
        dU, dN = torch.from_numpy(randU).to(dev), torch.from_numpy(randN).to(dev)
        P = torch.zeros(D * Np, dtype=torch.float64, device=dev)
        I = torch.zeros(M * Np, dtype=torch.int64, device=dev)
        Lb = torch.zeros(Np * M * L, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        plan.sample_streams_device(Np, Niter, dU, nU, dN, nN, True, P, I, Lb)
        torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy().reshape(Np, M).T, ri)
    lab = Lb.cpu().numpy().reshape(Np, M, L)
    want = np.array([[[glbs.labelsChoosen[s + 1][j + 1][l + 1] for l in range(L)] for j in range(M)] for s in range(Np)])
    assert np.array_equal(lab, want)
    assert_points(P.cpu().numpy().reshape(Np, D).T, rp.reshape(Np, D).T, circ, "caller streams")


def test_generic_fallback_plan():
    D, Ns, Np, Niter, circ = 2, [24, 31], 64, 2, [0, 1]
    g, o = refused_trees(77, D, Ns, circ)
    dd = [kdehip.DeviceDensity(t) for t in g]
    with kdehip.ProductPlan(g, manifold=circ) as plan:
        assert plan.fast_math_path == 0
        assert plan.kernel_name(Np) == "gibbs_product_kernel"
        pp, pi = plan.sample(Np, Niter=Niter, seed=5)
    rp, ri = kdehip.prodAppxMSGibbsS_resident(dd, Np=Np, Niter=Niter, seed=5, manifold=circ)
    assert np.array_equal(pp, rp) and np.array_equal(pi, ri)
    op, oi, _ = oracle_run(o, Ns, D, Np, Niter, circ, 5)
    assert np.array_equal(pi, oi)
    assert_points(pp, op, circ, "generic fallback")


def test_plan_diagnostics_and_the_euclidean_manifold():
    D, Ns, Np, Niter, circ, _ = SHAPES["d2"]
    g, _, _ = _shape("d2")
    with kdehip.ProductPlan(g, manifold=circ) as plan:
        assert plan.kernel_name(Np) == "gibbs_product_kernel"
        assert plan.kernel_name(4096) == "gibbs_product_kernel"
        ref = plan.sample(Np, Niter=Niter, seed=1)
        assert plan.screen_stats()["levels"] == 0
        assert plan.launch_geometry(Np) == {"waves": 4, "team": 1}
        assert plan.fallback_count() >= 0
        for v in (8, 16):   # the workgroup width never changes a result
            plan.set_variant(v)
            assert plan.launch_geometry(Np)["waves"] == v
            got = plan.sample(Np, Niter=Niter, seed=1)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    today = kdehip.prodAppxMSGibbsS(None, g, None, None, Niter=Niter, Np=Np, seed=1)   # (kdehip_prod_philox)
    for man in (None, [0, 0], ["euclid", "euclid"]):
        with kdehip.ProductPlan(g, manifold=man) as plan:
            assert plan.kernel_name(Np) == "gibbs_lean_kernel"
            p, i = plan.sample(Np, Niter=Niter, seed=1)
        assert np.array_equal(p, today[0]) and np.array_equal(i, today[1]), man
    assert not np.array_equal(ref[0], today[0])


def test_circular_plan_runs_can_be_captured_in_a_hip_graph():
    """As tests/test_gpu_edge.py captures a Euclidean plan: a linear graph of two runs at offsets 0 and 20 on a side stream,
    replayed once, equals the uncaptured runs."""
    import torch
    D, Ns, _, Niter, circ, _ = SHAPES["d2"]
    g, _, _ = _shape("d2")
    M, h, seed = len(Ns), 20, 3
    dev = torch.device("cuda", 0)
    with kdehip.ProductPlan(g, manifold=circ) as plan:
        ap, ai = plan.sample(h, Niter=Niter, seed=seed, sample_offset=0)
        bp, bi = plan.sample(h, Niter=Niter, seed=seed, sample_offset=h)
        P = torch.zeros(2 * h * D, dtype=torch.float64, device=dev)
        I = torch.zeros(2 * h * M, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            plan.sample_philox_device(h, Niter, seed, 0, True, P, I, None, side.cuda_stream)   # warm-up on this stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st = torch.cuda.current_stream(dev).cuda_stream
            plan.sample_philox_device(h, Niter, seed, 0, True, P, I, None, st)
            plan.sample_philox_device(h, Niter, seed, h, True, P[h * D:], I[h * M:], None, st)
        P.zero_()
        I.zero_()
        graph.replay()
        torch.cuda.synchronize()
        gp, gi = P.cpu().numpy().reshape(2 * h, D).T, I.cpu().numpy().reshape(2 * h, M).T
    assert np.array_equal(gp, np.concatenate([ap, bp], axis=1))
    assert np.array_equal(gi, np.concatenate([ai, bi], axis=1))
