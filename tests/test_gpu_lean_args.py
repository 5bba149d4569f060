"""The argument routes of the register-resident sampler (csrc/gibbs_lean.hip): what a kernel needs only before or after its
level loop -- the caller's random streams and their lengths, the Philox sample offset, the label trace, the output arrays
-- is read from the kernel-argument segment where it is used, and plans that are resident throughout run a build of their
own.  Smallest shapes that reach every route:

  case A  D = 2, three densities of 70, 90 and 130 points, 9 chains (a last workgroup with dead chains), Niter = 2
  case B  BASELINE config 3's shape (D = 6, 4 x 1000 points: resident, tabulated and resident screened levels), 9 and 17
          chains (17: tables and screen tiles get built, the resident build runs), Niter = 2

at 8 and 16 chains per workgroup (the widths that come as a resident / staged pair) and at the width a run that small gets
by itself.  Peer stores: tests/test_gpu_multi.py."""
import numpy as np
import pytest

import kdehip
from oracle import oracle
from tests.helpers import silverman_bw, synth_mixture

pytestmark = pytest.mark.gpu

CASES = {
    "A": (2, [70, 90, 130], [9], 2),
    "B": (6, [1000] * 4, [9, 17], 2),
}
_cache = {}


def _case(name):
    """the case's densities (library and oracle side), built once"""
    if name not in _cache:
        D, Ns, _, _ = CASES[name]
        rng = np.random.default_rng(4100 + ord(name))
        pts = [synth_mixture(rng, D, N) for N in Ns]
        bws = [np.where(silverman_bw(p) > 0, silverman_bw(p), 0.5) for p in pts]
        _cache[name] = (pts, bws, [kdehip.kde(p, b) for p, b in zip(pts, bws)],
                        [oracle.OracleDensity(p, b) for p, b in zip(pts, bws)])
    return _cache[name]


def _runs():
    return [(name, Np) for name, (_, _, Nps, _) in CASES.items() for Np in Nps]


@pytest.mark.parametrize("name,Np", _runs())
def test_caller_streams_entropy_and_label_trace(name, Np):
    """caller-supplied randU / randN, addEntropy 0 and 1, the label trace of every level: labels equal to the oracle's on
    the identical streams, points to 1e-12"""
    import torch
    D, Ns, _, Niter = CASES[name]
    _, _, g, o = _case(name)
    M, L = len(Ns), kdehip.nlevels(max(Ns))
    K, R, nU, nN = oracle.rng_sizes(M, D, Np, Niter, Ns)
    rng = np.random.default_rng(17 + Np)
    randU, randN = rng.random(nU), rng.standard_normal(nN)
    dev = torch.device("cuda", 0)
    dU, dN = torch.from_numpy(randU).to(dev), torch.from_numpy(randN).to(dev)
    with kdehip.ProductPlan(g) as plan:
        for addEntropy in (True, False):
            op, oi, ol = oracle.gibbs1(o, Np, Niter, randU, randN, addEntropy=addEntropy, want_labels=True)
            for variant in (0, 8, 16):
                plan.set_variant(variant)
                d_pts = torch.full((D * Np,), -7.0, dtype=torch.float64, device=dev)
                d_ind = torch.full((M * Np,), -7, dtype=torch.int64, device=dev)
                d_lab = torch.full((Np * M * L,), -7, dtype=torch.int32, device=dev)
                plan.sample_streams_device(Np, Niter, dU, nU, dN, nN, addEntropy, d_pts, d_ind, d_lab)
                torch.cuda.synchronize()
                gp = d_pts.cpu().numpy().reshape(Np, D).T
                gi = d_ind.cpu().numpy().reshape(Np, M).T
                gl = d_lab.cpu().numpy().reshape(Np, M, L)
                assert np.array_equal(gi, oi), (variant, addEntropy)
                assert np.array_equal(gl, np.asarray(ol).reshape(Np, M, L)), (variant, addEntropy)
                assert np.allclose(gp, op, rtol=1e-12, atol=1e-12), (variant, addEntropy)


@pytest.mark.parametrize("name,Np", _runs())
def test_device_philox_with_sample_offset(name, Np):
    """the one-shot device entry with a non-zero sample offset against the resident plan's run of the same product: bit for
    bit, label trace included, at every width"""
    import torch
    D, Ns, _, Niter = CASES[name]
    _, _, g, _ = _case(name)
    M, L = len(Ns), kdehip.nlevels(max(Ns))
    dev = torch.device("cuda", 0)
    seed, offset = 20260101, 3 * Np + 5

    def buffers():
        return (torch.full((D * Np,), -7.0, dtype=torch.float64, device=dev),
                torch.full((M * Np,), -7, dtype=torch.int64, device=dev),
                torch.full((Np * M * L,), -7, dtype=torch.int32, device=dev))

    dd = [kdehip.DeviceDensity(t) for t in g]
    try:
        P, I, Lb = buffers()
        kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=Niter, seed=seed, sample_offset=offset, d_labels=Lb)
        torch.cuda.synchronize()
        one = [P.cpu().numpy(), I.cpu().numpy(), Lb.cpu().numpy()]
    finally:
        for d in dd:
            d.close()
    assert one[1].min() >= 1 and one[2].min() >= 0   # (everything was written)
    with kdehip.ProductPlan(g) as plan:
        for variant in (0, 8, 16):
            plan.set_variant(variant)
            for _ in range(2):   # (the second run of a plan with 16 chains or more uses its tables and screen tiles)
                P, I, Lb = buffers()
                plan.sample_philox_device(Np, Niter, seed, offset, True, P, I, Lb)
                torch.cuda.synchronize()
                assert np.array_equal(I.cpu().numpy(), one[1]), variant
                assert np.array_equal(Lb.cpu().numpy(), one[2]), variant
                assert np.array_equal(P.cpu().numpy(), one[0]), variant


def test_batched_launch_of_two_products():
    """two case-A products in one batched call against their single calls: bit for bit"""
    import torch
    D, Ns, (Np,), Niter = CASES["A"]
    M, L = len(Ns), kdehip.nlevels(max(Ns))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(99)
    sets = [_case("A")[2]]
    pts = [synth_mixture(rng, D, N) for N in Ns]
    sets.append([kdehip.kde(p, np.where(silverman_bw(p) > 0, silverman_bw(p), 0.5)) for p in pts])
    dds = [[kdehip.DeviceDensity(t) for t in trees] for trees in sets]

    def buffers():
        return (torch.full((D * Np,), -7.0, dtype=torch.float64, device=dev),
                torch.full((M * Np,), -7, dtype=torch.int64, device=dev),
                torch.full((Np * M * L,), -7, dtype=torch.int32, device=dev))

    try:
        singles, prods = [], []
        for k, dd in enumerate(dds):
            P, I, Lb = buffers()
            kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=Niter, seed=600 + k, sample_offset=7 * k, d_labels=Lb)
            torch.cuda.synchronize()
            singles.append((P.cpu().numpy(), I.cpu().numpy(), Lb.cpu().numpy()))
            P, I, Lb = buffers()
            prods.append(dict(trees=dd, d_points=P, d_indices=I, d_labels=Lb, Np=Np, Niter=Niter, seed=600 + k,
                              sample_offset=7 * k))
        kdehip.prodAppxMSGibbsS_batch(prods)
        torch.cuda.synchronize()
        assert kdehip.batch_launches()["batched"] == 1
        for single, pr in zip(singles, prods):
            assert np.array_equal(pr["d_indices"].cpu().numpy(), single[1])
            assert np.array_equal(pr["d_labels"].cpu().numpy(), single[2])
            assert np.array_equal(pr["d_points"].cpu().numpy(), single[0])
    finally:
        for dd in dds:
            for d in dd:
                d.close()
