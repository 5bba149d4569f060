"""The fp32 screen's row loop (csrc/screen_device.hpp screen_rows) at every length of its pipeline's tail.

On shared-bandwidth tiles of more than 4 dimensions the loop keeps two row pairs in flight ahead of the one it evaluates
(three pairs per trip), elsewhere one (two per trip); a request past the last pair reads the last pair again, never past
the tile.  The cases below put screened levels with 1, 2, 3, 4, 5, 8 and 16 pairs per lane in front of it on
shared-bandwidth tiles, every remainder of both trip lengths, and with 2, 4 and 8 on per-node tiles (a per-node level of
65 .. 128 or 257 .. 384 nodes is never large enough to be streamed, which is what makes a level screened, so 1 and 3 do
not occur there at 4 densities).  A short density beside long ones does it: a level is screened when the M fp64 tiles
together exceed the LDS pool, whatever the size of each.  One case is weighted; one has a winning block of 32 rows.
Every case must give the unscreened run (plan variant 5; the general kernel for 8 densities) bit for bit and the oracle's
labels; the statistics show that the screen ran on every draw of the screened levels.  The inputs were checked on the CPU
to hold no duplicate points and the uniforms no repeated or zero value, so no draw sits on an exact tie."""
import numpy as np
import pytest

import kdehip
from oracle import oracle
from tests.helpers import silverman_bw, synth_mixture

pytestmark = pytest.mark.gpu

# (D, sizes, chains, Niter, weighted, screened levels, pairs per lane the short densities put on the screened levels)
CASES = [
    (6, [600, 1000, 1000, 1000], 64, 2, False, 2, "leaves 600: 5 pairs; 512 nodes: 4 (per-node); leaves 1000: 8"),
    (6, [330, 1000, 1000, 1000], 64, 2, False, 2, "256 nodes: 2 (per-node); leaves 330: 3"),
    (6, [128, 1000, 1000, 1000], 64, 2, False, 2, "leaves 128: 1"),
    (6, [200, 1000, 1000, 1000], 64, 2, False, 2, "leaves 200: 2"),
    (6, [330, 600, 1000, 1000], 96, 3, True, 2, "weighted: 3, 5 and 8 pairs at the leaves, 2 and 4 per-node"),
    (6, [2048, 1000, 1000, 1000], 64, 2, False, 4, "1024 nodes: 8 (per-node); leaves 2048: 16 pairs, a winning block of 32 rows"),
    (8, [300] * 4, 64, 2, False, None, "D = 8: 256 nodes: 2 (per-node)"),
    (3, [330, 520] + [700] * 6, 64, 2, False, None, "8 densities: leaves 330: 3; leaves 520: 5; 512 nodes: 4 (per-node)"),
]


def _trees(seed, D, Ns, weighted):
    rng = np.random.default_rng(seed)
    g, o = [], []
    for N in Ns:
        pts = synth_mixture(rng, D, N)
        ks = silverman_bw(pts)
        w = rng.uniform(0.2, 1.0, size=N) if weighted else None
        g.append(kdehip.kde(pts, ks, w))
        o.append(oracle.OracleDensity(pts, ks, w))
    return g, o


@pytest.mark.parametrize("D,Ns,Np,Niter,weighted,levels,what", CASES)
def test_every_tail_of_the_row_loop(D, Ns, Np, Niter, weighted, levels, what):
    g, o = _trees(9100 + D + sum(Ns), D, Ns, weighted)
    seed = 2718
    with kdehip.ProductPlan(g) as plan:
        assert plan.fast_math_path
        # (8 densities: the unscreened twin is the general kernel, variant 38; both launch geometries of the lean kernel)
        runs, ref_variant = ((8, 16), 38) if len(Ns) == 8 else ((0,), 5)
        res = {}
        for v in runs:
            plan.set_variant(v)
            res[v] = plan.sample(Np, Niter=Niter, seed=seed, want_labels=True)
        st = plan.screen_stats()
        plan.set_variant(ref_variant)
        ref = plan.sample(Np, Niter=Niter, seed=seed, want_labels=True)
        assert plan.screen_stats()["steps"] == st["steps"]  # (the twin draws nothing through the screen)
        K, R = plan.randu_per_sample(Niter), plan.randn_per_sample()
    print(f"\n{D=} {Ns=} {st=} ({what})")
    assert st["levels"] >= 1 and st["steps"] > 0, st
    if levels is not None:
        assert st["levels"] == levels, st
    assert st["steps"] == len(runs) * Np * len(Ns) * (Niter + 1) * st["levels"], st
    for v in runs:
        for a, b in zip(res[v], ref):
            assert np.array_equal(a, b), (v, what)
    u, n = kdehip.philox_streams(seed, 0, Np, K, R)
    op, oi, ol = oracle.gibbs1(o, Np, Niter, u, n, want_labels=True)
    pts, ind, lab = res[runs[0]]
    print(f"max |points - oracle| = {np.abs(pts - op).max():.3g}, bit-equal: {np.array_equal(pts, op)}")
    assert np.array_equal(ind, oi) and np.array_equal(lab, ol), what
    assert np.allclose(pts, op, rtol=1e-11, atol=1e-11), what
