"""Shared data of the circular plan / batch / multi-GPU tests: densities whose circular dimensions STRADDLE the cut (two
clusters at +3.0 and -3.0, bandwidth 0.3 -- about 0.28 apart on the circle, 6 apart on the line), so that differences wrap
and the Euclidean code cannot pass; and the comparison rule of tests/test_gpu_circular_resident.py (labels identical,
points within 1e-12, circular dimensions compared on the circle)."""
import numpy as np

ATOL = 1e-12


def wrap(t):
    return t - 2.0 * np.pi * np.floor((t + np.pi) / (2.0 * np.pi))


def cut_points(rng, D, n, circ):
    p = rng.standard_normal((D, n)) * 0.7
    for d in range(D):
        if circ[d]:
            side = np.where(rng.random(n) < 0.5, 3.0, -3.0)
            p[d] = wrap(side + 0.3 * rng.standard_normal(n))
    return p


def cut_bandwidths(rng, D, circ):
    return np.array([0.3 if circ[d] else rng.uniform(0.15, 0.5) for d in range(D)])


def cut_trees(seed, D, Ns, circ):
    """(kdehip host densities, oracle densities) of len(Ns) densities on the manifold `circ`"""
    import kdehip
    from oracle import oracle
    rng = np.random.default_rng(seed)
    g, o = [], []
    for n in Ns:
        p = cut_points(rng, D, n, circ)
        ks = cut_bandwidths(rng, D, circ)
        w = rng.uniform(0.3, 1.0, n)
        g.append(kdehip.kde(p, ks, w))
        o.append(oracle.OracleDensity(p, ks, w))
    return g, o


def refused_trees(seed, D, Ns, circ):
    """A density set the fast forms refuse (the construction of tests/test_gpu_circular_resident.py's generic-fallback case):
    one variance of 1e-320 at the root of the first density takes the variance products out of range."""
    import kdehip
    from oracle import oracle
    rng = np.random.default_rng(seed)
    g, o = [], []
    for k, n in enumerate(Ns):
        p = cut_points(rng, D, n, circ)
        t = kdehip.kde(p, cut_bandwidths(rng, D, circ))
        if k == 0:
            t.bandwidth[0] = 1e-320   # (flat [node * D + d]: dimension 0 of the root -- read at level 0 only)
        g.append(t)
        o.append(oracle.OracleDensity.from_arrays(D, n, t.means, t.bandwidth, t.bt.weights, t.bt.left_child, t.bt.right_child,
                                                  t.bt.permutation))
    return g, o


def assert_points(gp, op, circ, why):
    for d in range(gp.shape[0]):
        diff = gp[d] - op[d]
        if circ[d]:
            diff = wrap(diff)
        err = float(np.abs(diff).max())
        print(f"{why}: dimension {d} ({'circular' if circ[d] else 'euclid'}) max error {err:.3e}")
        assert err <= ATOL, (why, d, err)


def oracle_run(o, Ns, D, Np, Niter, circ, seed, *, addEntropy=True, mask=None, sample_offset=0):
    """okde_gibbs1_manifold on the host twin of the Philox streams of (seed, sample_offset): (points, indices, labels)"""
    import kdehip
    from oracle import oracle
    K, R, _, _ = oracle.rng_sizes(len(Ns), D, Np, Niter, Ns)
    randU, randN = kdehip.philox_streams(seed, sample_offset, Np, K, R)
    return oracle.gibbs1(o, Np, Niter, randU, randN, addEntropy=addEntropy, partialDimMask=mask, manifold=circ,
                         want_labels=True)
