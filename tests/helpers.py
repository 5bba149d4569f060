"""Shared helpers for the test-suite (parsing of the reference's MATLAB golden files, synthetic inputs)."""
import numpy as np


def parse_mat_print_kde(path):
    """Mirror of parseMatPrintKDE (reference test/runtests.jl:8-19): `name=[a, b, ...]` lines."""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if "=" not in line:
                continue
            name, rest = line.split("=", 1)
            body = rest.split("[", 1)[1].split("]", 1)[0]
            out[name] = np.array([float(x) for x in body.split(",") if x.strip()])
    return out


def inds_match(ref0, ours1):
    """Index rule of testSubtract/testInds (reference test/runtests.jl:55-68):
    golden is 0-based; ref<0 => ours == -1, else ours == ref+1."""
    ref0 = np.asarray(ref0).astype(np.int64)
    ours1 = np.asarray(ours1).astype(np.int64)
    ok = np.where(ref0 < 0, ours1 + 1 == 0, ref0 + 1 - ours1 == 0)
    return bool(ok.all())


def check_density_against_golden(d, gold, tol):
    """The full testSubtract comparison (reference test/runtests.jl:42-83)."""
    N = d.num_points
    assert int(gold["dims"][0]) == d.dims and int(gold["num_points"][0]) == N
    for name, ours in [("centers", d.centers), ("ranges", d.ranges), ("weights", d.weights),
                       ("means", d.means), ("bandwidth", d.bandwidth), ("bwMin", d.bandwidthMin),
                       ("bwMax", d.bandwidthMax)]:
        n = np.linalg.norm(gold[name] - np.asarray(ours))
        assert n <= tol, (name, n)
    assert inds_match(gold["left_child"], d.left_child)
    assert inds_match(gold["right_child"], d.right_child)
    assert inds_match(gold["lowest_leaf"], d.lowest_leaf)
    assert inds_match(gold["highest_leaf"], d.highest_leaf)
    assert inds_match(gold["permutation"][N:], d.permutation[N:])


def synth_mixture(rng, D, N, ncomp=3, spread=2.0, std=0.5):
    """3-component Gaussian mixture around the origin (SURVEY.md 8(d) recipe, numpy RNG variant)."""
    centres = rng.uniform(-spread, spread, size=(ncomp, D))
    comp = rng.integers(0, ncomp, size=N)
    pts = centres[comp] + std * rng.standard_normal((N, D))
    return np.ascontiguousarray(pts.T)  # D x N


def silverman_bw(pts):
    D, N = pts.shape
    return pts.std(axis=1, ddof=1) * (4.0 / ((D + 2.0) * N)) ** (1.0 / (D + 4.0))


# ---- closed-form streams of the committed Gibbs known-answer fixtures (tests/golden/gibbs_kat_*.npz)
def weyl(n, alpha, offset=0.0):
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.mod(offset + i * alpha, 1.0)


def weyl_normal(n, a1, a2):
    u1 = np.clip(weyl(n, a1, 0.11), 1e-12, 1.0)
    u2 = weyl(n, a2, 0.37)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)



def kat_streams(nU, nN):
    """randU / randN of the KAT fixtures (reference allocation sizes, src/MSGibbs01.jl:661-662)."""
    return weyl(nU, (np.sqrt(5.0) - 1.0) / 2.0, 0.0123), weyl_normal(nN, np.sqrt(7.0) % 1.0, np.sqrt(11.0) % 1.0)


# ---- the split of the all-pairs sums, restated from the comments of csrc/entry_helpers.hpp and csrc/summary.hip -------------
def _ceil_div(a, b):
    return -(-int(a) // int(b))


def device_cus():
    """compute units of cuda:0 as torch reports them (256 on an MI355X in SPX mode)"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def chunks_per_group(N, Nq, cus=None, chunk=128, threads=256, max_groups=64, nprob=1):
    """split_chunks: the ceil(N / 128) source chunks go to `want` groups of consecutive chunks, want = ceil(8 CUs / qblocks)
    clamped to [1, 64] and to the chunk count, qblocks = ceil(Nq / 256) query blocks (times the problems of a batch)"""
    cus = device_cus() if cus is None else cus
    nchunks = _ceil_div(N, chunk)
    qblocks = _ceil_div(Nq, threads) * max(1, nprob)
    want = max(1, min(_ceil_div(8 * cus, qblocks), max_groups, nchunks))
    return _ceil_div(nchunks, want)


def grid_chunks_per_group(N, Ngrid, cus=None):
    """the grid kernel's own split (csrc/summary.hip): 256-leaf chunks, 256 grid points per block, at most 256 groups"""
    return chunks_per_group(N, Ngrid, cus, chunk=256, threads=256, max_groups=256)


def loocv_chunks_per_group(D, N, cus=None, nb=1, chunk=128, threads=256, max_groups=64):
    """the bandwidth search's own split (csrc/loocv.hip LoocvSearch::begin, two-launch rounds): every one of the nm = nb * D
    marginals walks ceil(N / 128) chunks for ceil(N / 256) query blocks; want = ceil(8 CUs / (qblocks * nm)) groups, clamped to
    [1, 64] and to the chunk count"""
    cus = device_cus() if cus is None else cus
    nchunks = _ceil_div(N, chunk)
    qblocks = _ceil_div(N, threads)
    want = max(1, min(_ceil_div(8 * cus, qblocks * nb * D), max_groups, nchunks))
    return _ceil_div(nchunks, want)


def density_arrays(p):
    """(points (D, N), weights (N,), leaf variances (D,)) of a host density with one bandwidth vector, in original point order:
    the form the models of tests/*_model.py take a density in"""
    import kdehip
    N, D = p.bt.num_points, p.bt.dims
    return kdehip.getPoints(p), kdehip.getWeights(p), p.bandwidth[N * D:(N + 1) * D].copy()


def assert_chunks_per_group(N, Nq, want, grid=False):
    """the premise of a large-N case: on this device a group of the sweep walks `want` chunks"""
    cus = device_cus()
    got = grid_chunks_per_group(N, Nq, cus) if grid else chunks_per_group(N, Nq, cus)
    assert got == want, (f"with {cus} compute units the {'grid ' if grid else ''}split gives N = {N}, Nq = {Nq} groups of {got} "
                         f"chunk(s), not the {want} this case is here for: it would cover nothing")


def rescale_premise(pts, w, var, X, cpg, man=None, chunk=128):
    """Per query (column of X): does some group of `cpg` consecutive `chunk`-leaf chunks have BOTH a later
    chunk that raises the group's running maximum of a_i over S = {w_i > 0} by at least log 2 over a non-empty earlier chunk
    (the carried sums are rescaled by at most 1/2) AND a maximum within 30 of the query's overall maximum (the group counts in
    the result).  pts (D, N), w (N,) in LEAF order; var (D,); man: None or one 0 / 1 per dimension."""
    import math
    D, N = pts.shape
    nch = _ceil_div(N, chunk)
    hit = np.zeros(X.shape[1], dtype=bool)
    for q in range(X.shape[1]):
        d = X[:, q:q + 1] - pts
        if man is not None:
            c = np.asarray(man, dtype=bool)
            d[c] = d[c] - 2.0 * math.pi * np.floor((d[c] + math.pi) / (2.0 * math.pi))
        a = np.where(w > 0.0, -0.5 * np.sum(d * d / np.asarray(var)[:, None], axis=0), -np.inf)
        cmax = np.array([a[c * chunk:(c + 1) * chunk].max() for c in range(nch)])
        M = cmax.max()
        ok = False
        for g0 in range(0, nch, cpg):
            run = -np.inf
            fired = False
            for cm in cmax[g0:g0 + cpg]:
                if run > -np.inf and cm >= run + math.log(2.0):
                    fired = True
                run = max(run, cm)
            if fired and run >= M - 30.0:
                ok = True
                break
        hit[q] = ok
    return hit
