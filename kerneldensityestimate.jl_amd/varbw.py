"""Densities whose points each have a bandwidth of their own, and the two classical rules that choose one: `kde_varbw`,
`adaptive_scales`, `kde_adaptive` (include/kdehip.h sections 4 and 5o; builder in csrc/balltree.cpp, kernels in
csrc/varbw.hip).

The reference's layout allows such densities (`bandwidth` is D x 2N, `multibandwidth = 1`, src/BallTreeDensity01.jl:11-24)
but `kde!` never builds one.  A belief with one tight mode and a wide tail cannot be fitted with one bandwidth: it smears
the mode or leaves holes in the tail.  The sample-point adaptive estimator gives point i the bandwidth `h * lambda_i`, with
`lambda_i` small where the data are dense:

  Abramson     lambda_i proportional to p~(x_i)^-alpha, p~ a fixed-bandwidth pilot (alpha = 1/2 is Abramson's square-root law)
  k-th neighbour   lambda_i proportional to the distance from x_i to its k-th neighbour, measured in the pilot's bandwidths

both normalised to weighted geometric mean 1, so that `h` keeps its meaning.

What reads a per-point density: `evaluateDualTree` / `bd(pos)`, `evaluate_log`, `evalAvgLogL`, `entropy`, `kld`, `minkld` (and
`DeviceDensity.evaluate` / `.evaluate_log`), `sample`, products (the sampler packs non-uniform tiles), `kernel_sum` with
explicit variances, `knn` with the Euclidean or an explicit metric, `marginal` of a host density, `getBW`.  Not here:
`evaluate_tol`, gradients, Hessians and modes, `condition`, `box_mass` and quantiles, `kernel_sum(var=None)`,
`knn(metric="bandwidth")`, resident `marginal` / `condition`, choosing alpha or k by cross-validation.
"""
from __future__ import annotations

import numpy as np

from . import _lib, manifold as _mf
from ._lib import f64p, i64p, optr, ptr
from .density import BallTreeDensity, _empty_density, getBW, getPoints, getWeights, kde


def kde_varbw(points, bw, weights=None, tree_manifold=None) -> BallTreeDensity:
    """A density with a bandwidth per point (kdehip_make_density_varbw): points (D, N) or a length-N vector; bw (D, N)
    STANDARD DEVIATIONS, column i being point i's (a length-N vector for 1-D data); weights N values, normalised to sum 1.
    The tree, boxes, weights and means are `kde`'s -- they do not depend on the bandwidth --, `multibandwidth` is 1 and
    bandwidthMin / Max hold the extreme variances below every node.  tree_manifold as in `kde`."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts.reshape(1, -1)
    if pts.ndim != 2:
        raise ValueError("points must be a (D, N) matrix or a vector")
    D, N = pts.shape
    b = np.asarray(bw, dtype=np.float64)
    if b.ndim == 1 and D == 1:
        b = b.reshape(1, -1)
    if b.shape != (D, N):
        raise ValueError("kde_varbw: bw must be (D, N), one column of standard deviations per point")
    if not np.all(np.isfinite(b) & (b > 0.0)):
        raise ValueError("kde_varbw: every bandwidth must be finite and > 0")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())
        if w.size != N:
            raise ValueError("weights must have one entry per point")
    flat = np.ascontiguousarray(pts.T).ravel()  # column-major D x N
    bflat = np.ascontiguousarray(b.T).ravel()
    tman = _mf.parse(tree_manifold, D)
    bd = _empty_density(D, N, multibw=True)
    bt = bd.bt
    _lib.check(_lib.lib.kdehip_make_density_varbw(
        D, N, ptr(flat, f64p), ptr(bflat, f64p), optr(w, f64p),
        ptr(bt.centers, f64p), ptr(bt.ranges, f64p), ptr(bt.weights, f64p), ptr(bt.left_child, i64p),
        ptr(bt.right_child, i64p), ptr(bt.lowest_leaf, i64p), ptr(bt.highest_leaf, i64p),
        ptr(bt.permutation, i64p), ptr(bd.means, f64p), ptr(bd.bandwidth, f64p),
        ptr(bd.bandwidthMin, f64p), ptr(bd.bandwidthMax, f64p), _mf.pointer(tman)))
    bd.tree_manifold = tman
    return bd


def adaptive_scales(p, method="abramson", alpha=0.5, k=8, device=0, manifold=None):
    """The per-point scale factors lambda (N,), in original point order, of a uniform-bandwidth pilot `p`; their weighted
    geometric mean is 1 (sum_i w_i log lambda_i = 0).
      method="abramson":  log lambda_i = -alpha (lp_i - sum_j w_j lp_j), lp = evaluate_log(p, getPoints(p)) -- the pilot at
                          its own points WITH the self term, so no lp is -inf.  0 <= alpha <= 1.
      method="knn":       lambda_i proportional to the distance from point i to its k-th neighbour (itself left out) in the
                          bandwidth metric, knn(p, k=k, lvFlag=True, metric="bandwidth").  1 <= k <= 32.  A zero distance --
                          k + 1 coincident points -- has no scale: ValueError, with their number."""
    from .bandwidth import evaluate_log
    from .knn import knn
    if not isinstance(p, BallTreeDensity):
        raise TypeError("adaptive_scales: the pilot is a BallTreeDensity")
    if method not in ("abramson", "knn"):
        raise ValueError('adaptive_scales: method is "abramson" or "knn"')
    w = getWeights(p)
    if method == "abramson":
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("adaptive_scales: alpha must lie in [0, 1]")
        lp = evaluate_log(p, getPoints(p), manifold=manifold, device=device)
        return np.exp(-alpha * (lp - np.sum(w * lp)))
    k = int(k)
    if not 1 <= k <= 32:
        raise ValueError("adaptive_scales: k must lie in 1..32")
    dist, _ = knn(p, k=k, lvFlag=True, metric="bandwidth", manifold=manifold, device=device)
    dk = dist[k - 1]
    nzero = int(np.count_nonzero(dk == 0.0))
    if nzero:
        raise ValueError(f"adaptive_scales: {nzero} points have a k-th neighbour at distance 0 (duplicated points): "
                         "no scale can be taken from it")
    ld = np.log(dk)
    return np.exp(ld - np.sum(w * ld))


def kde_adaptive(points, ks=None, weights=None, *, method="abramson", alpha=0.5, k=8, device=0, manifold=None,
                 tree_manifold=None) -> BallTreeDensity:
    """The sample-point adaptive estimator: the pilot `kde(points, ks, weights)` (the LOOCV bandwidth when ks is None), its
    `adaptive_scales`, then `kde_varbw(points, outer(sd, lambda), weights)` with sd the pilot's bandwidth.  `manifold`: the
    pilot's search (ks None only) and the scale rule's differences; `tree_manifold`: both trees' operators.
    Products of per-point densities run on the sampler's non-uniform tiles, which is checked against the CPU oracle in
    tests/test_gpu_varbw.py."""
    if ks is None:
        pilot = kde(points, None, weights, device=device, manifold=manifold, tree_manifold=tree_manifold)
    else:
        pilot = kde(points, ks, weights, tree_manifold=tree_manifold)
    lam = adaptive_scales(pilot, method=method, alpha=alpha, k=k, device=device, manifold=manifold)
    sd = getBW(pilot)[:, 0]
    return kde_varbw(points, np.outer(sd, lam), weights, tree_manifold=tree_manifold)
