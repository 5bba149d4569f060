"""NumPy restatement of the refit of a ball-tree density (include/kdehip.h section 5r), written from the reference:
`calcStatsBall!` / `getMiniMaxi` (src/BallTree01.jl:249-336), `calcStatsDensity!` (src/BallTreeDensity01.jl:141-187) and the
loops of `changeWeights!` / `movePoints!` (src/BallTreeDensity01.jl:278-309) -- new leaf values through the permutation, then
every internal node from its two children, children first; the child arrays are GIVEN and stay.  Plain Python floats: IEEE
doubles, one rounding per operation, no fused multiply-add -- so the model can be compared bit for bit.

Two things differ from the reference's text on purpose, as the header says: the move is added to a leaf's centre AND mean
(the reference moves the centres only, and its leaf means go stale), and slot N -- which is no node -- is left alone (the
reference's loop `for i in num_points:-1:1` visits it)."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
TWO_PI, PI = 6.283185307179586476925286766559, 3.141592653589793238462643383279


def wrap(t):
    """to [-pi, pi): the library's one expression for a circular dimension"""
    return t - TWO_PI * math.floor((t + PI) / TWO_PI)


def arrays_of(bd):
    """the twelve arrays of a BallTreeDensity as a dict of copies"""
    bt = bd.bt
    return {"centers": bt.centers.copy(), "ranges": bt.ranges.copy(), "weights": bt.weights.copy(),
            "left_child": bt.left_child.copy(), "right_child": bt.right_child.copy(), "lowest_leaf": bt.lowest_leaf.copy(),
            "highest_leaf": bt.highest_leaf.copy(), "permutation": bt.permutation.copy(), "means": bd.means.copy(),
            "bandwidth": bd.bandwidth.copy(), "bandwidthMin": bd.bandwidthMin.copy(), "bandwidthMax": bd.bandwidthMax.copy()}


FIELDS = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation", "means",
          "bandwidth", "bandwidthMin", "bandwidthMax")


def same_bits(got, want, what=""):
    """all twelve arrays of two densities (a BallTreeDensity or a dict of arrays each), byte for byte"""
    g = got if isinstance(got, dict) else arrays_of(got)
    w = want if isinstance(want, dict) else arrays_of(want)
    for f in FIELDS:
        assert g[f].dtype == w[f].dtype and g[f].shape == w[f].shape, (what, f)
        assert g[f].tobytes() == w[f].tobytes(), (what, f)


def calc_stats(a, D, N, root, circ, varbw):
    """calcStatsDensity!(bd, root) on the dict of arrays `a` (1-based node ids)"""
    left, right = int(a["left_child"][root - 1]), int(a["right_child"][root - 1])
    if N == 1 and root == 1:
        right = left  # buildBall! summarises a single leaf with itself and sets NO_CHILD afterwards (BallTree01.jl:351-362)
    if not (0 < left <= 2 * N) or not (0 < right <= 2 * N):  # validIndex
        return
    c, r, w, mu, v = a["centers"], a["ranges"], a["weights"], a["means"], a["bandwidth"]
    Ni, NiL, NiR = D * (root - 1), D * (left - 1), D * (right - 1)
    for d in range(D):
        cl, rl, cr, rr = float(c[NiL + d]), float(r[NiL + d]), float(c[NiR + d]), float(r[NiR + d])
        if circ is not None and circ[d]:
            add, diff = (lambda x, y: wrap(x + y)), (lambda x, y: wrap(x - y))
        else:
            add, diff = (lambda x, y: x + y), (lambda x, y: x - y)
        up_l, up_r = add(cl, rl), add(cr, rr)      # getMiniMaxi
        maxi = up_l if up_l > up_r else up_r
        dn_l, dn_r = diff(cl, rl), diff(cr, rr)
        mini = dn_l if dn_l < dn_r else dn_r
        half = diff(maxi, mini) / 2.0
        r[Ni + d] = half
        c[Ni + d] = add(mini, half)
    wl, wr = float(w[left - 1]), float(w[right - 1])
    w[root - 1] = wl + wr if left != right else wl
    wt = wl + wr + EPS
    wl /= wt
    wr /= wt
    if varbw:
        mn, mx = a["bandwidthMin"], a["bandwidthMax"]
        for d in range(D):
            mx[Ni + d] = mx[NiL + d] if mx[NiL + d] > mx[NiR + d] else mx[NiR + d]
            mn[Ni + d] = mn[NiL + d] if mn[NiL + d] < mn[NiR + d] else mn[NiR + d]
    for d in range(D):
        ml, mr = float(mu[NiL + d]), float(mu[NiR + d])
        m = wl * ml + wr * mr
        mu[Ni + d] = m
        v[Ni + d] = wl * (float(v[NiL + d]) + ml * ml) + wr * (float(v[NiR + d]) + mr * mr) - m * m


def refit(arrays, D, N, new_weights=None, delta=None, circ=None, varbw=False):
    """The refitted twelve arrays (a new dict).  new_weights: N values by ORIGINAL point; delta: (D, N) by original point;
    circ: D booleans (the tree's operators) or None."""
    a = {k: np.array(v, copy=True) for k, v in arrays.items()}
    perm = a["permutation"]
    for leaf in range(N + 1, 2 * N + 1):
        src = int(perm[leaf - 1]) - 1  # getIndexOf
        if new_weights is not None:
            a["weights"][leaf - 1] = new_weights[src]
        if delta is not None:
            for d in range(D):
                for name in ("centers", "means"):
                    x = float(a[name][D * (leaf - 1) + d]) + float(delta[d, src])
                    a[name][D * (leaf - 1) + d] = wrap(x) if circ is not None and circ[d] else x
    # children first: the builder hands out ids parent before child (left subtree, then right), so descending ids do --
    # which is the order of the reference's loops
    for root in range(max(N - 1, 1), 0, -1):
        calc_stats(a, D, N, root, circ, varbw)
    return a
