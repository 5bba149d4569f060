"""The reference's tree construction with its operators as CALLABLES (test infrastructure only).

`kde!(points, ks, weights, addop, diffop)` (KDE01.jl:34-57) -> makeBallTreeDensity -> buildTree! -> buildBall! threads one
`addop` / `diffop` per dimension through exactly three functions: most_spread_coord (BallTree01.jl:142-173), select!
(:223-242) and getMiniMaxi / calcStatsBall! (:249-336).  calcStatsDensity! (BallTreeDensity01.jl:156-185) takes none.  This
file restates those functions with the operators as arguments, in the style of tests/pymodel.py (1-based lists, the
reference's names and loop structure), and shares pymodel's container, `swapDensity`, `_idx` and `wrapRad`.  With the
Euclidean callables it must equal `pymodel.kde` on every array (tests/test_tree_manifold_host.py pins that); with
`circ_add` / `circ_diff` it is what kdehip_make_density_tree must produce bit for bit.
"""
import numpy as np

from tests import pymodel
from tests.pymodel import _idx, swapDensity, validIndex

NO_CHILD = pymodel.NO_CHILD
EPS = pymodel.EPS


def euclid_add(a, b):
    return a + b


def euclid_diff(a, b):
    return a - b


circ_add = pymodel.circ_add    # wrapRad(a + b)
circ_diff = pymodel.circ_diff  # wrapRad(a - b)


def operators(manifold, D):
    """(addop, diffop): one callable per dimension (index 0 unused) from None or a sequence of 0 / 1"""
    man = [0] * D if manifold is None else [int(m) for m in manifold]
    assert len(man) == D
    return ([None] + [circ_add if m else euclid_add for m in man], [None] + [circ_diff if m else euclid_diff for m in man])


def most_spread_coord(bt, low, high, addop, diffop):  # :142-173
    max_variance = 0
    max_dim = 1
    w = 1.0 / (high - low)
    for dimension in range(1, bt.dims + 1):
        mean = 0
        # (dims*(low-1) + dimension):dims:(dims*(high-1))  -- the last leaf is never reached
        pts = range(bt.dims * (low - 1) + dimension, bt.dims * (high - 1) + 1, bt.dims)
        for p in pts:
            mean = addop[dimension](mean, w * bt.centers[p])
        variance = 0
        for p in pts:
            d = diffop[dimension](bt.centers[p], mean)
            variance += d * d
        if variance > max_variance:
            max_variance = variance
            max_dim = dimension
    return max_dim


def select(bd, dimension, position, low, high, diffop):  # :223-242
    while low < high:
        r = (low + high) // 2
        swapDensity(bd, r, low)
        m = low
        for i in range(low, high + 1):
            if diffop[dimension](bd.centers[dimension + bd.dims * (i - 1)], bd.centers[dimension + bd.dims * (low - 1)]) < 0.0:
                m += 1
                swapDensity(bd, m, i)
        swapDensity(bd, low, m)
        if m <= position:
            low = m + 1
        if m >= position:
            high = m - 1


def getMiniMaxi(bt, leftI, rightI, d, addop, diffop):  # :249-278
    D = bt.dims
    cL, rL = bt.centers[_idx(leftI, D, d)], bt.ranges[_idx(leftI, D, d)]
    cR, rR = bt.centers[_idx(rightI, D, d)], bt.ranges[_idx(rightI, D, d)]
    a = addop[d](cL, rL)
    b = addop[d](cR, rR)
    maxi = addop[d](cL, rL) if a > b else addop[d](cR, rR)
    c = diffop[d](cL, rL)
    c2 = diffop[d](cR, rR)
    mini = diffop[d](cL, rL) if c < c2 else diffop[d](cR, rR)
    return mini, maxi


def calcStats(bd, root, addop, diffop):  # calcStatsBall! :282-336 (operators), then calcStatsDensity! BallTreeDensity01.jl:141-187 (none)
    leftI, rightI = bd.left_child[root], bd.right_child[root]
    if not validIndex(bd, leftI) or not validIndex(bd, rightI):
        return
    D = bd.dims
    for d in range(1, D + 1):
        mini, maxi = getMiniMaxi(bd, leftI, rightI, d, addop, diffop)
        halfspan = diffop[d](maxi, mini) / 2.0
        bd.ranges[_idx(root, D, d)] = halfspan
        bd.centers[_idx(root, D, d)] = addop[d](mini, halfspan)
    if leftI != rightI:
        bd.weights[root] = bd.weights[leftI] + bd.weights[rightI]
    else:
        bd.weights[root] = bd.weights[leftI]
    Ni, NiL, NiR = D * (root - 1), D * (leftI - 1), D * (rightI - 1)
    wtL, wtR = bd.weights[leftI], bd.weights[rightI]
    wtT = wtL + wtR + EPS
    wtL /= wtT
    wtR /= wtT
    for k in range(1, D + 1):
        bd.means[Ni + k] = wtL * bd.means[NiL + k] + wtR * bd.means[NiR + k]
        bd.bandwidth[Ni + k] = (wtL * (bd.bandwidth[NiL + k] + bd.means[NiL + k] * bd.means[NiL + k]) +
                                wtR * (bd.bandwidth[NiR + k] + bd.means[NiR + k] * bd.means[NiR + k]) -
                                bd.means[Ni + k] * bd.means[Ni + k])


def buildBall(bd, low, high, root, addop, diffop):  # :342-411
    if low == high:
        bd.lowest_leaf[root] = low
        bd.highest_leaf[root] = high
        bd.left_child[root] = low
        bd.right_child[root] = high
        calcStats(bd, root, addop, diffop)
        bd.right_child[root] = NO_CHILD
        return
    coord = most_spread_coord(bd, low, high, addop, diffop)
    split = (low + high) // 2
    select(bd, coord, split, low, high, diffop)
    if split <= low:
        left = low
    else:
        left = bd.next
        bd.next += 1
    if split + 1 >= high:
        right = high
    else:
        right = bd.next
        bd.next += 1
    bd.lowest_leaf[root] = low
    bd.highest_leaf[root] = high
    bd.left_child[root] = left
    bd.right_child[root] = right
    if left != low:
        buildBall(bd, low, split, left, addop, diffop)
    if right != high:
        buildBall(bd, split + 1, high, right, addop, diffop)
    calcStats(bd, root, addop, diffop)


def kde(points, ks, weights=None, manifold=None):
    """kde!(points, ks, weights, addop, diffop) KDE01.jl:34-57 -> makeBallTreeDensity BallTreeDensity01.jl:192-231:
    points = list of N points of D floats; manifold = None or D values 0 / 1.  Arrays allocated and leaves initialised as
    pymodel.kde does (1-based lists in a pymodel.BT), then buildBall! with the operators."""
    N, D = len(points), len(points[0])
    addop, diffop = operators(manifold, D)
    if len(ks) == 1:
        ks = list(ks) * D
    ks = [k * k for k in ks]
    if weights is None:
        weights = [1.0] * N
    sw = 0.0
    for x in weights:
        sw += x
    weights = [x / sw for x in weights]
    bd = pymodel.BT()
    bd.dims, bd.num_points = D, N
    z = lambda n, v=0.0: [None] + [v] * n  # noqa: E731  (1-based array)
    bd.centers, bd.ranges, bd.means, bd.bandwidth = z(2 * N * D), z(2 * N * D), z(2 * N * D), z(2 * N * D)
    bd.weights = z(2 * N)
    bd.left_child, bd.right_child = z(2 * N, 1), z(2 * N, 1)
    bd.lowest_leaf, bd.highest_leaf = z(2 * N, 1), z(2 * N, 1)
    bd.permutation = z(2 * N, 0)
    for i in range(N):
        for k in range(D):
            bd.centers[N * D + i * D + k + 1] = points[i][k]
            bd.means[N * D + i * D + k + 1] = points[i][k]
            bd.bandwidth[N * D + i * D + k + 1] = ks[k]
        bd.weights[N + i + 1] = weights[i]
    # buildTree! BallTree01.jl:415-434
    i = N
    for j in range(1, N + 1):
        for k in range(1, D + 1):
            bd.ranges[i * D + k] = 0
        i += 1
        bd.lowest_leaf[i] = i
        bd.highest_leaf[i] = i
        bd.left_child[i] = i
        bd.right_child[i] = NO_CHILD
        bd.permutation[i] = j
    bd.next = 2
    buildBall(bd, N + 1, 2 * N, 1, addop, diffop)
    return bd


INT_FIELDS = ("left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
FLOAT_FIELDS = ("centers", "ranges", "weights", "means", "bandwidth")


def arrays(bd):
    """the model's ten node arrays 0-based, as numpy, under the names BallTree / BallTreeDensity give them, plus
    bandwidthMin / bandwidthMax (BallTreeDensity01.jl:215-223: the leaf variances, one row per point)"""
    N, D = bd.num_points, bd.dims
    out = {f: np.array(getattr(bd, f)[1:], dtype=np.float64) for f in FLOAT_FIELDS}
    out.update({f: np.array(getattr(bd, f)[1:], dtype=np.int64) for f in INT_FIELDS})
    leaf = out["bandwidth"][N * D:N * D + D]
    out["bandwidthMin"] = np.tile(leaf, N)
    out["bandwidthMax"] = np.tile(leaf, N)
    return out


# ---- the data of tests/test_tree_manifold_host.py and tests/test_gpu_tree_manifold.py ------------------------------------
KINDS = ("straddle", "uniform", "ties", "outside", "constant")


def tree_case(kind, seed, D, N, manifold, weighted=False, nks=1):
    """(points (D, N), ks, weights or None).  A circular dimension holds the kind's angles -- straddle: N(pi, 0.4) wrapped
    (a cluster across the cut); uniform: [-pi, pi); ties: {-pi, -pi/2, 0, pi/2} (a difference of exactly pi wraps to -pi and
    counts as "less"); outside: representatives in [0, 4 pi); constant: one value; unit: [-1, 1] (no hooked expression
    leaves [-pi, pi)) --, a Euclidean one N(0, 1.5) (constant / unit: as the circular ones)."""
    rng = np.random.default_rng(seed)
    pts = np.empty((D, N))
    for d in range(D):
        if kind == "constant":
            pts[d] = 2.5 - d
        elif kind == "unit":
            pts[d] = rng.uniform(-1.0, 1.0, N)
        elif not manifold[d]:
            pts[d] = 1.5 * rng.standard_normal(N)
        elif kind == "straddle":
            pts[d] = [pymodel.wrapRad(float(t)) for t in np.pi + 0.4 * rng.standard_normal(N)]
        elif kind == "uniform":
            pts[d] = rng.uniform(-np.pi, np.pi, N)
        elif kind == "ties":
            pts[d] = rng.choice([-np.pi, -np.pi / 2, 0.0, np.pi / 2], N)
        elif kind == "outside":
            pts[d] = rng.uniform(0.0, 4.0 * np.pi, N)
        else:
            raise ValueError(kind)
    ks = rng.uniform(0.1, 0.6, nks)
    w = rng.uniform(0.2, 2.0, N) if weighted else None
    return pts, ks, w


def model_arrays(pts, ks, w, manifold):
    return arrays(kde([list(pts[:, i]) for i in range(pts.shape[1])], list(ks), None if w is None else list(w), manifold))


ALL_FIELDS = FLOAT_FIELDS + INT_FIELDS + ("bandwidthMin", "bandwidthMax")


def density_arrays(bd):
    """the twelve arrays of a kdehip BallTreeDensity / an oracle.OracleDensity under the same names"""
    src = getattr(bd, "bt", bd)
    out = {f: np.asarray(getattr(src, f)) for f in ("centers", "ranges", "weights") + INT_FIELDS}
    out.update({f: np.asarray(getattr(bd, f)) for f in ("means", "bandwidth", "bandwidthMin", "bandwidthMax")})
    return out


def differing(a, b):
    """names of the arrays that are not the same bits"""
    return [f for f in ALL_FIELDS if a[f].dtype != b[f].dtype or a[f].shape != b[f].shape or a[f].tobytes() != b[f].tobytes()]
