"""Tree construction on a manifold (include/kdehip.h section 4), host builder, without a GPU: the model of
tests/manifold_tree_model.py (the reference's buildBall! chain with its operators as callables) pinned against
tests/pymodel.py and the oracle with Euclidean callables; kdehip_make_density_tree against the model, all twelve arrays bit
for bit; the identity cases; that the feature changes the tree of a density across the cut; the argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import f64p, i64p, ptr, u8p
from oracle import oracle
from tests import manifold_tree_model as tm
from tests import pymodel

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_make_density_tree", "kdehip_make_densities_device_tree", "kdehip_make_density_auto_tree",
       "kdehip_density_from_device_points_tree", "kdehip_mul_device_tree", "kdehip_mul_device_batch_tree"]
MIXED = {1: [[1]], 2: [[0, 1], [1, 1]], 3: [[1, 0, 1], [0, 1, 1]]}


def test_the_library_exports_the_new_entries():
    for name in NEW:
        assert hasattr(_lib.lib, name), name


@pytest.mark.parametrize("N", [2, 3, 5, 33, 64, 65, 200])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_model_with_euclidean_callables_is_pymodel_and_the_oracle(D, N):
    pts, ks, w = tm.tree_case("straddle", 7 * N + D, D, N, [1] * D, weighted=(N + D) % 2 == 0, nks=D if N % 2 else 1)
    cols = [list(pts[:, i]) for i in range(N)]
    ref = tm.arrays(pymodel.kde(cols, list(ks), None if w is None else list(w)))
    orc = tm.density_arrays(oracle.OracleDensity(pts, ks, w))
    for man in (None, [0] * D):
        mine = tm.model_arrays(pts, ks, w, man)
        assert tm.differing(mine, ref) == []
        assert tm.differing(mine, orc) == []


def _host_cases():
    """Every N with every data kind; D, the mask, the weighting and the bandwidth count rotate along that grid (a diagonal
    of the full cross product, not the product itself).  A second pass over the small sizes takes the OTHER weighting and
    the OTHER bandwidth count of each of its cases, and the next D."""
    out = []
    for second in (False, True):
        for n, N in enumerate([1, 2, 3, 5, 33, 64, 65, 200, 600]):
            if second and N > 65:
                continue
            for k, kind in enumerate(tm.KINDS):
                D = 1 + (n + k + second) % 3
                man = MIXED[D][(n + k // 3) % len(MIXED[D])]
                weighted = ((n + k) % 2 == 1) != second
                many = ((n + 2 * k) % 3 == 0) != second
                out.append(pytest.param(kind, D, N, man, weighted, D if many else 1,
                                        id=f"{kind}-D{D}-N{N}-{''.join('ec'[m] for m in man)}-{'w' if weighted else 'u'}{'D' if many else '1'}"))
    return out


@pytest.mark.parametrize("kind,D,N,man,weighted,nks", _host_cases())
def test_host_builder_is_the_model(kind, D, N, man, weighted, nks):
    """600 leaves cross the 512-leaf split of the pooled builder: the model is sequential, so equality there also says the
    arrays do not depend on the number of threads"""
    pts, ks, w = tm.tree_case(kind, 1000 + 31 * N + D, D, N, man, weighted, nks)
    got = kdehip.kde(pts, ks, w, tree_manifold=man)
    assert list(got.tree_manifold) == man
    assert tm.differing(tm.density_arrays(got), tm.model_arrays(pts, ks, w, man)) == []


@pytest.mark.parametrize("D,N", [(1, 33), (2, 200), (3, 600)])
def test_data_inside_the_unit_box_builds_the_euclidean_tree(D, N):
    pts, ks, w = tm.tree_case("unit", 5 + N, D, N, [1] * D, weighted=True, nks=D)
    assert tm.differing(tm.density_arrays(kdehip.kde(pts, ks, w, tree_manifold=[1] * D)), tm.density_arrays(kdehip.kde(pts, ks, w))) == []


def _raw_build(fn, D, N, flat, ks, w, *tail):
    bd = kdehip.density._empty_density(D, N)
    for a in tm.density_arrays(bd).values():
        a[...] = 77
    bt = bd.bt
    rc = fn(D, N, ptr(flat, f64p), ptr(ks, f64p), ks.size, None if w is None else ptr(w, f64p), ptr(bt.centers, f64p),
            ptr(bt.ranges, f64p), ptr(bt.weights, f64p), ptr(bt.left_child, i64p), ptr(bt.right_child, i64p),
            ptr(bt.lowest_leaf, i64p), ptr(bt.highest_leaf, i64p), ptr(bt.permutation, i64p), ptr(bd.means, f64p),
            ptr(bd.bandwidth, f64p), ptr(bd.bandwidthMin, f64p), ptr(bd.bandwidthMax, f64p), *tail)
    return rc, bd


@pytest.mark.parametrize("D,N", [(2, 65), (3, 600)])
def test_null_all_zeros_and_the_existing_entry_are_the_same_bits(D, N):
    pts, ks, w = tm.tree_case("straddle", 9 + N, D, N, [1] * D, weighted=True)
    flat = np.ascontiguousarray(pts.T).ravel()
    zeros = np.zeros(D, dtype=np.uint8)
    rc0, old = _raw_build(_lib.lib.kdehip_make_density, D, N, flat, ks, w)
    rc1, null = _raw_build(_lib.lib.kdehip_make_density_tree, D, N, flat, ks, w, None)
    rc2, zero = _raw_build(_lib.lib.kdehip_make_density_tree, D, N, flat, ks, w, ptr(zeros, u8p))
    assert (rc0, rc1, rc2) == (0, 0, 0)
    ref = tm.density_arrays(old)
    assert tm.differing(tm.density_arrays(null), ref) == []
    assert tm.differing(tm.density_arrays(zero), ref) == []
    assert tm.differing(tm.density_arrays(kdehip.kde(pts, ks, w, tree_manifold=[0] * D)), ref) == []
    assert tm.differing(ref, tm.density_arrays(oracle.OracleDensity(pts, ks, w))) == []


@pytest.mark.parametrize("D,N", [(1, 33), (2, 64), (2, 200), (3, 600)])
def test_a_density_across_the_cut_gets_another_tree(D, N):
    """N(pi, 0.4) wrapped: the Euclidean builder sees two clusters at the ends of [-pi, pi) and centres its root in the
    empty middle; the circular builder sees one cluster at the cut"""
    man = [1] + [0] * (D - 1)
    pts, ks, w = tm.tree_case("straddle", 40 + N, D, N, man)
    pts[1:] *= 0.01  # (the circular dimension is the widest for both builders)
    circ, eucl = kdehip.kde(pts, ks, tree_manifold=man), kdehip.kde(pts, ks)
    assert not np.array_equal(circ.bt.permutation, eucl.bt.permutation)
    assert abs(pymodel.wrapRad(circ.bt.centers[0] - math.pi)) < 0.5
    assert abs(eucl.bt.centers[0]) < 0.5


def test_a_byte_above_one_is_refused_before_anything_is_written():
    D, N = 2, 10
    pts, ks, w = tm.tree_case("uniform", 3, D, N, [1, 1])
    flat = np.ascontiguousarray(pts.T).ravel()
    bad = np.array([1, 2], dtype=np.uint8)
    rc, bd = _raw_build(_lib.lib.kdehip_make_density_tree, D, N, flat, ks, None, ptr(bad, u8p))
    assert rc == _lib.ERR_ARG
    assert all((a == 77).all() for a in tm.density_arrays(bd).values())
    # the entries that go to a device refuse it before they touch one
    bw = np.zeros(D)
    rc, bd = _raw_build(lambda D_, N_, p, k, nk, w_, *rest: _lib.lib.kdehip_make_density_auto_tree(
        D_, N_, p, ptr(bw, f64p), None, NO_SUCH_DEVICE, *rest), D, N, flat, ks, None, None, ptr(bad, u8p))
    assert rc == _lib.ERR_ARG
    assert all((a == 77).all() for a in tm.density_arrays(bd).values())
    h = C.c_void_p()
    assert _lib.lib.kdehip_density_from_device_points_tree(C.byref(h), C.c_void_p(256), D, N, NO_SUCH_DEVICE, None, None, None,
                                                           None, ptr(bad, u8p)) == _lib.ERR_ARG
    one = kdehip.density._empty_density(D, N)
    arrs = tm.density_arrays(one)

    def pp(a):
        return (C.c_void_p * 1)(a.ctypes.data)
    Ns = np.array([N], dtype=np.int64)
    rc = _lib.lib.kdehip_make_densities_device_tree(
        1, D, ptr(Ns, i64p), pp(flat), pp(ks), ks.size, None, pp(arrs["centers"]), pp(arrs["ranges"]), pp(arrs["weights"]),
        pp(arrs["left_child"]), pp(arrs["right_child"]), pp(arrs["lowest_leaf"]), pp(arrs["highest_leaf"]),
        pp(arrs["permutation"]), pp(arrs["means"]), pp(arrs["bandwidth"]), pp(arrs["bandwidthMin"]), pp(arrs["bandwidthMax"]),
        NO_SUCH_DEVICE, ptr(bad, u8p))
    assert rc == _lib.ERR_ARG


def test_wrong_lengths_and_the_old_refusal():
    pts = np.random.default_rng(0).uniform(-3, 3, (2, 20))
    with pytest.raises(ValueError):
        kdehip.kde(pts, [0.3], tree_manifold=[1])
    with pytest.raises(ValueError):
        kdehip.kde(pts, [0.3], tree_manifold=[1, 0, 0])
    with pytest.raises(ValueError):
        kdehip.kde_batch([(pts, [0.3])], device=NO_SUCH_DEVICE, tree_manifold=[1])
    with pytest.raises(ValueError):
        kdehip.kde(pts, tree_manifold=[1])  # (the automatic bandwidth: refused before the search starts)
    with pytest.raises(ValueError):
        kdehip.kde(pts, [0.3], manifold=[0, 1])  # an explicit bandwidth leaves nothing to search: as before
    with pytest.raises(ValueError):
        kdehip.kde(pts, [0.3], manifold=[0, 1], tree_manifold=[0, 1])
