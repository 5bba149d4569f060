"""Circular dimensions on resident plans, several GPUs and batched launches (include/kdehip.h sections 2, 2b, 2e) without a
GPU: the four new symbols are exported, and their manifold arguments are refused BEFORE any device is touched -- these
checks return the same codes on a machine without one."""
import ctypes as C
import inspect

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import f64p, i64p, ptr, u8p

NEW = ["kdehip_product_create_manifold", "kdehip_product_multi_create_manifold", "kdehip_prod_philox_manifold",
       "kdehip_prod_philox_batch_manifold"]


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def _host_trees(D, n=12, M=2):
    rng = np.random.default_rng(D)
    return [kdehip.kde(rng.standard_normal((D, n)), [0.3]) for _ in range(M)]


def _call(entry, trees, ndims, manifold, precision):
    """the named entry on host trees with `manifold` (a uint8 array); returns the library's code"""
    M = len(trees)
    arr = (_lib.CDensity * M)(*[t._cstruct() for t in trees])
    man = np.ascontiguousarray(manifold, dtype=np.uint8)
    h = C.c_void_p()
    if entry == "kdehip_product_create_manifold":
        return _lib.lib.kdehip_product_create_manifold(C.byref(h), M, arr, ndims, None, ptr(man, u8p), precision, 0)
    if entry == "kdehip_product_multi_create_manifold":
        return _lib.lib.kdehip_product_multi_create_manifold(C.byref(h), M, arr, ndims, None, ptr(man, u8p), precision, 0, 2)
    Np = 4
    pts, ind = np.zeros(ndims * Np), np.zeros(M * Np, dtype=np.int64)
    return _lib.lib.kdehip_prod_philox_manifold(M, arr, Np, 1, ptr(pts, f64p), ptr(ind, i64p), C.c_uint64(1), 1, ndims, None,
                                                ptr(man, u8p), precision, 0, 2, None)


@pytest.mark.parametrize("entry", NEW[:3])
def test_host_tree_entries_refuse_a_bad_manifold_before_any_device(entry):
    t2 = _host_trees(2)
    assert _call(entry, t2, 2, [0, 2], 64) == _lib.ERR_ARG                 # not a member of the enum
    assert _call(entry, t2, 2, [0, 1], 32) == _lib.ERR_UNSUPPORTED         # the circular operators are fp64 only
    assert _call(entry, t2, 9, [0] * 8 + [1], 64) == _lib.ERR_UNSUPPORTED  # more than KDEHIP_MAX_DIMS dimensions
    assert "ndims" in _lib.lib.kdehip_last_error().decode()


def test_batch_entry_refuses_a_bad_manifold_row_before_any_density_or_device():
    """The batch takes resident handles, which only a GPU machine can make (and which carry their own dimension count: a
    ninth dimension is not expressible without one): the rows are checked before the items are looked at, so an item without
    densities still gets the manifold's error."""
    items = (_lib.CBatchItem * 2)()
    for it in items:
        it.Ndens, it.Niter, it.Np = 2, 1, 4
    rows = np.zeros((2, _lib.MAX_DIMS), dtype=np.uint8)
    rows[1, 1] = 2
    assert _lib.lib.kdehip_prod_philox_batch_manifold(2, items, ptr(rows, u8p), 64, None) == _lib.ERR_ARG
    assert "manifold" in _lib.lib.kdehip_last_error().decode()
    rows[1, 1] = 1
    assert _lib.lib.kdehip_prod_philox_batch_manifold(2, items, ptr(rows, u8p), 32, None) == _lib.ERR_UNSUPPORTED
    assert "precision" in _lib.lib.kdehip_last_error().decode()


def test_python_argument_errors():
    t2 = _host_trees(2)
    for cls in (kdehip.ProductPlan, kdehip.MultiProductPlan):
        with pytest.raises(ValueError):
            cls(t2, manifold=[1])                    # one entry per dimension
        with pytest.raises(ValueError):
            cls(t2, manifold=[0, 1, 0])
        with pytest.raises(ValueError):
            cls(t2, manifold=["euclid", "torus"])    # a name outside the enum
        with pytest.raises(kdehip.KdeHipError) as e:
            cls(t2, manifold=[0, 2])                 # a value outside the enum: the library's check, no device needed
        assert e.value.code == _lib.ERR_ARG
        with pytest.raises(kdehip.KdeHipError) as e:
            cls(t2, manifold=[0, 1], precision=32)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        kdehip.prodAppxMSGibbsS(None, t2, None, None, Np=4, seed=1, manifold=[1], fast_circular=True)
    with pytest.raises(kdehip.KdeHipError) as e:
        kdehip.prodAppxMSGibbsS(None, t2, None, None, Np=4, seed=1, manifold=[0, 2], ngpus=2)
    assert e.value.code == _lib.ERR_ARG


def test_keywords_exist():
    for fn, kw in ((kdehip.ProductPlan.__init__, "manifold"), (kdehip.MultiProductPlan.__init__, "manifold"),
                   (kdehip.ProductBatch.__init__, "manifold"), (kdehip.prodAppxMSGibbsS_batch, "manifold"),
                   (kdehip.prodAppxMSGibbsS, "fast_circular")):
        assert kw in inspect.signature(fn).parameters, (fn, kw)
    assert inspect.signature(kdehip.prodAppxMSGibbsS).parameters["fast_circular"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(kdehip.prodAppxMSGibbsS).parameters["fast_circular"].default is False
