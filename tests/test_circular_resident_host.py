"""Circular dimensions on the resident entry points (include/kdehip.h sections 2c-2e) without a GPU: the four new symbols are
exported by libkdehip.so and declared in the header with the signatures the Python layer binds, and the handling of the
`manifold=` argument -- one manifold, one per product, one for all products -- before anything reaches the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip.product import _batch_manifolds, _manifold_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kdehip_prod_philox_device_manifold", "kdehip_prod_philox_resident_manifold", "kdehip_mul_device_manifold",
       "kdehip_mul_device_batch_manifold"]

# C parameter type -> the ctypes type the Python layer must bind it with
CTYPES = {
    "int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double *": _lib.f64p, "int64_t *": _lib.i64p,
    "int32_t *": _lib.i32p, "const uint8_t *": _lib.u8p, "void *": C.c_void_p,
    "kdehip_device_density *const *": C.POINTER(C.c_void_p), "kdehip_device_density **": C.POINTER(C.c_void_p),
    "const kdehip_mul_item *": C.POINTER(_lib.CMulItem),
}
# device arrays are passed as addresses: the binding may say void* where the header says a typed device pointer
DEVICE_ARRAYS = {"d_points", "d_indices", "d_labels"}


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/kdehip.h"
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        mm = re.match(r"(.*?)(\w+)$", p)
        params.append((mm.group(1).strip(), mm.group(2)))
    return params


@pytest.mark.parametrize("name", NEW)
def test_symbol_is_exported_and_bound_as_declared(name):
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int
    params = _declaration(name)
    assert len(params) == len(args), (params, args)
    for (ctype, pname), bound in zip(params, args):
        want = C.c_void_p if pname in DEVICE_ARRAYS else CTYPES[ctype]
        assert bound is want or bound == want, (name, pname, ctype, bound)
    assert any(pname in ("manifold", "manifolds") for _, pname in params)


def test_existing_entries_keep_their_declarations():
    for name in ("kdehip_prod_philox_device", "kdehip_prod_philox_resident", "kdehip_mul_device", "kdehip_mul_device_batch"):
        assert not any(p in ("manifold", "manifolds") for _, p in _declaration(name))


def test_manifold_array():
    assert _manifold_array(None, 3) is None
    m = _manifold_array([0, "circular", "euclid"], 3)
    assert m.dtype == np.uint8 and list(m) == [0, 1, 0]
    assert list(_manifold_array([0, 2], 2)) == [0, 2]   # (membership of the enum is the library's check)
    with pytest.raises(ValueError):
        _manifold_array([1], 2)
    with pytest.raises(ValueError):
        _manifold_array([1, 0, 0], 2)


def test_batch_manifolds_shared_and_per_product():
    assert _batch_manifolds(None, [2, 3]) == [None, None]
    shared = _batch_manifolds([0, 1], [2, 2, 2])          # one manifold for all products
    assert [list(m) for m in shared] == [[0, 1]] * 3
    shared = _batch_manifolds(["euclid", "circular"], [2])
    assert [list(m) for m in shared] == [[0, 1]]
    per = _batch_manifolds([[0, 1], None, [1, 0, 1]], [2, 6, 3])   # one per product, None = Euclidean
    assert list(per[0]) == [0, 1] and per[1] is None and list(per[2]) == [1, 0, 1]
    assert _batch_manifolds([None, None], [2, 2]) == [None, None]
    with pytest.raises(ValueError):
        _batch_manifolds([0, 1], [2, 3])                  # a shared manifold must fit every product
    with pytest.raises(ValueError):
        _batch_manifolds([[0, 1]], [2, 2])                # per product: one entry each
    with pytest.raises(ValueError):
        _batch_manifolds([[0, 1], [0]], [2, 2])           # ... of that product's dimensions


def test_keywords_exist():
    import inspect
    for fn in (kdehip.prodAppxMSGibbsS_device, kdehip.prodAppxMSGibbsS_resident, kdehip.mul_device, kdehip.mul_device_batch):
        assert "manifold" in inspect.signature(fn).parameters, fn.__name__
