"""The `manifold=` / `tree_manifold=` argument of the front end: parsing, the conventions of the batch calls, and the forms
the C ABI takes it in (include/kdehip.h "manifolds": NULL, or one byte per dimension, 0 = Euclidean, 1 = circular; the
`n x KDEHIP_MAX_DIMS` byte matrix of a batch; the `circular_mask` word of a batch item).  Every module of the package reads
the argument through this one; it imports nothing of the package but `_lib`.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_NAMES = {"euclid": 0, "euclidean": 0, "circular": 1, "circ": 1}


def parse(manifold, ndims, unknown_name=KeyError):
    """None, or a sequence of 0 / 'euclid' / 1 / 'circular' per dimension, as the uint8 enum array.  A wrong length is a
    ValueError; a name outside the enum is a KeyError, or a ValueError for the callers that say so (the plans).  Integers
    pass as they are: membership of the enum is the library's check."""
    if manifold is None:
        return None
    try:
        vals = [_NAMES[m.lower()] if isinstance(m, str) else int(m) for m in manifold]
    except KeyError as e:
        if unknown_name is KeyError:
            raise
        raise unknown_name(f"manifold: {e.args[0]!r} is not 'euclid' or 'circular'") from None
    if len(vals) != ndims:
        raise ValueError("manifold needs one entry per dimension")
    return np.ascontiguousarray(vals, dtype=np.uint8)


def resolve(p, manifold, ndims, attr="manifold"):
    """The argument of a call on the density `p` of `ndims` dimensions: "inherit" reads the density's record (`attr`); a
    wrong length or a value other than 0 / 1 is a ValueError (before any device is needed); all-Euclidean is None."""
    if isinstance(manifold, str):
        if manifold != "inherit":
            raise ValueError("manifold: a per-dimension sequence, None or 'inherit'")
        manifold = getattr(p, attr, None)
    man = parse(manifold, ndims)
    if man is None:
        return None
    if (man > 1).any():
        raise ValueError("manifold: every entry is 'euclid' (0) or 'circular' (1)")
    return man if man.any() else None


def select(man, dims):
    """the entries of an enum array at the selected dims; None when none of them is circular"""
    if man is None or not man[dims].any():
        return None
    return np.ascontiguousarray(man[dims])


def per_product(manifold, dims, own=None):
    """The argument of a batch as one enum array (or None) per product: None; ONE manifold for all products (a flat sequence
    of enum values, every product then has that many dimensions); or one entry per product (each None or a manifold of
    that product's dimensions).  `dims`: the products' dimension counts.  `own`: per product its own `manifold` value or
    None -- it wins."""
    n = len(dims)
    if manifold is None:
        out = [None] * n
    else:
        manifold = list(manifold)
        shared = len(manifold) > 0 and all(m is not None and (isinstance(m, str) or np.ndim(m) == 0) for m in manifold)
        if not shared and len(manifold) != n:
            raise ValueError("manifold: one manifold for all products, or one entry per product")
        out = [parse(manifold if shared else manifold[k], d) for k, d in enumerate(dims)]
    if own is not None:
        out = [m if o is None else parse(o, d) for o, d, m in zip(own, dims, out)]
    return out


def per_item(items, manifold):
    """The resolved manifold of every item of a batch of densities (dicts with `density`): one for all or one per item, an
    item's own `manifold` key wins, "inherit" reads the item's density; each distinct (dimension count, value) is parsed
    once."""
    dims = [it["density"].dims for it in items]
    if manifold is not None and all(isinstance(m, str) or np.ndim(m) == 0 for m in manifold):
        shared = [tuple(manifold)] * len(items)   # one for all: parsed below, once per dimension count
    else:
        shared = per_product(manifold, dims)
    seen, out = {}, []
    for it, D, sh in zip(items, dims, shared):
        m = it["manifold"] if "manifold" in it else sh
        if m is None or isinstance(m, str):
            out.append(resolve(it["density"], m, D))
            continue
        key = (D, tuple(m))
        if key not in seen:
            seen[key] = resolve(it["density"], m, D)
        out.append(seen[key])
    return out


def matrix(mans):
    """the `n x KDEHIP_MAX_DIMS` byte matrix of a batch: row k = product k's manifold (zeros = Euclidean)"""
    out = np.zeros((len(mans), _lib.MAX_DIMS), dtype=np.uint8)
    for k, m in enumerate(mans):
        if m is not None:
            out[k, :len(m)] = m
    return out


def mask(man) -> int:
    """the `circular_mask` word of a batch item: bit d = dimension d is circular"""
    return 0 if man is None else sum(1 << d for d in range(len(man)) if man[d])


def pointer(man):
    """the argument as the ABI takes it: NULL, or the bytes"""
    return None if man is None else man.ctypes.data_as(_lib.u8p)
