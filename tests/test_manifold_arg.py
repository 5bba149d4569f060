"""The return code of every C ABI entry that takes a `manifold` and / or `tree_manifold` byte argument, for the argument
values an entry can refuse or must accept -- a record of the library's behaviour, entry by entry, called through
`_lib.lib` (no Python wrapper in between):

  two_first / two_last   a byte of 2 in the first / last position
  ndims9                 nine dimensions with a non-NULL argument (entries that are told, or read, a dimension count)
  circ_fp32              a circular bit with precision 32 (entries that take a precision)
  null / zeros           NULL / all zeros: the Euclidean entry

Entries on host arrays (D = 2, N = 8) refuse before they look for a device: those rows are plain tests.  Their accepted
rows, and every row of an entry on handles or device arrays (D = 2, N = 64), need the GPU.  The batch entries whose items
carry a `circular_mask` word take no byte argument and have no row here.
"""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import ERR_ARG, ERR_UNSUPPORTED, KDEHIP_OK, f64p, i32p, i64p, ptr, u8p

OK, ARG, UNS = KDEHIP_OK, ERR_ARG, ERR_UNSUPPORTED
L = _lib.lib


def _bytes(vals):
    return None if vals is None else np.ascontiguousarray(vals, dtype=np.uint8)


def _p(a):
    return None if a is None else ptr(a, u8p)


def _points(D, N, seed=5):
    return np.random.default_rng(seed).standard_normal((D, N))


def _outs(D, N):
    """the twelve output arrays of a tree build, as ctypes pointers (and the arrays, kept alive)"""
    f = [np.zeros(2 * N * D) for _ in range(2)] + [np.zeros(2 * N)]
    i = [np.zeros(2 * N, dtype=np.int64) for _ in range(5)]
    g = [np.zeros(2 * N * D) for _ in range(2)] + [np.zeros(N * D) for _ in range(2)]
    return [ptr(a, f64p) for a in f] + [ptr(a, i64p) for a in i] + [ptr(a, f64p) for a in g], (f, i, g)


class Host:
    """densities on host arrays: two of D = 2 and two of D = 9, N = 8"""

    def __init__(self):
        self.d = {D: [kdehip.kde(_points(D, 8, s), [0.5]) for s in (1, 2)] for D in (2, 9)}

    def trees(self, D=2):
        return (_lib.CDensity * 2)(*[t._cstruct() for t in self.d[D]])


@pytest.fixture(scope="module")
def host():
    return Host()


# ---- entries on host arrays: f(host, D, manifold bytes, tree_manifold bytes, precision) -> rc ------------------------------
def _evaluate(h, D, m, t, prec):
    out = np.zeros(4)
    return L.kdehip_evaluate_manifold(C.byref(h.d[D][0]._cstruct()), ptr(_points(D, 4).T.copy(), f64p), 4, 0, ptr(out, f64p), 0, _p(m))


def _avg_logl(h, D, m, t, prec):
    out = C.c_double(0)
    return L.kdehip_eval_avg_logl_manifold(C.byref(h.d[D][0]._cstruct()), C.byref(h.d[D][1]._cstruct()), 0, C.byref(out), 0, _p(m))


def _auto_bandwidth(h, D, m, t, prec):
    bw, ne = np.zeros(D), C.c_int32(0)
    return L.kdehip_auto_bandwidth_manifold(D, 8, ptr(_points(D, 8).T.copy(), f64p), ptr(bw, f64p), C.byref(ne), 0, _p(m))


def _make_density_auto(tree):
    def f(h, D, m, t, prec):
        bw, ne = np.zeros(D), C.c_int32(0)
        outs, keep = _outs(D, 8)
        head = (D, 8, ptr(_points(D, 8).T.copy(), f64p), ptr(bw, f64p), C.byref(ne), 0, *outs, _p(m))
        return L.kdehip_make_density_auto_tree(*head, _p(t)) if tree else L.kdehip_make_density_auto_manifold(*head)
    return f


def _make_density_tree(h, D, m, t, prec):
    outs, keep = _outs(D, 8)
    ks = np.array([0.5])
    return L.kdehip_make_density_tree(D, 8, ptr(_points(D, 8).T.copy(), f64p), ptr(ks, f64p), 1, None, *outs, _p(t))


def _make_densities_device_tree(h, D, m, t, prec):
    outs, keep = _outs(D, 8)
    pts, ks, Ns = _points(D, 8).T.copy(), np.array([0.5]), np.array([8], dtype=np.int64)
    one = lambda a: (C.c_void_p * 1)(C.cast(a, C.c_void_p))  # noqa: E731
    return L.kdehip_make_densities_device_tree(1, D, ptr(Ns, i64p), one(ptr(pts, f64p)), one(ptr(ks, f64p)), 1, None,
                                               *[one(o) for o in outs], 0, _p(t))


def _gibbs1(h, D, m, t, prec):
    pts, ind, ru, rn = np.zeros(D * 4), np.ones(2 * 4, dtype=np.int64), np.full(4096, 0.5), np.zeros(4096)
    return L.kdehip_gibbs1_manifold(2, h.trees(), 4, 1, ptr(pts, f64p), ptr(ind, i64p), ptr(ru, f64p), ru.size, ptr(rn, f64p),
                                    rn.size, 1, D, None, _p(m), 0, None)


def _prod_philox(h, D, m, t, prec):
    pts, ind = np.zeros(D * 4), np.ones(2 * 4, dtype=np.int64)
    return L.kdehip_prod_philox_manifold(2, h.trees(), 4, 1, ptr(pts, f64p), ptr(ind, i64p), C.c_uint64(3), 1, D, None, _p(m),
                                         prec, 0, 1, None)


def _product_create(multi):
    def f(h, D, m, t, prec):
        out = C.c_void_p()
        if multi:
            rc = L.kdehip_product_multi_create_manifold(C.byref(out), 2, h.trees(), D, None, _p(m), prec, 0, 1)
            if out:
                L.kdehip_product_multi_destroy(out)
        else:
            rc = L.kdehip_product_create_manifold(C.byref(out), 2, h.trees(), D, None, _p(m), prec, 0)
            if out:
                L.kdehip_product_destroy(out)
        return rc
    return f


def _kde_max(h, D, m, t, prec):
    out = np.zeros(D)
    return L.kdehip_kde_max_manifold(C.byref(h.d[D][0]._cstruct()), 16, ptr(out, f64p), None, 0, _p(m))


def _inters(h, D, m, t, prec):
    out = C.c_double(0)
    return L.kdehip_inters_intg_appx_is_manifold(C.byref(h.d[D][0]._cstruct()), C.byref(h.d[D][1]._cstruct()), 16, C.byref(out), 0, _p(m))


def _sample(h, D, m, t, prec):
    pts, ind = np.zeros(D * 4), np.zeros(4, dtype=np.int64)
    return L.kdehip_sample_manifold(C.byref(h.d[D][0]._cstruct()), 4, C.c_uint64(3), 0, None, ptr(pts, f64p), ptr(ind, i64p), 0, _p(m))


# entry: (call, arguments it takes, has a precision, rc of ndims9 per argument)
HOST_ENTRIES = {
    "kdehip_evaluate_manifold": (_evaluate, "m", False, {"m": UNS}),
    "kdehip_eval_avg_logl_manifold": (_avg_logl, "m", False, {"m": UNS}),
    "kdehip_auto_bandwidth_manifold": (_auto_bandwidth, "m", False, {"m": UNS}),
    "kdehip_make_density_auto_manifold": (_make_density_auto(False), "m", False, {"m": UNS}),
    "kdehip_make_density_auto_tree": (_make_density_auto(True), "mt", False, {"m": UNS, "t": UNS}),
    "kdehip_make_density_tree": (_make_density_tree, "t", False, {"t": OK}),   # (the host builder has no dimension limit)
    "kdehip_make_densities_device_tree": (_make_densities_device_tree, "t", False, {"t": UNS}),
    "kdehip_gibbs1_manifold": (_gibbs1, "m", False, {"m": UNS}),
    "kdehip_prod_philox_manifold": (_prod_philox, "m", True, {"m": UNS}),
    "kdehip_product_create_manifold": (_product_create(False), "m", True, {"m": UNS}),
    "kdehip_product_multi_create_manifold": (_product_create(True), "m", True, {"m": UNS}),
    "kdehip_kde_max_manifold": (_kde_max, "m", False, {"m": UNS}),
    "kdehip_inters_intg_appx_is_manifold": (_inters, "m", False, {"m": UNS}),
    "kdehip_sample_manifold": (_sample, "m", False, {"m": UNS}),
}
# the one entry here that needs no device at all: its accepted rows are plain tests too
PURE_HOST = {"kdehip_make_density_tree"}


def _rows(entries, refused):
    """(entry, argument, case, D, bytes, precision, expected rc): the refusals, or the accepted values"""
    out = []
    for name, (_, args, has_prec, nine) in entries.items():
        for a in args:
            if refused:
                out.append((name, a, "two_first", 2, [2, 0], 64, ARG))
                out.append((name, a, "two_last", 2, [0, 2], 64, ARG))
                if nine is not None and a in nine:
                    out.append((name, a, "ndims9", 9, [1] + [0] * 8, 64, nine[a]))
                if has_prec and a == "m":
                    out.append((name, a, "circ_fp32", 2, [1, 0], 32, UNS))
            else:
                out.append((name, a, "null", 2, None, 64, OK))
                out.append((name, a, "zeros", 2, [0, 0], 64, OK))
    return out


def _ids(rows):
    return [f"{r[0]}-{'tree_manifold' if r[1] == 't' else 'manifold'}-{r[2]}" for r in rows]


def _run(entries, ctx, row):
    name, a, case, D, vals, prec, want = row
    b = _bytes(vals)
    rc = entries[name][0](ctx, D, b if a == "m" else None, b if a == "t" else None, prec)
    assert rc == want, (name, a, case, rc, L.kdehip_last_error().decode())


_HOST_REFUSED = [r for r in _rows(HOST_ENTRIES, True) if not (r[2] == "ndims9" and r[6] == OK)]
_HOST_PLAIN_OK = [r for r in _rows(HOST_ENTRIES, False) + _rows(HOST_ENTRIES, True)
                  if r[0] in PURE_HOST and r[6] == OK]
_HOST_GPU_OK = [r for r in _rows(HOST_ENTRIES, False) if r[0] not in PURE_HOST]


@pytest.mark.parametrize("row", _HOST_REFUSED + _HOST_PLAIN_OK, ids=_ids(_HOST_REFUSED + _HOST_PLAIN_OK))
def test_host_entry_without_a_device(host, row):
    _run(HOST_ENTRIES, host, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", _HOST_GPU_OK, ids=_ids(_HOST_GPU_OK))
def test_host_entry_accepts(host, row):
    _run(HOST_ENTRIES, host, row)


# ---- entries on handles and device arrays ----------------------------------------------------------------------------------
class Dev:
    """two resident densities of D = 2, N = 64, and device arrays for the outputs"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.d = [kdehip.DeviceDensity(kdehip.kde(_points(2, 64, s), [0.4]), device=0) for s in (1, 2)]
        self.h = (C.c_void_p * 2)(*[x._h for x in self.d])
        self.f64 = torch.zeros(4096, dtype=torch.float64, device=self.dev)
        self.i64 = torch.zeros(4096, dtype=torch.int64, device=self.dev)
        self.pts = {D: torch.from_numpy(_points(D, 64).T.copy()).to(self.dev) for D in (2, 9)}
        torch.cuda.synchronize()

    def sync(self):
        self.torch.cuda.synchronize()

    def free(self, out):
        self.sync()
        for h in out if isinstance(out, C.Array) else [out]:
            if h:
                L.kdehip_density_free(C.c_void_p(h) if isinstance(h, int) else h)


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _a(x):
    return C.c_void_p(x.data_ptr())


def _rows8(b):
    """an item's bytes as row 0 of a 1 x KDEHIP_MAX_DIMS matrix"""
    if b is None:
        return None
    r = np.zeros((1, _lib.MAX_DIMS), dtype=np.uint8)
    r[0, :len(b)] = b
    return r


def _evaluate_device(g, D, m, t, prec):
    rc = L.kdehip_evaluate_device_manifold(g.d[0]._h, _a(g.pts[2]), 64, 0, _a(g.f64), None, _p(m))
    g.sync()
    return rc


def _evaluate_device_at(g, D, m, t, prec):
    rc = L.kdehip_evaluate_device_at_manifold(g.d[0]._h, g.d[1]._h, _a(g.f64), None, _p(m))
    g.sync()
    return rc


def _avg_logl_device(g, D, m, t, prec):
    out = C.c_double(0)
    return L.kdehip_eval_avg_logl_device_manifold(g.d[0]._h, g.d[1]._h, 0, C.byref(out), _p(m))


def _from_device_points(tree):
    def f(g, D, m, t, prec):
        out, bw, ne = C.c_void_p(), np.zeros(D), C.c_int32(0)
        head = (C.byref(out), _a(g.pts[D]), D, 64, 0, None, ptr(bw, f64p), C.byref(ne), _p(m))
        rc = L.kdehip_density_from_device_points_tree(*head, _p(t)) if tree else L.kdehip_density_from_device_points_manifold(*head)
        g.free(out)
        return rc
    return f


def _mul_device(tree):
    def f(g, D, m, t, prec):
        out, bw, ne = C.c_void_p(), np.zeros(2), C.c_int32(0)
        head = (C.byref(out), 2, g.h, C.c_uint64(3), 1, ptr(bw, f64p), C.byref(ne), _p(m))
        rc = L.kdehip_mul_device_tree(*head, _p(t)) if tree else L.kdehip_mul_device_manifold(*head)
        g.free(out)
        return rc
    return f


def _mul_device_batch(tree):
    def f(g, D, m, t, prec):
        items = (_lib.CMulItem * 1)()
        items[0].Ndens, items[0].addEntropy, items[0].trees, items[0].seed = 2, 1, g.h, 3
        out, bw, ne = (C.c_void_p * 1)(), np.zeros((1, _lib.MAX_DIMS)), np.zeros(1, dtype=np.int32)
        mm, tt = _rows8(m), _rows8(t)
        if tree:
            rc = L.kdehip_mul_device_batch_tree(1, items, _p(mm), _p(tt), out, ptr(bw, f64p), ptr(ne, i32p))
        else:
            rc = L.kdehip_mul_device_batch_manifold(1, items, _p(mm), out, ptr(bw, f64p), ptr(ne, i32p))
        g.free(out)
        return rc
    return f


def _prod_device(g, D, m, t, prec):
    rc = L.kdehip_prod_philox_device_manifold(2, g.h, 16, 1, C.c_uint64(3), 0, 1, None, _p(m), prec, _a(g.f64), _a(g.i64), None, None)
    g.sync()
    return rc


def _prod_resident(g, D, m, t, prec):
    pts, ind = np.zeros(2 * 16), np.zeros(2 * 16, dtype=np.int64)
    return L.kdehip_prod_philox_resident_manifold(2, g.h, 16, 1, C.c_uint64(3), 1, None, _p(m), prec, ptr(pts, f64p), ptr(ind, i64p))


def _prod_batch(g, D, m, t, prec):
    items = (_lib.CBatchItem * 1)()
    it = items[0]
    it.Ndens, it.Niter, it.trees, it.Np, it.seed, it.addEntropy = 2, 1, g.h, 16, 3, 1
    it.d_points, it.d_indices = _a(g.f64), _a(g.i64)
    rc = L.kdehip_prod_philox_batch_manifold(1, items, _p(_rows8(m)), prec, None)
    g.sync()
    return rc


def _summary(g, D, m, t, prec):
    rng, mean = np.zeros(4), np.zeros(2)
    ext = C.c_double(0.1)
    return L.kdehip_density_summary_manifold(g.d[0]._h, C.byref(ext), 16, ptr(rng, f64p), ptr(mean, f64p), None, None, None, _p(m))


def _inters_device(g, D, m, t, prec):
    out = C.c_double(0)
    return L.kdehip_inters_intg_appx_is_device_manifold(g.d[0]._h, g.d[1]._h, 16, C.byref(out), _p(m))


def _marginal(g, D, m, t, prec):
    out, dims = C.c_void_p(), np.array([2, 1], dtype=np.int32)
    rc = L.kdehip_density_marginal_device_tree(C.byref(out), g.d[0]._h, 2, ptr(dims, i32p), _p(t))
    g.free(out)
    return rc


def _sample_device(g, D, m, t, prec):
    rc = L.kdehip_sample_device_manifold(g.d[0]._h, 16, C.c_uint64(3), 0, None, _a(g.f64), _a(g.i64), None, _p(m))
    g.sync()
    return rc


def _resample(g, D, m, t, prec):
    out, bw, ne = C.c_void_p(), np.zeros(2), C.c_int32(0)
    rc = L.kdehip_resample_device_manifold(C.byref(out), g.d[0]._h, 64, C.c_uint64(3), ptr(bw, f64p), C.byref(ne), _p(m), _p(t))
    g.free(out)
    return rc


# (a handle carries its own dimension count: only the two entries that are told D have an ndims9 row)
DEV_ENTRIES = {
    "kdehip_evaluate_device_manifold": (_evaluate_device, "m", False, None),
    "kdehip_evaluate_device_at_manifold": (_evaluate_device_at, "m", False, None),
    "kdehip_eval_avg_logl_device_manifold": (_avg_logl_device, "m", False, None),
    "kdehip_density_from_device_points_manifold": (_from_device_points(False), "m", False, {"m": UNS}),
    "kdehip_density_from_device_points_tree": (_from_device_points(True), "mt", False, {"m": UNS, "t": UNS}),
    "kdehip_mul_device_manifold": (_mul_device(False), "m", False, None),
    "kdehip_mul_device_tree": (_mul_device(True), "mt", False, None),
    "kdehip_mul_device_batch_manifold": (_mul_device_batch(False), "m", False, None),
    "kdehip_mul_device_batch_tree": (_mul_device_batch(True), "mt", False, None),
    "kdehip_prod_philox_device_manifold": (_prod_device, "m", True, None),
    "kdehip_prod_philox_resident_manifold": (_prod_resident, "m", True, None),
    "kdehip_prod_philox_batch_manifold": (_prod_batch, "m", True, None),
    "kdehip_density_summary_manifold": (_summary, "m", False, None),
    "kdehip_inters_intg_appx_is_device_manifold": (_inters_device, "m", False, None),
    "kdehip_density_marginal_device_tree": (_marginal, "t", False, None),
    "kdehip_sample_device_manifold": (_sample_device, "m", False, None),
    "kdehip_resample_device_manifold": (_resample, "mt", False, None),
}
_DEV_ROWS = _rows(DEV_ENTRIES, True) + _rows(DEV_ENTRIES, False)


@pytest.mark.gpu
@pytest.mark.parametrize("row", _DEV_ROWS, ids=_ids(_DEV_ROWS))
def test_device_entry(dev, row):
    _run(DEV_ENTRIES, dev, row)


def test_every_byte_argument_has_rows():
    """the table covers every entry of the ABI whose signature ends in, or holds, a manifold byte pointer"""
    named = {n for n in _lib.SIGNATURES if n.endswith(("_manifold", "_tree"))}
    masked = {"kdehip_eval_avg_logl_device_batch_manifold", "kdehip_summary_device_batch_manifold",
              "kdehip_sample_device_batch_manifold"}   # (items with a circular_mask word: no byte argument)
    assert named - masked == set(HOST_ENTRIES) | set(DEV_ENTRIES)
