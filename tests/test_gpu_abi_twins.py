"""The Euclidean entries the Python front end no longer calls (it calls their `_manifold` / `_tree` twins with NULL), each
through `_lib.lib` against its twin: the Euclidean entry, the twin with NULL, and the twin with zero bytes (or a zero
`circular_mask`) must return the same bytes.  D = 2 with N = 64 and D = 3 with N = 65 (not a multiple of the wavefront),
128 draws, Ngrid = 16, two items per batch.
"""
import ctypes as C

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from kdehip._lib import f64p, i32p, i64p, ptr, u8p

pytestmark = pytest.mark.gpu
L = _lib.lib
NDRAW, NGRID, SEED = 128, 16, 20240607


class Case:
    def __init__(self, D, N):
        import torch
        self.torch, self.D, self.N = torch, D, N
        self.dev = torch.device("cuda", 0)
        rng = np.random.default_rng(100 * D + N)
        self.host = [kdehip.kde(rng.standard_normal((D, N)) + k, [0.3 + 0.1 * k]) for k in range(2)]
        self.res = [kdehip.DeviceDensity(t, device=0) for t in self.host]
        self.zeros = np.zeros(D, dtype=np.uint8)

    def manifolds(self):
        """the three calls of a case: (twin?, manifold argument)"""
        return [(False, None), (True, None), (True, ptr(self.zeros, u8p))]

    def tensors(self, nf, ni):
        t = self.torch
        return (t.full((nf,), float("nan"), dtype=t.float64, device=self.dev), t.full((ni,), -7, dtype=t.int64, device=self.dev))

    def sync(self):
        self.torch.cuda.synchronize()


@pytest.fixture(scope="module", params=[(2, 64), (3, 65)], ids=["D2_N64", "D3_N65"])
def case(request):
    return Case(*request.param)


def _check(rc):
    assert rc == _lib.KDEHIP_OK, L.kdehip_last_error().decode()


def _same(outs):
    assert len(outs) == 3
    assert outs[0] == outs[1], "the twin with NULL differs from the Euclidean entry"
    assert outs[0] == outs[2], "the twin with zeros differs from the Euclidean entry"


def _a(x):
    return C.c_void_p(x.data_ptr())


def _dump(h):
    """every array of a resident density, as bytes (the handle is freed)"""
    with kdehip.DeviceDensity(device=0, _handle=h) as d:
        b = d.download()
    bt = b.bt
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (
        bt.centers, bt.ranges, bt.weights, bt.left_child, bt.right_child, bt.lowest_leaf, bt.highest_leaf, bt.permutation,
        b.means, b.bandwidth, b.bandwidthMin, b.bandwidthMax))


def test_sample(case):
    outs = []
    for twin, m in case.manifolds():
        pts, ind = np.full(case.D * NDRAW, np.nan), np.zeros(NDRAW, dtype=np.int64)
        args = (C.byref(case.host[0]._cstruct()), NDRAW, C.c_uint64(SEED), 0, None, ptr(pts, f64p), ptr(ind, i64p), 0)
        _check(L.kdehip_sample_manifold(*args, m) if twin else L.kdehip_sample(*args))
        assert not np.isnan(pts).any()
        outs.append(pts.tobytes() + ind.tobytes())
    _same(outs)


def test_sample_device(case):
    outs = []
    for twin, m in case.manifolds():
        P, I = case.tensors(case.D * NDRAW, NDRAW)
        args = (case.res[0]._h, NDRAW, C.c_uint64(SEED), 0, None, _a(P), _a(I), None)
        _check(L.kdehip_sample_device_manifold(*args, m) if twin else L.kdehip_sample_device(*args))
        case.sync()
        assert not case.torch.isnan(P).any()
        outs.append(P.cpu().numpy().tobytes() + I.cpu().numpy().tobytes())
    _same(outs)


def test_resample_device(case):
    outs = []
    for twin, m in case.manifolds():
        h, bw, ne = C.c_void_p(), np.zeros(case.D), C.c_int32(0)
        args = (C.byref(h), case.res[0]._h, NDRAW, C.c_uint64(SEED), ptr(bw, f64p), C.byref(ne))
        _check(L.kdehip_resample_device_manifold(*args, m, m) if twin else L.kdehip_resample_device(*args))
        outs.append(_dump(h) + bw.tobytes() + bytes(ne))
    _same(outs)


def test_density_summary(case):
    D, outs = case.D, []
    for twin, m in case.manifolds():
        bufs = [np.full(n, np.nan) for n in (2 * D, D, D * D, D, D * NGRID)]
        ext = C.c_double(0.1)
        args = (case.res[0]._h, C.byref(ext), NGRID, *[ptr(b, f64p) for b in bufs])
        _check(L.kdehip_density_summary_manifold(*args, m) if twin else L.kdehip_density_summary(*args))
        assert not any(np.isnan(b).any() for b in bufs)
        outs.append(b"".join(b.tobytes() for b in bufs))
    _same(outs)


def test_kde_max(case):
    D, outs = case.D, []
    for twin, m in case.manifolds():
        out, vals = np.full(D, np.nan), np.full(D * NGRID, np.nan)
        args = (C.byref(case.host[0]._cstruct()), NGRID, ptr(out, f64p), ptr(vals, f64p), 0)
        _check(L.kdehip_kde_max_manifold(*args, m) if twin else L.kdehip_kde_max(*args))
        assert not np.isnan(out).any() and not np.isnan(vals).any()
        outs.append(out.tobytes() + vals.tobytes())
    _same(outs)


def test_density_marginal_device(case):
    dims = np.array([case.D, 1], dtype=np.int32)   # (reordered)
    zeros2 = np.zeros(2, dtype=np.uint8)
    outs = []
    for twin, m in [(False, None), (True, None), (True, ptr(zeros2, u8p))]:
        h = C.c_void_p()
        args = (C.byref(h), case.res[0]._h, 2, ptr(dims, i32p))
        _check(L.kdehip_density_marginal_device_tree(*args, m) if twin else L.kdehip_density_marginal_device(*args))
        outs.append(_dump(h))
    _same(outs)


def test_sample_device_batch(case):
    outs = []
    for twin in (False, True, True):
        arr = ((_lib.CSampleManifoldItem if twin else _lib.CSampleItem) * 2)()
        bufs = []
        for k in range(2):
            P, I = case.tensors(case.D * NDRAW, NDRAW)
            bufs += [P, I]
            a = arr[k].item if twin else arr[k]
            a.density, a.Npts, a.seed, a.sample_offset = case.res[k]._h, NDRAW, SEED + k, 3 * k
            a.d_pts, a.d_ind = _a(P), _a(I)
            if twin:
                arr[k].circular_mask = 0
        _check((L.kdehip_sample_device_batch_manifold if twin else L.kdehip_sample_device_batch)(2, arr, None))
        case.sync()
        assert not any(case.torch.isnan(b).any() for b in bufs[0::2])
        outs.append(b"".join(b.cpu().numpy().tobytes() for b in bufs))
    _same(outs)


def test_summary_device_batch(case):
    D, outs = case.D, []
    for twin in (False, True, True):
        arr = ((_lib.CSummaryManifoldItem if twin else _lib.CSummaryItem) * 2)()
        bufs = []
        for k in range(2):
            b = [case.tensors(n, 1)[0] for n in (2 * D, D, D * D, D, D * NGRID)]
            bufs += b
            a = arr[k].item if twin else arr[k]
            a.density, a.extend, a.Ngrid = case.res[k]._h, 0.1 + 0.1 * k, NGRID
            a.d_range, a.d_mean, a.d_cov, a.d_argmax, a.d_values = (_a(x) for x in b)
            if twin:
                arr[k].circular_mask = 0
        _check((L.kdehip_summary_device_batch_manifold if twin else L.kdehip_summary_device_batch)(2, arr, None))
        case.sync()
        assert not any(case.torch.isnan(x).any() for x in bufs)
        outs.append(b"".join(x.cpu().numpy().tobytes() for x in bufs))
    _same(outs)


def test_prod_philox_batch(case):
    D, outs = case.D, []
    trees = (C.c_void_p * 2)(*[x._h for x in case.res])
    zeros = np.zeros((2, _lib.MAX_DIMS), dtype=np.uint8)
    for twin, m in [(False, None), (True, None), (True, ptr(zeros, u8p))]:
        items = (_lib.CBatchItem * 2)()
        bufs = []
        for k in range(2):
            P, I = case.tensors(D * NDRAW, 2 * NDRAW)
            bufs += [P, I]
            it = items[k]
            it.Ndens, it.Niter, it.trees, it.Np, it.seed, it.addEntropy = 2, 2 + k, trees, NDRAW, SEED + k, 1
            it.d_points, it.d_indices = _a(P), _a(I)
        if twin:
            _check(L.kdehip_prod_philox_batch_manifold(2, items, m, 64, None))
        else:
            _check(L.kdehip_prod_philox_batch(2, items, 64, None))
        case.sync()
        assert not any(case.torch.isnan(b).any() for b in bufs[0::2])
        outs.append(b"".join(b.cpu().numpy().tobytes() for b in bufs))
    _same(outs)
