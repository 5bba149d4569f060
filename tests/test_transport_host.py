"""Entropic optimal transport (include/kdehip.h section 5s) without a GPU: the three new symbols, every refusal the entries
make before they touch a device, the Python front end's refusals, the Julia shim's calls, and the model of
tests/transport_model.py pinned against a problem whose unregularised answer is known in closed form.

The refusals that read a resident handle (ndims that differ, a mask bit at or above ndims, per-point bandwidths without a
scale, a resident density without a weighted leaf) need real handles: they are in tests/test_gpu_transport.py; here the resident
entries are refused for their NULL handles."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import test_julia_shim_syntax as shim
from tests import transport_model as tm

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_sinkhorn", "kdehip_sinkhorn_device", "kdehip_sinkhorn_device_batch"]
METHODS = ["sinkhorn", "sinkhorn_divergence", "transport_map", "transport_to", "equalize"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    section = hdr[hdr.index("(5s)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name  # declared under (5s)
    assert "kdehip_sinkhorn_item" in section
    from kdehip import transport
    for name in METHODS:
        assert callable(getattr(kdehip.BallTreeDensity, name)), name
        assert callable(getattr(kdehip.DeviceDensity, name)), name
        assert callable(getattr(transport, name)), name
    assert callable(kdehip.DeviceDensity.sinkhorn_batch) and callable(transport.sinkhorn_batch)
    for name in METHODS + ["sinkhorn_batch"]:
        assert not hasattr(kdehip, name), name  # the surface is methods: no new name in the package


def test_version_stays_600():
    assert kdehip.version() == 600


def test_the_item_struct_has_the_headers_layout():
    """p, q, scale, scale_p, scale_q, reg, tol, four scalar results, iters, four vectors: 16 eight-byte fields, then two words
    (csrc/sinkhorn.hip asserts the same size of the C struct)"""
    assert C.sizeof(_lib.CSinkhornItem) == 16 * 8 + 8
    assert _lib.CSinkhornItem.maxiter.offset == 16 * 8 and _lib.CSinkhornItem.circular_mask.offset == 16 * 8 + 4


def _density(D=2, N=20, bw=0.3, seed=3, w=None):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw], w)


def _d(x):
    """a double by pointer, as the entries take reg and tol; None stays NULL"""
    return None if x is None else C.byref(C.c_double(x))


def _call(p, q, scale=None, reg=1.0, tol=1e-6, maxiter=5, man=None, miss=None, device=NO_SUCH_DEVICE):
    vals, it = np.zeros(4), np.zeros(1, dtype=np.int32)
    out = {k: C.cast(vals[j:].ctypes.data, _lib.f64p) for j, k in enumerate(("value", "transport_cost", "err", "mass"))}
    out["iters"] = _lib.ptr(it, _lib.i32p)
    if miss:
        out[miss] = None
    s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    cp = None if p is None else C.byref(p._cstruct())
    cq = cp if q is p else None if q is None else C.byref(q._cstruct())
    return L.kdehip_sinkhorn(cp, cq, _lib.optr(s, _lib.f64p), _d(reg), _d(tol), maxiter, out["value"], out["transport_cost"], out["err"],
                             out["mass"], out["iters"], None, None, None, None, device, man)


def _words():
    return L.kdehip_last_error().decode()


def test_null_arguments_are_refused():
    p, q = _density(), _density(seed=4)
    assert _call(None, q) == _lib.ERR_ARG and _call(p, None) == _lib.ERR_ARG
    for miss in ("value", "transport_cost", "err", "mass", "iters"):
        assert _call(p, q, miss=miss) == _lib.ERR_ARG, miss
    assert _call(p, q, reg=None) == _lib.ERR_ARG and _call(p, q, tol=None) == _lib.ERR_ARG
    d1, i1 = _lib.ptr(np.zeros(4), _lib.f64p), _lib.ptr(np.zeros(1, dtype=np.int32), _lib.i32p)
    assert L.kdehip_sinkhorn_device(None, None, None, _d(1.0), _d(1e-6), 5, d1, d1, d1, d1, i1, None, None, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_sinkhorn_device_batch(1, None) == _lib.ERR_ARG
    assert L.kdehip_sinkhorn_device_batch(-1, None) == _lib.ERR_ARG
    items = (_lib.CSinkhornItem * 1)()  # null handles
    assert L.kdehip_sinkhorn_device_batch(1, items) == _lib.ERR_ARG


def test_dimensions_that_differ_or_exceed_eight_are_refused():
    assert _call(_density(D=2), _density(D=3)) == _lib.ERR_ARG and "ndims" in _words()
    assert _call(_density(D=9, N=5), _density(D=9, N=5, seed=4)) == _lib.ERR_ARG and "ndims" in _words()


@pytest.mark.parametrize("bad", [0.0, -1.0, np.inf, -np.inf, np.nan])
def test_a_bad_reg_is_refused(bad):
    assert _call(_density(), _density(seed=4), reg=bad) == _lib.ERR_ARG and "reg" in _words()


@pytest.mark.parametrize("bad", [0.0, -0.5, np.inf, np.nan, 1e-200, 1e200])
def test_a_bad_scale_entry_is_refused(bad):
    """not finite or <= 0 -- and an entry whose square, which the cost divides by, is 0 or not finite"""
    assert _call(_density(), _density(seed=4), scale=[0.3, bad]) == _lib.ERR_ARG and "scale" in _words()


@pytest.mark.parametrize("bad", [-1e-300, -1.0, -np.inf, np.nan])
def test_a_bad_tolerance_is_refused(bad):
    assert _call(_density(), _density(seed=4), tol=bad) == _lib.ERR_ARG and "tol" in _words()


def test_a_negative_step_count_is_refused():
    assert _call(_density(), _density(seed=4), maxiter=-1) == _lib.ERR_ARG and "maxiter" in _words()


def test_a_side_without_a_weighted_leaf_is_refused():
    p = _density()
    none = p.changeWeights(np.zeros(20))
    for a, b in ((p, none), (none, p), (none, none)):
        assert _call(a, b) == _lib.ERR_ARG and "positive weight" in _words()


def test_a_manifold_byte_above_one_is_refused():
    bad = np.array([0, 2], dtype=np.uint8)
    assert _call(_density(), _density(seed=4), man=_lib.ptr(bad, _lib.u8p)) == _lib.ERR_ARG and "manifold" in _words()


def test_per_point_bandwidths_need_an_explicit_scale():
    p, q = _density(), _density(seed=5)
    N, D = q.bt.num_points, q.bt.dims
    q.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    for a, b in ((p, q), (q, p)):
        assert _call(a, b) == _lib.ERR_ARG and "per-point" in _words()
        rc = _call(a, b, scale=[0.5, 0.5])   # with a scale the call gets as far as the device
        assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE) and "device" in _words().lower()


def test_two_to_the_31_points_are_refused():
    """a struct that claims 2^31 points (its arrays are never read: the size is checked first)"""
    p = _density()
    big = _lib.CDensity.from_buffer_copy(p._cstruct())
    big.npts = 2 ** 31
    vals, it = np.zeros(4), np.zeros(1, dtype=np.int32)
    o = [C.cast(vals[j:].ctypes.data, _lib.f64p) for j in range(4)]
    one = np.ones(2)
    for a, b in ((big, p._cstruct()), (p._cstruct(), big)):
        rc = L.kdehip_sinkhorn(C.byref(a), C.byref(b), _lib.ptr(one, _lib.f64p), _d(1.0), _d(1e-6), 5, *o, _lib.ptr(it, _lib.i32p), None, None,
                               None, None, NO_SUCH_DEVICE, None)
        assert rc == _lib.ERR_ARG and "2^31" in _words()


def test_nothing_to_do_is_ok():
    assert L.kdehip_sinkhorn_device_batch(0, None) == _lib.KDEHIP_OK


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p, q = _density(), _density(seed=4)
    circ = np.array([1, 0], dtype=np.uint8)
    for rc in (_call(p, q), _call(p, p), _call(p, q, scale=[0.2, 0.4]), _call(p, q, tol=0.0, maxiter=0), _call(p, q, tol=np.inf),
               _call(p, q, man=_lib.ptr(circ, _lib.u8p))):
        assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
        assert "device" in _words().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake._host = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    fake.manifold = None
    return fake


def test_python_front_end_refusals():
    p, q, fake = _density(), _density(seed=4), _fake_device_density()
    with pytest.raises(TypeError):
        p.sinkhorn(fake)                              # one of each kind
    with pytest.raises(TypeError):
        p.sinkhorn(np.zeros((2, 3)))
    with pytest.raises(TypeError):
        kdehip.DeviceDensity.sinkhorn_batch([(p, q)])   # a batch takes resident densities
    with pytest.raises(ValueError):
        p.sinkhorn(_density(D=3))
    for d, e in ((p, q), (fake, fake)):
        for kw in (dict(reg=0.0), dict(reg=math.nan), dict(tol=-1.0), dict(tol=math.nan), dict(maxiter=-1), dict(scale=[0.3]),
                   dict(manifold=[1]), dict(manifold=[0, 2])):
            for name in ("sinkhorn", "sinkhorn_divergence", "transport_map", "transport_to"):
                with pytest.raises(ValueError):
                    getattr(d, name)(e, **kw)
    with pytest.raises(ValueError):
        kdehip.DeviceDensity.sinkhorn_batch([(fake, fake)], reg=-1.0)
    assert kdehip.DeviceDensity.sinkhorn_batch([]) == []
    assert p.sinkhorn_divergence(p) == 0.0 and fake.sinkhorn_divergence(fake) == 0.0   # by definition, without a launch


def test_julia_shim_calls_the_new_entry_as_the_header_declares_it():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    m = re.search(r"ccall\(\(:kdehip_sinkhorn,\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
    assert m
    types = [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert len(types) == len(params["kdehip_sinkhorn"]) == 17
    for jt, ct in zip(types, params["kdehip_sinkhorn"]):
        assert ct in shim.JULIA_TO_C[jt], (jt, ct)
    for fn in ("hip_sinkhorn", "hip_sinkhorn_divergence", "hip_transport_map"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    body = code[code.index("function hip_sinkhorn("):]
    assert "manifold_bytes(" in body[:body.index("\nend")]


# ---- the model itself ----------------------------------------------------------------------------------------------------
def _line_pair():
    rng = np.random.default_rng(5)
    x = np.sort(rng.standard_normal(200))[None, :]
    y = np.sort(1.5 + 0.7 * rng.standard_normal(200))[None, :]
    return x, y, np.full(200, 1.0 / 200), np.array([0.5])


@pytest.mark.parametrize("reg", [4.0, 1.0, 0.25])
def test_model_chain_of_inequalities_on_the_line(reg):
    """200 sorted, equally weighted points a side: W = 1/2 mean((x_sorted - y_sorted)^2 / s^2) is the unregularised optimum, and
    W <= <pi, c> (pi is a coupling, up to its row error) <= value (= <pi, c> + eps KL at convergence) <= <a x b, c> (the value
    of the independent coupling, whose KL term is 0)"""
    x, y, a, s = _line_pair()
    r = tm.iterate((x, a), (y, a), s, reg, 1e-9, 5000)
    W = tm.unregularised_1d(x, y, s[0])
    indep = float((tm.cost(x, y, s) * a[:, None] * a[None, :]).sum())
    print(f"reg {reg}: {r['iters']} steps, W {W:.4f} <= {r['transport_cost']:.4f} <= {r['value']:.4f} <= {indep:.4f}")
    assert r["iters"] > 0
    assert W <= r["transport_cost"] <= r["value"] <= indep
    assert abs(tm.unregularised_1d_weighted(x, a, y, a, s[0]) - W) <= 1e-12 * W


def test_model_plan_marginals_and_mean_at_convergence():
    x, y, a, s = _line_pair()
    r = tm.iterate((x, a), (y, a), s, 1.0, 1e-10, 5000)
    P = tm.plan((x, a), (y, a), s, 1.0, r["phi"], r["gamma"])
    assert np.abs(P.sum(axis=0) - a).max() <= 1e-14 and np.abs(P.sum(axis=1) - a).sum() <= 2e-10
    assert abs(P.sum() - r["mass"]) <= 1e-13
    assert abs(float((P * tm.cost(x, y, s)).sum()) - r["transport_cost"]) <= 1e-12 * r["transport_cost"]
    assert abs(float((r["map"] * a).sum()) - float((y * a).sum())) <= 1e-9


def test_model_self_item_is_symmetric_and_the_divergence_vanishes_on_a_copy():
    (x, a), (y, b) = tm.two_clusters_pair(2, 60, 50)
    s = np.array([0.7, 0.9])
    r = tm.iterate((x, a), None, s, 1.0, 1e-10, 5000)
    assert 0 < r["iters"] < 100 and np.array_equal(r["phi"], r["gamma"])
    S, (pq, pp, qq) = tm.divergence((x, a), (x.copy(), a.copy()), s, 1.0, 1e-10, 5000)
    assert abs(S) <= 1e-8 and abs(pq["value"] - pp["value"]) <= 1e-8
    S2, _ = tm.divergence((x, a), (y, b), s, 1.0, 1e-10, 5000)
    assert S2 > 0.01


def test_model_weightless_points_take_no_part_but_move():
    (x, a), (y, b) = tm.two_clusters_pair(2, 60, 50)
    s = np.array([0.7, 0.9])
    r = tm.iterate((x, a), (y, b), s, 1.0, 1e-9, 5000)
    y2 = y.copy()
    y2[:, ::5] += 100.0                                     # b's weightless points, moved far away: nothing changes
    r2 = tm.iterate((x, a), (y2, b), s, 1.0, 1e-9, 5000)
    assert r2["iters"] == r["iters"] and np.array_equal(r2["phi"], r["phi"]) and r2["value"] == r["value"]
    assert np.all(np.isfinite(r["map"][:, ::5])) and np.all(np.isfinite(r["phi"][::5]))   # a's weightless points have images


def test_model_angle_pair_across_the_cut_of_the_circle():
    """the premise of the GPU test of the same data: on the circle the two clusters are 0.3 apart, on the line some pairs are 2 pi apart"""
    (x, a), (y, b) = tm.angle_pair()
    s = np.array([0.5, 0.3])
    assert np.abs(tm.diffs(x, y)[1]).max() > math.pi and np.abs(tm.diffs(x, y, [0, 1])[1]).max() < 2.0
    circle = tm.iterate((x, a), (y, b), s, 1.0, 1e-6, 5000, [0, 1])
    line = tm.iterate((x, a), (y, b), s, 1.0, 1e-6, 5000)
    assert circle["iters"] > 0 and line["value"] > 2.0 * circle["value"]
    assert np.all(circle["map"][1] >= -math.pi) and np.all(circle["map"][1] < math.pi)
    shifted = tm.iterate((x + np.array([[0.0], [2.0 * math.pi]]), a), (y, b), s, 1.0, 1e-6, 5000, [0, 1])
    assert abs(shifted["value"] - circle["value"]) <= 1e-9


def _rel13(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = 1e-13 * np.maximum(1.0, np.abs(want))
    assert np.all(np.abs(got - want) <= bound), (name, float(np.max(np.abs(got - want) / bound)))


@pytest.mark.parametrize("rows", [128, 1024])
@pytest.mark.parametrize("self_item", [False, True])
def test_model_blocked_iteration_equals_the_dense_one(self_item, rows):
    """(2, 300, 257): 128 rows a block gives three blocks a side, the last one partial; 1024 is the default (one block).  1e-13
    relative to max(1, |.|): the blocks add the same numbers, and only the second half-step differs in how it is written
    (the rows of the transposed cost from diff(y, x) in the place of the columns of the cost from diff(x, y))"""
    (x, a), (y, b) = tm.two_clusters_pair(2, 300, 257)
    s = np.array([0.7, 0.9])
    q = None if self_item else (y, b)
    for maxiter, tol in ((3, 0.0), (1000, 1e-6)):
        want = tm.iterate((x, a), q, s, 2.0, tol, maxiter)
        got = tm.iterate_blocked((x, a), q, s, 2.0, tol, maxiter, rows=rows)
        assert got["iters"] == want["iters"] and len(got["errs"]) == len(want["errs"])
        for name in ("phi", "gamma", "delta", "map", "value", "transport_cost", "err", "mass", "errs"):
            _rel13(name, got[name], want[name])
    (ax, aa), (ay, ab) = tm.angle_pair()
    want = tm.iterate((ax, aa), (ay, ab), np.array([0.5, 0.3]), 1.0, 0.0, 4, [0, 1])
    got = tm.iterate_blocked((ax, aa), (ay, ab), np.array([0.5, 0.3]), 1.0, 0.0, 4, [0, 1], rows=16)
    for name in ("phi", "gamma", "delta", "map", "value", "transport_cost", "err", "mass"):
        _rel13("circular " + name, got[name], want[name])


_LAW_K = (-80, -30, 30, 80)
_BITS0 = ("phi", "gamma", "value", "transport_cost", "err", "mass", "iters")


def _law_pair(lattice):
    """(5, 257, 129), every fifth weight 0; lattice: every coordinate a multiple of 2^-20"""
    (x, a), (y, b) = tm.two_clusters_pair(5, 257, 129)
    s = np.random.default_rng(12).uniform(0.5, 1.5, size=5)
    if lattice:
        x, y = np.round(x * 2.0 ** 20) / 2.0 ** 20, np.round(y * 2.0 ** 20) / 2.0 ** 20
    return (x, a), (y, b), s


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()


@pytest.mark.parametrize("self_item", [False, True])
def test_model_obeys_the_rescaling_laws_of_the_equivariance_table(self_item):
    """the laws tests/equivariance_cases.py states for the `transport` row, in the model itself -- so that a wrong law is told
    apart from a wrong kernel: with the points and the scale multiplied by 2^k exactly, every difference, its square and the
    factor 1 / (2 s^2) scale exactly, the cost keeps its bits, and with it the potentials and every scalar; the displacement
    and the map are the base's times 2^k"""
    (x, a), (y, b), s = _law_pair(False)
    q = None if self_item else (y, b)
    base = tm.iterate((x, a), q, s, 1.0, 0.0, 8)
    assert base["iters"] == -8
    for k in _LAW_K:
        qk = None if self_item else (np.ldexp(y, k), b)
        got = tm.iterate((np.ldexp(x, k), a), qk, np.ldexp(s, k), 1.0, 0.0, 8)
        for name in _BITS0:
            assert _bits(got[name]) == _bits(base[name]), (k, name)
        for name in ("delta", "map"):
            assert _bits(got[name]) == _bits(np.ldexp(base[name], k)), (k, name)


@pytest.mark.parametrize("self_item", [False, True])
def test_model_obeys_the_translation_laws_of_the_equivariance_table(self_item):
    """inputs on the 2^-20 lattice below 2^6 and offsets of +-2^20, +-3 2^19: x + t is exact, every difference is the
    untranslated one, so all that is formed from differences keeps its bits; the map is a position -- fl(x + t + m) is within
    half a spacing of doubles at 2^20 of fl(x + m) + t"""
    (x, a), (y, b), s = _law_pair(True)
    assert np.abs(x).max() < 2.0 ** 6 and np.abs(y).max() < 2.0 ** 6
    t = np.array([2.0 ** 20, -3.0 * 2.0 ** 19, 3.0 * 2.0 ** 19, -2.0 ** 20, 2.0 ** 20])[:, None]
    assert np.array_equal((x + t) - t, x) and np.array_equal((y + t) - t, y)
    base = tm.iterate((x, a), None if self_item else (y, b), s, 1.0, 0.0, 8)
    got = tm.iterate((x + t, a), None if self_item else (y + t, b), s, 1.0, 0.0, 8)
    for name in _BITS0 + ("delta",):
        assert _bits(got[name]) == _bits(base[name]), name
    sp = float(np.spacing(np.abs(got["map"]).max()))
    assert sp == 2.0 ** -32 and np.abs((got["map"] - t) - base["map"]).max() <= sp
