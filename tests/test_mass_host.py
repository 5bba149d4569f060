"""The probability mass of a density (include/kdehip.h section 5l) without a GPU: the six new symbols, every refusal the
entries make before they touch a device, the Python front end's refusals, the Julia shim's calls, and the model of
tests/mass_model.py pinned against closed forms.

The refusals that read a resident handle (a mask bit at or above ndims, a circular bounded dimension, per-point bandwidths of
a resident density) need real handles: they are in tests/test_gpu_mass.py; here the resident entries are refused for their
NULL handles."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import mass_model as mm
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_box_mass", "kdehip_box_mass_device", "kdehip_box_mass_device_batch", "kdehip_quantile", "kdehip_quantile_device",
       "kdehip_quantile_device_batch"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    section = hdr[hdr.index("(5l)"):]
    assert hdr.index("(5l)") > hdr.index("(5k)")
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name  # declared under (5l)
    for words in ("kdehip_box_mass_item", "kdehip_quantile_item", "1 - (erfc(-a) + erfc(b)) / 2", "rtsafe", "Not here"):
        assert words in section, words
    for name in ("box_mass", "cdf", "quantile", "median", "interval", "grid_mass", "box_mass_device_batch", "quantile_device_batch"):
        assert callable(getattr(kdehip, name)), name
    for name in ("box_mass", "cdf", "quantile", "interval"):
        assert callable(getattr(kdehip.DeviceDensity, name)), name


def test_item_struct_sizes():
    assert [f for f, _ in _lib.CBoxMassItem._fields_] == ["bd", "d_lo", "d_hi", "Nq", "d_mass", "dim_mask", "circular_mask",
                                                          "reserved_"]
    assert C.sizeof(_lib.CBoxMassItem) == 56
    assert [f for f, _ in _lib.CQuantileItem._fields_] == ["bd", "d_alpha", "Nq", "d_x", "d_resid", "d_iters", "d_converged", "dim",
                                                           "circular_mask"]
    assert C.sizeof(_lib.CQuantileItem) == 64


def test_version_stays_600():
    assert kdehip.version() == 600


def _density(D=2, N=20, bw=0.3, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw])


def _u8(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint8)
    return a, _lib.ptr(a, _lib.u8p)


def _mass(p, mask=1, Nq=3, lo=True, hi=True, out=True, man=None):
    n = max(Nq, 1)
    lo_a, hi_a, m = np.zeros((n, 8)), np.ones((n, 8)), np.zeros(n)
    return L.kdehip_box_mass(None if p is None else C.byref(p._cstruct()), mask, _lib.ptr(lo_a, _lib.f64p) if lo else None,
                             _lib.ptr(hi_a, _lib.f64p) if hi else None, Nq, _lib.ptr(m, _lib.f64p) if out else None,
                             NO_SUCH_DEVICE, man)


def _quant(p, dim=0, Nq=3, alpha=True, tol=0.0, max_iter=0, x=True, full=True, man=None):
    n = max(Nq, 1)
    a, xo, r = np.full(n, 0.5), np.zeros(n), np.zeros(n)
    it, cv = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    tolp = None if tol is None else C.byref(C.c_double(tol))
    return L.kdehip_quantile(None if p is None else C.byref(p._cstruct()), dim, _lib.ptr(a, _lib.f64p) if alpha else None, Nq,
                             tolp, max_iter, _lib.ptr(xo, _lib.f64p) if x else None, _lib.ptr(r, _lib.f64p) if full else None,
                             _lib.ptr(it, _lib.i32p) if full else None, _lib.ptr(cv, _lib.i32p) if full else None,
                             NO_SUCH_DEVICE, man)


def test_null_arguments_are_refused():
    p = _density()
    assert _mass(None) == _lib.ERR_ARG
    assert _mass(p, lo=False) == _lib.ERR_ARG and _mass(p, hi=False) == _lib.ERR_ARG and _mass(p, out=False) == _lib.ERR_ARG
    assert _quant(None) == _lib.ERR_ARG
    assert _quant(p, alpha=False) == _lib.ERR_ARG and _quant(p, x=False) == _lib.ERR_ARG
    a = C.c_void_p(256)
    assert L.kdehip_box_mass_device(None, 1, a, a, 1, a, None, None) == _lib.ERR_ARG
    assert L.kdehip_quantile_device(None, 0, a, 1, None, 0, a, a, a, a, None, None) == _lib.ERR_ARG
    for fn, item in ((L.kdehip_box_mass_device_batch, _lib.CBoxMassItem), ):
        assert fn(1, None, None) == _lib.ERR_ARG and fn(-1, None, None) == _lib.ERR_ARG
        assert fn(1, (item * 1)(), None) == _lib.ERR_ARG  # a null handle
    fn = L.kdehip_quantile_device_batch
    assert fn(1, None, None, 0, None) == _lib.ERR_ARG and fn(-1, None, None, 0, None) == _lib.ERR_ARG
    assert fn(1, (_lib.CQuantileItem * 1)(), None, 0, None) == _lib.ERR_ARG


def test_a_negative_count_is_refused():
    assert _mass(_density(), Nq=-1) == _lib.ERR_ARG
    assert _quant(_density(), Nq=-1) == _lib.ERR_ARG


def test_a_bad_mask_or_dimension_is_refused():
    p = _density()  # D = 2
    for mask in (0, 1 << 2, 0b101, 1 << 31, 1 << 40):
        assert _mass(p, mask=mask) == _lib.ERR_ARG and "dim_mask" in L.kdehip_last_error().decode()
    for dim in (-1, 2, 8):
        assert _quant(p, dim=dim) == _lib.ERR_ARG and "dim" in L.kdehip_last_error().decode()


def test_a_manifold_byte_above_one_is_refused():
    keep, bad = _u8([0, 2])
    assert _mass(_density(), man=bad) == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()
    assert _quant(_density(), man=bad) == _lib.ERR_ARG and "manifold" in L.kdehip_last_error().decode()


def test_a_bad_tolerance_or_iteration_count_is_refused():
    p = _density()
    for tol in (-1e-12, 1e-15, math.nan, math.inf):
        assert _quant(p, tol=tol) == _lib.ERR_ARG and "tol" in L.kdehip_last_error().decode()
    assert _quant(p, max_iter=-1) == _lib.ERR_ARG and "max_iter" in L.kdehip_last_error().decode()
    assert L.kdehip_quantile_device_batch(0, None, C.byref(C.c_double(1e-15)), 0, None) == _lib.ERR_ARG


def test_dimensions_outside_one_to_eight_are_unsupported():
    assert _mass(_density(D=9, N=5)) == _lib.ERR_UNSUPPORTED
    assert _quant(_density(D=9, N=5)) == _lib.ERR_UNSUPPORTED


def test_a_circular_bounded_dimension_is_unsupported_and_an_unbounded_one_is_fine():
    p = _density()
    keep, circ0 = _u8([1, 0])
    assert _mass(p, mask=0b01, man=circ0) == _lib.ERR_UNSUPPORTED and "circular" in L.kdehip_last_error().decode()
    assert _mass(p, mask=0b11, man=circ0) == _lib.ERR_UNSUPPORTED
    assert _quant(p, dim=0, man=circ0) == _lib.ERR_UNSUPPORTED and "circular" in L.kdehip_last_error().decode()
    for call in (lambda: _mass(p, mask=0b10, man=circ0), lambda: _quant(p, dim=1, man=circ0)):  # as far as the device
        assert call() in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE) and "device" in L.kdehip_last_error().decode().lower()


def test_per_point_bandwidths_are_unsupported_in_evaluates_words():
    p = _density(seed=5)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    out = np.zeros(1)
    pos = np.zeros((1, D))
    assert L.kdehip_evaluate(C.byref(p._cstruct()), _lib.ptr(pos, _lib.f64p), 1, 0, _lib.ptr(out, _lib.f64p),
                             NO_SUCH_DEVICE) == _lib.ERR_UNSUPPORTED
    words = L.kdehip_last_error().decode()
    assert _mass(p) == _lib.ERR_UNSUPPORTED and L.kdehip_last_error().decode() == words
    assert _quant(p) == _lib.ERR_UNSUPPORTED and L.kdehip_last_error().decode() == words


def test_nothing_to_do_is_ok():
    p = _density()
    assert _mass(p, Nq=0) == _lib.KDEHIP_OK and _mass(p, Nq=0, lo=False, hi=False) == _lib.KDEHIP_OK
    assert _quant(p, Nq=0) == _lib.KDEHIP_OK and _quant(p, Nq=0, alpha=False) == _lib.KDEHIP_OK
    assert L.kdehip_box_mass_device_batch(0, None, None) == _lib.KDEHIP_OK
    assert L.kdehip_quantile_device_batch(0, None, None, 0, None) == _lib.KDEHIP_OK


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    for D in (1, 2, 8):
        p = _density(D=D)
        for mask in (1, (1 << D) - 1, 1 << (D - 1)):
            assert _mass(p, mask=mask) in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in L.kdehip_last_error().decode().lower()
        for kw in (dict(), dict(tol=None), dict(tol=1e-14, max_iter=1), dict(dim=D - 1, full=False)):
            assert _quant(p, **kw) in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
            assert "device" in L.kdehip_last_error().decode().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake._host = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    fake.manifold = None
    return fake


def test_python_front_end_refusals():
    p, fake = _density(), _fake_device_density()
    for fn in (lambda: kdehip.box_mass(None, 0.0, 1.0), lambda: kdehip.cdf(np.zeros(3), 0.0, 0), lambda: kdehip.quantile([p], 0.5, 0),
               lambda: kdehip.median(None, 0), lambda: kdehip.interval("p", 0), lambda: kdehip.grid_mass(None, [[0.0, 1.0]], [0]),
               lambda: kdehip.box_mass_device_batch([dict(density=p)]), lambda: kdehip.quantile_device_batch([dict(density=p)])):
        with pytest.raises(TypeError):
            fn()
    for d in (p, fake):
        for fn in (lambda: kdehip.box_mass(d, [0.0], [1.0], dims=[2]), lambda: kdehip.box_mass(d, [0.0], [1.0], dims=[]),
                   lambda: kdehip.box_mass(d, [[0.0], [0.0]], [[1.0], [1.0]], dims=[0, 0]),
                   lambda: kdehip.box_mass(d, np.zeros((3, 4)), np.ones((3, 4))),          # nb rows
                   lambda: kdehip.box_mass(d, np.zeros((2, 4)), np.ones((2, 5))),
                   lambda: kdehip.box_mass(d, 0.0, 1.0, dims=[0], manifold=[0, 2]),
                   lambda: kdehip.box_mass(d, 0.0, 1.0, dims=[0], manifold=[1]),            # one entry per dimension
                   lambda: kdehip.cdf(d, 0.0, 2), lambda: kdehip.cdf(d, 0.0, [0, 1]),
                   lambda: kdehip.quantile(d, 0.5, -1), lambda: kdehip.quantile(d, 0.5, 0, tol=1e-15),
                   lambda: kdehip.quantile(d, 0.5, 0, tol=-1.0), lambda: kdehip.quantile(d, 0.5, 0, max_iter=-1),
                   lambda: kdehip.interval(d, 0, 1.0), lambda: kdehip.interval(d, 0, 0.0),
                   lambda: kdehip.grid_mass(d, [[0.0, 1.0]], [0, 1]), lambda: kdehip.grid_mass(d, [[0.0]], [0])):
            with pytest.raises(ValueError):
                fn()


def test_batches_refuse_tensors_that_are_not_on_a_device():
    """the type, device and layout of every tensor are checked before the library is called"""
    import torch
    fake = _fake_device_density()
    z = torch.zeros((3, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        kdehip.box_mass_device_batch([dict(density=fake, lo=z, hi=z, mass=torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError):
        kdehip.quantile_device_batch([dict(density=fake, dim=0, alpha=torch.zeros(3, dtype=torch.float64),
                                           x=torch.zeros(3, dtype=torch.float64))])


def test_julia_shim_calls_the_new_entries_as_the_header_declares_them():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    for name, count in (("kdehip_box_mass", 8), ("kdehip_quantile", 12)):
        m = re.search(r"ccall\(\(:" + name + r",\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
        assert m, name
        types = [t.strip() for t in m.group(1).split(",") if t.strip()]
        assert len(types) == len(params[name]) == count
        for jt, ct in zip(types, params[name]):
            assert ct in shim.JULIA_TO_C[jt], (name, jt, ct)
    for fn in ("hip_box_mass", "hip_quantile"):
        assert re.search(r"\bfunction " + fn + r"\(", code), fn
        body = code[code.index("function " + fn + "("):]
        assert "manifold_bytes(" in body[:body.index("\nend")]


# ---- the model itself ----------------------------------------------------------------------------------------------------
def _model_density(D, N, seed):
    """two clusters, non-uniform weights with one zero"""
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 1.5, size=(D, 1))
    pts[:, N // 2:] += 3.0
    w = rng.uniform(0.05, 1.0, size=N)
    w[N // 3] = 0.0
    sd = rng.uniform(0.3, 0.6, size=D)
    return pts, w / w.sum(), sd * sd


def test_model_one_point_against_erfc_by_hand():
    dens = (np.array([[0.25], [-1.25]]), np.array([1.0]), np.array([0.04, 0.09]))
    s0, s1 = 1.0 / math.sqrt(0.08), 1.0 / math.sqrt(0.18)
    # dimension 0: a box right of the centre; dimension 1: one that holds it
    f0 = (math.erfc((0.3 - 0.25) * s0) - math.erfc((0.6 - 0.25) * s0)) / 2.0
    f1 = 1.0 - (math.erfc(-((-1.5 + 1.25) * s1)) + math.erfc((-1.0 + 1.25) * s1)) / 2.0
    assert mm.box_mass(dens, [[0.3], [-1.5]], [[0.6], [-1.0]])[0] == f0 * f1
    assert mm.box_mass(dens, [[0.3]], [[0.6]], [0])[0] == f0
    # left of the centre, by symmetry the same bits
    assert mm.box_mass(dens, [[0.25 - 0.35]], [[0.25 - 0.05]], [0])[0] == pytest.approx(f0, rel=1e-14)
    assert mm.cdf(dens, 0.25, 0) == 0.5 and mm.pdf(dens, 0.25, 0) == pytest.approx(1.0 / math.sqrt(2 * math.pi * 0.04), rel=1e-14)


def test_model_an_empty_box_is_exactly_zero_and_a_nan_bound_is_nan():
    dens = _model_density(3, 40, 1)
    assert mm.box_mass(dens, [[0.5], [-1.0], [-1.0]], [[0.5], [1.0], [1.0]])[0] == 0.0      # degenerate in one dimension
    assert mm.box_mass(dens, [[0.7], [-1.0], [-1.0]], [[0.5], [1.0], [1.0]])[0] == 0.0      # reversed
    assert mm.box_mass(dens, [[math.inf]], [[math.inf]], [1])[0] == 0.0
    assert math.isnan(mm.box_mass(dens, [[math.nan]], [[1.0]], [2])[0])


@pytest.mark.parametrize("D", [1, 3, 6, 8])
def test_model_all_infinite_bounds_give_the_sum_of_the_weights(D):
    pts, w, v = _model_density(D, 130, D)
    w = w * 0.75
    got = mm.box_mass((pts, w, v), np.full((D, 1), -math.inf), np.full((D, 1), math.inf))[0]
    assert got == math.fsum(w)


def test_model_grid_partition_sums_to_one():
    dens = _model_density(3, 130, 9)
    edges = [np.concatenate([[-math.inf], np.linspace(-2.0, 5.0, 5), [math.inf]])] * 3   # 6 x 6 x 6 cells
    lo = np.stack([g.reshape(-1) for g in np.meshgrid(*[e[:-1] for e in edges], indexing="ij")])
    hi = np.stack([g.reshape(-1) for g in np.meshgrid(*[e[1:] for e in edges], indexing="ij")])
    cells = mm.box_mass(dens, lo, hi)
    assert cells.shape == (216,) and np.all(cells >= 0.0)
    assert abs(math.fsum(cells) - 1.0) <= 1e-12


def test_model_cdf_is_monotone_and_is_the_box_mass_from_minus_infinity():
    dens = _model_density(2, 60, 4)
    xs = np.linspace(-6.0, 9.0, 200)
    F = np.array([mm.cdf(dens, x, 1) for x in xs])
    assert np.all(np.diff(F) >= 0.0) and F[0] < 1e-12 and abs(F[-1] - 1.0) < 1e-12
    for x in xs[::40]:
        assert mm.box_mass(dens, [[-math.inf]], [[x]], [1])[0] == pytest.approx(mm.cdf(dens, x, 1), rel=1e-14, abs=1e-300)


@pytest.mark.parametrize("alpha", [1e-9, 0.025, 0.5, 0.975, 1.0 - 1e-9])
def test_model_quantile_residual_is_within_tol(alpha):
    dens = _model_density(2, 60, 6)
    for tol in (1e-12, 1e-14):
        x, r, iters, conv = mm.quantile(dens, alpha, 0, tol=tol)
        assert conv and abs(r) <= tol and 1 <= iters <= 100 and abs(mm.cdf(dens, x, 0) - alpha) <= tol
    x1, r1, it1, c1 = mm.quantile(dens, alpha, 0, max_iter=1)
    live = dens[0][0, dens[1] > 0]
    assert it1 == 1 and not c1 and x1 == 0.5 * ((live.min() - 39 * math.sqrt(dens[2][0])) + (live.max() + 39 * math.sqrt(dens[2][0])))
    assert math.isnan(mm.quantile(dens, 0.0, 0)[0]) and math.isnan(mm.quantile(dens, 1.0, 0)[0]) and math.isnan(mm.quantile(dens, math.nan, 0)[0])
