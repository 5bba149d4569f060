"""Evaluation within a tolerance (include/kdehip.h section 5m) without a GPU: the rule as tests/evaltol_model.py restates it
holds its own bound against a direct math.fsum sum; the two new symbols, the refusals the entries make before they touch a
device, and the switch `setForceEvalDirect`.

The model's bound: p (1 - rel_tol) - abs_tol - 1e-12 p <= p_hat <= p (1 + 1e-12), p one math.fsum per query of the same
terms.  1e-12 is the project's tolerance for sums of positive terms (tests/test_gpu_ksum.py): the model adds at most 8200
terms, which one after the other would be 8200 ulp = 9.1e-13 (numpy's pairwise sums do better)."""
import ctypes as C
import os

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import evaltol_model as em

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_evaluate_tol", "kdehip_evaluate_device_at_tol"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
# (D, N, Nq) of tests/test_gpu_evaltol.py
SHAPES = [(1, 5, 3), (2, 129, 257), (3, 300, 7), (6, 257, 5), (8, 130, 3), (2, 8200, 300)]


def leaf_arrays(p):
    """(leaf centres (N, D), leaf weights, variances, 0-based original position of each leaf) of a host density"""
    N, D = p.bt.num_points, p.bt.dims
    return (np.ascontiguousarray(p.bt.centers[N * D:].reshape(N, D)), p.bt.weights[N:].copy(),
            p.bandwidth[N * D:(N + 1) * D].copy(), p.bt.permutation[N:] - 1)


def density(rng, D, N):
    """the density of tests/test_gpu_mass.py::_density: two clusters, non-uniform weights with one exact zero"""
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))
    pts[:, N // 2:] += 3.0
    w = rng.uniform(0.05, 1.0, size=N)
    if N > 1:
        w[N // 3] = 0.0
    return kdehip.kde(pts, rng.uniform(0.2, 0.6, size=D), w)


def queries(rng, p, Nq):
    """Nq columns among the data, spread a little"""
    pts = kdehip.getPoints(p)
    return pts[:, rng.integers(0, pts.shape[1], size=Nq)] + 0.3 * rng.standard_normal((pts.shape[0], Nq))


@pytest.mark.parametrize("D,N,Nq", SHAPES)
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("loo", [False, True])
def test_the_models_rule_keeps_its_bound(D, N, Nq, circular, loo):
    rng = np.random.default_rng(7000 * D + 10 * N + Nq)
    p = density(rng, D, N)
    pts, w, v, _ = leaf_arrays(p)
    qry = pts if loo else np.ascontiguousarray(queries(rng, p, Nq).T)
    circ = (D - 1,) if circular else ()
    direct = em.direct_fsum(pts, w, v, qry, loo, circ)
    for rel_tol in (1e-2, 1e-6):
        for abs_tol in (0.0, 1e-30):
            got, stats = em.evaluate_tol(pts, w, v, qry, rel_tol, abs_tol, loo, circ)
            assert 0 < stats[0] <= stats[1] == ((qry.shape[0] + 255) // 256) * ((N + 127) // 128)
            assert np.all(got <= direct * (1.0 + 1e-12))
            assert np.all(got >= direct * (1.0 - rel_tol) - abs_tol - 1e-12 * direct)
    got, stats = em.evaluate_tol(pts, w, v, qry, 0.0, 0.0, loo, circ)
    assert stats[0] == stats[1] and np.all(np.abs(got - direct) <= 1e-12 * direct)


def test_the_model_prunes_separated_clusters_to_a_quarter():
    """the setup of tests/test_gpu_evaltol.py's pruning test in a plain median k-d order: exactly one tile in four"""
    rng = np.random.default_rng(11)
    centres = np.array([[-20.0, -20.0], [-20.0, 20.0], [20.0, -20.0], [20.0, 20.0]])
    pts = np.concatenate([c + rng.standard_normal((256, 2)) for c in centres])  # cluster by cluster: compact 128-leaf runs
    w = np.full(1024, 1.0 / 1024)
    v = np.array([0.09, 0.09])
    pl = em.plan(pts, w, v, pts, 1e-3, 0.0, loo=True)
    assert np.all(pl["L"] > 0.0)
    assert int(pl["visited"].sum()) * 4 == pl["visited"].size


def test_new_symbols_are_exported_and_bound():
    lib = C.CDLL(kdehip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "kdehip.h")).read()
    assert hdr.index("(5m)") > hdr.index("(5l)")
    section = hdr[hdr.index("(5m)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name
    for words in ("a_min", "tau_q", "2^-20", "Not here"):
        assert words in section, words
    for name in ("evaluate_tol", "setForceEvalDirect", "getForceEvalDirect"):
        assert callable(getattr(kdehip, name)), name
    assert callable(kdehip.DeviceDensity.evaluate_tol)
    shim = open(os.path.join(ROOT, "kerneldensityestimate.jl_amd", "julia", "KernelDensityEstimateHIP.jl")).read()
    assert ":kdehip_evaluate_tol" in shim


def _tol(p, rel=1e-3, ab=0.0, Nq=1, loo=0, out=True, dev=NO_SUCH_DEVICE):
    D = 8 if p is None else p.bt.dims
    pos, o, stats = np.zeros((max(Nq, 1), D)), np.zeros(max(Nq, 1, 0 if p is None else p.bt.num_points)), np.zeros(2, dtype=np.int64)
    relp = None if rel is None else C.byref(C.c_double(rel))
    abp = None if ab is None else C.byref(C.c_double(ab))
    return L.kdehip_evaluate_tol(None if p is None else C.byref(p._cstruct()), _lib.ptr(pos, _lib.f64p), Nq, loo, relp, abp,
                                 _lib.ptr(o, _lib.f64p) if out else None, _lib.ptr(stats, _lib.i64p), dev, None)


def _small(D=2, N=20, seed=3):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [0.3])


def test_bad_tolerances_are_refused_before_anything_else():
    p = _small()
    for rel in (-1e-3, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert _tol(p, rel=rel) == _lib.ERR_ARG and "rel_tol" in L.kdehip_last_error().decode(), rel
    for ab in (-1e-30, float("nan"), float("inf")):
        assert _tol(p, ab=ab) == _lib.ERR_ARG and "abs_tol" in L.kdehip_last_error().decode(), ab
    a = C.c_void_p(256)
    for rel, ab in ((-1.0, 0.0), (1.0, 0.0), (float("nan"), 0.0), (1e-3, -1.0), (1e-3, float("inf"))):
        rc = L.kdehip_evaluate_device_at_tol(None, None, C.byref(C.c_double(rel)), C.byref(C.c_double(ab)), a, None, None, None)
        assert rc == _lib.ERR_ARG and "_tol" in L.kdehip_last_error().decode()
    # good tolerances (NULL: the defaults) get as far as the device, which does not exist: the refusal is not theirs
    for rel, ab in ((None, None), (0.0, 0.0), (0.999, 1e300)):
        assert _tol(p, rel=rel, ab=ab) != _lib.KDEHIP_OK and "_tol" not in L.kdehip_last_error().decode()


def test_null_arguments_and_bad_counts_are_refused():
    p = _small()
    assert _tol(None) == _lib.ERR_ARG and _tol(p, out=False) == _lib.ERR_ARG and _tol(p, Nq=-1) == _lib.ERR_ARG
    a = C.c_void_p(256)
    assert L.kdehip_evaluate_device_at_tol(None, None, None, None, a, None, None, None) == _lib.ERR_ARG
    stats = np.full(2, 7, dtype=np.int64)  # no queries: nothing to do, no device
    o = np.zeros(1)
    assert L.kdehip_evaluate_tol(C.byref(p._cstruct()), _lib.ptr(o, _lib.f64p), 0, 0, None, None, _lib.ptr(o, _lib.f64p),
                                 _lib.ptr(stats, _lib.i64p), NO_SUCH_DEVICE, None) == _lib.KDEHIP_OK
    assert stats.tolist() == [0, 0]


def test_per_point_bandwidths_and_nine_dimensions_are_unsupported():
    p = _small(seed=5)
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    assert _tol(p) == _lib.ERR_UNSUPPORTED and "per-point" in L.kdehip_last_error().decode()
    assert _tol(p, loo=1) == _lib.ERR_UNSUPPORTED
    assert _tol(_small(D=9)) == _lib.ERR_UNSUPPORTED


def test_the_switch_defaults_to_direct_and_keeps_its_state():
    assert kdehip.getForceEvalDirect() is True
    try:
        kdehip.setForceEvalDirect(False)
        assert kdehip.getForceEvalDirect() is False
        kdehip.setForceEvalDirect()  # the reference's spelling of "off" is the default argument
        assert kdehip.getForceEvalDirect() is False
        kdehip.setForceEvalDirect(True)
        assert kdehip.getForceEvalDirect() is True
    finally:
        kdehip.setForceEvalDirect(True)


def test_the_front_end_refuses_what_it_cannot_read():
    p = _small()
    with pytest.raises(ValueError):
        kdehip.evaluate_tol(p, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        kdehip.evaluate_tol(p, np.zeros((2, 4)), order="sorted")
    with pytest.raises(TypeError):
        kdehip.evaluate_tol(np.zeros((2, 4)), np.zeros((2, 4)))
    for rel in (-1.0, 1.0, float("nan")):
        with pytest.raises(kdehip.KdeHipError):
            kdehip.evaluate_tol(p, np.zeros((2, 4)), rel_tol=rel, device=NO_SUCH_DEVICE)
