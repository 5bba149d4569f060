"""Every public entry under exact rescaling and exact translation of its data (tests/equivariance_cases.py is the table, and
its docstring derives the laws; tests/test_equivariance_table.py keeps the table complete).

1. Rescaling.  The points, the queries, the bounds and the bandwidths of a case are multiplied by 2^k with np.ldexp,
   k in {-80, -30, +30, +80}.  An output under a bit law equals np.ldexp(base, e * k) under np.array_equal; an output under a
   tolerance law lies within the bound its family's own test module holds it to (copied, with the module named, at `_law`).
   No model enters these comparisons.
2. The base against a reference.  What rescaling proves is "equal to itself, rescaled"; the base result of every case is
   therefore held to its family's model at the family's existing tolerance (the `_check_*` functions, each naming where its
   bound comes from).  The cases are D = 4, 5, 7, 8, so these are also the first comparisons of the D = 4, 5, 7
   instantiations of the all-pairs kernels with a reference outside tests/test_gpu_curvature.py.  Where a model is a Python
   loop per query it runs on `c.sub`, 40 evenly spaced queries (all of them if there are fewer), in every check and at every
   D; every one of the 24 mean-shift starts is held to the model; the bit laws take all queries.  Some of the base's
   references are RELATIONS between the library's own outputs and not independent references, as in the family modules
   they follow: `laplace` against numpy's inverse of the entry's own Hessian (which `_check_hess` holds to the model at the
   queries, not at the starts), the summaries' grids against the package's `summary.grid`, `kde_adaptive` against
   `kde_varbw` of `adaptive_scales`' factors, the searched densities against `kde` of their own bandwidth.  Each says so.
3. The resident route, at k = -80: the call on DeviceDensity arguments returns the host call's bits.  The rows `refit` and
   `transport` make densities; the refit of an UPLOADED density has no arrays to download, so on this route a made density is
   compared by its values at the queries, and the device's own arithmetic (the Bayes update, the batches) runs inside the
   host call on a built twin whose arrays are part of the output.
4. Translation.  The same cases with every coordinate rounded to a multiple of 2^-20, |x| < 2^6, and per dimension an offset
   from +-2^20, +-3 2^19: x + t is exact.  Outputs the table marks "same" are bit for bit the untranslated ones; positions
   ("pos") are held to the family's model run on the translated inputs (the same `_check_*` functions), and to the
   untranslated output plus t within a counted number of spacings of doubles at 2^20 (`_POSITION`, the roundings named there,
   with the worst observed on one MI355X).  Of a tree's arrays the leaves are claimed ("leaves"); the conditional variance
   is "close": held to the model at the family's bound, for the reason at `MODEL_ONLY`.

Premises, asserted before anything is compared, with messages that say what would not be covered:
  * every base value that a law multiplies lies in [2^-150, 2^150] or is exactly 0, so that the scaled value is a normal
    number (the largest exponent is (D + 2) * 80 = 800) -- for the densities from tests/evaltol_model.py's direct sums before
    the library is called.  For the library's other outputs this module DEVIATES from that interval: each is asked, on the
    base output itself and before any scaled call, for what its own exponent needs, 0 or within
    [2^-(1022 - 80 |e|), 2^(1022 - 80 |e|)] -- still sufficient for the scaled value to be a normal number; the arrays of a
    conditioned density hold weights down to 1e-80 and inner-node means in proportion, outside [2^-150, 2^150];
  * the host-built trees at scale 1 and 2^k, and the translated one, have the same permutation, and leaf means and variances
    related exactly (`_tree_premise`).

The shapes: (D, N, Nq) = (4, 129, 257), (5, 257, 129), (7, 129, 257), (8, 130, 3); weighted, every fifth weight 0, a bandwidth
per dimension.  129 leaves one leaf to a second chunk, 257 one lane to a second query block.  The second density of a pair
takes the next case's N."""
import math

import numpy as np
import pytest

import kdehip
from kdehip import refit as rf
from tests import bwjoint_model as bm
from tests import conditional_model as cm
from tests import curvature_model as hm
from tests import equivariance_cases as ec
from tests import evaltol_model as em
from tests import knn_model as nm
from tests import ksum_model as km
from tests import logdensity_model as lm
from tests import mass_model as sm
from tests import modes_model as mm
from tests import prodexact_model as pm
from tests import pymodel
from tests import refit_model as rm
from tests import transport_model as tm
from tests import varbw_model as vm
from tests.helpers import density_arrays
from tests.test_refit_host import bayes_reference

pytestmark = pytest.mark.gpu

NCASES = len(ec.BASE_CASES)
ROWS = {r.name: r for r in ec.ROWS}
LATTICE = 2.0 ** -20
OFFSETS = np.array([2.0 ** 20, -3.0 * 2.0 ** 19, 3.0 * 2.0 ** 19, -2.0 ** 20])
NSTART = 24


# ---- inputs: numpy alone ---------------------------------------------------------------------------------------------------
def _inputs(ci, lattice=False):
    """the numbers of case ci, all in one namespace; lattice=True rounds every coordinate to a multiple of 2^-20"""
    D, N, Nq = ec.BASE_CASES[ci]
    N2 = ec.BASE_CASES[(ci + 1) % NCASES][1]
    rng = np.random.default_rng(33000 + 100 * D + N)
    rnd = (lambda a: np.round(a / LATTICE) * LATTICE) if lattice else (lambda a: a)

    def cloud(n, shift):
        return rnd(rng.standard_normal((D, n)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1)) + shift)

    def weights(n):
        w = rng.uniform(0.05, 1.0, size=n)
        w[::5] = 0.0
        return w

    pts, w, sd = cloud(N, 0.0), weights(N), rng.uniform(0.2, 0.6, size=D)
    pts2, w2, sd2 = cloud(N2, 0.4), weights(N2), rng.uniform(0.2, 0.6, size=D)
    # queries within the data's range: a point of the density each, moved by about a bandwidth
    X = rnd(pts[:, rng.integers(0, N, size=Nq)] + sd[:, None] * rng.standard_normal((D, Nq)))
    starts = rnd(pts[:, rng.integers(0, N, size=NSTART)] + 0.5 * sd[:, None] * rng.standard_normal((D, NSTART)))
    # boxes centred on the queries, between 0.6 and 4 bandwidths wide (tests/test_gpu_mass.py: at least half a bandwidth),
    # a fifth of the bounds infinite, the first box with one of each
    half = 0.5 * sd[:, None] * rng.uniform(0.6, 4.0, size=(D, Nq))
    lo, hi = rnd(X - half), rnd(X + half)
    assert np.all(hi - lo >= 0.5 * sd[:, None])
    lo[rng.uniform(size=lo.shape) < 0.2] = -math.inf
    hi[rng.uniform(size=hi.shape) < 0.2] = math.inf
    lo[0, 0], hi[-1, 0] = -math.inf, math.inf
    edges = [rnd(np.linspace(pts[d].min(), pts[d].max(), 5)) for d in (0, D - 1)]
    for e in edges:
        assert np.all(np.diff(e) > 0)
    sd3 = rng.uniform(0.3, 0.9, size=D)
    c = ec.namespace(ci=ci, D=D, N=N, Nq=Nq, N2=N2, k=0, t=np.zeros(D), sp=0.0, pts=pts, w=w, sd=sd, pts2=pts2, w2=w2, sd2=sd2,
                     X=X, starts=starts, lo=lo, hi=hi, edges=edges, v=sd3 * sd3, sd_mmd=rng.uniform(0.3, 0.9, size=D),
                     metric=rng.uniform(0.3, 3.0, size=D), bwpp=sd[:, None] * rng.uniform(0.5, 2.0, size=(D, N)),
                     labels=rng.integers(1, N + 1, size=ec.NDRAW), G=list(range(1, D, 2)), unit=1.0)
    # (drawn after everything above, so that the older rows keep their numbers) the refit's new weights with exact zeros, its
    # moves -- on the lattice too, so that x + t + delta is exact --, log-likelihoods that span a few hundred with one -Inf, and
    # a transport scale from the caller
    c.rw = rng.uniform(0.05, 2.0, size=N)
    c.rw[::7] = 0.0
    c.rdelta = rnd(0.3 * rng.standard_normal((D, N)))
    c.logl = rng.uniform(-300.0, 0.0, size=N)
    c.logl[1] = -math.inf
    c.ot_scale = rng.uniform(0.5, 1.5, size=D)
    if lattice:
        assert np.all(np.abs(c.rdelta) < 2.0 ** 6) and np.all(c.rdelta / LATTICE == np.round(c.rdelta / LATTICE))
        for a in (pts, pts2, X, starts, lo[np.isfinite(lo)], hi[np.isfinite(hi)], *edges):
            assert np.all(np.abs(a) < 2.0 ** 6) and np.all(a / LATTICE == np.round(a / LATTICE)), "an input left the lattice"
    return c


_POS = ("pts", "pts2", "X", "starts", "lo", "hi")


def _scaled(c0, k):
    c = ec.namespace(**vars(c0))
    c.k = k
    for name in _POS + ("sd", "sd2", "sd_mmd", "bwpp", "rdelta", "ot_scale"):
        setattr(c, name, np.ldexp(getattr(c0, name), k))
    c.edges = [np.ldexp(e, k) for e in c0.edges]
    c.v, c.metric, c.unit = np.ldexp(c0.v, 2 * k), np.ldexp(c0.metric, -2 * k), math.ldexp(1.0, k)
    return c


def _shifted(c0):
    c = ec.namespace(**vars(c0))
    c.t = OFFSETS[(np.arange(c0.D) + c0.ci) % 4]
    for name in _POS:
        a = getattr(c0, name) + c.t[:, None]
        back = a - c.t[:, None]
        assert np.array_equal(back, getattr(c0, name)), f"x + t - t != x in {name}: the translation is not exact and proves nothing"
        setattr(c, name, a)
    c.edges = [e + c.t[d] for e, d in zip(c0.edges, (0, c0.D - 1))]
    for e, e0, d in zip(c.edges, c0.edges, (0, c0.D - 1)):
        assert np.array_equal(e - c.t[d], e0)
    c.sp = float(np.spacing(max(float(np.max(np.abs(c.pts))), float(np.max(np.abs(c.X))))))
    assert c.sp == 2.0 ** -32
    return c


# ---- cases: the host densities of a set of inputs, built once, shared, never changed ----------------------------------------
_CASES = {}


def _finish(c):
    c.Y = np.ascontiguousarray(c.X[c.G])
    c.p, c.q = kdehip.kde(c.pts, c.sd, c.w), kdehip.kde(c.pts2, c.sd2, c.w2)
    c.pu, c.qu = kdehip.kde(c.pts, c.sd), kdehip.kde(c.pts2, c.sd2)      # uniform weights: the neighbour estimators
    c.at = kdehip.kde(c.X, [c.unit])                                      # the queries as a density (its bandwidth is not read)
    c.A, c.B = density_arrays(c.p), density_arrays(c.q)
    c.sub = np.arange(c.Nq) if c.Nq <= 40 else np.linspace(0, c.Nq - 1, 40).astype(int)
    return c


def _tree_premise(c, c0, what):
    """the tree of the transformed inputs is the base's tree: the same permutation, leaf means and variances related exactly"""
    D = c.D
    for a, b, n in ((c.p, c0.p, c.N), (c.q, c0.q, c.N2), (c.at, c0.at, c.Nq)):
        assert np.array_equal(a.bt.permutation, b.bt.permutation), \
            f"{what}: the tree builder ordered the leaves differently, so no output is comparable bit for bit"
        leaves = b.means[n * D:].reshape(n, D)
        want = np.ldexp(leaves, c.k) + c.t[None, :]
        assert np.array_equal(a.means[n * D:].reshape(n, D), want), f"{what}: leaf means are not the base's, transformed exactly"
        assert np.array_equal(a.bandwidth[n * D:], np.ldexp(b.bandwidth[n * D:], 2 * c.k)), f"{what}: leaf variances"


def _case(ci, variant):
    """variant: "base", a k of ec.K, "lattice" or "shifted" """
    key = (ci, variant)
    if key not in _CASES:
        if variant == "base":
            c = _inputs(ci)
            _density_premise(c)
            _finish(c)
        elif variant == "lattice":
            c = _finish(_inputs(ci, lattice=True))
        elif variant == "shifted":
            c0 = _case(ci, "lattice")
            c = _finish(_shifted(c0))
            _tree_premise(c, c0, "translation")
        else:
            c0 = _case(ci, "base")
            c = _finish(_scaled(c0, int(variant)))
            _tree_premise(c, c0, f"k = {variant}")
        _CASES[key] = c
    return _CASES[key]


def _in_range(a, bits=150):
    """every finite value is 0 or lies in [2^-bits, 2^bits].  150 is the premise of the densities; the outputs of the library
    are asked for what the law needs, 1022 - 80 |e|: the arrays of a conditioned density hold weights down to 1e-80 and
    inner-node means in proportion, which 2^(80) still leaves normal"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[np.isfinite(a)]
    return bool(np.all((a == 0.0) | ((a >= 2.0 ** -bits) & (a <= 2.0 ** bits))))


def _density_premise(c):
    """from numpy alone, before the library is called: the model's densities at the queries and at the data (leave-one-out)
    lie in [2^-150, 2^150], so that p * 2^(-D k) is a normal number at every k and the law is exact"""
    w = c.w / c.w.sum()
    v = c.sd * c.sd
    direct = em.direct_fsum(np.ascontiguousarray(c.pts.T), w, v, np.ascontiguousarray(c.X.T))
    loo = em.direct_fsum(np.ascontiguousarray(c.pts.T), w, v, np.ascontiguousarray(c.pts.T), loo=True)
    assert np.all(direct > 0.0) and _in_range(direct) and _in_range(loo), \
        "a model density left [2^-150, 2^150]: its scaled value may be subnormal or infinite and the bit law would not be exact"


class _Resident:
    """the resident twins of a case's densities, closed on exit"""

    def __init__(self, c):
        self.c, self.made = ec.namespace(**vars(c)), []

    def __enter__(self):
        for name in ("p", "q", "at", "pu", "qu"):
            d = kdehip.DeviceDensity(getattr(self.c, name))
            self.made.append(d)
            setattr(self.c, "d" + name, d)
        return self.c

    def __exit__(self, *exc):
        for d in self.made:
            d.close()
        return False


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def _worst(key, ratio):
    """the figure, printed before it is asserted (pytest shows it with -s or on failure), as the family modules print theirs"""
    print(f"{key}: {float(ratio):.3e} of the bound")


def _hold(key, got, want, bound):
    """|got - want| <= bound elementwise (inf and nan must coincide); prints the worst ratio"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (key, "non-finite values differ")
    err = np.abs(got[fin] - want[fin])
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bound[fin])
        _worst(key, np.max(ratio))
        assert np.all(err <= bound[fin]), (key, float(np.max(ratio)), "times the bound")


def _same(key, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":  # the bit patterns themselves (+0.0 is not -0.0); a NaN equals any NaN: its payload is no result
        got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
        bad = ~((got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want)))
        assert not bad.any(), (key, f"{int(bad.sum())} of {bad.size} values differ in bits; first",
                               got[bad].ravel()[:3].tolist(), want[bad].ravel()[:3].tolist())
    else:
        assert np.array_equal(got, want), key


def _law(row, name, law, c0, base, ck, got):
    """one output at one scale.  The tolerance laws' bounds, and where they come from:
      add   1e-12 * max(1, |ref|): tests/test_gpu_logdensity.py (`_close`), which the gradient, curvature, conditional and
            product modules copy for their log p and log Z; tests/test_gpu_bwjoint.py holds logl and the trace to the same
            against evalAvgLogL; the neighbour estimators' 1e-12 (tests/test_gpu_knn.py) is the same number
      inv   1e-12 * max(1, |ref| + D |k| ln 2): the two logs that cancel are each held to the bound above at their own size
      rel   n * 1e-12 * max(1, |log |ref||, D |k| ln 2) relative: exp of n values held to the two bounds above
      search  |e| * 1e-9 relative: test_loocv_bandwidth_parity_with_oracle (tests/test_gpu_bandwidth.py); plus rel's bound for
            each scale factor of adaptive_scales that multiplies the searched bandwidth (kde_adaptive with ks=None)
      near  1e-6 bandwidths: the distance tests/test_gpu_modes.py allows between the iteration's end points and the model's"""
    k, e = ck.k, law.e(c0)
    key = f"{row.name}.{name}"
    base_a, got_a = np.asarray(base), np.asarray(got)
    shift = c0.D * abs(k) * ec.LN2
    if law.kind == "bits":
        want = np.ldexp(base_a, e * k) if base_a.dtype.kind == "f" and e != 0 else base_a
        _same(f"{key} at k = {k}", got_a, want)
    elif law.kind == "add":
        want = base_a + e * k * ec.LN2
        _hold(key, got_a, want, 1e-12 * np.maximum(1.0, np.abs(want)))
    elif law.kind == "inv":
        _hold(key, got_a, base_a, 1e-12 * np.maximum(1.0, np.abs(base_a) + shift))
    elif law.kind == "rel":
        want = np.ldexp(base_a, e * k)
        with np.errstate(divide="ignore"):
            size = np.where(want != 0.0, np.abs(np.log(np.abs(np.where(want != 0.0, want, 1.0)))), 0.0)
        _hold(key, got_a, want, law.n * 1e-12 * np.maximum(np.maximum(1.0, size), shift) * np.abs(want))
    elif law.kind == "search":
        want = np.ldexp(base_a, e * k)
        lam = law.n * 1e-12 * max(1.0, shift)   # (scale factors are of order 1: |log lambda| stays below D |k| ln 2)
        _hold(key, got_a, want, (abs(e) * 1e-9 + lam) * np.abs(want))
    elif law.kind == "near":
        want = np.ldexp(base_a, e * k)
        _hold(key, got_a, want, 1e-6 * ck.sd.reshape((c0.D,) + (1,) * (want.ndim - 1)))
    else:
        raise AssertionError(law.kind)


# ---- the base (and the translated case) against the families' models --------------------------------------------------------
def _rel12(key, got, want):
    """1e-12 * want: the project's tolerance for sums of positive terms (tests/test_gpu_ksum.py `_close`)"""
    _hold(key, got, want, 1e-12 * np.abs(want))


def _log12(key, got, want):
    """1e-12 * max(1, |ref|) (tests/test_gpu_logdensity.py `_close`)"""
    _hold(key, got, want, 1e-12 * np.maximum(1.0, np.abs(np.asarray(want, dtype=np.float64))))


def _rows(a):
    return np.ascontiguousarray(np.asarray(a).T)


def _model_tree(pts, sd, w):
    m = pymodel.kde([list(map(float, pts[:, i])) for i in range(pts.shape[1])], [float(s) for s in sd],
                    None if w is None else [float(x) for x in w])
    return {n: np.array(getattr(m, n)[1:], dtype=np.int64 if n in ("left_child", "right_child", "lowest_leaf", "highest_leaf",
                                                                    "permutation") else np.float64)
            for n in ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation",
                      "means", "bandwidth")}


def _check_kde(c, o):
    """exactly, as tests/test_oracle_vs_pymodel.py holds the oracle to the same model; the GPU builder's arrays are the host's"""
    for prefix, sd, w in (("", c.sd, c.w), ("one_", c.sd[:1], None)):
        for n, want in _model_tree(c.pts, sd, w).items():
            _same(f"kde.{prefix}{n} against pymodel", o[prefix + n], want)
    for n, _, _ in ec.TREE_FIELDS:
        _same(f"kde.gpu_{n} against the host builder", o["gpu_" + n], o[n])


def _direct(c, A, qry_rows, loo=False):
    return em.direct_fsum(_rows(A[0]), A[1], A[2], qry_rows, loo)


def _check_evaluate(c, o):
    want = _direct(c, c.A, _rows(c.X[:, c.sub]))
    _rel12("evaluate.p model", o["p"][c.sub], want)
    _same("evaluate.functor", o["functor"], o["p"])
    _rel12("evaluate.loo model", o["loo"], _direct(c, c.A, _rows(c.A[0]), loo=True))
    _same("evaluate.at", o["at"], o["p"])   # at the queries as a density: its points in ITS original order


def _check_evaluate_log(c, o):
    pts, w, v = c.A
    _log12("evaluate_log.logp model", o["logp"][c.sub], lm.eval_log(pts, w, v, c.X[:, c.sub]))
    _log12("evaluate_log.loo model", o["loo"], lm.eval_log(pts, w, v, loo=True))


def _check_loglik(c, o):
    """log domain: tests/test_gpu_logdensity.py; direct: 1e-12 * sum W |log L| (tests/test_gpu_loglik.py `_close`)"""
    A, B = c.A, c.B
    ll, _ = lm.eval_avg_logl_log(A, (B[0], B[1], None))
    self_ll, _ = lm.eval_avg_logl_log(A)
    _log12("loglik.ll_log model", o["ll_log"], ll)
    _log12("loglik.ll_self_log model", o["ll_self_log"], self_ll)
    assert o["entropy_log"] == -o["ll_self_log"] and o["entropy"] == -o["ll_self"]
    kl = lm.kld_log(A, B)
    _hold("loglik.kld_log model", o["kld_log"], kl, 1e-12 * max(1.0, abs(self_ll) + abs(self_ll - kl)))
    L = _direct(c, A, _rows(B[0]))
    _hold("loglik.ll model", o["ll"], float(np.dot(np.log(L), B[1])), 1e-12 * float(np.dot(np.abs(np.log(L)), B[1])))
    Ls = _direct(c, A, _rows(A[0]), loo=True)
    use = A[1] > 0.0
    assert np.all(Ls[use] > 0.0)
    scale = float(np.dot(np.abs(np.log(Ls[use])), A[1][use]))
    _hold("loglik.ll_self model", o["ll_self"], float(np.dot(np.log(Ls[use]), A[1][use])), 1e-12 * scale)
    for s in ("", "_log"):
        assert o["minkld" + s] <= abs(o["kld" + s])


def _check_ksum(c, o):
    A, B = c.A, c.B
    want = km.kernel_sum(A, B, c.v)
    _rel12("ksum.S model", o["S"], want)
    _rel12("ksum.S_norm model", o["S_norm"], want / km.norm(c.v))
    _rel12("ksum.inters model", o["inters"], km.inters_intg(A, B))
    val, mag = km.ise(A, B)
    _hold("ksum.ise model", o["ise"], val, 1e-12 * mag)   # (the three terms' magnitudes: tests/test_gpu_ksum.py)
    val, mag = km.mmd(A, B, c.sd_mmd)
    _hold("ksum.mmd model", o["mmd"], val, 1e-12 * mag)


def _check_grad(c, o):
    """tests/test_gpu_modes.py: log p 1e-12 * max(1, |ref|), p 1e-12 * p, a gradient 1e-12 * A_k / (S_0 v_k)"""
    X = c.X[:, c.sub]
    want, wgrad, scale = mm.evaluate_grad(c.A, X)
    _log12("grad.logp model", o["logp"][c.sub], want)
    _hold("grad.grad model", o["grad"][:, c.sub], wgrad, 1e-12 * scale)
    want, wgrad, scale = mm.evaluate_grad(c.A, X, log=False)
    _rel12("grad.p model", o["p"][c.sub], want)
    _hold("grad.pgrad model", o["pgrad"][:, c.sub], wgrad, 1e-12 * scale)


def _check_meanshift(c, o):
    """the end points: the model's own step from the returned point is within tol (1e-9 bandwidths, the call's), to the
    1e-12 * A_k / S_0 a step is held to (tests/test_gpu_modes.py) and, at a translated position, one spacing for the rounding
    of the stored point's difference to each leaf; log p at them at its bound"""
    sd = np.sqrt(c.A[2])
    conv = o["iters"] > 0
    assert conv.all(), "a start did not converge in 500 steps: the end points prove nothing"
    for j in range(NSTART):
        _, dx, A = mm.step(c.A, o["x"][:, j])
        assert np.all(np.abs(dx) <= 1e-9 * sd * (1.0 + 1e-3) + 1e-12 * A + c.sp), (j, np.abs(dx) / sd)
        _hold("meanshift.logp model", o["logp"][j], mm.log_p(c.A, o["x"][:, j]),
              1e-12 * max(1.0, abs(o["logp"][j])) + _logp_slack(c, o["x"][:, j]))
    # modes: the merge of these end points, as the wrapper's docstring says it
    kept, labels = mm.merge(o["x"], o["logp"], o["iters"].astype(np.int64), sd, 1e-3)
    _same("meanshift.labels", o["labels"], labels)
    _same("meanshift.modes", o["modes"], np.ascontiguousarray(o["x"][:, kept]))
    _same("meanshift.modes_logp", o["modes_logp"], o["logp"][kept])
    _same("meanshift.mode", o["mode"], o["modes"][:, 0])
    assert abs(float(o["mass"].sum()) - 1.0) <= 1e-12


def _logp_slack(c, x):
    """a position stored at 2^20 is off by up to half a spacing: log p moves by at most |grad log p| times that"""
    if c.sp == 0.0:
        return 0.0
    _, g, _ = mm.evaluate_grad(c.A, np.asarray(x, dtype=np.float64).reshape(-1, 1))
    return float(np.sum(np.abs(g))) * c.sp


def _check_hess(c, o):
    """tests/test_gpu_curvature.py: gradient and Hessian 1e-12 of their scales; the linear forms are the wrapper's own
    products of the log-domain outputs"""
    sub = c.sub
    logp, grad, gs, hess, hs = hm.evaluate_hess(c.A, c.X[:, sub])
    _log12("hess.logp model", o["logp"][sub], logp)
    _hold("hess.grad model", o["grad"][:, sub], grad, 1e-12 * gs)
    _hold("hess.hess model", o["hess"][:, :, sub], hess, 1e-12 * hs)
    pv = np.exp(o["logp"])
    _same("hess.p", o["p"], pv)
    _same("hess.pgrad", o["pgrad"], pv * o["grad"])
    _same("hess.phess", o["phess"], pv * (o["hess"] + o["grad"][:, None, :] * o["grad"][None, :, :]))


def _check_laplace(c, o):
    """tests/test_gpu_curvature.py: cov against numpy's inverse of the entry's own -hess within curvature_model.cov_bound,
    64 u kappa max|cov|; definite where every eigenvalue of -hess is positive.  A relation between two outputs of the library,
    not an independent reference: the Hessian is held to curvature_model at the queries (`_check_hess`), not at these starts"""
    _, _, H = kdehip.evaluate_hess(c.p, c.starts)
    ndef = 0
    for q in range(NSTART):
        ev = np.linalg.eigvalsh(-H[:, :, q])
        if np.min(ev) <= 1e-9 * np.max(np.abs(ev)):
            if np.min(ev) < -1e-9 * np.max(np.abs(ev)):   # (a pivot on the edge may go either way)
                assert not o["definite"][q] and np.all(np.isnan(o["cov"][:, :, q]))
            continue
        assert o["definite"][q]
        ndef += 1
        want = np.linalg.inv(-H[:, :, q])
        _hold("laplace.cov model", o["cov"][:, :, q], want, hm.cov_bound(-H[:, :, q], want)[1])
    assert ndef >= 4, "fewer than four starts have a definite Hessian: the covariance is hardly compared"
    assert o["fit_is_laplace"].all(), "fit_modes / getKDEModeFit are not laplace at the modes"
    assert o["modes_definite"].all(), "a mode whose Hessian is not negative definite"
    covs, _ = kdehip.laplace(c.p, o["means"])
    v = c.A[2]
    for j in range(o["means"].shape[1]):  # at a mode cov - diag(v) is positive semidefinite (the wrapper's docstring)
        assert np.min(np.linalg.eigvalsh(covs[:, :, j] - np.diag(v))) >= -1e-9 * np.max(v)


def _leaf(p):
    N, D = p.bt.num_points, p.bt.dims
    return (p.means[N * D:].reshape(N, D).T.copy(), p.bt.weights[N:].copy(), p.bandwidth[N * D:(N + 1) * D].copy()), \
        p.bt.permutation[N:].copy()


_UNIT = {}


def _device_normals(nf, seed, offset, n):
    """the normals the device draws for indices offset .. offset + n - 1 of an nf-dimensional density (the device of
    tests/test_gpu_sample.py: a one-point density at the origin with unit variance returns them exactly)"""
    if nf not in _UNIT:
        _UNIT[nf] = kdehip.kde(np.zeros((nf, 1)), [1.0])
    x, lab = kdehip.sample(_UNIT[nf], n, seed=seed, sample_offset=offset)
    assert (lab == 1).all()
    return x


def _check_conditional(c, o):
    """tests/test_gpu_conditional.py: logz 1e-12 * max(1, |ref|); mean 1e-12 * (R_k + |ref|); var 1e-12 * (R_k^2 + v_k);
    omega 1e-12 * ref + 1e-300.  Translated: the mean is a sum of N products of weights and coordinates of size 2^20, so
    its bound is taken at that size (|ref| carries it); the variance is formed from differences and keeps its bound."""
    dens, perm = _leaf(c.p)
    F = cm.free_dims(c.D, c.G)
    R = (dens[0].max(axis=1) - dens[0].min(axis=1))[F]
    v = dens[2][F]
    for q in c.sub:
        logz, mean, var = cm.moments(dens, c.G, c.Y[:, q])
        _log12("conditional.logz model", o["logz"][q], logz)
        _hold("conditional.mean model", o["mean"][:, q], mean, 1e-12 * (R + np.abs(mean)))
        _hold("conditional.var model", o["var"][:, q], var, 1e-12 * (R * R + v))
        ref = cm.weights(dens, c.G, c.Y[:, q])
        _hold("conditional.W model", o["W"][q, perm - 1], ref, 1e-12 * ref + 1e-300)
    _same("conditional.wlogz", o["wlogz"], o["logz"])
    assert np.all(o["var"] >= v[:, None])
    # a draw: the centre of the drawn kernel in F plus bandwidth noise, from the device's own normals (bit for bit, as
    # tests/test_gpu_conditional.py holds it); the drawn kernel has weight in the conditional
    assert np.all(o["ind"] >= 1)
    normals = _device_normals(len(F), ec.SEED, 0, c.Nq)
    want = c.A[0][F][:, o["ind"] - 1] + np.sqrt(v)[:, None] * normals
    _same("conditional.draws", o["draws"], want)
    assert np.all(o["W"][np.arange(c.Nq), o["ind"] - 1] > 0.0)
    # condition: kde of the free coordinates with the weights of query 0
    want = kdehip.kde(c.A[0][F], np.sqrt(v), o["W"][0])
    for n, val in ec.fields(want, "cond_").items():
        _same("conditional." + n, o[n], val)


def _check_mass(c, o):
    """tests/test_gpu_mass.py: a mass 1e-12 * want; a quantile |F_model(x) - alpha| <= tol + 1e-12 and the residual within
    1e-12 of the model's.  Translated: x is stored to half a spacing of doubles at 2^20 and the bracket cannot close below
    one, so F carries f(x) * 1.5 spacings more (the rounding of x, and the last bracket)"""
    sub = c.sub
    _rel12("mass.box model", o["box"][sub], sm.box_mass(c.A, c.lo[:, sub], c.hi[:, sub]))
    _rel12("mass.box_dims model", o["box_dims"][sub], sm.box_mass(c.A, c.lo[c.G][:, sub], c.hi[c.G][:, sub], c.G))
    _rel12("mass.cdf model", o["cdf"][sub], np.array([sm.cdf(c.A, x, 0) for x in c.X[0, sub]]))
    e0, e1 = c.edges
    lo = np.stack([g.ravel() for g in np.meshgrid(e0[:-1], e1[:-1], indexing="ij")])
    hi = np.stack([g.ravel() for g in np.meshgrid(e0[1:], e1[1:], indexing="ij")])
    _rel12("mass.grid model", o["grid"].ravel(), sm.box_mass(c.A, lo, hi, [0, c.D - 1]))
    for x, r, a, dim, what in ([(x, r, a, 0, "quantile") for x, r, a in zip(o["quantile"], o["resid"], ec.LEVELS)]
                               + [(o["median"], None, 0.5, 1, "median"), (o["interval"][0], None, 0.05, c.D - 1, "interval"),
                                  (o["interval"][1], None, 0.95, c.D - 1, "interval")]):
        F, f = sm.cdf(c.A, x, dim), sm.pdf(c.A, x, dim)
        _hold(f"mass.{what} model", F, a, 1e-12 + 1e-12 + 1.5 * f * c.sp)
        if r is not None and c.sp == 0.0:
            assert abs(r) <= 1e-12, (what, r)   # the call's tol, as tests/test_gpu_mass.py asserts it
            _hold("mass.resid model", r, F - a, 1e-12)
    if c.sp == 0.0:
        assert o["converged"].all()
    else:
        # at 2^20 neighbouring doubles are f(x) 2^-32 apart in F, more than tol: a level either reaches tol or uses up its
        # max_iter = 100 evaluations and says so -- what `converged` means (kdehip.h section 5l)
        print("translated quantiles: converged", o["converged"].tolist(), "iters", o["iters"].tolist())
        assert np.all(o["converged"] | (o["iters"] == 100))
        assert np.all(np.abs(o["resid"][o["converged"]]) <= 1e-12)


def _check_evaltol(c, o):
    """tests/test_gpu_evaltol.py: direct (1 - rel_tol) - 1e-12 direct <= got <= direct (1 + 1e-12); no tolerance: the direct
    entry's bits; the tile total is a function of the shapes"""
    direct = _direct(c, c.A, _rows(c.X))
    for name, d in (("vals", direct), ("switch", direct), ("loo", _direct(c, c.A, _rows(c.A[0]), loo=True))):
        assert np.all(o[name] <= d * (1.0 + 1e-12)) and np.all(o[name] >= d * (1.0 - 1e-3) - 1e-12 * d), name
        with np.errstate(divide="ignore", invalid="ignore"):
            _worst(f"evaltol.{name} loss / rel_tol", np.nanmax(np.where(d > 0, (d - o[name]) / d, 0.0)) / 1e-3)
    _same("evaltol.exact", o["exact"], kdehip.evaluateDualTree(c.p, c.X))
    _same("evaltol.switch", o["switch"], o["vals"])
    assert o["stats"][1] == ((c.Nq + 255) // 256) * ((c.N + 127) // 128) and 0 < o["stats"][0] <= o["stats"][1]
    assert o["loo_stats"][1] == ((c.N + 255) // 256) * ((c.N + 127) // 128) and 0 < o["loo_stats"][0] <= o["loo_stats"][1]


def _check_knn(c, o):
    """tests/test_gpu_knn.py: indices and squared distances exactly the model's; the estimators 1e-12"""
    (leaves, _, v), perm = _leaf(c.p)
    L, Q = _rows(leaves), _rows(c.X)
    for pre, scale in (("", None), ("bw_", 1.0 / v), ("sc_", c.metric)):
        d2, idx = nm.knn(L, perm, Q, 8, scale=scale)
        _same(f"knn.{pre}idx model", o[pre + "idx"], np.ascontiguousarray(idx.T))
        _same(f"knn.{pre}d2 model", o[pre + "d2"], np.ascontiguousarray(d2.T))
    _same("knn.dist", o["dist"], np.sqrt(o["d2"]))
    d2, idx = nm.knn(L, perm, L, 8, loo=True)
    back = np.argsort(perm - 1)
    _same("knn.loo_idx model", o["loo_idx"], np.ascontiguousarray(idx[back].T))
    _same("knn.loo_d2 model", o["loo_d2"], np.ascontiguousarray(d2[back].T))
    # the estimators on the uniform twins, k = 4
    (Lu, _, _), pu = _leaf(c.pu)
    (Lq, _, _), pq = _leaf(c.qu)
    eps = np.sqrt(nm.knn(_rows(Lu), pu, _rows(Lu), 4, loo=True)[0][:, 3])
    nu = np.sqrt(nm.knn(_rows(Lq), pq, _rows(Lu), 4)[0][:, 3])
    _hold("knn.entropy_knn model", o["entropy_knn"], nm.entropy_kl(eps, c.D, 4), 1e-12 * max(1.0, abs(o["entropy_knn"])))
    _hold("knn.kld_knn model", o["kld_knn"], nm.kld_wkv(eps, nu, c.D, c.N2), 1e-12 * max(1.0, abs(o["kld_knn"])))


def _orig_rows(p, arr):
    N, D = p.bt.num_points, p.bt.dims
    out = np.zeros((D, N))
    out[:, p.bt.permutation[N:] - 1] = np.asarray(arr)[N * D:2 * N * D].reshape(N, D).T
    return out


def _check_varbw(c, o):
    """tests/test_gpu_varbw.py: log p 1e-12 * max(1, |ref|), p 1e-12 relative; the scale factors 1e-10 of the model's; the
    tree of a per-point density is kde's.  The variances of kde_adaptive are compared with kde_varbw of the library's own
    scale factors: a relation between outputs; the factors themselves are held to the model"""
    pv = kdehip.kde_varbw(c.pts, c.bwpp, c.w)
    var = _orig_rows(pv, pv.bandwidth)
    assert np.array_equal(var, c.bwpp * c.bwpp)
    pts, w, _ = c.A
    X = c.X[:, c.sub]
    _log12("varbw.logp model", o["logp"][c.sub], vm.eval_log(pts, w, var, X))
    _hold("varbw.p model", o["p"][c.sub], vm.eval_direct(pts, w, var, X), 1e-12 * np.abs(o["p"][c.sub]) + 1e-300)
    _log12("varbw.loo model", o["loo"], vm.eval_log(pts, w, var, loo=True))
    _log12("varbw.ll model", o["ll"], vm.eval_avg_logl((pts, w, var), log_domain=True))
    for n in ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation", "means"):
        where = c.p.bt if hasattr(c.p.bt, n) else c.p
        _same(f"varbw.pv_{n} against kde", o["pv_" + n], np.array(getattr(where, n)))
        _same(f"varbw.ad_{n} against kde", o["ad_" + n], np.array(getattr(where, n)))
    for n, want in (("lam_abramson", vm.scales_abramson(pts, w, c.A[2])), ("lam_knn", vm.scales_knn(pts, w, c.A[2], 8))):
        _hold(f"varbw.{n} model", o[n], want, 1e-10 * want)   # (relative, as test_kde_adaptive_on_the_two_scale_sample)
    ad = kdehip.kde_varbw(c.pts, np.outer(kdehip.getBW(c.p)[:, 0], o["lam_abramson"]), c.w)
    for n in ("bandwidth", "bandwidthMin", "bandwidthMax"):
        _same("varbw.ad_" + n, o["ad_" + n], np.array(getattr(ad, n)))


def _check_prodexact(c, o):
    """tests/test_gpu_prodexact.py: logz 1e-12 * max(1, |ref|); component weights and means 1e-12 (means: of max(1, |x|),
    its bound for points), their sum 1 within 1e-14; sd 1e-15; a draw is its component's mean plus sd times the device's
    normal, within the 1e-12 * max(1, |x|) the module holds points to"""
    want = pm.logz(c.A, c.B)
    _log12("prodexact.logz model", o["logz"], want)
    _log12("prodexact.log_inters model", o["log_inters"], want)
    _same("prodexact.log_inters is logz", np.float64(o["log_inters"]), np.float64(o["logz"]))
    means, w, var = pm.components(c.A, c.B)
    _hold("prodexact.weights model", o["weights"], w, 1e-12)
    _hold("prodexact.means model", o["means"], means.T, 1e-12 * np.maximum(1.0, np.abs(means.T)))
    assert abs(math.fsum(o["weights"].tolist()) - 1.0) <= 1e-14
    _hold("prodexact.sd model", o["sd"], np.sqrt(var), 1e-15 * np.sqrt(var))
    ind = o["ind"]
    assert ind.shape == (2, ec.NDRAW) and np.all(ind >= 1)
    comp = (ind[0] - 1) * c.N2 + (ind[1] - 1)
    assert np.all(o["weights"][comp] > 0.0)
    normals = _device_normals(c.D, ec.SEED, 0, ec.NDRAW)
    want = o["means"][:, comp] + o["sd"][:, None] * normals
    _hold("prodexact.draws model", o["draws"], want, 1e-12 * np.maximum(1.0, np.abs(want)))


def _check_bwjoint(c, o):
    """tests/test_gpu_bwjoint.py: the bandwidth 1e-9 relative per iterate, logl and the trace 1e-9 * max(1, |L|) against the
    model, 1e-12 * max(1, |L|) against evalAvgLogL of the density rebuilt with the result"""
    assert o["iters"] > 0 and o["status"] == 0, "the iteration did not converge within 200 steps"
    # (the model takes the entry's number of steps: a step whose reach lies within rounding of tol may stop either of them)
    bw, logl, iters, status, trace = bm.iterate(c.A, None, 1e-3, int(o["iters"]))
    assert abs(iters) == o["iters"] and status == 0
    _hold("bwjoint.bw model", o["bw"], bw, 1e-9 * bw)
    _hold("bwjoint.logl model", o["logl"], logl, 1e-9 * max(1.0, abs(logl)))
    _hold("bwjoint.trace model", o["trace"], trace, 1e-9 * np.maximum(1.0, np.abs(trace)))
    _same("bwjoint.var", o["var"], o["bw"] * o["bw"])
    q = kdehip.kde(c.pts, o["bw"], c.w)
    _log12("bwjoint.logl against evalAvgLogL", o["logl"], kdehip.evalAvgLogL(q, q, log_domain=True))
    _hold("bwjoint.bw_start model", o["bw_start"], bm.iterate(c.A, c.sd2, 1e-3, 3)[0], 1e-9 * o["bw_start"])
    p0 = kdehip.kde(c.pts, c.sd, c.w)
    want = kdehip.kde(c.pts, kdehip.joint_bandwidth(p0, None, 1e-3, 5), c.w)
    for n, val in ec.fields(want, "kj_").items():
        _same("bwjoint." + n, o[n], val)


def _check_summary(c, o):
    """section 5e's formulas in numpy (tests/test_gpu_summary.py): mean and range exactly, the covariance 1e-12 of its largest
    entry against np.longdouble, the grid values 1e-12 relative to the direct sum of the 1-D marginal, the argmax within
    1e-11 of the grid's largest value.  The grids themselves come from the package's `summary.grid`: for `getKDERangeLinspace`
    and the points of `getKDEMax` this is a relation between outputs, not an independent reference; the values ON the grid are
    held to tests/evaltol_model.py"""
    pts = c.A[0]
    s = np.cumsum(np.concatenate([np.zeros((c.D, 1)), pts], axis=1), axis=1)[:, -1]
    _same("summary.mean", o["mean"], s / np.float64(c.N))
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    _same("summary.range", o["range"], np.stack([lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)], axis=1))
    _same("summary.fit_mean", o["fit_mean"], o["mean"])
    Xc = pts.astype(np.longdouble) - pts.astype(np.longdouble).mean(axis=1, keepdims=True)
    want = np.asarray((Xc @ Xc.T) / c.N, dtype=np.float64)
    _hold("summary.fit_cov model", o["fit_cov"], want, 1e-12 * float(np.max(np.abs(want))) + 2.0 * c.sp * float(np.max(hi - lo)))
    for d in range(c.D):
        dr = 0.1 * (hi[d] - lo[d])
        xs = kdehip.summary.grid(lo[d] - dr, hi[d] + dr, 65)
        model = em.direct_fsum(pts[d][:, None], c.A[1], c.A[2][d:d + 1], xs[:, None])
        _rel12("summary.max_values model", o["max_values"][d], model)
        got = int(np.argmin(np.abs(xs - o["max"][d])))
        assert xs[got] == o["max"][d], "the argmax is not a point of the grid"
        assert abs(model[got] - model.max()) <= 1e-11 * model.max()
    d1 = 0.1 * (hi[1] - lo[1])
    _same("summary.linspace", o["linspace"], kdehip.summary.grid(lo[1] - d1, hi[1] + d1, 33))
    dims = [0, c.D - 1]
    want = kdehip.kde(pts[dims], np.sqrt(c.A[2][dims]), c.A[1])
    for n, val in ec.fields(want, "marg_").items():
        _same("summary." + n, o[n], val)
    # intersIntgAppxIS: the sum over the 33 x 33 grid over p's ranges with extend 0.3, times the cell size
    g = [kdehip.summary.grid(lo[d] - 0.3 * (hi[d] - lo[d]), hi[d] + 0.3 * (hi[d] - lo[d]), 33) for d in dims]
    G = np.stack([a.ravel() for a in np.meshgrid(g[0], g[1], indexing="ij")])
    pv = em.direct_fsum(_rows(pts[dims]), c.A[1], c.A[2][dims], _rows(G))
    qv = em.direct_fsum(_rows(c.B[0][dims]), c.B[1], c.B[2][dims], _rows(G))
    want = math.fsum((pv * qv).tolist()) * (g[0][1] - g[0][0]) * (g[1][1] - g[1][0])
    _hold("summary.appx model", o["appx"], want, 1e-12 * abs(want) + 4.0 * c.sp / (g[0][1] - g[0][0]) * abs(want))


def _check_sample(c, o):
    """tests/test_gpu_sample.py: labels by the inverse CDF of the cumulated weights, points exactly the label's centre plus
    its bandwidth times the device's own normal"""
    u, _ = kdehip.philox_streams(ec.SEED, 0, ec.NDRAW, 1, 1)
    C = np.cumsum(c.A[1])
    C /= C[-1]
    _same("sample.ind model", o["ind"], np.searchsorted(C, u, side="right").astype(np.int64).ravel() + 1)
    sd = np.sqrt(c.A[2])[:, None]
    _same("sample.draws model", o["draws"], c.A[0][:, o["ind"] - 1] + sd * _device_normals(c.D, ec.SEED, 0, ec.NDRAW))
    _same("sample.given_ind", o["given_ind"], c.labels.astype(np.int64))
    _same("sample.given model", o["given"], c.A[0][:, c.labels - 1] + sd * _device_normals(c.D, ec.SEED, 7, ec.NDRAW))
    _same("sample.rand", o["rand"], o["draws"])


def _check_auto(c, o):
    """test_loocv_bandwidth_parity_with_oracle (tests/test_gpu_bandwidth.py): 1e-9 relative to the oracle's search"""
    from oracle import oracle
    want = np.asarray(oracle.auto_bandwidth(c.pts)[0], dtype=np.float64)
    _hold("auto.bw oracle", o["bw"], want, 1e-9 * want)
    ref = kdehip.kde(c.pts, o["bw"])
    for pre in ("auto_", "kde_"):
        for n, val in ec.fields(ref, pre).items():
            _same("auto." + n, o[n], val)
    # kde_adaptive(points): a RELATION between the library's outputs, not an independent reference -- the pilot is the density
    # above, its scale factors are adaptive_scales' (held to tests/varbw_model.py in the `varbw` row), the result kde_varbw's
    lam = kdehip.adaptive_scales(ref)
    want = kdehip.kde_varbw(c.pts, np.outer(kdehip.getBW(ref)[:, 0], lam))
    for n, val in ec.fields(want, "adp_").items():
        _same("auto." + n, o[n], val)


def _searched_density(key, o, prefix, pts):
    """a density the library built from points it drew: its bandwidth against the oracle's search on those points (1e-9, as
    `_check_auto`), its arrays those of kde(points, that bandwidth).  The premise of the search's law: no two neighbours of a
    marginal of the points closer than 1e-6, at the scale of the case"""
    from oracle import oracle
    D = pts.shape[0]
    gaps = np.diff(np.sort(pts, axis=1), axis=1)
    assert gaps.min() >= 1e-6, f"{key}: two drawn neighbours are closer than 1e-6: the reference's clamp would act"
    var = o[prefix + "bandwidth"][pts.shape[1] * D:(pts.shape[1] + 1) * D]
    want = np.asarray(oracle.auto_bandwidth(pts)[0], dtype=np.float64)
    _hold(f"{key}.bw oracle", np.sqrt(var), want, 1e-9 * want)
    for n, val in ec.fields(kdehip.kde(pts, np.sqrt(var)), prefix).items():
        if not n.endswith(("bandwidth", "bandwidthMin", "bandwidthMax")):  # (sqrt(v)^2 need not be v)
            _same(f"{key}.{n}", o[n], val)


def _check_resample(c, o):
    """resample is kde(sample(p, Np)[0]): the points are `sample`'s draws, bit for bit (tests/test_gpu_sample.py); "discrete":
    the points of the drawn labels with p's first kernel size"""
    pts, lab = kdehip.sample(c.p, ec.NDRAW, seed=ec.SEED)
    _searched_density("resample", o, "rs_", pts)
    want = kdehip.kde(c.A[0][:, lab - 1], kdehip.getBW(c.p)[:, 0])
    for n, val in ec.fields(want, "rd_").items():
        _same("resample." + n, o[n], val)


def _check_mul_exact(c, o):
    """mul_exact is kde of prod_exact's draws (tests/test_gpu_prodexact.py): the points bit for bit, `bw` the root of the leaf
    variances within the last bit"""
    pts, _ = kdehip.prod_exact(c.p, c.q, ec.NDRAW, seed=ec.SEED)
    _searched_density("mul_exact", o, "mx_", pts)
    var = o["mx_bandwidth"][ec.NDRAW * c.D:(ec.NDRAW + 1) * c.D]
    _same("mul_exact.bw", o["bw"] * o["bw"], var)
    assert o["evals"] > 0


def _tree(o, prefix):
    return {f: o[prefix + f] for f in rm.FIELDS}


def _check_refit(c, o):
    """at the terms of tests/test_gpu_refit.py: the arrays bit for bit tests/refit_model.py's (to which tests/test_refit_host.py
    pins the host entry) -- the host's from the arrays of c.p, the device's from those of its built source (dsrc_) --; the
    Bayes weights 1e-12 relative (+ 1e-300: subnormal weights), the evidence 1e-12 * max(1, |ref|) and the ess 1e-12 relative
    against the formula in extended precision, and the updated arrays those of changeWeights of the weights the update made;
    the values of the refitted densities at the queries 1e-12 relative to the direct sum (tests/evaltol_model.py)"""
    D, N = c.D, c.N
    dsrc = _tree(o, "dsrc_")
    # the built twin: the points of c.p in its leaf order, and the weights within rounding of its renormalisation
    _same("refit.dsrc_permutation", dsrc["permutation"], c.p.bt.permutation)
    _same("refit.dsrc_ leaf means", dsrc["means"][N * D:], c.p.means[N * D:])
    _hold("refit.dsrc_weights", dsrc["weights"], c.p.bt.weights, 1e-14)
    perm = c.p.bt.permutation[N:] - 1
    for src, pres in ((rm.arrays_of(c.p), ("cw_", "mv_", "both_", "by_")), (dsrc, ("dcw_", "dmv_", "dboth_", "dby_"))):
        rm.same_bits(_tree(o, pres[0]), rm.refit(src, D, N, new_weights=c.rw), f"refit.{pres[0]} model")
        rm.same_bits(_tree(o, pres[1]), rm.refit(src, D, N, delta=c.rdelta), f"refit.{pres[1]} model")
        rm.same_bits(_tree(o, pres[2]), rm.refit(src, D, N, new_weights=c.rw, delta=c.rdelta), f"refit.{pres[2]} model")
        pre = pres[3]
        le, ess = (o["log_evidence"], o["ess"]) if pre == "by_" else (o["dev_log_evidence"], o["dev_ess"])
        w0, got = np.empty(N), np.empty(N)
        w0[perm], got[perm] = src["weights"][N:], o[pre + "weights"][N:]
        wn, le_ref, ess_ref = bayes_reference(w0, c.logl)
        _hold(f"refit.{pre}weights reference", got, wn, 1e-12 * np.abs(wn) + 1e-300)
        assert got[1] == 0.0 and np.all(got[c.w == 0.0] == 0.0) and np.count_nonzero(got) > N // 2
        _hold(f"refit.{pre}log_evidence reference", le, le_ref, 1e-12 * max(1.0, abs(le_ref)))
        _hold(f"refit.{pre}ess reference", ess, ess_ref, 1e-12 * ess_ref)
        rm.same_bits(_tree(o, pre), rm.refit(src, D, N, new_weights=got), f"refit.{pre} is changeWeights of its weights")
    assert o["batch_is_singles"].all(), "an item of refit_batch differs from the single call"
    X = _rows(c.X[:, c.sub])
    for name, pts, w in (("cw_p", c.A[0], c.rw), ("mv_p", c.A[0] + c.rdelta, c.A[1]), ("both_p", c.A[0] + c.rdelta, c.rw)):
        _rel12(f"refit.{name} model", o[name][c.sub], em.direct_fsum(_rows(pts), w, c.A[2], X))


def _ot_against(key, o, prefix, want):
    """tests/test_gpu_transport.py (`_check_item`, `_close`): the potentials 1e-9 * max(1, max |phi|, max |gamma|), the four
    scalars and the map 1e-9 * max(1, |.|), the displacement 1e-9 * max(1, |map|)"""
    big = max(1.0, float(np.abs(want["phi"]).max()), float(np.abs(want["gamma"]).max()))
    assert o[prefix + "iters"] == want["iters"] == -ec.OT["maxiter"]
    for name in ("phi", "gamma"):
        assert np.all(np.isfinite(o[prefix + name]))
        _hold(f"{key}.{prefix}{name} model", o[prefix + name], want[name], 1e-9 * big)
    for name in ("value", "transport_cost", "err", "mass"):
        _hold(f"{key}.{prefix}{name} model", o[prefix + name], want[name], 1e-9 * max(1.0, abs(want[name])))
    size = np.maximum(1.0, np.abs(want["map"]))
    assert np.all(np.isfinite(o[prefix + "map"])) and np.all(np.isfinite(o[prefix + "delta"]))
    _hold(f"{key}.{prefix}map model", o[prefix + "map"], want["map"], 1e-9 * size)
    _hold(f"{key}.{prefix}delta model", o[prefix + "delta"], want["delta"], 1e-9 * size)


def _check_transport(c, o):
    vp, vq = (c.A[0], c.A[1]), (c.B[0], c.B[1])
    s, s_self = tm.default_scale(c.A[2], c.B[2]), tm.default_scale(c.A[2], c.A[2])
    kw = (ec.OT["reg"], ec.OT["tol"], ec.OT["maxiter"])
    _ot_against("transport", o, "", tm.iterate(vp, vq, s, *kw))
    _ot_against("transport", o, "s_", tm.iterate(vp, vq, c.ot_scale, *kw))
    _ot_against("transport", o, "self_", tm.iterate(vp, None, s_self, *kw))
    _same("transport.self_gamma is self_phi", o["self_gamma"], o["self_phi"])
    for pre, scale in (("", s), ("s_", c.ot_scale)):  # tests/test_gpu_transport.py G7: 1e-9 * max(1, |value(p, q)|)
        want, (pq, pp, qq) = tm.divergence(vp, vq, scale, *kw)
        _hold(f"transport.{pre}S model", o[pre + "S"], want, 1e-9 * max(1.0, abs(pq["value"])))
        _hold(f"transport.{pre}S_self_p model", o[pre + "S_self_p"], pp["value"], 1e-9 * max(1.0, abs(pp["value"])))
        _hold(f"transport.{pre}S_self_q model", o[pre + "S_self_q"], qq["value"], 1e-9 * max(1.0, abs(qq["value"])))
    _same("transport.S_cross", np.float64(o["S_cross"]), np.float64(o["value"]))
    assert list(o["S_iters"]) == [-ec.OT["maxiter"]] * 3
    assert o["map_is_info"].all() and o["batch_is_singles"].all()
    # the moved densities: movePoints by the displacement the call returns, and their points ARE the map (G5); their values at
    # the queries 1e-12 relative to the direct sum over those points (tests/evaltol_model.py)
    X = _rows(c.X[:, c.sub])
    for pre in ("", "s_"):
        moved = c.p.movePoints(o[pre + "delta"])
        rm.same_bits(_tree(o, pre + "to_"), moved, f"transport.{pre}to_ is movePoints(delta)")
        _same(f"transport.{pre}to_ points are the map", kdehip.getPoints(moved), o[pre + "map"])
        _rel12(f"transport.{pre}to_p model", o[pre + "to_p"][c.sub], em.direct_fsum(_rows(o[pre + "map"]), c.A[1], c.A[2], X))
    # equalize: equal weights transported onto p as it is, one refit with both
    u = np.full(c.N, 1.0 / c.N)
    out, info = c.p.equalize(return_info=True, **ec.OT)
    _ot_against("transport", ec._ot_item(info, "eq_"), "eq_", tm.iterate((c.A[0], u), vp, s_self, *kw))
    rm.same_bits(_tree(o, "eq_"), out, "transport.eq_ run after run")
    rm.same_bits(out, rf.refit_host(c.p, new_weights=u, delta=info["delta"]), "transport.eq_ is one refit")
    _rel12("transport.eq_p model", o["eq_p"][c.sub], em.direct_fsum(_rows(info["map"]), u, c.A[2], X))


CHECKS = {name[len("_check_"):]: fn for name, fn in list(globals().items()) if name.startswith("_check_")}

# ---- positions under translation: the untranslated output plus t, within a bound stated per output --------------------------
# SP = one spacing of doubles at the translated coordinates (2^-32).  Each entry: (which dimensions the rows are, bound(c0, o0)).
_ALL = lambda c: list(range(c.D))                     # noqa: E731
_FREE = lambda c: cm.free_dims(c.D, c.G)              # noqa: E731
_POSITION = {
    # (spacings allowed, then the family's bound in bandwidths; "observed" = the worst seen, in spacings)
    # a draw is fl(c + fl(sd n)): the sum's rounding at 2^20, half a spacing; the base's own rounding is far below it
    # (observed 0.50)
    ("sample", "draws"): (_ALL, 1.0, 0.0), ("sample", "given"): (_ALL, 1.0, 0.0), ("sample", "rand"): (_ALL, 1.0, 0.0),
    ("conditional", "draws"): (_FREE, 1.0, 0.0),
    # a + (b - a) u / s: the sum's rounding, and the product's on a difference of lattice points (exact): one spacing
    # (observed 0.50); a draw adds the rounding of its own sum (observed 1.0)
    ("prodexact", "means"): (_ALL, 1.0, 0.0), ("prodexact", "draws"): (_ALL, 2.0, 0.0),
    # sum_i omega_i c_i at 2^20: N roundings of at most half a spacing each if summed one by one; the family's own bound
    # 1e-12 * (R + |ref|) at |ref| = 2^20 is 1e-6 and would say nothing: counted instead, 8 spacings for the sums' trees
    # (observed 0.5)
    ("conditional", "mean"): (_FREE, 8.0, 0.0),
    # mean shift ends where a step is below tol = 1e-9 bandwidths; two runs that stop there differ by the family's
    # 1e-6 bandwidths (tests/test_gpu_modes.py: distance from the model's end points) plus the stored point's spacing
    # (observed 2.9e-3 of that bound, about five spacings)
    ("meanshift", "x"): (_ALL, 2.0, 1e-6), ("meanshift", "modes"): (_ALL, 2.0, 1e-6), ("meanshift", "mode"): (_ALL, 2.0, 1e-6),
    ("laplace", "means"): (_ALL, 2.0, 1e-6), ("laplace", "mode"): (_ALL, 2.0, 1e-6),
    # the mean is a sequential sum of N values at 2^20 (N half-spacings at most, at the size of the SUM: N 2^20), then / N:
    # N / 2 spacings of the result's size in the worst case (allowed 130 for N <= 257; observed 0.45)
    ("summary", "mean"): (_ALL, 130.0, 0.0), ("summary", "fit_mean"): (_ALL, 130.0, 0.0),
    # lo - dr, hi + dr: one rounding (observed 0); the grid point lo + k h: k h, the sum and h itself, three (observed 0.8)
    ("summary", "range"): (_ALL, 1.0, 0.0), ("summary", "linspace"): (None, 3.0, 0.0),
    # the image of a point is fl(x + m), m the displacement, which is formed from differences and keeps its bits: the sum's
    # rounding at 2^20, half a spacing; the base's own rounding is far below it
    ("transport", "map"): (_ALL, 1.0, 0.0), ("transport", "s_map"): (_ALL, 1.0, 0.0), ("transport", "self_map"): (_ALL, 1.0, 0.0),
}


def _position(row, name, c0, ct, base, got):
    """got == base + t within the entry's spacings and bandwidth fraction; outputs without an entry are held by CHECKS alone"""
    spec = _POSITION.get((row.name, name))
    if spec is None:
        return False
    dims, nsp, frac = spec
    base, got = np.asarray(base, dtype=np.float64), np.asarray(got, dtype=np.float64)
    if dims is None:  # (getKDERangeLinspace of the marginal of dimension 1)
        t, sd = ct.t[1], c0.sd[1]
    else:
        d = dims(c0)
        shape = (len(d),) + (1,) * (base.ndim - 1)
        t, sd = ct.t[d].reshape(shape), c0.sd[d].reshape(shape)
    _hold(f"{row.name}.{name} translated", got - t, base, nsp * ct.sp + frac * sd)
    return True


# ---- the tests -------------------------------------------------------------------------------------------------------------
_BASE = {}


def _base(row, ci, variant="base"):
    key = (row.name, ci, variant)
    if key not in _BASE:
        _BASE[key] = row.call(kdehip, _case(ci, variant))
    return _BASE[key]


PAIRS = [(r.name, ci) for r in ec.ROWS for ci in range(NCASES)]


@pytest.mark.parametrize("rowname,ci", PAIRS)
def test_rescaling_by_powers_of_two(rowname, ci):
    row = ROWS[rowname]
    c0 = _case(ci, "base")
    if rowname == "auto":  # the premise of the rows that go through the bandwidth search: the 1e-6 clamp never acts
        gaps = np.diff(np.sort(c0.pts, axis=1), axis=1)
        assert gaps.min() >= 1e-6, "two neighbours of a marginal are closer than 1e-6: the reference's clamp would act at k = 0"
    base = _base(row, ci)
    assert set(base) == set(row.laws), (sorted(set(base) ^ set(row.laws)), "outputs without a law, or laws without an output")
    CHECKS[rowname](c0, base)                     # the base against the family's model
    for name, law in row.laws.items():            # premise: a scaled value is a normal number
        if law.kind in ("bits", "rel", "near", "search") and law.e(c0) != 0 and np.asarray(base[name]).dtype.kind == "f":
            assert _in_range(base[name], 1022 - 80 * abs(law.e(c0))), \
                f"{rowname}.{name}: a base value times 2^({law.e(c0)} k) is not a normal number at every k: its law is not exact"
    for k in ec.scales_of(row):
        ck = _case(ci, k)
        got = row.call(kdehip, ck)
        for name, law in row.laws.items():
            _law(row, name, law, c0, base[name], ck, got[name])
        if k == -80 and row.resident is not None:  # the resident route: the upload packs on the device
            with _Resident(ck) as cr:
                res = row.resident(kdehip, cr)
            assert res, rowname
            for name, val in res.items():
                if (rowname, name) == ("summary", "fit_cov"):
                    # the host forms X X^T / N in numpy, the device in its own order: 1e-12 of the largest entry, as
                    # tests/test_gpu_summary.py holds the resident covariance
                    _hold("summary.fit_cov resident", val, got[name], 1e-12 * float(np.max(np.abs(got[name]))))
                else:
                    _same(f"{rowname}.{name} resident at k = -80", val, got[name])


@pytest.mark.parametrize("rowname,ci", PAIRS)
def test_translation_by_exact_offsets(rowname, ci):
    row = ROWS[rowname]
    c0, ct = _case(ci, "lattice"), _case(ci, "shifted")
    base = _base(row, ci, "lattice")
    got = row.call(kdehip, ct)
    CHECKS[rowname](ct, got)                      # positions (and everything else) against the model on the translated inputs
    for name, law in row.laws.items():
        if law.t == "same":
            _same(f"{rowname}.{name} translated", np.asarray(got[name]), np.asarray(base[name]))
        elif law.t == "leaves":
            # a density's arrays: the leaves are the inputs and move by t exactly, with the bandwidth they were given
            dims = _FREE(c0) if name.startswith("cond_") else [0, c0.D - 1] if name.startswith("marg_") else _ALL(c0)
            d = len(dims)
            n = np.asarray(base[name]).size // (2 * d)
            leaves0 = np.asarray(base[name])[n * d:].reshape(n, d)
            leaves = np.asarray(got[name])[n * d:].reshape(n, d)
            move = 0.0 if name.endswith("bandwidth") else ct.t[dims][None, :]
            _same(f"{rowname}.{name} leaves translated", leaves, leaves0 + move)
        elif law.t == "pos":
            held = _position(row, name, c0, ct, base[name], got[name])
            assert held or (rowname, name) in MODEL_ONLY, f"{rowname}.{name}: a position that nothing holds"
        elif law.t == "close":
            assert (rowname, name) in MODEL_ONLY, f"{rowname}.{name}: no reason on record"
            if (rowname, name) == ("conditional", "var"):
                F = _FREE(c0)
                R = (c0.pts.max(axis=1) - c0.pts.min(axis=1))[F][:, None]
                _hold("conditional.var translated", got[name], base[name], 2e-12 * (R * R + (c0.sd * c0.sd)[F][:, None]))


# positions under translation that are held by their model alone (CHECKS on the translated case), with the reason
MODEL_ONLY = {
    ("mass", "quantile"), ("mass", "median"), ("mass", "interval"),  # F_model(x) = alpha within the stated bound: x itself is
    # the root of an iteration that stops on the cdf, so two runs may stop a Newton step apart
    ("summary", "max"),  # a grid point: the argmax may move to a neighbour of equal height; the model holds its height
    # "close", not a position.  Section 5i takes the first and second moments about r, the ROOT NODE'S MEAN, and forms
    # var_k = v_k + S2_k / S_0 - (S1_k / S_0)^2.  r is a weighted mean of all points, rounded at 2^20 where the data are
    # translated: r(x + t) != r(x) + t in the last bits, every difference c_ik - r_k moves with it, and so does the rounding of
    # the two moments that cancel.  The header promises an absolute error in proportion to the squared range, which is what
    # `_check_conditional` holds the translated result to; between the two runs twice that is allowed.
    ("conditional", "var"),
}
