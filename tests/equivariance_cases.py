"""The table of tests/test_gpu_equivariance.py: one row per public entry of the package, with the law every output of the entry
obeys when its data are rescaled by s = 2^k in ALL dimensions, and what the output does when the data are translated by an
exactly representable offset.  Imports without a GPU and without the library: a row's `call(kd, c)` takes the package as an
argument and a case as a namespace, and is only ever run by the GPU module.

"Every" is checked: tests/test_equivariance_table.py reads kerneldensityestimate.jl_amd/__init__.py as text and wants each
public name in exactly one row's `entries` or in EXCLUDED (with the reason), both in this file -- and likewise, under the
name `module.name`, each public function and class of a module of the package that __init__.py imports nothing from (the
families whose surface is methods of BallTreeDensity / DeviceDensity plus such a module: `refit`, `transport`).

The laws, derived from the formulas of include/kdehip.h and not from the kernels.  With the points, the queries, the bounds
and the bandwidths (standard deviations) multiplied by 2^k -- np.ldexp, so exactly -- every difference d, its square, the
factor -1/(2 v) and their product scale exactly, `fma(d * d, -1/(2v), acc)` rounds the same real number, and every correctly
rounded root and quotient of exactly scaled operands is the exactly scaled result.  The exponents a_i are therefore the same
bits, and so is everything formed from them and the weights alone.  What remains is how often the unit of length enters:

  bits(e)   the output is the base output times 2^(e k), bit for bit: np.array_equal(np.ldexp(base, e * k), scaled).  e = 0:
            the same bits (integers -- labels, iteration counts, flags, tile counts -- are compared with ==).
  add(c)    the output is the base output plus c k ln 2, within the family's own bound for a log density,
            |delta| <= 1e-12 * max(1, |ref|) (tests/test_gpu_logdensity.py): log of a norm that holds 2^(c k) is not exact.
  inv()     the output does not change, within 1e-12 * max(1, |ref| + D |k| ln 2): a difference or a weighted mean of logs,
            each of which obeys add() and is held to its bound at its own magnitude.
  rel(e)    the output is the base output times 2^(e k) within n * 1e-12 * max(1, |log |value||, D |k| ln 2) relative: the
            exponential, formed on the host, of n values that obey add() or inv() and are held to their bounds.
  near(e)   (the modes alone) the base output times 2^(e k) within 1e-6 bandwidths, the bound tests/test_gpu_modes.py holds
            the end points of the iteration to: a mode is the first, in descending log p, of the converged points that
            reached it, and log p obeys add().
  search    (the bandwidth search alone) the base output times 2^(e k) within e * 1e-9 relative, the bound of
            test_loocv_bandwidth_parity_with_oracle, with the same number of likelihood evaluations; where the searched
            bandwidth is multiplied by n scale factors of `adaptive_scales` (kde_adaptive with ks=None) rel()'s bound for
            them is added.
  field by field   a density (`kde`, `marginal`, `condition`, `kde_varbw`, ...) is returned as its arrays: centers, ranges,
            means scale with e = 1, the variances with e = 2, the weights and every index array with e = 0.

Under a translation by t (per dimension one of +-2^20, +-3 2^19; every coordinate a multiple of 2^-20 below 2^6, so that x + t
is exact) an output is either "same" -- bit for bit the untranslated one: everything formed from differences -- or "pos": a
position, held to its family's model on the translated inputs by the GPU module, "close" -- not a position, but held to the
model at the family's bound and not to bits, the operation responsible named in the GPU module --, or None where the module
states no claim.

`scales`: the k a row is run at.  None: all of K.  The rows that go through the reference's bandwidth search run at k >= 0
only, with the reason in `restriction`.

Circular dimensions are out of scope: a period of 2 pi cannot be rescaled, and rescaling only the other dimensions changes
which dimension the tree builder finds widest, so the tree is another tree and no output is comparable bit for bit.  The
manifold arguments are left at their defaults everywhere in this table."""
import math
from types import SimpleNamespace

import numpy as np

K = (-80, -30, 30, 80)
BASE_CASES = [(4, 129, 257), (5, 257, 129), (7, 129, 257), (8, 130, 3)]  # (D, N, Nq); the second density takes the next N
NDRAW = 96
LEVELS = np.array([0.025, 0.3, 0.5, 0.975])
SEED = 20261020


class Law:
    """kind: bits / add / inv / rel; e: the exponent's multiple of k (or the additive law's c), a number or a function of the
    case; t: "same", "pos" or None or "close" under translation; why: for an output that is not a bit law, the operation that is not
    scale-exact"""

    def __init__(self, kind, e=0, t="same", why=None, n=1):
        self.kind, self._e, self.t, self.why, self.n = kind, e, t, why, n

    def e(self, c):
        return int(self._e(c)) if callable(self._e) else int(self._e)


def bits(e=0, t="same"):
    return Law("bits", e, t)


def add(c, t="same", why="log of a norm or of a distance that holds a power of the unit of length"):
    return Law("add", c, t, why)


def inv(t="same", why="a difference or weighted mean of logs, each shifted by a multiple of k ln 2"):
    return Law("inv", 0, t, why)


def rel(e, t="same", why="exp, on the host, of a log density that obeys the additive law", n=1):
    return Law("rel", e, t, why, n)


def search(e, t="same", lam=0):
    """lam: the number of factors lambda of adaptive_scales (each under rel()) that multiply the searched bandwidth"""
    return Law("search", e, t, "the golden-section search stops on a relative tolerance and its likelihoods are sums of logs", lam)


def near(e, t="pos"):
    return Law("near", e, t, "the merge of the converged points, on the host, takes them in descending log p, which obeys a "
               "tolerance law: among points that reached the same mode another one may come first and found it")


D_ = lambda c: c.D          # noqa: E731
mD = lambda c: -c.D         # noqa: E731
mD1 = lambda c: -c.D - 1    # noqa: E731
mD2 = lambda c: -c.D - 2    # noqa: E731
mG = lambda c: -len(c.G)    # noqa: E731

# the arrays of a density, field by field: (name, where it lives, exponent)
TREE_FIELDS = [("centers", "bt", 1), ("ranges", "bt", 1), ("weights", "bt", 0), ("left_child", "bt", 0), ("right_child", "bt", 0),
               ("lowest_leaf", "bt", 0), ("highest_leaf", "bt", 0), ("permutation", "bt", 0), ("means", "bd", 1),
               ("bandwidth", "bd", 2), ("bandwidthMin", "bd", 2), ("bandwidthMax", "bd", 2)]


def fields(bd, prefix=""):
    """a host density as {prefix + field: a copy of the array}"""
    return {prefix + name: np.array(getattr(bd.bt if where == "bt" else bd, name)) for name, where, _ in TREE_FIELDS}


def field_laws(prefix="", bandwidth=None, translated=True):
    """the field-by-field law of a density; under translation the topology, the weights, the ranges and the extreme variances
    stay; of the centres, the means and the variances the LEAVES are claimed ("leaves": the inputs, moved by t exactly, and
    the bandwidth as given) -- an inner node's mean is a weighted mean formed at 2^20 and its variance holds the spread of
    those means.  `bandwidth`: another law for the three variance arrays"""
    out = {}
    for name, _, e in TREE_FIELDS:
        law = bits(e, "leaves" if name in ("centers", "means", "bandwidth") else "same")
        if bandwidth is not None and name.startswith("bandwidth"):
            law = Law(bandwidth.kind, bandwidth._e, law.t, bandwidth.why, bandwidth.n)
        if not translated:  # a density of DRAWS: its points are positions that round at 2^20, so the tree is not claimed
            law.t = None
        out[prefix + name] = law
    return out


class Row:
    """`entries`: the public names the row covers; `model`: the family's model in tests/, or the words "no model" and what the
    base is held to instead; `call(kd, c)` -> {output: array or number}; `laws[output]`; `resident(kd, c)`, where the family has
    a DeviceDensity entry, -> some of the same outputs from resident densities (c.dp, c.dq, ...), equal to the host call's bit
    for bit"""

    def __init__(self, name, entries, model, call, laws, resident=None, scales=None, restriction=None):
        self.name, self.entries, self.model, self.call, self.laws = name, tuple(entries), model, call, laws
        self.resident, self.scales, self.restriction = resident, scales, restriction


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def _kde(kd, c):
    out = fields(kd.kde(c.pts, c.sd, c.w))
    out.update(fields(kd.kde_b(c.pts, c.sd[:1], None), "one_"))               # one bandwidth for all dimensions, no weights
    out.update(fields(kd.kde_batch([(c.pts, c.sd, c.w)], device=0)[0], "gpu_"))  # the GPU builder
    return out


def _evaluate(kd, c):
    return dict(p=kd.evaluateDualTree(c.p, c.X), functor=c.p(c.X), loo=kd.evaluateDualTree(c.p, lvFlag=True),
                at=kd.evaluateDualTree(c.p, c.at))


def _evaluate_resident(kd, c):
    return dict(p=c.dp.evaluate(c.X), functor=c.dp(c.X), loo=c.dp.evaluate(lvFlag=True), at=c.dp.evaluate(c.dat))


def _evaluate_log(kd, c):
    return dict(logp=kd.evaluate_log(c.p, c.X), loo=kd.evaluate_log(c.p, lvFlag=True))


def _evaluate_log_resident(kd, c):
    return dict(logp=c.dp.evaluate_log(c.X), loo=c.dp.evaluate_log(lvFlag=True))


def _loglik(kd, c, p=None, q=None):
    p, q = (c.p, c.q) if p is None else (p, q)
    out = {}
    for name, kw in (("", {}), ("_log", dict(log_domain=True))):
        out["ll" + name] = kd.evalAvgLogL(p, q, **kw)
        out["ll_self" + name] = kd.evalAvgLogL(p, p, **kw)
        out["entropy" + name] = kd.entropy(p, **kw)
        out["kld" + name] = kd.kld(p, q, **kw)
        out["minkld" + name] = kd.minkld(p, q, **kw)
    return out


def _loglik_resident(kd, c):
    return _loglik(kd, c, c.dp, c.dq)


def _ksum(kd, c, p=None, q=None):
    p, q = (c.p, c.q) if p is None else (p, q)
    return dict(S=kd.kernel_sum(p, q, c.v), S_norm=kd.kernel_sum(p, q, c.v, normalize=True), inters=kd.intersIntg(p, q),
                ise=kd.ise(p, q), mmd=kd.mmd(p, q, c.sd_mmd))


def _ksum_resident(kd, c):
    return _ksum(kd, c, c.dp, c.dq)


def _grad(kd, c, p=None):
    p = c.p if p is None else p
    logp, g = kd.evaluate_grad(p, c.X)
    val, pg = kd.evaluate_grad(p, c.X, log=False)
    return dict(logp=logp, grad=g, p=val, pgrad=pg)


def _grad_resident(kd, c):
    return _grad(kd, c, c.dp)


def _meanshift(kd, c, p=None):
    p = c.p if p is None else p
    x, logp, iters = kd.meanshift(p, c.starts)
    m, mlogp, mass, labels = kd.modes(p, c.starts)
    return dict(x=x, logp=logp, iters=iters, modes=m, modes_logp=mlogp, mass=mass, labels=labels,
                mode=kd.getKDEMode(p, starts=c.starts))


def _meanshift_resident(kd, c):
    return _meanshift(kd, c, c.dp)


def _hess(kd, c, p=None):
    p = c.p if p is None else p
    logp, g, h = kd.evaluate_hess(p, c.X)
    val, pg, ph = kd.evaluate_hess(p, c.X, log=False)
    return dict(logp=logp, grad=g, hess=h, p=val, pgrad=pg, phess=ph)


def _hess_resident(kd, c):
    return _hess(kd, c, c.dp)


def _laplace(kd, c, p=None):
    p = c.p if p is None else p
    cov, definite = kd.laplace(p, c.starts)
    means, covs, mass, logp, mdef = kd.fit_modes(p, c.starts)
    mode, mcov = kd.getKDEModeFit(p, starts=c.starts)
    # the covariances of the modes are `laplace` at the modes, bit for bit: which converged point founds a mode depends on
    # the order of log p (see near()), so the covariances themselves obey no bit law, their being laplace's does
    again, adef = kd.laplace(p, means)
    same = (np.array_equal(covs, again, equal_nan=True) and np.array_equal(mdef, adef) and np.array_equal(mcov, covs[:, :, 0])
            and np.array_equal(mode, means[:, 0]))
    return dict(cov=cov, definite=definite, means=means, fit_is_laplace=np.array([same]), mass=mass, logp=logp,
                modes_definite=mdef, mode=mode)


def _laplace_resident(kd, c):
    return _laplace(kd, c, c.dp)


def _conditional(kd, c, p=None):
    p = c.p if p is None else p
    logz, mean, var = kd.conditional_moments(p, c.G, c.Y)
    W, wlogz = kd.conditional_weights(p, c.G, c.Y)
    pts, ind = kd.sample_conditional(p, c.G, c.Y, seed=SEED)
    out = dict(logz=logz, mean=mean, var=var, W=W, wlogz=wlogz, draws=pts, ind=ind)
    pc = kd.condition(p, c.G, c.Y[:, 0])
    out.update(fields(pc if hasattr(pc, "bt") else pc.download(), "cond_"))
    return out


def _conditional_resident(kd, c):
    return _conditional(kd, c, c.dp)


def _mass(kd, c, p=None):
    p = c.p if p is None else p
    x, resid, iters, conv = kd.quantile(p, LEVELS, 0, full=True)
    lo, hi = kd.interval(p, c.D - 1, 0.9)
    return dict(box=kd.box_mass(p, c.lo, c.hi), box_dims=kd.box_mass(p, c.lo[c.G], c.hi[c.G], c.G), cdf=kd.cdf(p, c.X[0], 0),
                grid=kd.grid_mass(p, c.edges, [0, c.D - 1]), quantile=x, resid=resid, iters=iters, converged=conv,
                median=kd.median(p, 1), interval=np.array([lo, hi]))


def _mass_resident(kd, c):
    return _mass(kd, c, c.dp)


def _evaltol(kd, c, p=None, at=None):
    p, at = (c.p, c.at) if p is None else (p, at)
    vals, stats = kd.evaluate_tol(p, at, rel_tol=1e-3, return_stats=True)
    loo, lstats = kd.evaluate_tol(p, None, rel_tol=1e-3, lvFlag=True, return_stats=True)
    exact = kd.evaluate_tol(p, at, rel_tol=0.0)
    out = dict(vals=vals, stats=np.array(stats), loo=loo, loo_stats=np.array(lstats), exact=exact)
    if p is c.p:  # the reference's switch: evaluateDualTree itself goes within errTol while it is off
        assert kd.getForceEvalDirect()
        kd.setForceEvalDirect(False)
        try:
            out["switch"] = kd.evaluateDualTree(c.p, c.at, errTol=1e-3)
        finally:
            kd.setForceEvalDirect(True)
    return out


def _evaltol_resident(kd, c):
    return _evaltol(kd, c, c.dp, c.dat)


def _knn(kd, c, p=None, at=None, pu=None, qu=None):
    p, at, pu, qu = (c.p, c.at, c.pu, c.qu) if p is None else (p, at, pu, qu)
    d2, idx, stats = kd.knn(p, at, k=8, squared=True, return_stats=True)
    dist, _ = kd.knn(p, at, k=8)
    l2, lidx = kd.knn(p, k=8, lvFlag=True, squared=True)
    b2, bidx = kd.knn(p, at, k=8, metric="bandwidth", squared=True)
    s2, sidx = kd.knn(p, at, k=8, metric=c.metric, squared=True)
    return dict(d2=d2, idx=idx, stats=np.array(stats), dist=dist, loo_d2=l2, loo_idx=lidx, bw_d2=b2, bw_idx=bidx, sc_d2=s2,
                sc_idx=sidx, entropy_knn=kd.entropy_knn(pu), kld_knn=kd.kld_knn(pu, qu))


def _knn_resident(kd, c):
    return _knn(kd, c, c.dp, c.dat, c.dpu, c.dqu)


def _varbw(kd, c):
    pv = kd.kde_varbw(c.pts, c.bwpp, c.w)
    out = fields(pv, "pv_")
    out.update(p=kd.evaluateDualTree(pv, c.X), logp=kd.evaluate_log(pv, c.X), loo=kd.evaluate_log(pv, lvFlag=True),
               ll=kd.evalAvgLogL(pv, pv, log_domain=True), lam_abramson=kd.adaptive_scales(c.p),
               lam_knn=kd.adaptive_scales(c.p, method="knn"))
    out.update(fields(kd.kde_adaptive(c.pts, c.sd, c.w), "ad_"))
    return out


def _varbw_resident(kd, c):
    with kd.DeviceDensity(kd.kde_varbw(c.pts, c.bwpp, c.w)) as dv:
        return dict(p=dv.evaluate(c.X), logp=dv.evaluate_log(c.X), loo=dv.evaluate_log(lvFlag=True),
                    ll=kd.evalAvgLogL(dv, dv, log_domain=True))


def _prodexact(kd, c, p=None, q=None):
    p, q = (c.p, c.q) if p is None else (p, q)
    pts, ind, logz = kd.prod_exact(p, q, NDRAW, seed=SEED, return_logz=True)
    means, w, sd = kd.product_components(p, q)
    return dict(draws=pts, ind=ind, logz=logz, means=means, weights=w, sd=sd, log_inters=kd.log_intersIntg(p, q))


def _prodexact_resident(kd, c):
    return _prodexact(kd, c, c.dp, c.dq)


def _bwjoint(kd, c, p=None):
    p = c.p if p is None else p
    bw, info = kd.joint_bandwidth(p, return_info=True)
    out = dict(bw=bw, var=bw * bw, logl=info["logl"], iters=info["iters"], status=info["status"], trace=info["trace"],
               bw_start=kd.joint_bandwidth(p, start=c.sd2, maxiter=3))
    if p is c.p:
        out.update(fields(kd.kde_joint(c.pts, c.w, start=c.sd, maxiter=5), "kj_"))
    return out


def _bwjoint_resident(kd, c):
    return _bwjoint(kd, c, c.dp)


def _summary(kd, c, p=None, q=None):
    p, q = (c.p, c.q) if p is None else (p, q)
    mu, cov = kd.getKDEfit(p)
    mx, vals = kd.getKDEMax(p, 65, values=True)
    p1, p2, q2 = kd.marginal(p, [1]), kd.marginal(p, [0, c.D - 1]), kd.marginal(q, [0, c.D - 1])
    out = dict(mean=kd.getKDEMean(p), range=kd.getKDERange(p, 0.25), fit_mean=mu, fit_cov=cov, max=mx, max_values=vals,
               linspace=kd.getKDERangeLinspace(p1, 0.1, 33), appx=kd.intersIntgAppxIS(p2, q2, 33))
    out.update(fields(p2 if hasattr(p2, "bt") else p2.download(), "marg_"))
    return out


def _summary_resident(kd, c):
    return _summary(kd, c, c.dp, c.dq)


def _sample(kd, c, p=None):
    p = c.p if p is None else p
    pts, ind = kd.sample(p, NDRAW, seed=SEED)
    given, gind = kd.sample(p, NDRAW, ind=c.labels, seed=SEED, sample_offset=7)
    out = dict(draws=pts, ind=ind, given=given, given_ind=gind)
    if p is c.p:
        out["rand"] = kd.rand(p, NDRAW, seed=SEED)
    return out


def _sample_resident(kd, c):
    return _sample(kd, c, c.dp)


def _auto(kd, c):
    bw, evals = kd.auto_bandwidth(c.pts, return_evals=True)
    out = dict(bw=bw, evals=evals)
    out.update(fields(kd.kde_auto(c.pts), "auto_"))
    out.update(fields(kd.kde(c.pts), "kde_"))
    out.update(fields(kd.kde_adaptive(c.pts), "adp_"))   # ks=None: the pilot is kde(points)
    return out


def _resample(kd, c, p=None):
    p = c.p if p is None else p
    r = kd.resample(p, NDRAW, seed=SEED)
    if hasattr(r, "bt"):
        out = fields(r, "rs_")
    else:
        out = fields(r.download(), "rs_")
        r.close()
    if p is c.p:
        out.update(fields(kd.resample(p, NDRAW, "discrete", seed=SEED), "rd_"))
    return out


def _resample_resident(kd, c):
    return _resample(kd, c, c.dp)


def _mul_exact(kd, c):
    with kd.DeviceDensity(c.p) as dp, kd.DeviceDensity(c.q) as dq:
        out = kd.mul_exact(dp, dq, NDRAW, seed=SEED)
        got = dict(fields(out.download(), "mx_"), bw=np.array(out.bw), evals=out.nevals)
        out.close()
    return got


def _module(kd, name):
    """a module of the package that its __init__ does not import"""
    import importlib
    return importlib.import_module(kd.__name__ + "." + name)


def _all_dims(kd, dp):
    """a BUILT twin of an uploaded density -- its marginal over all dimensions, made on the device without a bandwidth search
    (tests/test_gpu_refit.py G8) --: the refit of a built density keeps the twelve arrays and can be downloaded"""
    return dp.marginal(list(range(dp.dims)))


def _refit_on_device(kd, dm, c):
    """the four refits of the built resident density dm, downloaded, and whether a batch of the same four gives their bits"""
    from tests import refit_model as rm
    rf = _module(kd, "refit")
    made = [dm.changeWeights(c.rw), dm.movePoints(c.rdelta), rf.refit_device(dm, c.rw, rf.WEIGHTS, c.rdelta)[0]]
    upd, le, ess = dm.bayes_update(c.logl)
    made.append(upd)
    batch = kd.DeviceDensity.refit_batch([dict(density=dm, weights=c.rw), dict(density=dm, delta=c.rdelta),
                                          dict(density=dm, weights=c.rw, delta=c.rdelta), dict(density=dm, logl=c.logl)])
    host = [d.download() for d in made]
    same = batch[3][1:] == (le, ess) and all(b[1] is None and b[2] is None for b in batch[:3])
    for (b, _, _), h in zip(batch, host):
        try:
            rm.same_bits(b.download(), h, "a batch item")
        except AssertionError:
            same = False
        b.close()
    for d in made:
        d.close()
    return host, le, ess, same


def _refit(kd, c):
    p = c.p
    rf = _module(kd, "refit")
    made = [p.changeWeights(c.rw), p.movePoints(c.rdelta), rf.refit_host(p, new_weights=c.rw, delta=c.rdelta)]
    upd, le, ess = p.bayes_update(c.logl)
    out = dict(log_evidence=le, ess=ess)
    for d, pre in zip(made + [upd], ("cw_", "mv_", "both_", "by_")):
        out.update(fields(d, pre))
    # the results as inputs of a consumer: what the resident route is compared by (the refit of an UPLOADED density has no
    # arrays to download)
    out.update(cw_p=kd.evaluateDualTree(made[0], c.X), mv_p=kd.evaluateDualTree(made[1], c.X), both_p=kd.evaluateDualTree(made[2], c.X))
    # the device's refit has arithmetic of its own in the Bayes update (the host's is numpy's), so it gets laws of its own; on
    # a built twin, whose arrays (dsrc_) are part of the output
    with kd.DeviceDensity(p) as up, _all_dims(kd, up) as dm:
        out.update(fields(dm.download(), "dsrc_"))
        host, dle, dess, same = _refit_on_device(kd, dm, c)
    for d, pre in zip(host, ("dcw_", "dmv_", "dboth_", "dby_")):
        out.update(fields(d, pre))
    out.update(dev_log_evidence=dle, dev_ess=dess, batch_is_singles=np.array([same]))
    return out


def _refit_resident(kd, c):
    rf = _module(kd, "refit")
    with c.dp.changeWeights(c.rw) as a, c.dp.movePoints(c.rdelta) as b, rf.refit_device(c.dp, c.rw, rf.WEIGHTS, c.rdelta)[0] as ab:
        return dict(cw_p=a.evaluate(c.X), mv_p=b.evaluate(c.X), both_p=ab.evaluate(c.X))


OT = dict(reg=1.0, tol=0.0, maxiter=8)   # a fixed number of steps, ending on a round boundary: no comparison with a tolerance
_OT_SCALARS = ("value", "transport_cost", "err", "mass", "iters")
_OT_VECTORS = ("phi", "gamma", "delta", "map")


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _ot_item(info, prefix, leaf=None):
    """the outputs of one item; a resident item's displacement comes in leaf order and goes back to the order of getPoints"""
    out = {prefix + k: info[k] for k in _OT_SCALARS}
    out.update({prefix + k: np.ascontiguousarray(_np(info[k])) for k in ("phi", "gamma", "map")})
    if "delta" in info:
        out[prefix + "delta"] = info["delta"]
    else:
        delta = np.empty_like(out[prefix + "map"])
        delta[:, leaf] = _np(info["delta_leaf"])
        out[prefix + "delta"] = delta
    return out


def _moved(kd, c, d, prefix):
    """a moved density: its values at the queries -- on both routes -- and, of a host density, its arrays"""
    if hasattr(d, "bt"):
        return {prefix + "p": kd.evaluateDualTree(d, c.X), **fields(d, prefix)}
    with d:
        return {prefix + "p": d.evaluate(c.X)}


def _transport(kd, c, p=None, q=None):
    p, q = (c.p, c.q) if p is None else (p, q)
    leaf = c.p.bt.permutation[c.N:] - 1
    out = {}
    T, info = p.transport_map(q, return_info=True, **OT)
    out.update(_ot_item(info, "", leaf))
    out.update(_ot_item(p.sinkhorn(q, scale=c.ot_scale, return_info=True, **OT)[1], "s_", leaf))
    out.update(_ot_item(p.sinkhorn(p, return_info=True, **OT)[1], "self_", leaf))
    S, dv = p.sinkhorn_divergence(q, return_info=True, **OT)
    S2, dv2 = p.sinkhorn_divergence(q, scale=c.ot_scale, return_info=True, **OT)
    out.update(S=S, S_cross=dv["cross"], S_self_p=dv["self_p"], S_self_q=dv["self_q"], S_iters=np.array(dv["iters"]),
               s_S=S2, s_S_self_p=dv2["self_p"], s_S_self_q=dv2["self_q"])
    out["map_is_info"] = np.array([np.array_equal(_np(T), out["map"]) and info["value"] == p.sinkhorn(q, **OT)])
    out.update(_moved(kd, c, p.transport_to(q, **OT), "to_"))
    out.update(_moved(kd, c, p.transport_to(q, scale=c.ot_scale, **OT), "s_to_"))
    out.update(_moved(kd, c, p.equalize(**OT), "eq_"))
    if p is c.p:  # the batch of the same pairs on resident twins: each item bit for bit the single call's
        with kd.DeviceDensity(c.p) as dp, kd.DeviceDensity(c.q) as dq:
            batch = kd.DeviceDensity.sinkhorn_batch([dict(p=dp, q=dq), dict(p=dp, q=dq, scale=c.ot_scale), dict(p=dp, q=dp)],
                                                    vectors=True, **OT)
            same = True
            for item, prefix in zip(batch, ("", "s_", "self_")):
                got = _ot_item(item, prefix, leaf)
                same = same and all(np.float64(got[k]).tobytes() == np.float64(out[k]).tobytes()
                                    for k in (prefix + n for n in _OT_SCALARS))
                same = same and all(np.array_equal(got[k], out[k]) for k in (prefix + n for n in _OT_VECTORS))
        out["batch_is_singles"] = np.array([same])
    return out


def _transport_resident(kd, c):
    return _transport(kd, c, c.dp, c.dq)


def _moved_laws(prefix):
    """a density whose points are images under the map: under translation they are positions that round at 2^20, so of its
    arrays the weights and the topology are claimed and the centres, ranges, means and variances are not"""
    out = {prefix + name: bits(e, "same" if where == "bt" and e == 0 else None) for name, where, e in TREE_FIELDS}
    out[prefix + "p"] = bits(mD, None)   # its values at the queries: what the resident route is compared by
    return out


def _ot_laws(prefix):
    return {**{prefix + k: bits(0) for k in _OT_SCALARS + ("phi", "gamma")}, prefix + "delta": bits(1), prefix + "map": bits(1, "pos")}


# the search's result: the base bandwidth times 2^k within the 1e-9 relative bound of test_loocv_bandwidth_parity_with_oracle
_NO_CLAMP = ("the reference clamps the search's lower end, minm, to 1e-6 (src/CrossValidation.jl, golden_init in csrc/loocv.hip): an "
             "absolute length.  For k >= 0 the premise is that the smallest gap between sorted neighbours of every marginal of the "
             "base is at least 1e-6, so the clamp never acts at any scale that is run")

ROWS = [
    Row("kde", ["kde", "kde_b", "kde_batch"], "tests/pymodel.py (kde), the second restatement of the reference's builder",
        _kde, {**field_laws(), **field_laws("one_"), **field_laws("gpu_")}),
    Row("evaluate", ["evaluateDualTree", "DeviceDensity"], "tests/evaltol_model.py (direct_fsum: one exactly rounded sum per query)",
        _evaluate, dict(p=bits(mD), functor=bits(mD), loo=bits(mD), at=bits(mD)), _evaluate_resident),
    Row("evaluate_log", ["evaluate_log"], "tests/logdensity_model.py",
        _evaluate_log, dict(logp=add(mD), loo=add(mD)), _evaluate_log_resident),
    Row("loglik", ["evalAvgLogL", "entropy", "kld", "minkld"], "tests/logdensity_model.py (eval_avg_logl_log, kld_log)",
        _loglik, {**{n + s: add(mD) for n in ("ll", "ll_self") for s in ("", "_log")},
                  **{"entropy" + s: add(D_) for s in ("", "_log")},
                  **{n + s: inv() for n in ("kld", "minkld") for s in ("", "_log")}}, _loglik_resident),
    Row("ksum", ["kernel_sum", "intersIntg", "ise", "mmd"], "tests/ksum_model.py",
        _ksum, dict(S=bits(0), S_norm=bits(mD), inters=bits(mD), ise=bits(mD), mmd=bits(0)), _ksum_resident),
    Row("grad", ["evaluate_grad"], "tests/modes_model.py (evaluate_grad)",
        _grad, dict(logp=add(mD), grad=bits(-1), p=bits(mD), pgrad=bits(mD1)), _grad_resident),
    Row("meanshift", ["meanshift", "modes", "getKDEMode"], "tests/modes_model.py (step, meanshift)",
        _meanshift, dict(x=bits(1, "pos"), logp=add(mD, None), iters=bits(0, None), modes=near(1), modes_logp=add(mD, None),
                         mass=bits(0), labels=bits(0), mode=near(1)), _meanshift_resident),
    Row("hess", ["evaluate_hess"], "tests/curvature_model.py (evaluate_hess)",
        _hess, dict(logp=add(mD), grad=bits(-1), hess=bits(-2), p=rel(mD), pgrad=rel(mD1), phess=rel(mD2)), _hess_resident),
    Row("laplace", ["laplace", "fit_modes", "getKDEModeFit"], "tests/curvature_model.py (laplace, cov_bound)",
        _laplace, dict(cov=bits(2), definite=bits(0), means=near(1), fit_is_laplace=bits(0), mass=bits(0), logp=add(mD, None),
                       modes_definite=bits(0), mode=near(1)), _laplace_resident),
    Row("conditional", ["conditional_moments", "conditional_weights", "sample_conditional", "condition"],
        "tests/conditional_model.py",
        _conditional, {**dict(logz=add(mG), mean=bits(1, "pos"), var=bits(2, "close"), W=bits(0), wlogz=add(mG), draws=bits(1, "pos"),
                              ind=bits(0)), **field_laws("cond_")}, _conditional_resident),
    Row("mass", ["box_mass", "cdf", "grid_mass", "quantile", "median", "interval"], "tests/mass_model.py",
        _mass, dict(box=bits(0), box_dims=bits(0), cdf=bits(0), grid=bits(0), quantile=bits(1, "pos"), resid=bits(0, None),
                    iters=bits(0, None), converged=bits(0, None), median=bits(1, "pos"), interval=bits(1, "pos")), _mass_resident),
    Row("evaltol", ["evaluate_tol", "setForceEvalDirect", "getForceEvalDirect"],
        "tests/evaltol_model.py (direct_fsum and the guarantee of section 5m; plan for the tile counts)",
        _evaltol, dict(vals=bits(mD), stats=bits(0), loo=bits(mD), loo_stats=bits(0), exact=bits(mD), switch=bits(mD)),
        _evaltol_resident),
    Row("knn", ["knn", "entropy_knn", "kld_knn"], "tests/knn_model.py",
        _knn, dict(d2=bits(2), idx=bits(0), stats=bits(0), dist=bits(1), loo_d2=bits(2), loo_idx=bits(0), bw_d2=bits(0),
                   bw_idx=bits(0), sc_d2=bits(0), sc_idx=bits(0), entropy_knn=add(D_, why="a sum of logs of distances"),
                   kld_knn=inv(why="a mean of logs of ratios of distances: log(nu / rho), the ratio exact")), _knn_resident),
    Row("varbw", ["kde_varbw", "adaptive_scales", "kde_adaptive"], "tests/varbw_model.py",
        _varbw, {**field_laws("pv_"), **dict(p=bits(mD), logp=add(mD), loo=add(mD), ll=add(mD),
                                             lam_abramson=rel(0, why="exp of a weighted mean of log densities, on the host"),
                                             lam_knn=rel(0, why="exp of a weighted mean of logs of distances, on the host")),
                 **field_laws("ad_", bandwidth=rel(2, why="the pilot's variance times lambda^2, lambda from adaptive_scales", n=2))},
        _varbw_resident),
    Row("prodexact", ["prod_exact", "product_components", "log_intersIntg"], "tests/prodexact_model.py",
        _prodexact, dict(draws=bits(1, "pos"), ind=bits(0), logz=add(mD), means=bits(1, "pos"), weights=bits(0), sd=bits(1),
                         log_inters=add(mD)), _prodexact_resident),
    Row("bwjoint", ["joint_bandwidth", "kde_joint"], "tests/bwjoint_model.py",
        _bwjoint, {**dict(bw=bits(1), var=bits(2), logl=add(mD), iters=bits(0), status=bits(0), trace=add(mD), bw_start=bits(1)),
                   **field_laws("kj_")}, _bwjoint_resident),
    Row("summary", ["getKDEMean", "getKDERange", "getKDERangeLinspace", "getKDEMax", "getKDEfit", "marginal", "intersIntgAppxIS"],
        "no model of its own in tests/ for Euclidean data (tests/summary_circular_model.py is the circle's): the base is held "
        "to the formulas of section 5e written out in numpy, and the grid values to tests/evaltol_model.py's direct sum",
        _summary, {**dict(mean=bits(1, "pos"), range=bits(1, "pos"), fit_mean=bits(1, "pos"), fit_cov=bits(2, None),
                          max=bits(1, "pos"), max_values=bits(-1, None), linspace=bits(1, "pos"), appx=bits(-2, None)),
                   **field_laws("marg_")}, _summary_resident),
    Row("sample", ["sample", "rand"], "no model in tests/: the base is held to the centre of the drawn label plus the "
        "bandwidth times the device's own normals, as tests/test_gpu_sample.py does",
        _sample, dict(draws=bits(1, "pos"), ind=bits(0), given=bits(1, "pos"), given_ind=bits(0), rand=bits(1, "pos")),
        _sample_resident),
    Row("auto", ["auto_bandwidth", "kde_auto"], "no model in tests/: the oracle's search (oracle.auto_bandwidth), the reference of "
        "test_loocv_bandwidth_parity_with_oracle, at its 1e-9",
        _auto, {**dict(bw=search(1), evals=bits(0)), **field_laws("auto_", bandwidth=search(2)),
                **field_laws("kde_", bandwidth=search(2)), **field_laws("adp_", bandwidth=search(2, lam=2))},
        scales=(30, 80), restriction=_NO_CLAMP),
    Row("resample", ["resample"], "no model in tests/: the draws are `sample`'s (its row holds them to the label's centre plus the "
        "bandwidth times the device's normals), the bandwidth is held to the oracle's search on those draws",
        _resample, {**field_laws("rs_", bandwidth=search(2), translated=False), **field_laws("rd_")}, _resample_resident,
        scales=(30, 80), restriction=_NO_CLAMP + "; here the points are the draws, and the premise is asserted on them"),
    Row("mul_exact", ["mul_exact"], "tests/prodexact_model.py through `prod_exact`'s row: the points are its draws, bit for bit; "
        "the bandwidth is held to the oracle's search on those draws",
        _mul_exact, {**field_laws("mx_", bandwidth=search(2), translated=False), **dict(bw=search(1, None), evals=bits(0, None))},
        scales=(30, 80), restriction=_NO_CLAMP + "; here the points are the draws, and the premise is asserted on them"),
    # the two families whose surface is methods (BallTreeDensity / DeviceDensity) plus a module that __init__ does not re-export
    Row("refit", ["refit.refit_host", "refit.bayes_weights", "refit.host_bayes_update", "refit.refit_device",
                  "refit.device_bayes_update", "refit.refit_batch"],
        "tests/refit_model.py (the arrays, bit for bit); the Bayes weights, evidence and ess against the formula in extended "
        "precision (tests/test_refit_host.py bayes_reference)",
        _refit, {**{n: law for pre in ("cw_", "mv_", "both_", "by_", "dsrc_", "dcw_", "dmv_", "dboth_", "dby_")
                    for n, law in field_laws(pre).items()},
                 **dict(cw_p=bits(mD), mv_p=bits(mD), both_p=bits(mD)),
                 **dict(log_evidence=bits(0), ess=bits(0), dev_log_evidence=bits(0), dev_ess=bits(0), batch_is_singles=bits(0))},
        _refit_resident),
    Row("transport", ["transport.sinkhorn", "transport.sinkhorn_batch", "transport.sinkhorn_divergence", "transport.transport_map",
                      "transport.transport_to", "transport.equalize"],
        "tests/transport_model.py (iterate, divergence).  reg = 1, tol = 0 and eight steps, so that the step count is no "
        "comparison with a tolerance; once at the default scale and once (s_) at a scale from the caller that is rescaled with "
        "the data.  The moved densities (to_, s_to_, eq_): under translation their points are positions that round at 2^20, so "
        "the statistics of their inner nodes differ and only the weights and the topology are claimed",
        _transport, {**_ot_laws(""), **_ot_laws("s_"), **_ot_laws("self_"),
                     **{k: bits(0) for k in ("S", "S_cross", "S_self_p", "S_self_q", "S_iters", "s_S", "s_S_self_p", "s_S_self_q",
                                             "map_is_info", "batch_is_singles")},
                     **_moved_laws("to_"), **_moved_laws("s_to_"), **_moved_laws("eq_")},
        _transport_resident),
]

EXCLUDED = {
    # the Gibbs products: the contract itself is not equivariant
    **{name: "Gibbs product: the reference's rule `pT < 1e-99` (src/MSGibbs01.jl, sampleIndex) replaces the label by a uniform "
             "draw, and 1e-99 is absolute in density units, so the contract itself is not equivariant"
       for name in ("prodAppxMSGibbsS", "prodAppxMSGibbsS_batch", "prodAppxMSGibbsS_device", "prodAppxMSGibbsS_resident", "gibbs1",
                    "mul", "mul_device", "mul_device_batch")},
    # plans and what belongs to them
    **{name: "a plan or its bookkeeping: it holds packed Gibbs levels and computes nothing of its own"
       for name in ("ProductPlan", "MultiProductPlan", "ProductBatch", "batch_launches", "nlevels", "GbGlb", "makeEmptyGbGlb")},
    "philox_streams": "random numbers from a seed: no data and no unit enter it",
    # the batches: plumbing around the single entries
    **{name: "batch plumbing: every item's results are bit for bit the single entry's, which has a row and is what the batch's "
             "own tests compare with"
       for name in ("sample_device_batch", "eval_avg_logl_device_batch", "kld_batch", "ise_batch", "kernel_sum_device_batch",
                    "mmd_batch", "meanshift_device_batch", "evaluate_hess_device_batch", "conditional_device_batch",
                    "prod_exact_device_batch", "box_mass_device_batch", "quantile_device_batch", "joint_bandwidth_device_batch",
                    "summary_device_batch")},
    # getters, containers and the library itself
    **{name: "a getter: it returns arrays that `kde`'s row already compares field by field"
       for name in ("getPoints", "getBW", "getWeights", "Ndim", "Npts")},
    **{name: "a container of arrays with no arithmetic of its own" for name in ("BallTree", "BallTreeDensity")},
    "density_from_arrays": "wraps arrays the caller built: nothing is computed from them",
    "KdeHipError": "the exception type of the package",
    "LIB_PATH": "the path of the shared library: a string",
    "device_count": "asks the runtime for the number of devices",
    "version": "the version number of the library",
    # modules that __init__ imports nothing from, by their qualified names
    **{"manifold." + name: "parses and packs the manifold argument: it touches no data of a density"
       for name in ("parse", "resolve", "select", "per_product", "per_item", "matrix", "mask", "pointer")},
    **{"sharded." + name: "a wrapper over several processes whose numerics are prodAppxMSGibbsS's, excluded above: the Gibbs "
                          "product's contract is not equivariant"
       for name in ("shard_range", "ShardedProduct", "PendingProduct")},
}


def scales_of(row):
    return K if row.scales is None else tuple(row.scales)


def all_entries():
    """[(public name, where)] over the rows and EXCLUDED"""
    out = [(n, "row " + r.name) for r in ROWS for n in r.entries]
    return out + [(n, "EXCLUDED") for n in EXCLUDED]


def namespace(**kw):
    return SimpleNamespace(**kw)


LN2 = math.log(2.0)
