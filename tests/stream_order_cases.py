"""The case table of tests/test_gpu_stream_order.py: one row per enqueue-only entry of include/kdehip.h.

A row holds the resident densities its entry needs, five argument sets of IDENTICAL shapes -- `true`, `decoy` and `alt1..3`;
where an entry's only inputs are densities, a set names which of the row's equally shaped densities it evaluates --, a closure `enqueue(args, outputs, stream)` that makes the call through `_lib.lib` or the stream-taking
Python wrapper and never synchronises, and `want[set]`, the arrays the BLOCKING entry returns for that set (computed once, when
the row is built, with the device idle).  Because every set of a row has the same shapes and densities, a call that ran with
another call's recycled descriptors would read and write valid memory of the right size: a wrong answer, never a wild access.

Shapes: D = 2, N = 300 leaves (three 128-leaf chunks, the last ragged), Nq = 257 queries (two 256-query blocks, the last with
one lane); batches are three items of the mixed shapes BATCH; draws are 1000 samples; quantiles take five levels.

The premise of a row, asserted when it is built, on the blocking entry's results alone: between any two argument sets
  "all"      every element of the output differs;
  "half"     at least half do (index outputs: two draws may pick the same label);
  "nonzero"  every element that is not exactly 0 in both differs, and at least half of all do (the conditional weights: a leaf
             of weight 0 keeps exactly 0 for every query, and far leaves underflow to it);
  None       the output is compared in every scenario but cannot tell two calls apart, so it carries no premise: `stats`
             (the tile total is a function of the shapes alone), the iteration counts and the converged / definite flags (the
             same small integers for every set), the quantile's residual (of the size of the tolerance, 0 included) and the
             Laplace covariance (NaN wherever the Hessian is not definite).
"""
import ctypes as C
import itertools

import numpy as np

import kdehip
from kdehip import _lib
from tests.helpers import silverman_bw, synth_mixture
from tests.test_gpu_mass import _density

SETS = ("true", "decoy", "alt1", "alt2", "alt3")
D, N, NQ = 2, 300, 257
BATCH = [(1, 5, 3), (2, 129, 257), (3, 300, 7)]          # (D, N, Nq)
COND_BATCH = [(2, 5, 3), (2, 129, 257), (3, 300, 7)]     # (a 1-D density has no dimension left to condition on)
NDRAW, NLEVELS, KNN_K, NGRID = 1000, 5, 8, 17
PROD_NS, PROD_NP, PROD_NITER = (150, 160, 170), 96, 3

_DTYPES = {"f64": np.float64, "i64": np.int64, "i32": np.int32}
_FILL = {"f64": np.nan, "i64": -7, "i32": -7}


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _differ(a, b):
    same = a == b
    if a.dtype.kind == "f":
        same |= np.isnan(a) & np.isnan(b)
    return ~same


def _tells_apart(premise, a, b):
    """the premise of one output between two argument sets (the module's docstring)"""
    d = _differ(a, b)
    if premise == "all":
        return bool(d.all())
    if premise == "half":
        return 2 * int(d.sum()) >= d.size
    if premise == "nonzero":
        return bool(d[(a != 0) | (b != 0)].all()) and 2 * int(d.sum()) >= d.size
    return True


class Row:
    """one entry: `outputs` = [(name, shape, dtype, premise)], `args[set]` = the parameters of a call with its device inputs
    under "inputs", `want[set]` = {output name: array}"""

    def __init__(self, name, kind, outputs, enqueue, densities):
        self.name, self.kind, self.outputs, self.enqueue, self.densities = name, kind, outputs, enqueue, densities
        self.args, self.want = {}, {}

    def add(self, setname, args, want):
        spec = {o[0]: o for o in self.outputs}
        assert set(want) == set(spec), (self.name, sorted(want), sorted(spec))
        self.args[setname] = args
        self.want[setname] = {k: np.ascontiguousarray(v, dtype=_DTYPES[spec[k][2]]).reshape(spec[k][1]) for k, v in want.items()}

    def new_outputs(self):
        """device outputs of this row's shapes, floats NaN and integers -7"""
        import torch
        return {name: torch.full(shape, _FILL[dt], dtype=getattr(torch, {"f64": "float64", "i64": "int64", "i32": "int32"}[dt]),
                                 device="cuda:0") for name, shape, dt, _ in self.outputs}

    def work_inputs(self, setname):
        """caller-owned input arrays of their own, holding `setname`'s values"""
        return {k: t.clone() for k, t in self.args[setname]["inputs"].items()}

    def with_inputs(self, setname, work):
        return dict(self.args[setname], inputs=work)

    def check_premise(self):
        for s, t in itertools.combinations(SETS, 2):
            for k in self.args[s].get("inputs", {}):
                assert self.args[s]["inputs"][k].shape == self.args[t]["inputs"][k].shape, (self.name, k)
            for name, _, _, premise in self.outputs:
                a, b = self.want[s][name], self.want[t][name]
                assert a.shape == b.shape
                assert premise in ("all", "half", "nonzero", None)
                assert _tells_apart(premise, a, b), \
                    f"{self.name}: {name} of {s} and {t}: {int(_differ(a, b).sum())} of {a.size} elements differ"

    def close(self):
        for d in self.densities:
            d.close()
        self.densities = []


def _queries(rng, p, nq):
    """nq positions inside the data: a point of the density each, moved by a bandwidth or so (p > 0 at every one)"""
    pts = kdehip.getPoints(p)
    if pts.shape[1] <= 8:
        # a handful of points: beside one of them a single kernel carries the whole sum, and the curvature, a mean-shift step
        # and a conditional draw no longer depend on where exactly the query lies.  Between a weighted point and its nearest
        # weighted neighbour two kernels do.
        live = pts[:, kdehip.getWeights(p) > 0.0]
        i = rng.integers(0, live.shape[1], size=nq)
        d2 = ((live[:, :, None] - live[:, None, :]) ** 2).sum(axis=0)
        np.fill_diagonal(d2, np.inf)
        j = np.argmin(d2, axis=1)[i]
        t = rng.uniform(0.4, 0.6, size=nq)
        return live[:, i] + t * (live[:, j] - live[:, i])
    k = rng.integers(0, pts.shape[1], size=nq)
    return pts[:, k] + 0.3 * rng.standard_normal((pts.shape[0], nq))


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def _st(stream):
    return _lib.addr(stream)


# ---- rows with a caller-owned device input -------------------------------------------------------------------------------
def _positions_row(name, outputs, call, want, nq=NQ):
    """an entry of one resident density at device positions: `call(d, pos, Nq, out, stream)`, `want(p, pos)`"""
    rng = _rng(name)
    p = _density(rng, D, N)
    d = kdehip.DeviceDensity(p)
    row = Row(name, "input", outputs, lambda a, o, st: call(d, a["inputs"]["pos"], nq, o, _st(st)), [d])
    for s in SETS:
        pos = _queries(rng, p, nq)
        row.add(s, dict(inputs=dict(pos=_dev(pos.T))), want(p, pos))
    return row


def _evaluate_device():
    L = _lib.lib
    return _positions_row("kdehip_evaluate_device", [("p", (NQ,), "f64", "all")],
                          lambda d, pos, nq, o, st: _lib.check(L.kdehip_evaluate_device(d._h, _lib.addr(pos), nq, 0, _lib.addr(o["p"]), st)),
                          lambda p, pos: dict(p=kdehip.evaluateDualTree(p, pos)))


def _evaluate_device_manifold():
    L = _lib.lib
    man = np.array([1, 0], dtype=np.uint8)  # dimension 0 circular
    return _positions_row("kdehip_evaluate_device_manifold", [("p", (NQ,), "f64", "all")],
                          lambda d, pos, nq, o, st: _lib.check(L.kdehip_evaluate_device_manifold(
                              d._h, _lib.addr(pos), nq, 0, _lib.addr(o["p"]), st, _lib.ptr(man, _lib.u8p))),
                          lambda p, pos: dict(p=kdehip.evaluateDualTree(p, pos, manifold=[1, 0])))


def _evaluate_log_device():
    L = _lib.lib
    return _positions_row("kdehip_evaluate_log_device", [("logp", (NQ,), "f64", "all")],
                          lambda d, pos, nq, o, st: _lib.check(L.kdehip_evaluate_log_device(d._h, _lib.addr(pos), nq, 0,
                                                                                              _lib.addr(o["logp"]), st, None)),
                          lambda p, pos: dict(logp=kdehip.evaluate_log(p, pos)))


def _evaluate_grad_device():
    L = _lib.lib

    def want(p, pos):
        val, grad = kdehip.evaluate_grad(p, pos)
        return dict(val=val, grad=grad.T)
    return _positions_row("kdehip_evaluate_grad_device", [("val", (NQ,), "f64", "all"), ("grad", (NQ, D), "f64", "all")],
                          lambda d, pos, nq, o, st: _lib.check(L.kdehip_evaluate_grad_device(
                              d._h, _lib.addr(pos), nq, 1, _lib.addr(o["val"]), _lib.addr(o["grad"]), None, st)), want)


def _hess_outputs(nq, dim, prefix=""):
    return [(prefix + "logp", (nq,), "f64", "all"), (prefix + "grad", (nq, dim), "f64", "all"),
            (prefix + "hess", (nq, dim, dim), "f64", "all"), (prefix + "cov", (nq, dim, dim), "f64", None),
            (prefix + "definite", (nq,), "i32", None)]


def _hess_want(p, pos, prefix=""):
    logp, grad, hess = kdehip.evaluate_hess(p, pos)
    cov, definite = kdehip.laplace(p, pos)
    return {prefix + "logp": logp, prefix + "grad": grad.T, prefix + "hess": hess.transpose(2, 0, 1),
            prefix + "cov": cov.transpose(2, 0, 1), prefix + "definite": definite.astype(np.int32)}


def _evaluate_hess_device():
    L = _lib.lib
    return _positions_row("kdehip_evaluate_hess_device", _hess_outputs(NQ, D),
                          lambda d, pos, nq, o, st: _lib.check(L.kdehip_evaluate_hess_device(
                              d._h, _lib.addr(pos), nq, _lib.addr(o["logp"]), _lib.addr(o["grad"]), _lib.addr(o["hess"]),
                              _lib.addr(o["cov"]), _lib.addr(o["definite"]), None, st)), _hess_want)


def _batch_row(name, shapes, outputs_of, item_args, call, want_of, kind="input"):
    """a batched entry over three items of mixed shape: `outputs_of(j, D, N, Nq)` the item's outputs (names prefixed "j."),
    `item_args(rng, j, p, Nq)` -> (device inputs, parameters, host values), `call(items, stream)` with items = dicts of
    density / inputs / parameters / outputs, `want_of(j, p, host, parameters)`"""
    rng = _rng(name)
    ps = [_density(rng, dd, nn) for dd, nn, _ in shapes]
    ds = [kdehip.DeviceDensity(p) for p in ps]
    outputs = [o for j, (dd, nn, nq) in enumerate(shapes) for o in outputs_of(f"{j}.", dd, nn, nq)]

    def enqueue(a, o, st):
        call([dict(density=ds[j], inp={k.split(".", 1)[1]: t for k, t in a["inputs"].items() if k.startswith(f"{j}.")},
                   par=a["par"][j], out={k.split(".", 1)[1]: t for k, t in o.items() if k.startswith(f"{j}.")})
              for j in range(len(shapes))], st)
    row = Row(name, kind, outputs, enqueue, ds)
    for s in SETS:
        inputs, pars, want = {}, [], {}
        for j, (dd, nn, nq) in enumerate(shapes):
            # The arguments of an item are drawn again until the BLOCKING entry's results tell this set from every earlier
            # one (the premise; it is asserted for the whole row below): an item of three queries over five points would
            # otherwise repeat a label or a converged point now and then.
            premise = {o[0]: o[3] for o in outputs_of("", dd, nn, nq)}
            for _ in range(64):
                inp, par, host = item_args(rng, j, ps[j], nq)
                w = {k: np.asarray(v) for k, v in want_of(j, ps[j], host, par).items()}
                if all(_tells_apart(premise[k], np.asarray(row.want[t][f"{j}.{k}"]).reshape(-1),
                                    v.astype(row.want[t][f"{j}.{k}"].dtype).reshape(-1)) for t in row.want for k, v in w.items()):
                    break
            inputs.update({f"{j}.{k}": _dev(v) for k, v in inp.items()})
            pars.append(par)
            want.update({f"{j}.{k}": v for k, v in w.items()})
        row.add(s, dict(inputs=inputs, par=pars), want)
    return row


def _positions_item(rng, j, p, nq):
    pos = _queries(rng, p, nq)
    return dict(pos=pos.T), {}, pos


def _evaluate_hess_device_batch():
    return _batch_row("kdehip_evaluate_hess_device_batch", BATCH, lambda pre, dd, nn, nq: _hess_outputs(nq, dd, pre), _positions_item,
                      lambda items, st: kdehip.evaluate_hess_device_batch(
                          [dict(density=it["density"], pos=it["inp"]["pos"], **it["out"]) for it in items], stream=st),
                      lambda j, p, pos, par: _hess_want(p, pos))


MS_TOL, MS_NITER = 1e-9, 3


def _meanshift_device_batch():
    def want(j, p, pos, par):
        x, logp, iters = kdehip.meanshift(p, pos, tol=MS_TOL, maxiter=MS_NITER)
        return dict(x=x.T, logp=logp, iters=iters)
    return _batch_row("kdehip_meanshift_device_batch", BATCH,
                      lambda pre, dd, nn, nq: [(pre + "x", (nq, dd), "f64", "all"), (pre + "logp", (nq,), "f64", "all"),
                                               (pre + "iters", (nq,), "i32", None)], _positions_item,
                      lambda items, st: kdehip.meanshift_device_batch(
                          [dict(density=it["density"], starts=it["inp"]["pos"], **it["out"]) for it in items], MS_TOL, MS_NITER, stream=st),
                      want)


def _cond_outputs(nq, nf, pre=""):
    return [(pre + "logz", (nq,), "f64", "all"), (pre + "mean", (nq, nf), "f64", "all"), (pre + "var", (nq, nf), "f64", "all"),
            (pre + "pts", (nq, nf), "f64", "all"), (pre + "ind", (nq,), "i64", "half")]


def _cond_want(p, Y, seed):
    """the host entry, every output in one call as the resident call asks for them; dimension 0 is given"""
    from kdehip.conditional import _call
    r = _call(p, [0], Y, logz=True, moments=True, draw=True, seed=seed)
    return {k: r[k] for k in ("logz", "mean", "var", "pts", "ind")}


def _conditional_device():
    L = _lib.lib
    name = "kdehip_conditional_device"
    rng = _rng(name)
    p = _density(rng, D, N)
    d = kdehip.DeviceDensity(p)

    def enqueue(a, o, st):
        _lib.check(L.kdehip_conditional_device(d._h, 1, _lib.addr(a["inputs"]["given"]), NQ, _lib.u64(a["seed"]), 0,
                                               *[_lib.addr(o[k]) for k in ("logz", "mean", "var", "pts", "ind")], None, _st(st)))
    row = Row(name, "input", _cond_outputs(NQ, D - 1), enqueue, [d])
    for k, s in enumerate(SETS):
        Y = _queries(rng, p, NQ)[:1]
        row.add(s, dict(inputs=dict(given=_dev(Y.T)), seed=700 + k), _cond_want(p, Y, 700 + k))
    return row


def _condition_weights_device():
    L = _lib.lib
    name = "kdehip_condition_weights_device"
    rng = _rng(name)
    p = _density(rng, D, N)
    d = kdehip.DeviceDensity(p)

    def enqueue(a, o, st):
        _lib.check(L.kdehip_condition_weights_device(d._h, 1, _lib.addr(a["inputs"]["given"]), NQ, _lib.addr(o["w"]),
                                                     _lib.addr(o["logz"]), None, _st(st)))
    row = Row(name, "input", [("w", (NQ, N), "f64", "nonzero"), ("logz", (NQ,), "f64", "all")], enqueue, [d])
    for s in SETS:
        Y = _queries(rng, p, NQ)[:1]
        W, logz = kdehip.conditional_weights(p, [0], Y)
        row.add(s, dict(inputs=dict(given=_dev(Y.T))), dict(w=W, logz=logz))
    return row


def _conditional_device_batch():
    def item(rng, j, p, nq):
        Y = _queries(rng, p, nq)[:1]
        return dict(given=Y.T), dict(seed=int(rng.integers(1, 2 ** 40))), Y
    return _batch_row("kdehip_conditional_device_batch", COND_BATCH, lambda pre, dd, nn, nq: _cond_outputs(nq, dd - 1, pre), item,
                      lambda items, st: kdehip.conditional_device_batch(
                          [dict(density=it["density"], dims=[0], given=it["inp"]["given"], seed=it["par"]["seed"], **it["out"])
                           for it in items], stream=st),
                      lambda j, p, Y, par: _cond_want(p, Y, par["seed"]))


def _boxes(rng, p, nq):
    """nq finite boxes over every dimension, centred on positions inside the data, one to four units wide"""
    c = _queries(rng, p, nq)
    half = rng.uniform(0.5, 2.0, size=c.shape)
    return c - half, c + half


def _box_mass_device():
    L = _lib.lib
    name = "kdehip_box_mass_device"
    rng = _rng(name)
    p = _density(rng, D, N)
    d = kdehip.DeviceDensity(p)

    def enqueue(a, o, st):
        _lib.check(L.kdehip_box_mass_device(d._h, (1 << D) - 1, _lib.addr(a["inputs"]["lo"]), _lib.addr(a["inputs"]["hi"]), NQ,
                                            _lib.addr(o["mass"]), None, _st(st)))
    row = Row(name, "input", [("mass", (NQ,), "f64", "all")], enqueue, [d])
    for s in SETS:
        lo, hi = _boxes(rng, p, NQ)
        row.add(s, dict(inputs=dict(lo=_dev(lo.T), hi=_dev(hi.T))), dict(mass=kdehip.box_mass(p, lo, hi)))
    return row


def _box_mass_device_batch():
    def item(rng, j, p, nq):
        lo, hi = _boxes(rng, p, nq)
        return dict(lo=lo.T, hi=hi.T), {}, (lo, hi)
    return _batch_row("kdehip_box_mass_device_batch", BATCH, lambda pre, dd, nn, nq: [(pre + "mass", (nq,), "f64", "all")], item,
                      lambda items, st: kdehip.box_mass_device_batch(
                          [dict(density=it["density"], lo=it["inp"]["lo"], hi=it["inp"]["hi"], mass=it["out"]["mass"]) for it in items],
                          stream=st),
                      lambda j, p, host, par: dict(mass=kdehip.box_mass(p, host[0], host[1])))


def _quantile_outputs(pre=""):
    return [(pre + "x", (NLEVELS,), "f64", "all"), (pre + "resid", (NLEVELS,), "f64", None), (pre + "iters", (NLEVELS,), "i32", None),
            (pre + "converged", (NLEVELS,), "i32", None)]


def _quantile_want(p, alpha, dim):
    x, resid, iters, conv = kdehip.quantile(p, alpha, dim, full=True)
    return dict(x=x, resid=resid, iters=iters, converged=conv.astype(np.int32))


def _quantile_device():
    L = _lib.lib
    name = "kdehip_quantile_device"
    rng = _rng(name)
    p = _density(rng, D, N)
    d = kdehip.DeviceDensity(p)

    def enqueue(a, o, st):
        _lib.check(L.kdehip_quantile_device(d._h, 1, _lib.addr(a["inputs"]["alpha"]), NLEVELS, C.byref(C.c_double(1e-12)), 100,
                                            *[_lib.addr(o[k]) for k in ("x", "resid", "iters", "converged")], None, _st(st)))
    row = Row(name, "input", _quantile_outputs(), enqueue, [d])
    for s in SETS:
        alpha = rng.uniform(0.02, 0.98, size=NLEVELS)
        row.add(s, dict(inputs=dict(alpha=_dev(alpha))), _quantile_want(p, alpha, 1))
    return row


def _quantile_device_batch():
    def item(rng, j, p, nq):
        alpha = rng.uniform(0.02, 0.98, size=NLEVELS)
        return dict(alpha=alpha), {}, alpha
    return _batch_row("kdehip_quantile_device_batch", BATCH, lambda pre, dd, nn, nq: _quantile_outputs(pre), item,
                      lambda items, st: kdehip.quantile_device_batch(
                          [dict(density=it["density"], dim=0, alpha=it["inp"]["alpha"], **it["out"]) for it in items], stream=st),
                      lambda j, p, alpha, par: _quantile_want(p, alpha, 0))


def _sample_want(p, labels, seed):
    pts, ind = kdehip.sample(p, NDRAW, ind=labels, seed=seed)
    return dict(pts=pts.T, ind=ind)


def _sample_device():
    L = _lib.lib
    name = "kdehip_sample_device"
    rng = _rng(name)
    p = _density(rng, D, N)
    d = kdehip.DeviceDensity(p)

    def enqueue(a, o, st):
        _lib.check(L.kdehip_sample_device(d._h, NDRAW, _lib.u64(a["seed"]), 0, _lib.addr(a["inputs"]["labels"]), _lib.addr(o["pts"]),
                                          _lib.addr(o["ind"]), _st(st)))
    row = Row(name, "input", [("pts", (NDRAW, D), "f64", "all"), ("ind", (NDRAW,), "i64", "half")], enqueue, [d])
    for k, s in enumerate(SETS):
        labels = rng.integers(1, N + 1, size=NDRAW).astype(np.int64)
        row.add(s, dict(inputs=dict(labels=_dev(labels)), seed=900 + k), _sample_want(p, labels, 900 + k))
    return row


def _sample_device_batch():
    def item(rng, j, p, nq):
        labels = rng.integers(1, p.bt.num_points + 1, size=NDRAW).astype(np.int64)
        return dict(labels=labels), dict(seed=int(rng.integers(1, 2 ** 40))), labels
    return _batch_row("kdehip_sample_device_batch", BATCH,
                      lambda pre, dd, nn, nq: [(pre + "pts", (NDRAW, dd), "f64", "all"), (pre + "ind", (NDRAW,), "i64", "half")], item,
                      lambda items, st: kdehip.sample_device_batch(
                          [dict(density=it["density"], Npts=NDRAW, seed=it["par"]["seed"], ind=it["inp"]["labels"],
                                d_pts=it["out"]["pts"], d_ind=it["out"]["ind"]) for it in items], stream=st),
                      lambda j, p, labels, par: _sample_want(p, labels, par["seed"]))


# ---- rows whose inputs are resident densities only -------------------------------------------------------------------------
def _at_row(name, outputs, call, want):
    """an entry of a resident density `bd` at the points of a resident density `at` (257 points): the five sets are five
    densities bd of one shape; `call(bd, at, out, stream)`, `want(bd_host, at_host)`"""
    rng = _rng(name)
    at = _density(rng, D, NQ)
    bds = [_density(rng, D, N) for _ in SETS]
    d_at = kdehip.DeviceDensity(at)
    d_bds = [kdehip.DeviceDensity(p) for p in bds]
    row = Row(name, "density", outputs, lambda a, o, st: call(d_bds[a["bd"]], d_at, o, _st(st)), d_bds + [d_at])
    for k, s in enumerate(SETS):
        row.add(s, dict(bd=k), want(bds[k], at))
    return row


def _evaluate_device_at():
    L = _lib.lib
    return _at_row("kdehip_evaluate_device_at", [("p", (NQ,), "f64", "all")],
                   lambda bd, at, o, st: _lib.check(L.kdehip_evaluate_device_at(bd._h, at._h, _lib.addr(o["p"]), st)),
                   lambda bd, at: dict(p=kdehip.evaluateDualTree(bd, at)))


def _evaluate_log_device_at():
    L = _lib.lib
    return _at_row("kdehip_evaluate_log_device_at", [("logp", (NQ,), "f64", "all")],
                   lambda bd, at, o, st: _lib.check(L.kdehip_evaluate_log_device_at(bd._h, at._h, _lib.addr(o["logp"]), st, None)),
                   lambda bd, at: dict(logp=kdehip.evaluate_log(bd, at)))


def _evaluate_device_at_tol():
    L = _lib.lib

    def want(bd, at):
        vals, stats = kdehip.evaluate_tol(bd, at, rel_tol=1e-2, return_stats=True)
        return dict(p=vals, stats=np.array(stats))
    return _at_row("kdehip_evaluate_device_at_tol", [("p", (NQ,), "f64", "all"), ("stats", (2,), "i64", None)],
                   lambda bd, at, o, st: _lib.check(L.kdehip_evaluate_device_at_tol(
                       bd._h, at._h, C.byref(C.c_double(1e-2)), None, _lib.addr(o["p"]), _lib.addr(o["stats"]), st, None)), want)


def _knn_device_at():
    L = _lib.lib

    def want(bd, at):
        d2, idx, stats = kdehip.knn(bd, at, k=KNN_K, squared=True, return_stats=True)
        return dict(d2=d2.T, idx=idx.T, stats=np.array(stats))
    return _at_row("kdehip_knn_device_at", [("d2", (NQ, KNN_K), "f64", "all"), ("idx", (NQ, KNN_K), "i64", "half"),
                                            ("stats", (2,), "i64", None)],
                   lambda bd, at, o, st: _lib.check(L.kdehip_knn_device_at(bd._h, at._h, KNN_K, None, _lib.addr(o["d2"]),
                                                                          _lib.addr(o["idx"]), _lib.addr(o["stats"]), st, None)), want)


def _pairs_row(name, call, want):
    """a batched scalar of three (bd, at) pairs of the mixed shapes: the sets are five bd per item; `call(pairs, out, stream)`"""
    rng = _rng(name)
    ats = [_density(rng, dd, nq) for dd, _, nq in BATCH]
    bds = [[_density(rng, dd, nn) for dd, nn, _ in BATCH] for _ in SETS]
    d_ats = [kdehip.DeviceDensity(p) for p in ats]
    d_bds = [[kdehip.DeviceDensity(p) for p in ps] for ps in bds]
    row = Row(name, "density", [("out", (len(BATCH),), "f64", "all")],
              lambda a, o, st: call([(d_bds[a["bd"]][j], d_ats[j]) for j in range(len(BATCH))], o["out"], st),
              [d for ds in d_bds for d in ds] + d_ats)
    for k, s in enumerate(SETS):
        row.add(s, dict(bd=k), dict(out=np.array([want(bds[k][j], ats[j]) for j in range(len(BATCH))])))
    return row


def _eval_avg_logl_device_batch():
    return _pairs_row("kdehip_eval_avg_logl_device_batch", lambda pairs, out, st: kdehip.eval_avg_logl_device_batch(pairs, out, stream=st),
                      lambda bd, at: kdehip.evalAvgLogL(bd, at))


def _eval_avg_logl_log_device_batch():
    return _pairs_row("kdehip_eval_avg_logl_log_device_batch",
                      lambda pairs, out, st: kdehip.eval_avg_logl_device_batch(pairs, out, stream=st, log_domain=True),
                      lambda bd, at: kdehip.evalAvgLogL(bd, at, log_domain=True))


def _kernel_sum_device_batch():
    return _pairs_row("kdehip_kernel_sum_device_batch",
                      lambda pairs, out, st: kdehip.kernel_sum_device_batch([dict(a=a, b=b, normalize=True) for a, b in pairs], out, stream=st),
                      lambda a, b: kdehip.kernel_sum(a, b, None, normalize=True))


def _summary_device_batch():
    L = _lib.lib
    name = "kdehip_summary_device_batch"
    rng = _rng(name)
    ps = [[_density(rng, dd, nn) for dd, nn, _ in BATCH] for _ in SETS]
    ds = [[kdehip.DeviceDensity(p) for p in row] for row in ps]
    names = ("range", "mean", "cov", "argmax", "values")
    outputs = [(f"{j}.{k}", shape, "f64", "all") for j, (dd, _, _) in enumerate(BATCH)
               for k, shape in zip(names, ((2 * dd,), (dd,), (dd * dd,), (dd,), (dd * NGRID,)))]

    def enqueue(a, o, st):
        kdehip.summary_device_batch([dict(density=ds[a["set"]][j], extend=0.1, Ngrid=NGRID, **{k: o[f"{j}.{k}"] for k in names})
                                     for j in range(len(BATCH))], stream=st)
    row = Row(name, "density", outputs, enqueue, [d for r in ds for d in r])
    for k, s in enumerate(SETS):
        want = {}
        for j, (dd, _, _) in enumerate(BATCH):  # the blocking entry of one resident density, host outputs as the ABI lays them out
            bufs = [np.zeros(n) for n in (2 * dd, dd, dd * dd, dd, dd * NGRID)]
            _lib.check(L.kdehip_density_summary(ds[k][j]._h, C.byref(C.c_double(0.1)), NGRID, *[_lib.ptr(b, _lib.f64p) for b in bufs]))
            want.update({f"{j}.{n}": b for n, b in zip(names, bufs)})
        row.add(s, dict(set=k), want)
    return row


def _prod_philox_device():
    """ONE 2-D product of three resident densities of 150, 160 and 170 points, 96 chains, 3 iterations, as
    tests/test_gpu_batch.py builds them; the sets are five seeds.  The header's contract for this entry is "same results as
    kdehip_prod_philox, bit for bit", and the existing tests compare labels and points with array_equal: so do these."""
    name = "kdehip_prod_philox_device"
    rng = np.random.default_rng(60)
    trees = []
    for n in PROD_NS:
        pts = synth_mixture(rng, 2, n)
        trees.append(kdehip.kde(pts, silverman_bw(pts)))
    ds = [kdehip.DeviceDensity(t) for t in trees]
    M = len(trees)

    def enqueue(a, o, st):
        kdehip.prodAppxMSGibbsS_device(ds, o["points"], o["indices"], Np=PROD_NP, Niter=PROD_NITER, seed=a["seed"], stream=st)
    row = Row(name, "density", [("points", (PROD_NP, 2), "f64", "all"), ("indices", (PROD_NP, M), "i64", "half")], enqueue, ds)
    for k, s in enumerate(SETS):
        pts, ind = kdehip.prodAppxMSGibbsS(None, trees, None, None, Niter=PROD_NITER, Np=PROD_NP, seed=4100 + k)
        row.add(s, dict(seed=4100 + k), dict(points=pts.T, indices=ind.T))
    return row


_BUILDERS = {
    "kdehip_evaluate_device": _evaluate_device,
    "kdehip_evaluate_device_manifold": _evaluate_device_manifold,
    "kdehip_evaluate_log_device": _evaluate_log_device,
    "kdehip_evaluate_grad_device": _evaluate_grad_device,
    "kdehip_evaluate_hess_device": _evaluate_hess_device,
    "kdehip_evaluate_hess_device_batch": _evaluate_hess_device_batch,
    "kdehip_meanshift_device_batch": _meanshift_device_batch,
    "kdehip_conditional_device": _conditional_device,
    "kdehip_condition_weights_device": _condition_weights_device,
    "kdehip_conditional_device_batch": _conditional_device_batch,
    "kdehip_box_mass_device": _box_mass_device,
    "kdehip_box_mass_device_batch": _box_mass_device_batch,
    "kdehip_quantile_device": _quantile_device,
    "kdehip_quantile_device_batch": _quantile_device_batch,
    "kdehip_sample_device": _sample_device,
    "kdehip_sample_device_batch": _sample_device_batch,
    "kdehip_evaluate_device_at": _evaluate_device_at,
    "kdehip_evaluate_log_device_at": _evaluate_log_device_at,
    "kdehip_evaluate_device_at_tol": _evaluate_device_at_tol,
    "kdehip_knn_device_at": _knn_device_at,
    "kdehip_eval_avg_logl_device_batch": _eval_avg_logl_device_batch,
    "kdehip_eval_avg_logl_log_device_batch": _eval_avg_logl_log_device_batch,
    "kdehip_kernel_sum_device_batch": _kernel_sum_device_batch,
    "kdehip_summary_device_batch": _summary_device_batch,
    "kdehip_prod_philox_device": _prod_philox_device,
}
DENSITY_ROWS = ["kdehip_evaluate_device_at", "kdehip_evaluate_log_device_at", "kdehip_evaluate_device_at_tol", "kdehip_knn_device_at",
                "kdehip_eval_avg_logl_device_batch", "kdehip_eval_avg_logl_log_device_batch", "kdehip_kernel_sum_device_batch",
                "kdehip_summary_device_batch", "kdehip_prod_philox_device"]
INPUT_ROWS = [n for n in _BUILDERS if n not in DENSITY_ROWS]
ALL_ROWS = INPUT_ROWS + DENSITY_ROWS
# Not in the table: kdehip_meanshift_device and kdehip_kernel_sum_device.  Their ABI has no stream argument: they return their
# results to HOST arrays and block on the calling thread's stream (include/kdehip.h sections 5h, 5g); the enqueue-only forms
# are the two _device_batch rows above.


def build(name):
    """a fresh row of its own densities, its premise asserted; the caller closes it"""
    row = _BUILDERS[name]()
    assert row.kind == ("density" if name in DENSITY_ROWS else "input") and set(row.args) == set(SETS)
    try:
        row.check_premise()
    except AssertionError:
        row.close()
        raise
    return row
