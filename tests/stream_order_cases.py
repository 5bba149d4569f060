"""The case table of tests/test_gpu_stream_order.py: one row per enqueue-only entry of include/kdehip.h.

"Every" is checked: tests/test_stream_order_table.py reads the header and wants each function with a `stream` / `streams`
parameter in ALL_ROWS, in BLOCKING_WAITS (blocking entries that wait for a stream: a test of their own) or in NO_ROW (with the
reason), all three at the foot of this file.

A row holds the resident densities its entry needs, five argument sets of IDENTICAL shapes -- `true`, `decoy` and `alt1..3`;
where an entry's only inputs are densities, a set names which of the row's equally shaped densities it evaluates --, a closure `enqueue(args, outputs, stream)` that makes the call through `_lib.lib` or the stream-taking
Python wrapper and never synchronises, and `want[set]`, the arrays the BLOCKING entry returns for that set (computed once, when
the row is built, with the device idle).  Because every set of a row has the same shapes and densities, a call that ran with
another call's recycled descriptors would read and write valid memory of the right size: a wrong answer, never a wild access.

Shapes: D = 2, N = 300 leaves (three 128-leaf chunks, the last ragged), Nq = 257 queries (two 256-query blocks, the last with
one lane); batches are three items of the mixed shapes BATCH; draws are 1000 samples; quantiles take five levels.  The circular
twins take the shapes of the Euclidean row beside them with dimension 0 circular and angles that straddle +-pi.

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
def _positions_row(name, outputs, call, want, nq=NQ, density=_density):
    """an entry of one resident density at device positions: `call(d, pos, Nq, out, stream)`, `want(p, pos)`"""
    rng = _rng(name)
    p = density(rng, D, N)
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


def _batch_row(name, shapes, outputs_of, item_args, call, want_of, kind="input", density=_density):
    """a batched entry over three items of mixed shape: `outputs_of(j, D, N, Nq)` the item's outputs (names prefixed "j."),
    `item_args(rng, j, p, Nq)` -> (device inputs, parameters, host values), `call(items, stream)` with items = dicts of
    density / inputs / parameters / outputs, `want_of(j, p, host, parameters)`"""
    rng = _rng(name)
    ps = [density(rng, dd, nn) for dd, nn, _ in shapes]
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

    def call(items, st):   # (the Python mirror always goes through the _manifold twin: this row calls the entry itself)
        arr = (_lib.CSampleItem * len(items))()
        for k, it in enumerate(items):
            a = arr[k]
            a.density, a.Npts, a.seed, a.sample_offset = it["density"]._h, NDRAW, it["par"]["seed"], 0
            a.d_ind_in, a.d_pts, a.d_ind = _lib.addr(it["inp"]["labels"]), _lib.addr(it["out"]["pts"]), _lib.addr(it["out"]["ind"])
        _lib.check(_lib.lib.kdehip_sample_device_batch(len(items), arr, _st(st)))
    return _batch_row("kdehip_sample_device_batch", BATCH,
                      lambda pre, dd, nn, nq: [(pre + "pts", (NDRAW, dd), "f64", "all"), (pre + "ind", (NDRAW,), "i64", "half")], item,
                      call, lambda j, p, labels, par: _sample_want(p, labels, par["seed"]))


# ---- rows whose inputs are resident densities only -------------------------------------------------------------------------
def _at_row(name, outputs, call, want, density=_density):
    """an entry of a resident density `bd` at the points of a resident density `at` (257 points): the five sets are five
    densities bd of one shape; `call(bd, at, out, stream)`, `want(bd_host, at_host)`"""
    rng = _rng(name)
    at = density(rng, D, NQ)
    bds = [density(rng, D, N) for _ in SETS]
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


def _pairs_row(name, call, want, density=_density):
    """a batched scalar of three (bd, at) pairs of the mixed shapes: the sets are five bd per item; `call(pairs, out, stream)`"""
    rng = _rng(name)
    ats = [density(rng, dd, nq) for dd, _, nq in BATCH]
    bds = [[density(rng, dd, nn) for dd, nn, _ in BATCH] for _ in SETS]
    d_ats = [kdehip.DeviceDensity(p) for p in ats]
    d_bds = [[kdehip.DeviceDensity(p) for p in ps] for ps in bds]
    row = Row(name, "density", [("out", (len(BATCH),), "f64", "all")],
              lambda a, o, st: call([(d_bds[a["bd"]][j], d_ats[j]) for j in range(len(BATCH))], o["out"], st),
              [d for ds in d_bds for d in ds] + d_ats)
    for k, s in enumerate(SETS):
        row.add(s, dict(bd=k), dict(out=np.array([want(bds[k][j], ats[j]) for j in range(len(BATCH))])))
    return row


def _eval_avg_logl_device_batch():
    def call(pairs, out, st):   # (the Python mirror always goes through the _manifold twin: this row calls the entry itself)
        arr = (_lib.CLoglItem * len(pairs))()
        for k, (bd, at) in enumerate(pairs):
            arr[k].bd, arr[k].at, arr[k].leave_one_out = bd._h, at._h, 0
        _lib.check(_lib.lib.kdehip_eval_avg_logl_device_batch(len(pairs), arr, _lib.addr(out), _st(st)))
    return _pairs_row("kdehip_eval_avg_logl_device_batch", call, lambda bd, at: kdehip.evalAvgLogL(bd, at))


def _eval_avg_logl_log_device_batch():
    return _pairs_row("kdehip_eval_avg_logl_log_device_batch",
                      lambda pairs, out, st: kdehip.eval_avg_logl_device_batch(pairs, out, stream=st, log_domain=True),
                      lambda bd, at: kdehip.evalAvgLogL(bd, at, log_domain=True))


def _kernel_sum_device_batch():
    return _pairs_row("kdehip_kernel_sum_device_batch",
                      lambda pairs, out, st: kdehip.kernel_sum_device_batch([dict(a=a, b=b, normalize=True) for a, b in pairs], out, stream=st),
                      lambda a, b: kdehip.kernel_sum(a, b, None, normalize=True))


def _summary_row(name, density, enqueue_items, blocking):
    """the summaries of three densities of the mixed shapes in one call: `enqueue_items(items, stream)` with items = dicts of
    density / extend / Ngrid / the five outputs, `blocking(d, extend, Ngrid, bufs)` the entry of ONE resident density"""
    rng = _rng(name)
    ps = [[density(rng, dd, nn) for dd, nn, _ in BATCH] for _ in SETS]
    ds = [[kdehip.DeviceDensity(p) for p in row] for row in ps]
    names = ("range", "mean", "cov", "argmax", "values")
    outputs = [(f"{j}.{k}", shape, "f64", "all") for j, (dd, _, _) in enumerate(BATCH)
               for k, shape in zip(names, ((2 * dd,), (dd,), (dd * dd,), (dd,), (dd * NGRID,)))]

    def enqueue(a, o, st):
        enqueue_items([dict(density=ds[a["set"]][j], extend=0.1, Ngrid=NGRID, **{k: o[f"{j}.{k}"] for k in names})
                       for j in range(len(BATCH))], st)
    row = Row(name, "density", outputs, enqueue, [d for r in ds for d in r])
    for k, s in enumerate(SETS):
        want = {}
        for j, (dd, _, _) in enumerate(BATCH):  # the blocking entry of one resident density, host outputs as the ABI lays them out
            bufs = [np.zeros(n) for n in (2 * dd, dd, dd * dd, dd, dd * NGRID)]
            blocking(ds[k][j], 0.1, NGRID, bufs)
            want.update({f"{j}.{n}": b for n, b in zip(names, bufs)})
        row.add(s, dict(set=k), want)
    return row


def _summary_device_batch():
    L = _lib.lib

    def call(items, st):   # (the Python mirror always goes through the _manifold twin: this row calls the entry itself)
        arr = (_lib.CSummaryItem * len(items))()
        for k, it in enumerate(items):
            a = arr[k]
            a.density, a.extend, a.Ngrid = it["density"]._h, it["extend"], it["Ngrid"]
            a.d_range, a.d_mean, a.d_cov, a.d_argmax, a.d_values = (_lib.addr(it[x]) for x in ("range", "mean", "cov", "argmax", "values"))
        _lib.check(L.kdehip_summary_device_batch(len(items), arr, _st(st)))
    return _summary_row("kdehip_summary_device_batch", _density, call,
                        lambda d, extend, ngrid, bufs: _lib.check(L.kdehip_density_summary(
                            d._h, C.byref(C.c_double(extend)), ngrid, *[_lib.ptr(b, _lib.f64p) for b in bufs])))


def _prod_philox_device():
    """ONE 2-D product of three resident densities of 150, 160 and 170 points, 96 chains, 3 iterations, as
    tests/test_gpu_batch.py builds them; the sets are five seeds.  The header's contract for this entry is "same results as
    kdehip_prod_philox, bit for bit", and the existing tests compare labels and points with array_equal: so do these."""
    name = "kdehip_prod_philox_device"
    trees = _prod_trees()
    ds = [kdehip.DeviceDensity(t) for t in trees]
    M = len(trees)
    arr = (C.c_void_p * M)(*[d._h for d in ds])

    def enqueue(a, o, st):   # (prodAppxMSGibbsS_device always goes through the _manifold twin: this row calls the entry itself)
        _lib.check(_lib.lib.kdehip_prod_philox_device(M, arr, PROD_NP, PROD_NITER, _lib.u64(a["seed"]), 0, 1, None, 64,
                                                      _lib.addr(o["points"]), _lib.addr(o["indices"]), None, _st(st)))
    row = Row(name, "density", [("points", (PROD_NP, 2), "f64", "all"), ("indices", (PROD_NP, M), "i64", "half")], enqueue, ds)
    for k, s in enumerate(SETS):
        pts, ind = kdehip.prodAppxMSGibbsS(None, trees, None, None, Niter=PROD_NITER, Np=PROD_NP, seed=4100 + k)
        row.add(s, dict(seed=4100 + k), dict(points=pts.T, indices=ind.T))
    return row


# ---- per-point bandwidths (include/kdehip.h section 5o) --------------------------------------------------------------------
def _varbw_density(rng, dd, nn):
    """the points and weights of `_density` (two clusters, one exact zero weight); every leaf has its own column of standard
    deviations: one value in 0.2..0.6 per dimension times a factor in 0.5..2 per point"""
    pts = rng.standard_normal((dd, nn)) * rng.uniform(0.5, 2.0, size=(dd, 1)) + rng.uniform(-1, 1, size=(dd, 1))
    pts[:, nn // 2:] += 3.0
    w = rng.uniform(0.05, 1.0, size=nn)
    if nn > 1:
        w[nn // 3] = 0.0
    bw = rng.uniform(0.2, 0.6, size=(dd, 1)) * rng.uniform(0.5, 2.0, size=(1, nn))
    return kdehip.kde_varbw(pts, bw, w)


def _evaluate_varbw_device():
    """the direct step (log_domain = 0): the prepass folds c_i = w_i / prod sqrt(v_ik) into the call's block, the sweep reads it"""
    L = _lib.lib
    return _positions_row("kdehip_evaluate_varbw_device", [("p", (NQ,), "f64", "all")],
                          lambda d, pos, nq, o, st: _lib.check(L.kdehip_evaluate_varbw_device(d._h, _lib.addr(pos), nq, 0,
                                                                                                _lib.addr(o["p"]), st, None)),
                          lambda p, pos: dict(p=kdehip.evaluateDualTree(p, pos)), density=_varbw_density)


def _evaluate_varbw_device_at():
    """the log step (log_domain = 1) at the points of another resident density"""
    L = _lib.lib
    return _at_row("kdehip_evaluate_varbw_device_at", [("logp", (NQ,), "f64", "all")],
                   lambda bd, at, o, st: _lib.check(L.kdehip_evaluate_varbw_device_at(bd._h, at._h, 0, 1, _lib.addr(o["logp"]), st, None)),
                   lambda bd, at: dict(logp=kdehip.evaluate_log(bd, at)), density=_varbw_density)


def _eval_avg_logl_varbw_device():
    """the direct log-likelihood of bd at the points of another density `at` (no leave-one-out), ONE double"""
    L = _lib.lib
    return _at_row("kdehip_eval_avg_logl_varbw_device", [("out", (1,), "f64", "all")],
                   lambda bd, at, o, st: _lib.check(L.kdehip_eval_avg_logl_varbw_device(bd._h, at._h, 0, 0, _lib.addr(o["out"]), st, None)),
                   lambda bd, at: dict(out=np.array([kdehip.evalAvgLogL(bd, at)])), density=_varbw_density)


# ---- the exact product of two densities (include/kdehip.h section 5p) ------------------------------------------------------
def _prod_exact_outputs(np_, dd, pre="", ind="half"):
    return [(pre + "pts", (np_, dd), "f64", "all"), (pre + "ind", (np_, 2), "i64", ind), (pre + "logz", (1,), "f64", "all")]


def _prod_exact_want(p, q, np_, seed, pre=""):
    pts, ind, lz = kdehip.prod_exact(p, q, np_, seed=seed, return_logz=True)   # (host densities: kdehip_prod_exact)
    return {pre + "pts": pts.T, pre + "ind": ind.T, pre + "logz": np.array([lz])}


def _prod_exact_device():
    """five p of 300 leaves and five seeds against ONE q of 257 leaves, 1000 draws: four dependent launches (rows, finish,
    one-block scan, draw) through the call's scratch [partial | rows | cum | mr], which the draw kernel bisects"""
    L = _lib.lib
    name = "kdehip_prod_exact_device"
    rng = _rng(name)
    q = _density(rng, D, NQ)
    ps = [_density(rng, D, N) for _ in SETS]
    d_q = kdehip.DeviceDensity(q)
    d_ps = [kdehip.DeviceDensity(p) for p in ps]

    def enqueue(a, o, st):
        _lib.check(L.kdehip_prod_exact_device(d_ps[a["p"]]._h, d_q._h, NDRAW, _lib.u64(a["seed"]), 0, _lib.addr(o["pts"]),
                                              _lib.addr(o["ind"]), _lib.addr(o["logz"]), _st(st)))
    row = Row(name, "density", _prod_exact_outputs(NDRAW, D), enqueue, d_ps + [d_q])
    for k, s in enumerate(SETS):
        row.add(s, dict(p=k, seed=5300 + k), _prod_exact_want(ps[k], q, NDRAW, 5300 + k))
    return row


# (D, N1, N2, Np) of the exact-product batch.  The last item keeps 8 leaves a side (7 of positive weight each: 49 components):
# one chunk, one block.  Its densities come from a generator of their own, PROD_EXACT_SMALL_SEED.
PROD_EXACT_BATCH = [(2, 300, 257, NDRAW), (3, 129, 130, 257), (1, 8, 8, 77)]
PROD_EXACT_SMALL_SEED = 8


def prod_exact_small_item():
    """(q, the five p) of the smallest item of the exact-product batch, host densities"""
    dd, n1, n2, _ = PROD_EXACT_BATCH[-1]
    rng = np.random.default_rng(PROD_EXACT_SMALL_SEED)
    return _density(rng, dd, n2), [_density(rng, dd, n1) for _ in SETS]


def _prod_exact_device_batch():
    """three items of mixed (D, N1, N2) and Np = 1000, 257 and 77 in ONE call; five p and five seeds per item.
    The smallest item has 49 components, and two independent draws of so few can share many labels.  Its shape and the seed
    of its generator were chosen on the CPU from the component weights tests/prodexact_model.py gives: between any two
    of the five sets the expected share of equal labels is the mean of sum_i P_i P'_i and sum_j Q_j Q'_j (P, Q the marginal
    weights of the two labels), at most 0.20 here (the best of 40 seeds of (1, 8, 8); none was above 0.5), and the labels the
    model draws from the Philox uniforms of the row's seeds agree in at most 21 % of the 154 entries.  So the `half` premise HOLDS for this item's `ind` too: no output of this row
    goes without a premise."""
    name = "kdehip_prod_exact_device_batch"
    rng = _rng(name)
    qs = [_density(rng, dd, n2) for dd, _, n2, _ in PROD_EXACT_BATCH[:-1]]
    ps = [[_density(rng, dd, n1) for dd, n1, _, _ in PROD_EXACT_BATCH[:-1]] for _ in SETS]
    q_small, p_small = prod_exact_small_item()
    qs.append(q_small)
    for k in range(len(SETS)):
        ps[k].append(p_small[k])
    d_qs = [kdehip.DeviceDensity(q) for q in qs]
    d_ps = [[kdehip.DeviceDensity(p) for p in r] for r in ps]
    outputs = [o for j, (dd, _, _, np_) in enumerate(PROD_EXACT_BATCH) for o in _prod_exact_outputs(np_, dd, f"{j}.")]

    def enqueue(a, o, st):
        kdehip.prod_exact_device_batch([dict(p=d_ps[a["set"]][j], q=d_qs[j], Np=np_, seed=a["seeds"][j], pts=o[f"{j}.pts"],
                                             ind=o[f"{j}.ind"], logz=o[f"{j}.logz"])
                                        for j, (_, _, _, np_) in enumerate(PROD_EXACT_BATCH)], stream=st)
    row = Row(name, "density", outputs, enqueue, [d for r in d_ps for d in r] + d_qs)
    for k, s in enumerate(SETS):
        seeds = [prod_exact_batch_seed(k, j) for j in range(len(PROD_EXACT_BATCH))]
        want = {}
        for j, (_, _, _, np_) in enumerate(PROD_EXACT_BATCH):
            want.update(_prod_exact_want(ps[k][j], qs[j], np_, seeds[j], f"{j}."))
        row.add(s, dict(set=k, seeds=seeds), want)
    return row


def prod_exact_batch_seed(k, j):
    """the seed of item j in argument set k of the exact-product batch"""
    return 5400 + 10 * k + j


PC_N2 = 129   # 300 x 129 = 38 700 components


def _product_components_device():
    """the mixture itself, 300 x 129 components; the five p have five bandwidth vectors, so `var` differs too"""
    L = _lib.lib
    name = "kdehip_product_components_device"
    rng = _rng(name)
    q = _density(rng, D, PC_N2)
    ps = [_density(rng, D, N) for _ in SETS]
    d_q = kdehip.DeviceDensity(q)
    d_ps = [kdehip.DeviceDensity(p) for p in ps]
    nc = N * PC_N2

    def enqueue(a, o, st):
        _lib.check(L.kdehip_product_components_device(d_ps[a["p"]]._h, d_q._h, _lib.addr(o["means"]), _lib.addr(o["weights"]),
                                                      _lib.addr(o["var"]), _st(st)))
    row = Row(name, "density", [("means", (nc, D), "f64", "all"), ("weights", (nc,), "f64", "nonzero"), ("var", (D,), "f64", "all")],
              enqueue, d_ps + [d_q])
    cq = q._cstruct()
    for k, s in enumerate(SETS):   # the blocking entry as the ABI lays its results out (the Python mirror returns sqrt(var))
        means, w, var = np.zeros((nc, D)), np.zeros(nc), np.zeros(D)
        cp = ps[k]._cstruct()
        _lib.check(L.kdehip_product_components(C.byref(cp), C.byref(cq), _lib.ptr(means, _lib.f64p), _lib.ptr(w, _lib.f64p),
                                               _lib.ptr(var, _lib.f64p), 0))
        row.add(s, dict(p=k), dict(means=means, weights=w, var=var))
    return row


# ---- the circular twins: dimension 0 circular, on the shapes of the Euclidean row beside them ------------------------------
def _man(dd):
    return [1] + [0] * (dd - 1)


def _wrap(t):
    return t - 2.0 * np.pi * np.floor((t + np.pi) / (2.0 * np.pi))


def _circ_density(rng, dd, nn):
    """`_density` with dimension 0 an angle: one cluster 0.3 rad wide that straddles the cut at +-pi, stored wrapped to
    [-pi, pi) -- differences wrap, so the Euclidean kernels give other numbers (tests/test_gpu_summary_circular.py "straddle";
    every tangent offset from point 1 stays far inside half a turn)"""
    pts = rng.standard_normal((dd, nn)) * rng.uniform(0.5, 2.0, size=(dd, 1)) + rng.uniform(-1, 1, size=(dd, 1))
    pts[1:, nn // 2:] += 3.0
    pts[0] = _wrap(np.pi + 0.3 * rng.standard_normal(nn))
    w = rng.uniform(0.05, 1.0, size=nn)
    if nn > 1:
        w[nn // 3] = 0.0
    return kdehip.kde(pts, rng.uniform(0.2, 0.6, size=dd), w)


def _evaluate_device_at_manifold():
    L = _lib.lib
    man = np.array(_man(D), dtype=np.uint8)
    return _at_row("kdehip_evaluate_device_at_manifold", [("p", (NQ,), "f64", "all")],
                   lambda bd, at, o, st: _lib.check(L.kdehip_evaluate_device_at_manifold(bd._h, at._h, _lib.addr(o["p"]), st,
                                                                                        _lib.ptr(man, _lib.u8p))),
                   lambda bd, at: dict(p=kdehip.evaluateDualTree(bd, at, manifold=_man(D))), density=_circ_density)


def _eval_avg_logl_device_batch_manifold():
    return _pairs_row("kdehip_eval_avg_logl_device_batch_manifold",
                      lambda pairs, out, st: kdehip.eval_avg_logl_device_batch(pairs, out, stream=st,
                                                                               manifolds=[_man(bd.dims) for bd, _ in pairs]),
                      lambda bd, at: kdehip.evalAvgLogL(bd, at, manifold=_man(bd.bt.dims)), density=_circ_density)


def _summary_device_batch_manifold():
    L = _lib.lib

    def blocking(d, extend, ngrid, bufs):
        man = np.array(_man(d.dims), dtype=np.uint8)
        _lib.check(L.kdehip_density_summary_manifold(d._h, C.byref(C.c_double(extend)), ngrid, *[_lib.ptr(b, _lib.f64p) for b in bufs],
                                                     _lib.ptr(man, _lib.u8p)))
    return _summary_row("kdehip_summary_device_batch_manifold", _circ_density,
                        lambda items, st: kdehip.summary_device_batch([dict(it, manifold=_man(it["density"].dims)) for it in items],
                                                                      stream=st), blocking)


def _sample_device_manifold():
    L = _lib.lib
    name = "kdehip_sample_device_manifold"
    rng = _rng(name)
    p = _circ_density(rng, D, N)
    d = kdehip.DeviceDensity(p)
    man = np.array(_man(D), dtype=np.uint8)

    def enqueue(a, o, st):
        _lib.check(L.kdehip_sample_device_manifold(d._h, NDRAW, _lib.u64(a["seed"]), 0, _lib.addr(a["inputs"]["labels"]),
                                                   _lib.addr(o["pts"]), _lib.addr(o["ind"]), _st(st), _lib.ptr(man, _lib.u8p)))
    row = Row(name, "input", [("pts", (NDRAW, D), "f64", "all"), ("ind", (NDRAW,), "i64", "half")], enqueue, [d])
    for k, s in enumerate(SETS):
        labels = rng.integers(1, N + 1, size=NDRAW).astype(np.int64)
        pts, ind = kdehip.sample(p, NDRAW, ind=labels, seed=950 + k, manifold=_man(D))
        row.add(s, dict(inputs=dict(labels=_dev(labels)), seed=950 + k), dict(pts=pts.T, ind=ind))
    return row


def _sample_device_batch_manifold():
    def item(rng, j, p, nq):
        labels = rng.integers(1, p.bt.num_points + 1, size=NDRAW).astype(np.int64)
        return dict(labels=labels), dict(seed=int(rng.integers(1, 2 ** 40))), labels

    def want(j, p, labels, par):
        pts, ind = kdehip.sample(p, NDRAW, ind=labels, seed=par["seed"], manifold=_man(p.bt.dims))
        return dict(pts=pts.T, ind=ind)
    return _batch_row("kdehip_sample_device_batch_manifold", BATCH,
                      lambda pre, dd, nn, nq: [(pre + "pts", (NDRAW, dd), "f64", "all"), (pre + "ind", (NDRAW,), "i64", "half")], item,
                      lambda items, st: kdehip.sample_device_batch(
                          [dict(density=it["density"], Npts=NDRAW, seed=it["par"]["seed"], ind=it["inp"]["labels"],
                                d_pts=it["out"]["pts"], d_ind=it["out"]["ind"], manifold=_man(it["density"].dims)) for it in items],
                          stream=st), want, density=_circ_density)


# ---- the samplers -----------------------------------------------------------------------------------------------------------
def _prod_trees():
    """the three host densities of the kdehip_prod_philox_device row"""
    rng = np.random.default_rng(60)
    trees = []
    for n in PROD_NS:
        pts = synth_mixture(rng, 2, n)
        trees.append(kdehip.kde(pts, silverman_bw(pts)))
    return trees


def _prod_philox_device_manifold():
    """the densities of the kdehip_prod_philox_device row with dimension 0 circular: the general kernel, no tables and no
    screens.  The contract is kdehip_prod_philox_resident_manifold's: "kdehip_prod_philox_device_manifold (sample offset 0)
    with host output buffers, bit for bit".  At most eight calls are in flight per device and stream, as for the Euclidean
    entry; six back to back stay inside that."""
    name = "kdehip_prod_philox_device_manifold"
    trees = _prod_trees()
    ds = [kdehip.DeviceDensity(t) for t in trees]
    M = len(trees)

    def enqueue(a, o, st):
        kdehip.prodAppxMSGibbsS_device(ds, o["points"], o["indices"], Np=PROD_NP, Niter=PROD_NITER, seed=a["seed"], stream=st,
                                       manifold=_man(2))
    row = Row(name, "density", [("points", (PROD_NP, 2), "f64", "all"), ("indices", (PROD_NP, M), "i64", "half")], enqueue, ds)
    for k, s in enumerate(SETS):
        pts, ind = kdehip.prodAppxMSGibbsS_resident(ds, Np=PROD_NP, Niter=PROD_NITER, seed=4200 + k, manifold=_man(2))
        row.add(s, dict(seed=4200 + k), dict(points=pts.T, indices=ind.T))
    return row


# (D, M) of the batched products: 2, 3 and 4 densities, D = 2 for two of them and D = 3 for the third -- and each of the three
# a second time with other densities.  The Euclidean entry forms its launches per (D, M) and enqueues a group of ONE member
# on its own ("a group of one gains nothing from the batched kernel", csrc/product.hip), the circular entry forms them per D:
# three lone products would all take the one-by-one route, which is not what these rows are about.  With the twins every
# product rides a batched launch: three launches in the Euclidean call, two in the circular one.
PROD_BATCH = [(2, 2), (2, 3), (3, 4)] * 2
PROD_BATCH_NS = PROD_NS + (155,)


def _prod_batch_row(name, circular):
    """fp64 products of 2, 3 and 4 resident densities of 150..170 points (PROD_BATCH: each shape twice), every dimension
    active, 96 chains, 3 iterations, in ONE call: one device block and one gather launch for all of them in front of the sampling launches.  The
    sets are five seeds per item.  The header promises every item the bits of kdehip_prod_philox_device[_manifold] with
    the same arguments, and kdehip_prod_philox_resident[_manifold] -- the blocking twin used here -- is that entry with host
    buffers.  Every call of the row asserts that no item was enqueued one by one (kdehip_prod_philox_batch_launches is the
    calling thread's last call: a host-side counter, no wait): the row is about the batched launch."""
    from tests.circular_plan_cases import cut_bandwidths, cut_points
    rng = _rng(name)
    dss, mans = [], []
    for dd, m in PROD_BATCH:
        man = _man(dd) if circular else None
        trees = []
        for n in PROD_BATCH_NS[:m]:
            if circular:   # two clusters at +-3 rad with bandwidth 0.3: the plans reach the circular fast mode
                trees.append(kdehip.kde(cut_points(rng, dd, n, man), cut_bandwidths(rng, dd, man), rng.uniform(0.3, 1.0, n)))
            else:
                pts = synth_mixture(rng, dd, n)
                trees.append(kdehip.kde(pts, silverman_bw(pts)))
        dss.append([kdehip.DeviceDensity(t) for t in trees])
        mans.append(man)
    outputs = [o for j, (dd, m) in enumerate(PROD_BATCH)
               for o in ((f"{j}.points", (PROD_NP, dd), "f64", "all"), (f"{j}.indices", (PROD_NP, m), "i64", "half"))]

    def enqueue(a, o, st):
        pb = kdehip.ProductBatch([dict(trees=dss[j], d_points=o[f"{j}.points"], d_indices=o[f"{j}.indices"], Np=PROD_NP,
                                       Niter=PROD_NITER, seed=a["seeds"][j], manifold=mans[j]) for j in range(len(PROD_BATCH))])
        if circular:
            pb.enqueue(st)   # (kdehip_prod_philox_batch_manifold)
        else:                # the wrapper always goes through the _manifold twin: the Euclidean entry is called directly
            assert pb._marr is None
            _lib.check(_lib.lib.kdehip_prod_philox_batch(pb.n, pb.items, pb.precision, _st(st)))
        launches = kdehip.batch_launches()
        assert launches == {"batched": 2 if circular else 3, "singles": 0}, launches
    row = Row(name, "density", outputs, enqueue, [d for ds in dss for d in ds])
    for k, s in enumerate(SETS):
        seeds = [4300 + 100 * int(circular) + 10 * k + j for j in range(len(PROD_BATCH))]
        want = {}
        for j in range(len(PROD_BATCH)):
            pts, ind = kdehip.prodAppxMSGibbsS_resident(dss[j], Np=PROD_NP, Niter=PROD_NITER, seed=seeds[j], manifold=mans[j])
            want.update({f"{j}.points": pts.T, f"{j}.indices": ind.T})
        row.add(s, dict(seeds=seeds), want)
    return row


def _prod_philox_batch():
    return _prod_batch_row("kdehip_prod_philox_batch", False)


def _prod_philox_batch_manifold():
    return _prod_batch_row("kdehip_prod_philox_batch_manifold", True)


def _product_sample_philox():
    """ONE resident plan over the three densities of the kdehip_prod_philox_device row; the sets are five seeds.  The plan is
    in the row's `densities`, so `close()` is kdehip_product_destroy, and every call on two streams is a call on ONE plan."""
    name = "kdehip_product_sample_philox"
    plan = kdehip.ProductPlan(_prod_trees())
    M = plan.Ndens

    def enqueue(a, o, st):
        plan.sample_philox_device(PROD_NP, PROD_NITER, a["seed"], 0, True, o["points"], o["indices"], None, st)
    row = Row(name, "density", [("points", (PROD_NP, 2), "f64", "all"), ("indices", (PROD_NP, M), "i64", "half")], enqueue, [plan])
    for k, s in enumerate(SETS):
        pts, ind = plan.sample(PROD_NP, Niter=PROD_NITER, seed=4500 + k)   # (kdehip_product_sample_philox_host)
        row.add(s, dict(seed=4500 + k), dict(points=pts.T, indices=ind.T))
    return row


def _product_sample_streams():
    """the same plan with caller-owned random numbers on the device: d_randU and d_randN for 96 chains, the Philox streams of
    five seeds.
    The twin is the plan's OWN call, made once per set with the device idle and synchronised: sections 1 and 2 of the header
    state how kdehip_gibbs1 and a plan consume the arrays, not that the two give the same bits (the one-shot entry may pick
    another arithmetic for the densities it packs, and the tests of the two compare points to 1e-12, not bit for bit)."""
    import torch
    name = "kdehip_product_sample_streams"
    plan = kdehip.ProductPlan(_prod_trees())
    M = plan.Ndens
    K, R = plan.randu_per_sample(PROD_NITER), plan.randn_per_sample()
    nU, nN = PROD_NP * K, PROD_NP * R

    def enqueue(a, o, st):
        plan.sample_streams_device(PROD_NP, PROD_NITER, a["inputs"]["randU"], nU, a["inputs"]["randN"], nN, True, o["points"],
                                   o["indices"], None, st)
    row = Row(name, "input", [("points", (PROD_NP, 2), "f64", "all"), ("indices", (PROD_NP, M), "i64", "half")], enqueue, [plan])
    for k, s in enumerate(SETS):
        u, n = kdehip.philox_streams(4600 + k, 0, PROD_NP, K, R)
        args = dict(inputs=dict(randU=_dev(u), randN=_dev(n)))
        outs = row.new_outputs()
        torch.cuda.synchronize()
        enqueue(args, outs, None)
        torch.cuda.synchronize()
        row.add(s, args, {key: t.cpu().numpy() for key, t in outs.items()})
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
    "kdehip_evaluate_varbw_device": _evaluate_varbw_device,
    "kdehip_sample_device_manifold": _sample_device_manifold,
    "kdehip_sample_device_batch_manifold": _sample_device_batch_manifold,
    "kdehip_product_sample_streams": _product_sample_streams,
    "kdehip_evaluate_varbw_device_at": _evaluate_varbw_device_at,
    "kdehip_eval_avg_logl_varbw_device": _eval_avg_logl_varbw_device,
    "kdehip_prod_exact_device": _prod_exact_device,
    "kdehip_prod_exact_device_batch": _prod_exact_device_batch,
    "kdehip_product_components_device": _product_components_device,
    "kdehip_evaluate_device_at_manifold": _evaluate_device_at_manifold,
    "kdehip_eval_avg_logl_device_batch_manifold": _eval_avg_logl_device_batch_manifold,
    "kdehip_summary_device_batch_manifold": _summary_device_batch_manifold,
    "kdehip_prod_philox_device_manifold": _prod_philox_device_manifold,
    "kdehip_prod_philox_batch": _prod_philox_batch,
    "kdehip_prod_philox_batch_manifold": _prod_philox_batch_manifold,
    "kdehip_product_sample_philox": _product_sample_philox,
}
DENSITY_ROWS = ["kdehip_evaluate_device_at", "kdehip_evaluate_log_device_at", "kdehip_evaluate_device_at_tol", "kdehip_knn_device_at",
                "kdehip_eval_avg_logl_device_batch", "kdehip_eval_avg_logl_log_device_batch", "kdehip_kernel_sum_device_batch",
                "kdehip_summary_device_batch", "kdehip_prod_philox_device",
                "kdehip_evaluate_varbw_device_at", "kdehip_eval_avg_logl_varbw_device", "kdehip_prod_exact_device",
                "kdehip_prod_exact_device_batch", "kdehip_product_components_device", "kdehip_evaluate_device_at_manifold",
                "kdehip_eval_avg_logl_device_batch_manifold", "kdehip_summary_device_batch_manifold",
                "kdehip_prod_philox_device_manifold", "kdehip_prod_philox_batch", "kdehip_prod_philox_batch_manifold",
                "kdehip_product_sample_philox"]
INPUT_ROWS = [n for n in _BUILDERS if n not in DENSITY_ROWS]
ALL_ROWS = INPUT_ROWS + DENSITY_ROWS

# Blocking entries that take the stream their device matrix was produced on and wait for it (include/kdehip.h section 2d:
# "`stream` = the hipStream_t that produced it, waited for").  They return a handle, not arrays, so they have no row: one
# parametrised test of tests/test_gpu_stream_order.py produces the matrix late on a held stream.
BLOCKING_WAITS = ["kdehip_density_from_device_points", "kdehip_density_from_device_points_manifold",
                  "kdehip_density_from_device_points_tree"]

# Entries with a stream argument that have neither a row nor such a test, and why.  tests/test_stream_order_table.py checks
# that every function of include/kdehip.h with a `stream` / `streams` parameter is in exactly one of ALL_ROWS, BLOCKING_WAITS
# and NO_ROW: a new one needs a row or a reason here.
# (kdehip_meanshift_device and kdehip_kernel_sum_device are not listed and the check does not see them: their ABI has no
# stream argument, they return their results to HOST arrays and block on the calling thread's stream -- include/kdehip.h
# sections 5h, 5g; the enqueue-only forms are the two _device_batch rows.)
NO_ROW = {
    "kdehip_product_multi_sample_philox": "takes one stream per device and needs several GPUs; tests/test_gpu_multi.py covers it",
    "kdehip_profile_sampler_read": "a diagnostic that waits for the stream it reads",
}


def _circ_matrix(rng):
    """a (D, N) matrix whose dimension 0 is an angle straddling +-pi (the search of a circular call wraps its differences)"""
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + rng.uniform(-1, 1, size=(D, 1))
    pts[0] = _wrap(np.pi + 0.3 * rng.standard_normal(N))
    return pts


def blocking_case(name):
    """(true, decoy): two (D, N) host matrices for the entry `name` of BLOCKING_WAITS"""
    rng = _rng(name)
    return _circ_matrix(rng), _circ_matrix(rng)


def blocking_build(name, d_points, stream):
    """the entry `name` of BLOCKING_WAITS on the device matrix d_points ((N, D) row-major = D x N column-major), called
    directly; the _manifold entry with dimension 0 circular, the _tree entry with that and a circular tree.  Returns the
    DeviceDensity, with `bw` and `nevals`."""
    L = _lib.lib
    h, bw, ne = C.c_void_p(), np.empty(D), C.c_int32(0)
    man = np.array(_man(D), dtype=np.uint8)
    head = (C.byref(h), _lib.addr(d_points), D, N, 0, _lib.addr(stream), _lib.ptr(bw, _lib.f64p), C.byref(ne))
    if name == "kdehip_density_from_device_points":
        _lib.check(L.kdehip_density_from_device_points(*head))
        return kdehip.DeviceDensity._built(h, 0, bw, int(ne.value))
    if name == "kdehip_density_from_device_points_manifold":
        _lib.check(L.kdehip_density_from_device_points_manifold(*head, _lib.ptr(man, _lib.u8p)))
        return kdehip.DeviceDensity._built(h, 0, bw, int(ne.value), man)
    assert name == "kdehip_density_from_device_points_tree"
    _lib.check(L.kdehip_density_from_device_points_tree(*head, _lib.ptr(man, _lib.u8p), _lib.ptr(man, _lib.u8p)))
    return kdehip.DeviceDensity._built(h, 0, bw, int(ne.value), man, man)


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
