#!/usr/bin/env python
"""The refusals of the entry points on top of PairRun (csrc/evaluate.hip, varbw.hip, ksum.hip, modes.hip, conditional.hip,
mass.hip) as a table: a fixed list of bad calls, each made once, with the code it returns and the words kdehip_last_error()
has afterwards.  tests/refusals_recorded.json is that table, recorded from the library BEFORE a change to the entries' checks;
tests/test_refusals_recorded.py replays it against the library of the day.

    KDEHIP_LIB=/path/to/the/old/libkdehip.so python scripts/record_refusals.py              # the cases that need no GPU
    KDEHIP_LIB=/path/to/the/old/libkdehip.so python scripts/record_refusals.py --resident   # those on resident handles

Each run rewrites its own kind of rows in --out (default tests/refusals_recorded.json) and keeps the other kind.  Every call
returns before anything is launched: the densities are D = 2, N = 20, one of them with per-point bandwidths.  A row is
{"entry", "case", "code", "message", "resident"}; "reordered": true marks a case whose two faults have the same code and
whose message may therefore be that of either check."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "tests", "refusals_recorded.json")
NO_SUCH_DEVICE = 9999      # the host entries: every refusal is the argument's, not the device's
FAKE = C.c_void_p(256)     # a device address nobody reads: the call is refused first
D, N = 2, 20


class Ctx:
    """The densities of the table, and (resident) their handles."""

    def __init__(self, resident):
        import kdehip
        from kdehip import _lib
        self.k, self.l, self.L = kdehip, _lib, _lib.lib
        rng = np.random.default_rng(11)
        self.p = kdehip.kde(rng.standard_normal((D, N)), [0.3])
        self.q = kdehip.kde(rng.standard_normal((D, N)), [0.4])
        self.p3 = kdehip.kde(rng.standard_normal((3, N)), [0.3])
        self.v = kdehip.kde_varbw(rng.standard_normal((D, N)), rng.uniform(0.2, 0.5, size=(D, N)))
        self.keep = []
        self.hp, self.hq, self.h3, self.hv = (self.host(t) for t in (self.p, self.q, self.p3, self.v))
        if resident:
            self.dd = [kdehip.DeviceDensity(t) for t in (self.p, self.q, self.p3, self.v)]
            self.rp, self.rq, self.r3, self.rv = (d._h for d in self.dd)

    def host(self, tree, **change):
        cs0 = tree._cstruct()
        cs = type(cs0).from_buffer_copy(cs0)  # (a copy: the tree's own struct stays as it is)
        for name, val in change.items():
            setattr(cs, name, val)
        self.keep.append(cs)
        return C.byref(cs)

    def f64(self, *shape):
        a = np.full(shape, 0.25)
        self.keep.append(a)
        return self.l.ptr(a, self.l.f64p)

    def i32(self, n):
        a = np.zeros(n, dtype=np.int32)
        self.keep.append(a)
        return self.l.ptr(a, self.l.i32p)

    def i64(self, n):
        a = np.zeros(n, dtype=np.int64)
        self.keep.append(a)
        return self.l.ptr(a, self.l.i64p)

    def man(self, *vals):
        a = np.ascontiguousarray(vals, dtype=np.uint8)
        self.keep.append(a)
        return self.l.ptr(a, self.l.u8p)

    def dbl(self, x):
        v = C.c_double(x)
        self.keep.append(v)
        return C.byref(v)


def entries(c, resident):
    """(entry, good arguments by name in ABI order, roles: which argument is the density / the second density / the required
    output / the positions / their count / the manifold).  Host entries when not resident, the `_device` ones otherwise."""
    E = []

    def add(name, args, **roles):
        E.append((name, args, roles))

    if not resident:
        bd, at, bd3, bdv, dev = c.hp, c.hq, c.h3, c.hv, NO_SUCH_DEVICE
        pos, out = c.f64(3, D), c.f64(3 * N)
        ev = dict(bd="bd", out="out", pos="pos", nq="Nq", man="man")
        add("kdehip_evaluate", dict(bd=bd, pos=pos, Nq=3, loo=0, out=out, device=dev), bd="bd", out="out", pos="pos", nq="Nq")
        for name in ("kdehip_evaluate_manifold", "kdehip_evaluate_log"):
            add(name, dict(bd=bd, pos=pos, Nq=3, loo=0, out=out, device=dev, man=None), **ev)
        add("kdehip_evaluate_tol", dict(bd=bd, pos=pos, Nq=3, loo=0, rel=None, abs=None, out=out, stats=None, device=dev, man=None), **ev)
        add("kdehip_evaluate_varbw", dict(bd=bd, pos=pos, Nq=3, loo=0, log=0, out=out, device=dev, man=None), varbw_ok=True, **ev)
        pr = dict(bd="bd", at="at", out="out", man="man")
        add("kdehip_eval_avg_logl", dict(bd=bd, at=at, loo=0, out=out, device=dev), bd="bd", at="at", out="out")
        for name in ("kdehip_eval_avg_logl_manifold", "kdehip_eval_avg_logl_log"):
            add(name, dict(bd=bd, at=at, loo=0, out=out, device=dev, man=None), **pr)
        add("kdehip_eval_avg_logl_varbw", dict(bd=bd, at=at, loo=0, log=0, out=out, device=dev, man=None), varbw_ok=True, **pr)
        add("kdehip_kernel_sum", dict(bd=bd, at=at, var=None, normalize=1, out=out, device=dev, man=None), **pr)
        add("kdehip_evaluate_grad", dict(bd=bd, pos=pos, Nq=3, log=0, out=out, grad=None, device=dev, man=None), **ev)
        add("kdehip_meanshift", dict(bd=bd, pos=pos, Nq=3, tol=c.dbl(1e-9), maxiter=5, out=c.f64(3 * D), logp=c.f64(3), iters=c.i32(3),
                                     device=dev, man=None), **ev)
        add("kdehip_evaluate_hess", dict(bd=bd, pos=pos, Nq=3, out=out, grad=None, hess=None, cov=None, definite=None, device=dev,
                                         man=None), **ev)
        add("kdehip_box_mass", dict(bd=bd, mask=1, pos=pos, hi=c.f64(3, D), Nq=3, out=out, device=dev, man=None), **ev)
        add("kdehip_quantile", dict(bd=bd, dim=0, pos=pos, Nq=3, tol=None, max_iter=0, out=out, resid=None, iters=None, conv=None,
                                    device=dev, man=None), **ev)
        add("kdehip_conditional", dict(bd=bd, gmask=1, pos=pos, Nq=3, seed=1, offset=0, out=out, mean=None, var=None, pts=None,
                                       ind=None, device=dev, man=None), **ev)
        add("kdehip_condition_weights", dict(bd=bd, gmask=1, pos=pos, Nq=3, out=out, logz=None, device=dev, man=None), **ev)
        return E, dict(bd3=bd3, bdv=bdv)
    bd, at, bd3, bdv = c.rp, c.rq, c.r3, c.rv
    ev = dict(bd="bd", out="out", pos="pos", nq="Nq", man="man")
    add("kdehip_evaluate_device", dict(bd=bd, pos=FAKE, Nq=3, loo=0, out=FAKE, stream=None), bd="bd", out="out", pos="pos", nq="Nq")
    for name in ("kdehip_evaluate_device_manifold", "kdehip_evaluate_log_device"):
        add(name, dict(bd=bd, pos=FAKE, Nq=3, loo=0, out=FAKE, stream=None, man=None), **ev)
    add("kdehip_evaluate_varbw_device", dict(bd=bd, pos=FAKE, Nq=3, log=0, out=FAKE, stream=None, man=None), varbw_ok=True, **ev)
    pr = dict(bd="bd", at="at", out="out", man="man")
    add("kdehip_evaluate_device_at", dict(bd=bd, at=at, out=FAKE, stream=None), bd="bd", at="at", out="out")
    for name in ("kdehip_evaluate_device_at_manifold", "kdehip_evaluate_log_device_at"):
        add(name, dict(bd=bd, at=at, out=FAKE, stream=None, man=None), **pr)
    add("kdehip_evaluate_device_at_tol", dict(bd=bd, at=at, rel=None, abs=None, out=FAKE, stats=None, stream=None, man=None), **pr)
    add("kdehip_eval_avg_logl_device", dict(bd=bd, at=at, loo=0, out=c.f64(1)), bd="bd", at="at", out="out", loo="loo")
    for name in ("kdehip_eval_avg_logl_device_manifold", "kdehip_eval_avg_logl_log_device"):
        add(name, dict(bd=bd, at=at, loo=0, out=c.f64(1), man=None), loo="loo", **pr)
    for name in ("kdehip_evaluate_varbw_device_at", "kdehip_eval_avg_logl_varbw_device"):
        add(name, dict(bd=bd, at=at, loo=0, log=0, out=FAKE, stream=None, man=None), varbw_ok=True, loo="loo", **pr)
    add("kdehip_kernel_sum_device", dict(bd=bd, at=at, var=None, normalize=1, out=c.f64(1), man=None), **pr)
    add("kdehip_evaluate_grad_device", dict(bd=bd, pos=FAKE, Nq=3, log=0, out=FAKE, grad=None, man=None, stream=None), **ev)
    add("kdehip_meanshift_device", dict(bd=bd, pos=FAKE, Nq=3, tol=c.dbl(1e-9), maxiter=5, out=c.f64(3 * D), logp=c.f64(3),
                                        iters=c.i32(3), man=None), **ev)
    add("kdehip_evaluate_hess_device", dict(bd=bd, pos=FAKE, Nq=3, out=FAKE, grad=None, hess=None, cov=None, definite=None, man=None,
                                            stream=None), **ev)
    add("kdehip_box_mass_device", dict(bd=bd, mask=1, pos=FAKE, hi=FAKE, Nq=3, out=FAKE, man=None, stream=None), **ev)
    add("kdehip_quantile_device", dict(bd=bd, dim=0, pos=FAKE, Nq=3, tol=None, max_iter=0, out=FAKE, resid=None, iters=None, conv=None,
                                       man=None, stream=None), **ev)
    add("kdehip_conditional_device", dict(bd=bd, gmask=1, pos=FAKE, Nq=3, seed=1, offset=0, out=FAKE, mean=None, var=None, pts=None,
                                          ind=None, man=None, stream=None), **ev)
    add("kdehip_condition_weights_device", dict(bd=bd, gmask=1, pos=FAKE, Nq=3, out=FAKE, logz=None, man=None, stream=None), **ev)
    return E, dict(bd3=bd3, bdv=bdv)


def batches(c, resident):
    """(entry, item class, a good item's fields, the arguments behind (n, items), whether a density with per-point bandwidths
    is accepted).  Without handles only the list and a zeroed item can be tried."""
    l = c.l
    h = dict(bd=c.rp, at=c.rq) if resident else dict(bd=None, at=None)
    tol = c.dbl(1e-9)
    pair = dict(bd=h["bd"], at=h["at"], leave_one_out=0)
    return [
        ("kdehip_eval_avg_logl_device_batch", l.CLoglItem, pair, (FAKE, None)),
        ("kdehip_eval_avg_logl_device_batch_manifold", l.CLoglManifoldItem, pair, (FAKE, None)),
        ("kdehip_eval_avg_logl_log_device_batch", l.CLoglManifoldItem, pair, (FAKE, None)),
        ("kdehip_kernel_sum_device_batch", l.CKsumItem, dict(a=h["bd"], b=h["at"], normalize=1), (FAKE, None)),
        ("kdehip_meanshift_device_batch", l.CMeanshiftItem, dict(bd=h["bd"], d_start=FAKE, nstart=3, d_x=FAKE, d_logp=FAKE, d_iters=FAKE),
         (tol, 5, None)),
        ("kdehip_evaluate_hess_device_batch", l.CHessItem, dict(bd=h["bd"], d_pos=FAKE, Nq=3, d_logp=FAKE), (None,)),
        ("kdehip_box_mass_device_batch", l.CBoxMassItem, dict(bd=h["bd"], d_lo=FAKE, d_hi=FAKE, Nq=3, d_mass=FAKE, dim_mask=1), (None,)),
        ("kdehip_quantile_device_batch", l.CQuantileItem, dict(bd=h["bd"], d_alpha=FAKE, Nq=3, d_x=FAKE, dim=0), (None, 0, None)),
        ("kdehip_conditional_device_batch", l.CConditionalItem, dict(bd=h["bd"], d_given=FAKE, Nq=3, d_logz=FAKE, given_mask=1), (None,)),
    ]


def cases(c, resident):
    """[(entry, case, thunk)]: the unflagged cases (no handle is read), or the flagged ones."""
    out = []
    E, other = entries(c, resident)
    for name, good, r in E:
        fn = getattr(c.L, name)

        def case(label, _fn=fn, _good=good, _name=name, **change):
            args = dict(_good)
            args.update(change)
            out.append((_name, label, lambda: _fn(*args.values())))

        if resident:
            case("null output", **{r["out"]: None})
            if "at" in r:
                case("more dimensions than the pair's", **{r["bd"]: other["bd3"]})
                case("a null second density", **{r["at"]: None})
            if "loo" in r:
                case("leave-one-out at another density", loo=1)
            if "nq" in r:
                case("Nq = -1", **{r["nq"]: -1})
                case("null positions, Nq = 3", **{r["pos"]: None})
            if "man" in r:
                case("a bad manifold byte", **{r["man"]: c.man(0, 2)})
                case("a bad manifold byte and a null output", **{r["man"]: c.man(0, 2), r["out"]: None})
            if not r.get("varbw_ok"):  # (the varbw entries take such a density: no refusal, and the call would run)
                case("per-point bandwidths", **{r["bd"]: other["bdv"]})
            continue
        case("null density", **{r["bd"]: None})
        case("null output", **{r["out"]: None})
        tree = c.p
        for label, change in (("ndim 0", dict(ndim=0)), ("ndim 9", dict(ndim=9)), ("null means", dict(means=None)),
                              ("npts 0", dict(npts=0))):
            case(label, **{r["bd"]: c.host(tree, **change)})
        if "nq" in r:
            case("Nq = -1", **{r["nq"]: -1})
            case("null positions, Nq = 3", **{r["pos"]: None})
        if "man" in r:
            case("a bad manifold byte", **{r["man"]: c.man(0, 2)})
            case("a bad manifold byte and null means", **{r["man"]: c.man(0, 2), r["bd"]: c.host(tree, means=None)})
        if not r.get("varbw_ok"):  # (the varbw entries take such a density: no refusal, and the call would run)
            case("per-point bandwidths", **{r["bd"]: other["bdv"]})
        if "at" in r:
            case("a null second density", **{r["at"]: None})
            case("more dimensions than the pair's", **{r["at"]: other["bd3"]})
            if "loo" in good:
                case("leave-one-out at another density", loo=1)
    if not resident:  # the `_device` entries refuse a NULL handle without reading one
        for name, good, r in entries_null_handles(c):
            fn = getattr(c.L, name)
            out.append((name, "null density", lambda _fn=fn, _a=good: _fn(*_a.values())))
    for name, cls, fields, rest in batches(c, resident):
        fn = getattr(c.L, name)

        def batch(label, n, items, _fn=fn, _rest=rest, _name=name):
            out.append((_name, label, lambda: _fn(n, items, *_rest)))

        def item(**change):
            it = (cls * 1)()
            for k, v in {**fields, **change}.items():
                setattr(it[0], k, v.value if isinstance(v, C.c_void_p) else v)
            c.keep.append(it)
            return it

        if not resident:
            batch("n = -1", -1, None)
            batch("a null item list", 1, None)
            batch("a zeroed item", 1, (cls * 1)())
            continue
        dens = "a" if "a" in fields else "bd"
        if hasattr(cls, "circular_mask"):
            batch("a mask bit at D", 1, item(circular_mask=1 << D))
        batch("per-point bandwidths", 1, item(**{dens: c.rv}))
        nq = "nstart" if "nstart" in fields else "Nq" if "Nq" in fields else None
        if nq:
            batch("Nq = -1", 1, item(**{nq: -1}))
            first = [k for k in fields if k.startswith("d_")][0]
            batch("null positions, Nq = 3", 1, item(**{first: None}))
        if "at" in fields or "b" in fields:
            second = "b" if "b" in fields else "at"
            batch("more dimensions than the pair's", 1, item(**{dens: c.r3}))
            batch("a null second density", 1, item(**{second: None}))
        if "leave_one_out" in fields:
            batch("leave-one-out at another density", 1, item(leave_one_out=1))
    return out


def entries_null_handles(c):
    """the `_device` entries with every argument good but the handle, which is NULL"""
    saved = {k: getattr(c, k, None) for k in ("rp", "rq", "r3", "rv")}
    c.rp = c.rq = c.r3 = c.rv = None
    E, _ = entries(c, True)
    for k, v in saved.items():
        setattr(c, k, v)
    return E


def record(resident):
    c = Ctx(resident)
    rows = []
    for entry, label, thunk in cases(c, resident):
        code = int(thunk())
        msg = c.L.kdehip_last_error().decode("utf-8", "replace") if code != 0 else ""
        rows.append({"entry": entry, "case": label, "code": code, "message": msg, "resident": bool(resident)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--resident", action="store_true", help="the cases that read a resident handle (needs a GPU)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else []
    marked = {(r["entry"], r["case"]) for r in old if r.get("reordered")}
    rows = [r for r in old if r["resident"] != a.resident] + record(a.resident)
    for r in rows:
        if (r["entry"], r["case"]) in marked:
            r["reordered"] = True
    rows.sort(key=lambda r: (r["resident"], r["entry"], r["case"]))
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows in {a.out} ({sum(r['resident'] for r in rows)} resident), library {os.environ.get('KDEHIP_LIB', 'in tree')}")


if __name__ == "__main__":
    main()
