#!/usr/bin/env python3
"""Timings of evaluation with per-point bandwidths (csrc/varbw.hip, include/kdehip.h section 5o) beside the one-bandwidth
path, interleaved in ONE process on ONE device: kdehip_evaluate_varbw against kdehip_evaluate / kdehip_evaluate_log on the
SAME points (the per-point density has the uniform one's bandwidth times a factor in [0.5, 2] per point and dimension).

  f2    6-D, 10,000 sources x 65,536 queries
  loo   3-D, 65,536 points, leave-one-out

Times are the events the library puts around its own launches while kdehip_profile_sampler is on
(kdehip_profile_phase_read(1)): for the one-bandwidth path the partial and finish kernels, for the per-point path the
prepass as well.  Each round runs `--steps` calls per variant, the variants in turn; per variant the median over the rounds
and the spread (max - min) / median are printed, then the ratios.  Nothing is gated on them.

Every step on the GPU runs under its own time limit:

    timeout -k 10 300 python scripts/time_varbw.py --out profiles/varbw_timing.txt
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_varbw.py needs a GPU: a timing taken anywhere else says nothing")
    lib = _lib.lib

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"rc {rc}: {lib.kdehip_last_error().decode()}")

    def phase():
        ms, n = C.c_double(0.0), C.c_int64(0)
        lib.kdehip_profile_phase_read(1, C.byref(ms), C.byref(n))
        return ms.value, n.value

    lines = ["# evaluation with per-point bandwidths beside the one-bandwidth path, same points; kernel time per call, ms",
             f"# {args.rounds} rounds of {args.steps} calls per variant, the variants in turn; median over the rounds (spread = (max - min) / median)",
             "# shape | uniform direct | per-point direct | ratio | uniform log | per-point log | ratio"]
    for name, D, N, Nq, loo in (("f2", 6, 10000, 65536, 0), ("loo", 3, 65536, 65536, 1)):
        rng = np.random.default_rng(D)
        pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))
        sd = rng.uniform(0.2, 0.5, size=D)
        uni = kdehip.kde(pts, sd)
        var = kdehip.kde_varbw(pts, sd[:, None] * rng.uniform(0.5, 2.0, size=(D, N)))
        pos = None if loo else np.ascontiguousarray((rng.standard_normal((D, Nq)) * 1.2).T).ravel()
        pp = None if loo else _lib.ptr(pos, _lib.f64p)
        out = np.zeros(Nq)
        cu, cv = uni._cstruct(), var._cstruct()

        def old(entry):
            return lambda: check(entry(C.byref(cu), pp, 0 if loo else Nq, loo, _lib.ptr(out, _lib.f64p), 0, None))

        def new(log):
            return lambda: check(lib.kdehip_evaluate_varbw(C.byref(cv), pp, 0 if loo else Nq, loo, log, _lib.ptr(out, _lib.f64p), 0,
                                                           None))
        variants = {"uniform direct": old(lib.kdehip_evaluate_manifold), "per-point direct": new(0),
                    "uniform log": old(lib.kdehip_evaluate_log), "per-point log": new(1)}

        def run(fn, steps):
            lib.kdehip_profile_sampler(1)  # (also resets the sums)
            phase()
            for _ in range(steps):
                fn()
            ms, n = phase()
            lib.kdehip_profile_sampler(0)
            assert n == steps, (n, steps)
            return ms / steps
        for fn in variants.values():  # warm-up: code objects, pools
            run(fn, 2)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(run(fn, args.steps))
        med = {k: float(np.median(t)) for k, t in times.items()}
        spread = {k: (max(t) - min(t)) / med[k] for k, t in times.items()}
        cell = lambda k: f"{med[k]:.4f} ({spread[k] * 100:.1f} %)"
        line = (f"{name}: {D}-D, {N} x {Nq}{' leave-one-out' if loo else ''} | {cell('uniform direct')} | {cell('per-point direct')} | "
                f"{med['per-point direct'] / med['uniform direct']:.3f} | {cell('uniform log')} | {cell('per-point log')} | "
                f"{med['per-point log'] / med['uniform log']:.3f}")
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
