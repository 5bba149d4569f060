#!/usr/bin/env python3
"""Timings of evaluation within a tolerance (csrc/evaltol.hip, include/kdehip.h section 5m) against the direct evaluation,
in ONE process on ONE device, warm, the variants in turn within a round.

Workload: leave-one-out self-evaluation of a two-cluster mixture with the bandwidth `kde_auto` selects (what a bandwidth
search or an entropy does all day): 2-D, 3-D and 6-D at N = 65,536 and 3-D at N = 5,000; rel_tol 1e-3, 1e-6 and 0 (every tile
visited: what the box and plan passes cost when nothing can be skipped).

Times are the events the library puts around its own launches while kdehip_profile_sampler is on
(kdehip_profile_phase_read): 1 = the whole call's kernels (direct: partial + finish; within a tolerance: the three passes and
the finish), 3 / 4 / 5 = the box pass, the plan pass and the sweep over the flagged chunks.  Per variant the median over the
rounds of the per-call time.  Nothing is gated on them.

    timeout -k 10 600 python scripts/time_evaltol.py --out profiles/evaltol_timing.txt
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SHAPES = [(2, 65536), (3, 65536), (6, 65536), (3, 5000)]
TOLS = [1e-3, 1e-6, 0.0]


def phase(lib, which):
    ms, n = C.c_double(0.0), C.c_int64(0)
    lib.kdehip_profile_phase_read(which, C.byref(ms), C.byref(n))
    return ms.value, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3, help="calls per variant and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_evaltol.py needs a GPU: a timing taken anywhere else says nothing")
    lib = _lib.lib
    lines = ["# evaluation within a tolerance against the direct evaluation: leave-one-out, two-cluster mixture, kde_auto bandwidth",
             f"# {args.rounds} rounds of {args.steps} calls per variant, the variants in turn; medians over the rounds, ms per call",
             "# D N rel_tol | direct_ms | tol_call_ms box_ms plan_ms sweep_ms | tiles_visited tiles_total share | worst_rel_err | tol/direct"]
    for D, N in SHAPES:
        rng = np.random.default_rng(10 * D + N % 7)
        pts = rng.standard_normal((D, N))
        pts[:, N // 2:] += 3.0
        p = kdehip.kde_auto(pts)
        direct = kdehip.evaluateDualTree(p, lvFlag=True)

        def run_direct():
            lib.kdehip_profile_sampler(1)
            phase(lib, 1)
            for _ in range(args.steps):
                kdehip.evaluateDualTree(p, lvFlag=True)
            ms, n = phase(lib, 1)
            lib.kdehip_profile_sampler(0)
            assert n == args.steps
            return {"call": ms / n}

        def make_tol(rel):
            def run():
                lib.kdehip_profile_sampler(1)
                for w in (1, 3, 4, 5):
                    phase(lib, w)
                for _ in range(args.steps):
                    kdehip.evaluate_tol(p, None, rel, 0.0, lvFlag=True)
                out = {}
                for name, w in (("call", 1), ("box", 3), ("plan", 4), ("sweep", 5)):
                    ms, n = phase(lib, w)
                    assert n == args.steps, (name, n)
                    out[name] = ms / n
                lib.kdehip_profile_sampler(0)
                return out
            return run

        variants = {"direct": run_direct}
        for rel in TOLS:
            variants[rel] = make_tol(rel)
        for fn in variants.values():  # warm-up: code objects, pools
            fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(fn())
        med = {k: {f: float(np.median([t[f] for t in ts])) for f in ts[0]} for k, ts in times.items()}
        for rel in TOLS:
            got, stats = kdehip.evaluate_tol(p, None, rel, 0.0, lvFlag=True, return_stats=True)
            ok = direct > 0
            err = float(np.max((direct[ok] - got[ok]) / direct[ok])) if ok.any() else 0.0
            assert np.all(got <= direct * (1 + 1e-12)) and np.all(got >= direct * (1 - rel) - 1e-12 * direct)
            m = med[rel]
            lines.append(f"{D} {N} {rel:g} | {med['direct']['call']:.4f} | {m['call']:.4f} {m['box']:.4f} {m['plan']:.4f} "
                         f"{m['sweep']:.4f} | {stats[0]} {stats[1]} {stats[0] / stats[1]:.3f} | {err:.2e} | "
                         f"{m['call'] / med['direct']['call']:.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
