#!/usr/bin/env python3
"""Timings of the nearest-neighbour search (csrc/knn.hip, include/kdehip.h section 5n) beside the direct evaluation and the
evaluation within a tolerance at the same shapes, in ONE process on ONE device, warm, the variants in turn within a round.

Workload: the one of scripts/time_evaltol.py -- leave-one-out on a two-cluster mixture with the bandwidth `kde_auto` selects:
2-D, 3-D and 6-D at N = 65,536 and 3-D at N = 5,000; k = 1, 8 and 32.

Times are the events the library puts around its own launches while kdehip_profile_sampler is on
(kdehip_profile_phase_read): 1 = the direct evaluation's kernels; 6 / 7 / 8 = the search's box pass, plan pass and sweep over
the flagged chunks.  Per variant the median over the rounds of the per-call time.  The last column is the rel_tol = 1e-3 line
of profiles/evaltol_timing.txt at the same shape (call ms, share of tiles), copied from that file when it is there.  Nothing
is gated on any of it.

    timeout -k 10 600 python scripts/time_knn.py --out profiles/knn_timing.txt
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SHAPES = [(2, 65536), (3, 65536), (6, 65536), (3, 5000)]
KS = [1, 8, 32]


def phase(lib, which):
    ms, n = C.c_double(0.0), C.c_int64(0)
    lib.kdehip_profile_phase_read(which, C.byref(ms), C.byref(n))
    return ms.value, n.value


def evaltol_lines():
    """{(D, N): "call_ms share"} of the rel_tol = 1e-3 lines of profiles/evaltol_timing.txt"""
    out = {}
    path = os.path.join(ROOT, "profiles", "evaltol_timing.txt")
    if os.path.exists(path):
        for line in open(path):
            f = line.replace("|", " ").split()
            if not line.startswith("#") and len(f) > 10 and float(f[2]) == 1e-3:
                out[(int(f[0]), int(f[1]))] = f"{f[4]} {f[10]}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3, help="calls per variant and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_knn.py needs a GPU: a timing taken anywhere else says nothing")
    lib = _lib.lib
    tol = evaltol_lines()
    lines = ["# k nearest neighbours, leave-one-out, two-cluster mixture (the data of scripts/time_evaltol.py)",
             f"# {args.rounds} rounds of {args.steps} calls per variant, the variants in turn; medians over the rounds, ms per call",
             "# D N k | direct_evaluate_ms | knn_ms box_ms plan_ms sweep_ms | tiles_visited tiles_total share | knn/direct | "
             "evaluate_tol(1e-3): call_ms share"]
    for D, N in SHAPES:
        rng = np.random.default_rng(10 * D + N % 7)
        pts = rng.standard_normal((D, N))
        pts[:, N // 2:] += 3.0
        p = kdehip.kde_auto(pts)

        def run_direct():
            lib.kdehip_profile_sampler(1)
            phase(lib, 1)
            for _ in range(args.steps):
                kdehip.evaluateDualTree(p, lvFlag=True)
            ms, n = phase(lib, 1)
            lib.kdehip_profile_sampler(0)
            assert n == args.steps
            return {"call": ms / n}

        def make_knn(k):
            def run():
                lib.kdehip_profile_sampler(1)
                for w in (6, 7, 8):
                    phase(lib, w)
                for _ in range(args.steps):
                    kdehip.knn(p, k=k, lvFlag=True, squared=True)
                out = {}
                for name, w in (("box", 6), ("plan", 7), ("sweep", 8)):
                    ms, n = phase(lib, w)
                    assert n == args.steps, (name, n)
                    out[name] = ms / n
                lib.kdehip_profile_sampler(0)
                out["call"] = out["box"] + out["plan"] + out["sweep"]
                return out
            return run

        variants = {"direct": run_direct}
        for k in KS:
            variants[k] = make_knn(k)
        for fn in variants.values():  # warm-up: code objects, pools
            fn()
        times = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, fn in variants.items():
                times[v].append(fn())
        med = {v: {f: float(np.median([t[f] for t in ts])) for f in ts[0]} for v, ts in times.items()}
        for k in KS:
            _, _, stats = kdehip.knn(p, k=k, lvFlag=True, squared=True, return_stats=True)
            m = med[k]
            lines.append(f"{D} {N} {k} | {med['direct']['call']:.4f} | {m['call']:.4f} {m['box']:.4f} {m['plan']:.4f} "
                         f"{m['sweep']:.4f} | {stats[0]} {stats[1]} {stats[0] / stats[1]:.3f} | "
                         f"{m['call'] / med['direct']['call']:.3f} | {tol.get((D, N), '- -')}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
