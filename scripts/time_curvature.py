#!/usr/bin/env python3
"""Timings of the curvature sweep (csrc/modes.hip, include/kdehip.h section 5k).  Nothing is gated on them.

  --case kernels   evaluate_hess (curvature_partial_kernel + curvature_finish_kernel) against evaluate_grad
                   (moments_partial_kernel + moments_finish_kernel), resident and enqueue-only, in the same process, warm and
                   alternating, 6-D at 10,000 sources x 65,536 queries and at 2048 x 2048: device time per call between
                   two events on the launch stream, the median over `--rounds` rounds.  Run under
                   `rocprofv3 --kernel-trace --stats` (a run of its own, the program after `--`) for the partial kernels alone.
  --case batch     64 resident 2048-point 6-D densities x 3 query points: ONE evaluate_hess_device_batch against 64 single
                   resident calls, wall clock to the end of the stream.

  --case trace     no GPU work: reads the database(s) `rocprofv3 --kernel-trace --stats -d DIR` wrote for a `--case kernels` run
                   (`--trace DIR`, every *.db below it) and prints, per kernel and grid, the median, minimum and maximum
                   duration over the timed rounds (the first three dispatches of a kernel at a grid are the warm-up rounds)
                   and the curvature / moments ratios; then the VALU instructions per pair of the two 6-D Euclidean partial
                   kernels, counted in their ISA (VALU_PER_PAIR below says how).

Every step on the GPU runs under its own time limit, the steps chained; start from an empty file, `--out` appends:

    timeout -k 10 300 python scripts/time_curvature.py --case kernels --out profiles/curvature_timing.txt &&
    timeout -k 10 300 python scripts/time_curvature.py --case batch --out profiles/curvature_timing.txt &&
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d trace_out -- python scripts/time_curvature.py --case kernels &&
    python scripts/time_curvature.py --case trace --trace trace_out --out profiles/curvature_timing.txt

`--out` appends what was printed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from time_modes import clusters  # noqa: E402  (scripts/ is this script's own directory: three clusters, a multimodal belief)


# VALU instructions per (query, source) pair in the loops of the 6-D Euclidean instantiations, counted in the ISA of
# `hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S csrc/modes.hip` (the instructions whose mnemonic begins with v_
# between a loop's header and its back edge, over the pairs one trip handles): pass one is a body of 93 for four pairs in
# both kernels; pass two is 101 for two pairs in moments_partial_kernel and 78 for one pair in curvature_partial_kernel.
# Recount after any change to those kernels or to pair_sweep.hpp.
VALU_PER_PAIR = {"moments_partial_kernel": (93 / 4, 101 / 2), "curvature_partial_kernel": (93 / 4, 78 / 1)}


def write_out(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def trace_lines(root, say):
    """the kernel durations of a traced `--case kernels` run, from rocprofv3's rocpd database(s) below `root`"""
    import collections
    import glob
    import re
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 database (*.db) below {root}")
    by = collections.defaultdict(list)
    for db in dbs:
        for name, start, end, grid in sqlite3.connect(db).execute("select name, start, end, grid_x from kernels order by start"):
            m = re.search(r"(moments|curvature)_(partial|finish)_kernel", name)
            if m:
                by[(m.group(2), int(grid), m.group(0))].append((end - start) / 1e3)
    med = {}
    for key in sorted(by):
        v = np.array(by[key][3:])  # (the warm-up rounds)
        med[key] = float(np.median(v))
        say(f"trace {key[0]} grid={key[1]} {key[2]}: median {med[key]:.1f} us over {len(v)} dispatches (min {v.min():.1f}, max {v.max():.1f})")
    for (kind, grid, name), m in sorted(med.items()):
        other = (kind, grid, name.replace("curvature", "moments"))
        if name.startswith("curvature") and other in med:
            say(f"trace {kind} grid={grid} ratio curvature / moments = {m / med[other]:.3f}")
    tot = {k: sum(v) for k, v in VALU_PER_PAIR.items()}
    say("VALU instructions per pair in the 6-D Euclidean ISA (pass one + pass two): " +
        ", ".join(f"{k} {v[0]:.2f} + {v[1]:.2f} = {tot[k]:.2f}" for k, v in VALU_PER_PAIR.items()) +
        f", ratio {tot['curvature_partial_kernel'] / tot['moments_partial_kernel']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["kernels", "batch", "trace"], required=True)
    ap.add_argument("--trace", default=None, help="--case trace: the directory rocprofv3 wrote to")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if args.case == "trace":
        if not args.trace:
            raise SystemExit("--case trace needs --trace DIR")
        trace_lines(args.trace, say)
        write_out(args.out, lines)
        return
    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_curvature.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    f64 = dict(dtype=torch.float64, device=dev)

    if args.case == "kernels":
        for D, N, Nq in ((6, 10000, 65536), (6, 2048, 2048)):
            d = kdehip.DeviceDensity(kdehip.kde(rng.standard_normal((D, N)), rng.uniform(0.3, 0.6, size=D)))
            pos = torch.from_numpy(rng.standard_normal((Nq, D))).to(dev)
            val, grad = torch.zeros(Nq, **f64), torch.zeros((Nq, D), **f64)
            hess, cov = torch.zeros((Nq, D, D), **f64), torch.zeros((Nq, D, D), **f64)
            definite = torch.zeros(Nq, dtype=torch.int32, device=dev)
            st = torch.cuda.current_stream(dev)
            sp = _lib.addr(st.cuda_stream)

            def grad_call():
                _lib.check(_lib.lib.kdehip_evaluate_grad_device(d._h, _lib.addr(pos), Nq, 1, _lib.addr(val), _lib.addr(grad),
                                                                None, sp))

            def hess_call():
                _lib.check(_lib.lib.kdehip_evaluate_hess_device(d._h, _lib.addr(pos), Nq, _lib.addr(val), _lib.addr(grad),
                                                                _lib.addr(hess), _lib.addr(cov), _lib.addr(definite), None, sp))

            times = {"evaluate_grad": [], "evaluate_hess": []}
            for rnd in range(args.rounds + 3):  # three warm-up rounds
                for name, call in (("evaluate_grad", grad_call), ("evaluate_hess", hess_call)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    call()
                    e1.record(st)
                    e1.synchronize()
                    if rnd >= 3:
                        times[name].append(e0.elapsed_time(e1) * 1e3)
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, v in times.items():
                say(f"kernels D={D} N={N} Nq={Nq} {k}: median {med[k]:.1f} us over {len(v)} calls "
                    f"(min {min(v):.1f}, max {max(v):.1f})")
            say(f"kernels D={D} N={N} Nq={Nq} ratio evaluate_hess / evaluate_grad = {med['evaluate_hess'] / med['evaluate_grad']:.3f}")
            d.close()
    else:
        D, N, many, Nq = 6, 2048, 64, 3
        dens = [kdehip.DeviceDensity(kdehip.kde(clusters(rng, D, N), [0.4])) for _ in range(many)]
        items = [dict(density=d, pos=torch.from_numpy(rng.standard_normal((Nq, D))).to(dev), logp=torch.zeros(Nq, **f64),
                      grad=torch.zeros((Nq, D), **f64), hess=torch.zeros((Nq, D, D), **f64), cov=torch.zeros((Nq, D, D), **f64),
                      definite=torch.zeros(Nq, dtype=torch.int32, device=dev)) for d in dens]
        st = torch.cuda.current_stream(dev)
        sp = _lib.addr(st.cuda_stream)

        def singles():
            for it in items:
                _lib.check(_lib.lib.kdehip_evaluate_hess_device(it["density"]._h, _lib.addr(it["pos"]), Nq, _lib.addr(it["logp"]),
                                                                _lib.addr(it["grad"]), _lib.addr(it["hess"]), _lib.addr(it["cov"]),
                                                                _lib.addr(it["definite"]), None, sp))

        def batch():
            kdehip.evaluate_hess_device_batch(items, stream=st.cuda_stream)

        times = {"64 single calls": [], "one batch": []}
        kept = {}
        for rnd in range(args.rounds + 3):
            for name, call in (("64 single calls", singles), ("one batch", batch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                st.synchronize()
                if rnd >= 3:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                kept[name] = items[0]["hess"].cpu().numpy().copy()
        assert np.array_equal(kept["64 single calls"], kept["one batch"])
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k, v in times.items():
            say(f"batch D={D} N={N} Nq={Nq} x {many}: {k}: median {med[k]:.3f} ms wall over {len(v)} (min {min(v):.3f}, max {max(v):.3f})")
        say(f"batch ratio 64 single calls / one batch = {med['64 single calls'] / med['one batch']:.2f}")
        for d in dens:
            d.close()
    write_out(args.out, lines)


if __name__ == "__main__":
    main()
