#!/usr/bin/env python3
"""Timings of entropic optimal transport (csrc/sinkhorn.hip, include/kdehip.h section 5s).  Nothing is gated on them.

  --case run     per shape -- 6-D 2048 x 2048 and 3-D 65,536 x 65,536 --: the wall clock per half-step from two resident calls
                 of fixed lengths (tol = 0, whole rounds) and, on the same two resident densities, `evaluate_log` of q at
                 p's points, device time per call between two events on the launch stream.  Then whole calls of
                 `sinkhorn_divergence` and `equalize` at 6-D x 2048 with reg = 1 and their step counts, and 64 pairs of
                 2-D x 200 in ONE `sinkhorn_batch` against 64 single resident calls.
  --case trace   no GPU work: reads the database(s) `rocprofv3 --kernel-trace --stats -d DIR` wrote for a `--case run` run
                 (`--trace DIR`, every *.db below it) and prints, per kernel, the median, minimum and maximum device
                 duration (the first three dispatches of a kernel are warm-up), then per shape the device time of one
                 half-step (partial + finish + update, the half whose queries are p's points) beside the log evaluation's
                 (partial + finish) and their ratio.  The blocking entries take no stream, so this is where the device
                 time per half-step comes from.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 400 python scripts/time_transport.py --case run --out profiles/transport_timing.txt &&
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d trace_out -- python scripts/time_transport.py --case run --rounds 3 &&
    python scripts/time_transport.py --case trace --trace trace_out --out profiles/transport_timing.txt

`--out` appends what was printed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SINGLE = ((6, 2048, 8, 24), (3, 65536, 2, 6))   # D, N = M, the two fixed lengths
BATCH = (64, 2, 200)


def clusters(rng, D, N, shift=0.0):
    """two clusters of different widths: what a bimodal belief looks like"""
    lab = rng.integers(0, 2, size=N)
    centre = np.stack([np.full(D, -1.5), np.full(D, 1.5)], axis=1)
    return np.ascontiguousarray(centre[:, lab] + rng.standard_normal((D, N)) * np.where(lab == 0, 1.0, 0.6)[None, :] + shift)


def silverman(pts):
    D, N = pts.shape
    return pts.std(axis=1, ddof=1) * (4.0 / ((D + 2.0) * N)) ** (1.0 / (D + 4.0))


def write_out(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def wall(fn, rounds, warm=1):
    out = []
    for rnd in range(rounds + warm):
        t0 = time.perf_counter()
        fn()
        if rnd >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def trace_lines(root, say):
    """the kernel durations of a traced `--case run`, from rocprofv3's rocpd database(s) below `root`: a finish or update kernel
    belongs to the partial kernel of its family that ran last before it"""
    import collections
    import glob
    import re
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 database (*.db) below {root}")
    by = collections.defaultdict(list)
    for db in dbs:
        last = {}
        for name, start, end, grid in sqlite3.connect(db).execute("select name, start, end, grid_x from kernels order by start"):
            m = re.search(r"ot_(partial|finish|update)_kernel<(?:(\d), (?:false|true), )?(\d)>", name)
            e = re.search(r"eval_(partial|finish)_log_kernel(?:<(\d), (?:false|true)>)?", name)
            if m:
                family, kind = f"half-step side {m.group(3)}", m.group(1)
                if kind == "partial":
                    last[family] = (int(m.group(2)), int(grid))
            elif e:
                family, kind = "evaluate_log", e.group(1)
                if kind == "partial":
                    last[family] = (int(e.group(2)), int(grid))
            else:
                continue
            if family in last:
                by[(last[family], family, kind)].append((end - start) / 1e3)
    med = collections.defaultdict(dict)
    for (shape, family, kind), v in sorted(by.items()):
        v = np.array(v[3:] if len(v) > 3 else v)  # (the warm-up dispatches)
        med[shape].setdefault(family, {})[kind] = float(np.median(v))
        say(f"trace D={shape[0]} partial grid={shape[1]} {family} {kind}: median {np.median(v):.1f} us over {len(v)} dispatches "
            f"(min {v.min():.1f}, max {v.max():.1f})")
    for shape, fams in sorted(med.items()):
        tot = {f: sum(k.values()) for f, k in fams.items()}
        if "half-step side 0" in tot and "evaluate_log" in tot:
            say(f"trace D={shape[0]} partial grid={shape[1]}: one half-step {tot['half-step side 0']:.1f} us on the device; "
                f"evaluate_log {tot['evaluate_log']:.1f} us; ratio half-step / evaluate_log = "
                f"{tot['half-step side 0'] / tot['evaluate_log']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["run", "trace"], required=True)
    ap.add_argument("--trace", default=None, help="--case trace: the directory rocprofv3 wrote to")
    ap.add_argument("--rounds", type=int, default=10)
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
        raise SystemExit("time_transport.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    for D, N, short_n, long_n in SINGLE:
        x, y = clusters(rng, D, N), clusters(rng, D, N, 0.5)
        p, q = kdehip.DeviceDensity(kdehip.kde(x, silverman(x))), kdehip.DeviceDensity(kdehip.kde(y, silverman(y)))
        tag = f"D={D} {N} x {N}"
        short = wall(lambda: p.sinkhorn(q, tol=0.0, maxiter=short_n - 1), args.rounds)
        long_ = wall(lambda: p.sinkhorn(q, tol=0.0, maxiter=long_n - 1), args.rounds)
        per = 1e3 * (np.median(long_) - np.median(short)) / (2 * (long_n - short_n))
        say(f"{tag}: {short_n} iterations {np.median(short):.3f} ms, {long_n} iterations {np.median(long_):.3f} ms wall: "
            f"{per:.1f} us wall per half-step (two a iteration, rounds of 8, one read each)")
        val = torch.zeros(N, dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        sp = _lib.addr(st.cuda_stream)
        t = []
        for rnd in range(args.rounds + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _lib.check(_lib.lib.kdehip_evaluate_log_device_at(q._h, p._h, _lib.addr(val), sp, None))
            e1.record(st)
            e1.synchronize()
            if rnd >= 3:
                t.append(e0.elapsed_time(e1) * 1e3)
        say(f"{tag}: evaluate_log of q at p's points, median {np.median(t):.1f} us between events over {len(t)} calls "
            f"(min {min(t):.1f}, max {max(t):.1f})")
        if N <= 4096:
            S, info = p.sinkhorn_divergence(q, reg=1.0, return_info=True)
            whole = wall(lambda: p.sinkhorn_divergence(q, reg=1.0), args.rounds)
            say(f"{tag}: sinkhorn_divergence (reg = 1, tol = 1e-6) = {S:.6f}, steps cross / self / self {info['iters']}; the whole "
                f"call, median {np.median(whole):.2f} ms wall over {len(whole)} (min {whole.min():.2f}, max {whole.max():.2f})")
            logl = torch.from_numpy(-0.5 * ((x - 0.5) ** 2).sum(axis=0) / 4.0).to(dev)
            pw, _, ess = p.bayes_update(logl)
            eq, einfo = pw.equalize(reg=1.0, return_info=True)
            eq.close()

            def equalize():
                pw.equalize(reg=1.0).close()

            whole = wall(equalize, args.rounds)
            say(f"{tag}: equalize (reg = 1, tol = 1e-6) of a density of effective sample size {ess:.0f}: {einfo['iters']} steps, "
                f"err {einfo['err']:.2e}; the whole call, median {np.median(whole):.2f} ms wall over {len(whole)} "
                f"(min {whole.min():.2f}, max {whole.max():.2f})")
            pw.close()
        p.close()
        q.close()
    many, D, N = BATCH
    pairs = []
    for _ in range(many):
        x, y = clusters(rng, D, N), clusters(rng, D, N, 0.5)
        pairs.append((kdehip.DeviceDensity(kdehip.kde(x, silverman(x))), kdehip.DeviceDensity(kdehip.kde(y, silverman(y)))))
    res = kdehip.DeviceDensity.sinkhorn_batch(pairs)
    iters = [r["iters"] for r in res]
    say(f"batch {many} x (D={D} {N} x {N}): steps to tol = 1e-6 at reg = 1: min {min(iters)}, median {int(np.median(iters))}, max "
        f"{max(iters)}; unconverged {sum(i < 0 for i in iters)}")
    assert all(r["value"] == a.sinkhorn(b) for r, (a, b) in zip(res, pairs))
    one = wall(lambda: kdehip.DeviceDensity.sinkhorn_batch(pairs), args.rounds)
    each = wall(lambda: [a.sinkhorn(b) for a, b in pairs], args.rounds)
    say(f"batch {many} x (D={D} {N} x {N}): ONE sinkhorn_batch, median {np.median(one):.2f} ms wall over {len(one)} "
        f"(min {one.min():.2f}, max {one.max():.2f}); per pair {np.median(one) / many:.3f} ms")
    say(f"batch {many} x (D={D} {N} x {N}): {many} single resident calls, median {np.median(each):.2f} ms wall over {len(each)} "
        f"(min {each.min():.2f}, max {each.max():.2f}); per pair {np.median(each) / many:.3f} ms")
    for a, b in pairs:
        a.close()
        b.close()
    write_out(args.out, lines)


if __name__ == "__main__":
    main()
