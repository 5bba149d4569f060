#!/usr/bin/env python3
"""Timings of compression by kernel herding (csrc/compress.hip, include/kdehip.h section 5t).  Nothing is gated on them.

  --case run     warm wall clock of whole blocking calls on resident densities, and from two run lengths the time per step:
                 the z pass (a run to M = 1) at 6-D 2048 and 3-D 65,536 beside `evaluate` of the density at its own points
                 (device time between two events on the launch stream, the parent's code path, same run); route A at 6-D
                 2048 -> 128; route B at 3-D 65,536 -> 256, at 6-D 2048 -> 128 (forced) and at 1-D 256 -> 256 (forced: one
                 block a launch, all but an empty launch); 64 densities of 2-D x 200 -> 32 in ONE batch against 64 single
                 calls; the quality (MMD^2 beside 50 weighted random subsets) and the whole call beside `resample(p, M)`.
  --case trace   no GPU work: reads the database(s) `rocprofv3 --kernel-trace --stats -d DIR` wrote for a `--case run` run
                 and prints per kernel the median, minimum and maximum device duration.  The blocking entries take no stream,
                 so this is where the device times of the z pass, of route A's launch and of route B's steps come from.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 400 python scripts/time_compress.py --case run --out profiles/compress_timing.txt &&
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d trace_out -- python scripts/time_compress.py --case run --rounds 3 &&
    python scripts/time_compress.py --case trace --trace trace_out --out profiles/compress_timing.txt

`--out` appends what was printed."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

KS = 0.4
QUALITY = ((2, 300, 30), (6, 513, 64), (2, 2048, 128))
BATCH = (64, 2, 200, 32)


def clusters(rng, D, N):
    """two clusters of different widths and uneven weights: what a bimodal belief looks like"""
    lab = rng.integers(0, 2, size=N)
    centre = np.stack([np.full(D, -1.5), np.full(D, 1.5)], axis=1)
    pts = centre[:, lab] + rng.standard_normal((D, N)) * np.where(lab == 0, 1.0, 0.6)[None, :]
    w = rng.uniform(0.5, 1.5, size=N)
    return np.ascontiguousarray(pts), w / w.sum()


def write_out(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def wall(fn, rounds, warm=2):
    out = []
    for rnd in range(rounds + warm):
        t0 = time.perf_counter()
        fn()
        if rnd >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def fmt(v):
    return f"median {np.median(v):.3f} ms over {len(v)} (min {v.min():.3f}, max {v.max():.3f})"


def trace_lines(root, say):
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
            m = re.search(r"(compress_\w+_kernel|eval_partial_kernel|eval_finish_kernel)(?:<(\d)[^>]*>)?", name)
            if m:
                by[(m.group(1), m.group(2) or "-", int(grid))].append((end - start) / 1e3)
    for (kernel, D, grid), v in sorted(by.items()):
        v = np.array(v[3:] if len(v) > 3 else v)  # (the warm-up dispatches)
        say(f"trace {kernel} D={D} grid={grid}: median {np.median(v):.1f} us over {len(v)} dispatches "
            f"(min {v.min():.1f}, max {v.max():.1f})")


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
        raise SystemExit("time_compress.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    R = args.rounds

    def per_step(d, short, long_, stepwise):
        a = wall(lambda: d.herding_order(short, stepwise=stepwise), R)
        b = wall(lambda: d.herding_order(long_, stepwise=stepwise), R)
        return a, b, 1e3 * (np.median(b) - np.median(a)) / (long_ - short)

    for D, N, M in ((6, 2048, 128), (3, 65536, 256)):
        pts, w = clusters(rng, D, N)
        p = kdehip.kde(pts, [KS], w)
        d, at = kdehip.DeviceDensity(p), kdehip.DeviceDensity(p)
        tag = f"D={D} N={N}"
        zpass = wall(lambda: d.herding_order(1), R)
        say(f"{tag}: a run to M = 1 (the z pass, the self sum, one step; upload, download and synchronisation included), {fmt(zpass)} wall")
        val = torch.zeros(N, dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        t = []
        for rnd in range(R + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _lib.check(_lib.lib.kdehip_evaluate_device_at(d._h, at._h, _lib.addr(val), _lib.addr(st.cuda_stream)))
            e1.record(st)
            e1.synchronize()
            if rnd >= 3:
                t.append(e0.elapsed_time(e1))
        say(f"{tag}: evaluate of the density at its own points, {fmt(np.array(t))} between events")
        routes = ((False, "route A"), (True, "route B (forced)")) if N <= 2048 else ((False, "route B"),)
        for stepwise, name in routes:
            a, b, us = per_step(d, 2, M, stepwise)
            say(f"{tag} -> {M}, {name}: the whole call {fmt(b)} wall; a run to 2 {np.median(a):.3f} ms: {us:.2f} us wall per step")
        d.close()
        at.close()
    pts, w = clusters(rng, 1, 256)
    with kdehip.DeviceDensity(kdehip.kde(pts, [KS], w)) as d:
        a, b, us = per_step(d, 2, 256, True)
        say(f"D=1 N=256 -> 256, route B (forced), one block a launch: {us:.2f} us wall per step (what a launch costs)")
    many, D, N, M = BATCH
    ds = []
    for _ in range(many):
        pts, w = clusters(rng, D, N)
        ds.append(kdehip.DeviceDensity(kdehip.kde(pts, [KS], w)))

    def close_all(out):
        for q in out:
            q.close()

    one = wall(lambda: close_all(kdehip.DeviceDensity.compress_batch(ds, M)), R)
    each = wall(lambda: close_all([d.compress(M) for d in ds]), R)
    say(f"batch {many} x (D={D} N={N} -> {M}): ONE compress_batch, {fmt(one)} wall; per density {np.median(one) / many:.4f} ms")
    say(f"batch {many} x (D={D} N={N} -> {M}): {many} single compress calls, {fmt(each)} wall; per density {np.median(each) / many:.4f} ms")
    close_all(ds)
    for D, N, M in QUALITY:
        pts, w = clusters(rng, D, N)
        p = kdehip.kde(pts, [KS], w)
        bw = math.sqrt(2.0) * KS
        herded = kdehip.mmd(p, p.compress(M), bw)
        rnd = [kdehip.mmd(p, kdehip.kde(pts[:, rng.choice(N, size=M, replace=False, p=w)], [KS]), bw) for _ in range(50)]
        say(f"quality D={D} N={N} -> {M}: MMD^2 of compress {herded:.4e}; 50 weighted random subsets: mean {np.mean(rnd):.4e}, "
            f"best {np.min(rnd):.4e}; ratio mean / compress {np.mean(rnd) / herded:.1f}")
        with kdehip.DeviceDensity(p) as d:
            c = wall(lambda: d.compress(M).close(), R)
            r = wall(lambda: d.resample(M, seed=1).close(), R)
            say(f"quality D={D} N={N} -> {M}: the whole call, resident: compress {fmt(c)} wall; resample(p, {M}) {fmt(r)} wall")
    write_out(args.out, lines)


if __name__ == "__main__":
    main()
