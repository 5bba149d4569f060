#!/usr/bin/env python3
"""Timings of joint bandwidth selection (csrc/bwjoint.hip, include/kdehip.h section 5q).  Nothing is gated on them.

  --case run     per shape -- 6-D x 2048 points, 3-D x 65,536 points, and a batch of 64 x (2-D, 200 points) --: the sweeps
                 to tol = 1e-3 from the LOOCV start (`kde(points)`'s bandwidth) and the whole `joint_bandwidth` call, wall
                 clock; the wall clock per sweep from two calls of fixed lengths (tol = 0; 8 and 40 sweeps, whole rounds);
                 beside them, on the same resident density, `evaluate_grad` at the density's own points and leave-one-out
                 `evaluate_log`, device time per call between two events on the launch stream.  The batch: ONE
                 `joint_bandwidth_device_batch` against 64 single resident calls.
  --case trace   no GPU work: reads the database(s) `rocprofv3 --kernel-trace --stats -d DIR` wrote for a `--case run` run
                 (`--trace DIR`, every *.db below it) and prints, per kernel, the median, minimum and maximum device
                 duration (the first three dispatches of a kernel are warm-up), then per shape the device time of one
                 sweep (partial + finish + update) beside the gradient's (moments partial + finish) and the leave-one-out
                 log evaluation's (partial + finish) and their ratios.  The blocking entries take no stream, so this is
                 where the device time per sweep comes from.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 400 python scripts/time_bwjoint.py --case run --out profiles/bwjoint_timing.txt &&
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d trace_out -- python scripts/time_bwjoint.py --case run --rounds 3 &&
    python scripts/time_bwjoint.py --case trace --trace trace_out --out profiles/bwjoint_timing.txt

`--out` appends what was printed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SINGLE = ((6, 2048), (3, 65536))
BATCH = (64, 2, 200)


def clusters(rng, D, N):
    """two clusters of different widths: what a bimodal belief looks like"""
    lab = rng.integers(0, 2, size=N)
    centre = np.stack([np.full(D, -1.5), np.full(D, 1.5)], axis=1)
    return np.ascontiguousarray(centre[:, lab] + rng.standard_normal((D, N)) * np.where(lab == 0, 1.0, 0.6)[None, :])


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
    """the kernel durations of a traced `--case run`, from rocprofv3's rocpd database(s) below `root`: a finish, update or
    reduce kernel belongs to the partial kernel of its family that ran last before it"""
    import collections
    import glob
    import re
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 database (*.db) below {root}")
    fam = {"bwjoint": "sweep", "moments": "grad", "eval": "loo log"}
    by = collections.defaultdict(list)
    for db in dbs:
        last = {}
        for name, start, end, grid in sqlite3.connect(db).execute("select name, start, end, grid_x from kernels order by start"):
            m = re.search(r"(bwjoint|moments)_(partial|finish|update)_kernel(<\d, (?:false|true)>)?|(eval)_(partial|finish)_log_kernel(<\d, (?:false|true)>)?", name)
            if not m:
                continue
            family, kind, targs = (m.group(1), m.group(2), m.group(3)) if m.group(1) else (m.group(4), m.group(5), m.group(6))
            if kind == "partial":
                last[family] = (targs or "", int(grid))
            if family in last:
                by[(last[family], fam[family], kind)].append((end - start) / 1e3)
    med = collections.defaultdict(dict)
    for (shape, family, kind), v in sorted(by.items()):
        v = np.array(v[3:] if len(v) > 3 else v)  # (the warm-up dispatches)
        med[shape].setdefault(family, {})[kind] = float(np.median(v))
        say(f"trace D,circular={shape[0]} partial grid={shape[1]} {family} {kind}: median {np.median(v):.1f} us over {len(v)} "
            f"dispatches (min {v.min():.1f}, max {v.max():.1f})")
    for shape, fams in sorted(med.items()):
        tot = {f: sum(k.values()) for f, k in fams.items()}
        if "sweep" not in tot:
            continue
        line = f"trace D,circular={shape[0]} partial grid={shape[1]}: one sweep {tot['sweep']:.1f} us on the device"
        for other in ("grad", "loo log"):
            if other in tot:
                line += f"; {other} {tot[other]:.1f} us, ratio sweep / {other} = {tot['sweep'] / tot[other]:.3f}"
        say(line)


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
        raise SystemExit("time_bwjoint.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    for D, N in SINGLE:
        pts = clusters(rng, D, N)
        p = kdehip.kde(pts)  # the LOOCV start
        d = kdehip.DeviceDensity(p)
        tag = f"D={D} N={N}"
        bw, info = d.joint_bandwidth(return_info=True)
        say(f"{tag}: {info['iters']} sweeps to tol = 1e-3 from the LOOCV start, L {info['trace'][0]:.4f} -> {info['logl']:.4f}, "
            f"status {info['status']}")
        whole = wall(lambda: d.joint_bandwidth(), args.rounds)
        say(f"{tag}: the whole joint_bandwidth call (resident), median {np.median(whole):.2f} ms wall over {len(whole)} "
            f"(min {whole.min():.2f}, max {whole.max():.2f})")
        host = wall(lambda: kdehip.joint_bandwidth(p), args.rounds)
        say(f"{tag}: the whole joint_bandwidth call (host density), median {np.median(host):.2f} ms wall over {len(host)} "
            f"(min {host.min():.2f}, max {host.max():.2f})")
        short = wall(lambda: d.joint_bandwidth(tol=0.0, maxiter=7), args.rounds)
        long_ = wall(lambda: d.joint_bandwidth(tol=0.0, maxiter=39), args.rounds)
        say(f"{tag}: 8 sweeps {np.median(short):.3f} ms, 40 sweeps {np.median(long_):.3f} ms wall: "
            f"{1e3 * (np.median(long_) - np.median(short)) / 32:.1f} us wall per sweep (rounds of 8, one read each)")
        pos = torch.from_numpy(np.ascontiguousarray(pts.T)).to(dev)
        val = torch.zeros(N, dtype=torch.float64, device=dev)
        grad = torch.zeros((N, D), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev)
        sp = _lib.addr(st.cuda_stream)

        def grad_call():
            _lib.check(_lib.lib.kdehip_evaluate_grad_device(d._h, _lib.addr(pos), N, 1, _lib.addr(val), _lib.addr(grad), None, sp))

        def loo_call():
            _lib.check(_lib.lib.kdehip_evaluate_log_device_at(d._h, d._h, _lib.addr(val), sp, None))

        for name, call in (("evaluate_grad at its own points", grad_call), ("leave-one-out evaluate_log", loo_call)):
            t = []
            for rnd in range(args.rounds + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                if rnd >= 3:
                    t.append(e0.elapsed_time(e1) * 1e3)
            say(f"{tag}: {name}, median {np.median(t):.1f} us between events over {len(t)} calls (min {min(t):.1f}, max {max(t):.1f})")
        d.close()
    many, D, N = BATCH
    dens = [kdehip.DeviceDensity(kdehip.kde(clusters(rng, D, N))) for _ in range(many)]
    items = [dict(density=d) for d in dens]
    res = kdehip.joint_bandwidth_device_batch(items)
    iters = [r[1]["iters"] for r in res]
    say(f"batch {many} x (D={D} N={N}): sweeps to tol = 1e-3 from the LOOCV starts: min {min(iters)}, median "
        f"{int(np.median(iters))}, max {max(iters)}; unconverged {sum(i < 0 for i in iters)}")
    one = wall(lambda: kdehip.joint_bandwidth_device_batch(items), args.rounds)
    each = wall(lambda: [d.joint_bandwidth() for d in dens], args.rounds)
    assert all(np.array_equal(r[0], d.joint_bandwidth()) for r, d in zip(res, dens))
    say(f"batch {many} x (D={D} N={N}): ONE joint_bandwidth_device_batch, median {np.median(one):.2f} ms wall over {len(one)} "
        f"(min {one.min():.2f}, max {one.max():.2f}); per density {np.median(one) / many:.3f} ms")
    say(f"batch {many} x (D={D} N={N}): {many} single resident calls, median {np.median(each):.2f} ms wall over {len(each)} "
        f"(min {each.min():.2f}, max {each.max():.2f}); per density {np.median(each) / many:.3f} ms")
    for d in dens:
        d.close()
    write_out(args.out, lines)


if __name__ == "__main__":
    main()
