#!/usr/bin/env python3
"""Timings of the exact product of two densities (csrc/prodexact.hip, include/kdehip.h section 5p) on one device, beside the
routes the library already had.  Everything of a case runs interleaved in ONE process: a difference is read against the
run-to-run spread of the same code.

  small   2-D, 2 x 200 points, Np = 200 (for two inputs the shape of the benchmark's config 2)
  large   6-D, 2 x 2048 points, Np = 2048
            rows + scan      kdehip_prod_exact_device with d_logz alone: the row pass, the finish and the scan
            all passes       ... with d_pts, d_ind and d_logz: the same and the draw pass (the draw pass = the difference)
            sampler          prodAppxMSGibbsS_device of the same two inputs at the default Niter
            evaluate_log     kdehip_evaluate_log_device_at, Nq = N1 queries at N = N2 sources: the row pass's sweep alone
  batch   2-D, 64 pairs of 200 points, Np = 200: ONE kdehip_prod_exact_device_batch call beside 64 single calls

Device time per call: two events on the launch stream around `--steps` calls.  Each round runs every variant in turn; per
variant the script prints the median over the rounds and the spread (max - min over the rounds) / median.  Before anything
is timed logz is compared with log(intersIntg) (1e-10).  Nothing is gated on the times.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 240 python scripts/time_prodexact.py --case small --out profiles/prodexact_timing.txt &&
    timeout -k 10 240 python scripts/time_prodexact.py --case large --out profiles/prodexact_timing.txt &&
    timeout -k 10 240 python scripts/time_prodexact.py --case batch --out profiles/prodexact_timing.txt

`--out` appends what was printed."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["small", "large", "batch"], required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0, help="calls per variant and round (default: 200; 50 for batch)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_prodexact.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    D, N, pairs = {"small": (2, 200, 1), "large": (6, 2048, 1), "batch": (2, 200, 64)}[args.case]
    Np = N
    steps = args.steps or (50 if args.case == "batch" else 200)
    rng = np.random.default_rng(7)
    st = torch.cuda.current_stream(dev)
    L, a = _lib.lib, _lib.addr
    dens, keep = [], []
    for k in range(pairs):
        hp = kdehip.kde(rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)), rng.uniform(0.2, 0.5, size=D))
        hq = kdehip.kde(rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + 0.3, rng.uniform(0.2, 0.5, size=D))
        dp, dq = kdehip.DeviceDensity(hp), kdehip.DeviceDensity(hq)
        dens.append((hp, hq, dp, dq))
        keep += [dp, dq]
    pts = torch.zeros((pairs, Np, D), dtype=torch.float64, device=dev)
    ind = torch.zeros((pairs, Np, 2), dtype=torch.int64, device=dev)
    lz = torch.zeros(pairs, dtype=torch.float64, device=dev)
    s_pts = torch.zeros((Np, D), dtype=torch.float64, device=dev)
    s_ind = torch.zeros((Np, 2), dtype=torch.int64, device=dev)
    vals = torch.zeros(N, dtype=torch.float64, device=dev)
    one = pts.element_size() * Np * D, ind.element_size() * Np * 2

    def single(k, draws=True):
        _, _, dp, dq = dens[k]
        _lib.check(L.kdehip_prod_exact_device(dp._h, dq._h, Np if draws else 0, 11, 0,
                                              a(pts.data_ptr() + k * one[0]) if draws else None,
                                              a(ind.data_ptr() + k * one[1]) if draws else None,
                                              a(lz.data_ptr() + 8 * k), a(st.cuda_stream)))

    arr = (_lib.CProdExactItem * pairs)()  # the descriptors are built once: the timed call is the library's entry itself
    for k, (_, _, dp, dq) in enumerate(dens):
        arr[k].p, arr[k].q, arr[k].Np, arr[k].seed, arr[k].sample_offset = dp._h, dq._h, Np, 11, 0
        arr[k].d_pts, arr[k].d_ind = a(pts.data_ptr() + k * one[0]), a(ind.data_ptr() + k * one[1])
        arr[k].d_logz = a(lz.data_ptr() + 8 * k)

    if args.case == "batch":
        variants = {
            "one batch call of 64 items": lambda: _lib.check(L.kdehip_prod_exact_device_batch(pairs, arr, a(st.cuda_stream))),
            "64 single calls": lambda: [single(k) for k in range(pairs)],
        }
    else:
        _, _, dp, dq = dens[0]
        variants = {
            "prod_exact: rows + scan (logz alone)": lambda: single(0, draws=False),
            "prod_exact: all passes (draws + logz)": lambda: single(0),
            "prodAppxMSGibbsS_device, 2 inputs, Niter 3": lambda: kdehip.prodAppxMSGibbsS_device(
                [dp, dq], s_pts, s_ind, Np=Np, seed=11, stream=st.cuda_stream),
            "evaluate_log_device_at (Nq = N1, N = N2)": lambda: _lib.check(L.kdehip_evaluate_log_device_at(
                dq._h, dp._h, a(vals), a(st.cuda_stream), None)),
        }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        for _ in range(steps):
            fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    for fn in variants.values():  # warm-up: code objects, pools
        for _ in range(5):
            fn()
    st.synchronize()
    got = lz.cpu().numpy()
    for k, (hp, hq, _, _) in enumerate(dens):
        want = math.log(kdehip.intersIntg(hp, hq))
        assert abs(got[k] - want) <= 1e-10, ("logz differs from log(intersIntg)", k, got[k], want)
    assert int(ind.min()) >= 1 and int(ind.max()) <= N and bool(torch.isfinite(pts).all())
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    title = (f"{args.case}: {D}-D, {N} x {N} points, Np = {Np}, {pairs} pair(s); device time per call, {args.rounds} rounds of "
             f"{steps} calls per variant, the variants in turn within a round")
    lines = [title, f"{'variant':<46} {'median us':>10} {'min us':>10} {'max us':>10} {'spread':>8}"]
    med = {}
    for k, ts in times.items():
        m = float(np.median(ts))
        med[k] = m
        lines.append(f"{k:<46} {m:>10.1f} {min(ts):>10.1f} {max(ts):>10.1f} {(max(ts) - min(ts)) / m * 100:>7.1f}%")
    names = list(variants)
    if args.case == "batch":
        lines.append(f"batch / 64 single calls: {med[names[0]] / med[names[1]]:.3f}")
    else:
        lines.append(f"draw pass (all passes - rows + scan): {med[names[1]] - med[names[0]]:.1f} us")
        lines.append(f"all passes / sampler: {med[names[1]] / med[names[2]]:.3f}")
        lines.append(f"rows + scan / evaluate_log: {med[names[0]] / med[names[3]]:.3f}")
    lines.append("")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    for d in keep:
        d.close()


if __name__ == "__main__":
    main()
