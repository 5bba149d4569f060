#!/usr/bin/env python3
"""Timings of the kernel sum (csrc/ksum.hip, include/kdehip.h section 5g) against the route the library offered to the same
number before it: `kdehip_evaluate_device_at` of a pre-built density with bandwidth sqrt(v) at b's points (the all-pairs
kernel, its [ngroups][M] scratch and the finish kernel), followed by a torch dot with b's weights.  Both routes run
interleaved in ONE process on ONE device: a difference is read against the run-to-run spread of the same code.

  single  6-D, N = M = 2048, one S: one kdehip_kernel_sum_device_batch call of one item / one evaluate_device_at + one dot
  batch   2-D, 200 x 200, 64 resident pairs: ONE batch call of 64 items / 64 evaluate_device_at calls + 64 dots

Device time per call: two events on the launch stream around `--steps` calls.  Each round runs every variant in turn; per
variant the script prints the median over the rounds and the spread (max - min over the rounds) / median, then the ratio.
Before anything is timed the two routes' values are compared (1e-12 relative).  Nothing is gated on the times.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 240 python scripts/time_ksum.py --case single --out profiles/ksum_timing.txt &&
    timeout -k 10 240 python scripts/time_ksum.py --case batch --out profiles/ksum_timing.txt

`--out` appends what was printed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["single", "batch"], required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0, help="calls per variant and round (default: 200 for single, 50 for batch)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_ksum.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    D, N, pairs = (6, 2048, 1) if args.case == "single" else (2, 200, 64)
    steps = args.steps or (200 if args.case == "single" else 50)
    rng = np.random.default_rng(7)
    sd = rng.uniform(0.4, 0.8, size=D)
    v = sd * sd
    items, route, keep = [], [], []
    for k in range(pairs):
        pa = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))
        pb = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1)) + 0.3
        a, b = kdehip.kde(pa, rng.uniform(0.2, 0.5, size=D)), kdehip.kde(pb, rng.uniform(0.2, 0.5, size=D))
        da, db = kdehip.DeviceDensity(a), kdehip.DeviceDensity(b)
        dav = kdehip.DeviceDensity(kdehip.kde(pa, sd))  # the same points with variances sd * sd == v: the other route's density
        wb = torch.from_numpy(kdehip.getWeights(b)).to(dev)  # original order, as evaluate_device_at returns its values
        items.append(dict(a=da, b=db, var=v, normalize=True))
        route.append((dav, db, wb, torch.empty(N, dtype=torch.float64, device=dev)))
        keep += [da, db, dav]
    out_new = torch.zeros(pairs, dtype=torch.float64, device=dev)
    out_old = torch.zeros(pairs, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    at = _lib.lib.kdehip_evaluate_device_at_manifold

    arr = (_lib.CKsumItem * pairs)()  # the descriptors are built once: the timed call is the library's entry itself
    for k, it in enumerate(items):
        arr[k].a, arr[k].b, arr[k].var = it["a"]._h, it["b"]._h, _lib.ptr(v, _lib.f64p)
        arr[k].circular_mask, arr[k].normalize = 0, 1

    def new():
        _lib.check(_lib.lib.kdehip_kernel_sum_device_batch(pairs, arr, _lib.addr(out_new), _lib.addr(st.cuda_stream)))

    def old():
        for k, (dav, db, wb, vals) in enumerate(route):
            _lib.check(at(dav._h, db._h, _lib.addr(vals), _lib.addr(st.cuda_stream), None))
            torch.dot(vals, wb, out=out_old[k])

    variants = {"kernel sum (one batch call)": new, f"evaluate_device_at + dot ({pairs} of each)": old}

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
    x, y = out_new.cpu().numpy(), out_old.cpu().numpy()
    assert np.all(x > 0.0) and np.all(np.abs(x - y) <= 1e-12 * y), "the two routes differ"
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    title = (f"{args.case}: {D}-D, {N} x {N}, {pairs} pair(s); device time per call of the whole set, {args.rounds} rounds of "
             f"{steps} calls per variant, the variants in turn within a round")
    lines = [title, f"{'variant':<44} {'median us':>10} {'min us':>10} {'max us':>10} {'spread':>8}"]
    med = {}
    for k, ts in times.items():
        m = float(np.median(ts))
        med[k] = m
        lines.append(f"{k:<44} {m:>10.1f} {min(ts):>10.1f} {max(ts):>10.1f} {(max(ts) - min(ts)) / m * 100:>7.1f}%")
    names = list(variants)
    lines.append(f"kernel sum / (evaluate_device_at + dot): {med[names[0]] / med[names[1]]:.3f}")
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
