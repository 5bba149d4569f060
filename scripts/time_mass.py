#!/usr/bin/env python3
"""Timings of the box mass and the quantiles (csrc/mass.hip, include/kdehip.h section 5l).  Nothing is gated on them.

  --case kernels   box_mass (mass_partial_kernel + mass_finish_kernel) against evaluate (eval_partial_kernel +
                   eval_finish_kernel, the parent's kernel: the yardstick), resident and enqueue-only, in the same process,
                   warm and alternating, 6-D at 10,000 leaves x 65,536 queries, with all six dimensions bounded and with one:
                   device time per call between two events on the launch stream, the median over `--rounds` rounds.
  --case batch     64 resident 2048-point 6-D densities x 3 boxes: ONE box_mass_device_batch against 64 single resident
                   calls, wall clock to the end of the stream.
  --case quantile  3 levels x 6 dimensions: for one resident 2048-point density as 6 single calls and as one batch, and for 64
                   densities as 384 single calls and as one batch (ONE launch), wall clock to the end of the stream.

Every step on the GPU runs under its own time limit, the steps chained; start from an empty file, `--out` appends:

    timeout -k 10 300 python scripts/time_mass.py --case kernels --out profiles/mass_timing.txt &&
    timeout -k 10 300 python scripts/time_mass.py --case batch --out profiles/mass_timing.txt &&
    timeout -k 10 300 python scripts/time_mass.py --case quantile --out profiles/mass_timing.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from time_modes import clusters  # noqa: E402  (scripts/ is this script's own directory: three clusters, a multimodal belief)


def write_out(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def boxes(rng, D, nb, Nq):
    """Nq boxes over nb dimensions of data of unit scale: centres inside the data, one to three units wide"""
    c = rng.standard_normal((Nq, nb))
    half = 0.5 * rng.uniform(1.0, 3.0, size=(Nq, nb))
    return c - half, c + half


def wall(calls, rounds, st, torch):
    """median wall time in ms of each named call to the end of the stream, alternating, after three warm-up rounds"""
    times = {name: [] for name, _ in calls}
    for rnd in range(rounds + 3):
        for name, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            st.synchronize()
            if rnd >= 3:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["kernels", "batch", "quantile"], required=True)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_mass.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    f64 = dict(dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    sp = _lib.addr(st.cuda_stream)

    if args.case == "kernels":
        D, N, Nq = 6, 10000, 65536
        d = kdehip.DeviceDensity(kdehip.kde(rng.standard_normal((D, N)), rng.uniform(0.3, 0.6, size=D)))
        pos = torch.from_numpy(rng.standard_normal((Nq, D))).to(dev)
        val, mass = torch.zeros(Nq, **f64), torch.zeros(Nq, **f64)

        def evaluate_call():
            _lib.check(_lib.lib.kdehip_evaluate_device(d._h, _lib.addr(pos), Nq, 0, _lib.addr(val), sp))

        for nb, mask in ((D, (1 << D) - 1), (1, 1 << 2)):
            lo, hi = (torch.from_numpy(a).to(dev) for a in boxes(rng, D, nb, Nq))

            def mass_call():
                _lib.check(_lib.lib.kdehip_box_mass_device(d._h, mask, _lib.addr(lo), _lib.addr(hi), Nq, _lib.addr(mass), None, sp))

            times = {"evaluate": [], "box_mass": []}
            for rnd in range(args.rounds + 3):  # three warm-up rounds
                for name, call in (("evaluate", evaluate_call), ("box_mass", mass_call)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    call()
                    e1.record(st)
                    e1.synchronize()
                    if rnd >= 3:
                        times[name].append(e0.elapsed_time(e1) * 1e3)
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, v in times.items():
                say(f"kernels D={D} N={N} Nq={Nq} bounded={nb} {k}: median {med[k]:.1f} us over {len(v)} calls "
                    f"(min {min(v):.1f}, max {max(v):.1f})")
            say(f"kernels D={D} N={N} Nq={Nq} bounded={nb} ratio box_mass / evaluate = {med['box_mass'] / med['evaluate']:.2f}")
        d.close()
    elif args.case == "batch":
        D, N, many, Nq = 6, 2048, 64, 3
        dens = [kdehip.DeviceDensity(kdehip.kde(clusters(rng, D, N), [0.4])) for _ in range(many)]
        items = []
        for d in dens:
            lo, hi = (torch.from_numpy(a).to(dev) for a in boxes(rng, D, D, Nq))
            items.append(dict(density=d, lo=lo, hi=hi, mass=torch.zeros(Nq, **f64)))

        def singles():
            for it in items:
                _lib.check(_lib.lib.kdehip_box_mass_device(it["density"]._h, (1 << D) - 1, _lib.addr(it["lo"]), _lib.addr(it["hi"]),
                                                           Nq, _lib.addr(it["mass"]), None, sp))

        def batch():
            kdehip.box_mass_device_batch(items, stream=st.cuda_stream)

        kept = {}
        for name, call in (("64 single calls", singles), ("one batch", batch)):
            call()
            st.synchronize()
            kept[name] = np.stack([it["mass"].cpu().numpy() for it in items])
        assert np.array_equal(kept["64 single calls"], kept["one batch"])
        times = wall((("64 single calls", singles), ("one batch", batch)), args.rounds, st, torch)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k, v in times.items():
            say(f"batch D={D} N={N} boxes={Nq} x {many}: {k}: median {med[k]:.3f} ms wall over {len(v)} (min {min(v):.3f}, max {max(v):.3f})")
        say(f"batch ratio 64 single calls / one batch = {med['64 single calls'] / med['one batch']:.2f}")
        for d in dens:
            d.close()
    else:
        D, N, many = 6, 2048, 64
        levels = torch.tensor([0.025, 0.5, 0.975], **f64)
        dens = [kdehip.DeviceDensity(kdehip.kde(clusters(rng, D, N), [0.4])) for _ in range(many)]
        items = [dict(density=d, dim=k, alpha=levels, x=torch.zeros(3, **f64), iters=torch.zeros(3, dtype=torch.int32, device=dev))
                 for d in dens for k in range(D)]

        def singles(its):
            def run():
                for it in its:
                    _lib.check(_lib.lib.kdehip_quantile_device(it["density"]._h, it["dim"], _lib.addr(levels), 3, None, 0,
                                                               _lib.addr(it["x"]), None, _lib.addr(it["iters"]), None, None, sp))
            return run

        def batch(its):
            return lambda: kdehip.quantile_device_batch(its, stream=st.cuda_stream)

        for label, its in (("1 density", items[:D]), (f"{many} densities", items)):
            names = (f"{len(its)} single calls", "one batch")
            kept = {}
            for name, call in zip(names, (singles(its), batch(its))):
                call()
                st.synchronize()
                kept[name] = np.stack([it["x"].cpu().numpy() for it in its])
            assert np.array_equal(kept[names[0]], kept[names[1]])
            evals = np.stack([it["iters"].cpu().numpy() for it in its])
            times = wall(tuple(zip(names, (singles(its), batch(its)))), args.rounds, st, torch)
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, v in times.items():
                say(f"quantile D={D} N={N} levels=3 x dims={D} x {label}: {k}: median {med[k]:.3f} ms wall over {len(v)} "
                    f"(min {min(v):.3f}, max {max(v):.3f})")
            say(f"quantile {label}: cdf evaluations per level: median {int(np.median(evals))}, max {int(evals.max())}; "
                f"ratio single calls / one batch = {med[names[0]] / med[names[1]]:.2f}")
        for d in dens:
            d.close()
    write_out(args.out, lines)


if __name__ == "__main__":
    main()
