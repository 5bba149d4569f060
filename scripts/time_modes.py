#!/usr/bin/env python3
"""Timings of the moments sweep and of mode finding (csrc/modes.hip, include/kdehip.h section 5h).  Nothing is gated on them.

  --case kernels   evaluate_grad (moments_partial_kernel + moments_finish_kernel) against evaluate_log
                   (eval_partial_log_kernel + eval_finish_log_kernel), resident and enqueue-only, at the evaluation's
                   bench shape (6-D, 10,000 sources x 65,536 queries) and at 6-D 2048 x 2048: device time per call between
                   two events on the launch stream, the median over `--rounds` warm rounds.  Run under
                   `rocprofv3 --kernel-trace --stats` (a run of its own) for the partial kernels alone.
  --case modes     one full `modes` of a resident 6-D 2048-point density (blocking: rounds of sweeps, the read-backs, the
                   merge on the host), wall clock, against 64 such densities in ONE `meanshift_device_batch` of as many
                   sweeps as the slowest start of the single call took, wall clock to the end of the stream.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 300 python scripts/time_modes.py --case kernels --out profiles/modes_timing.txt &&
    timeout -k 10 300 python scripts/time_modes.py --case modes --out profiles/modes_timing.txt

`--out` appends what was printed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def clusters(rng, D, N):
    """three clusters of sd 0.3, three apart, bandwidth 0.4: what a multimodal belief looks like"""
    centres = np.zeros((D, 3))
    centres[0, 1], centres[1, 2] = 3.0, -3.0
    return centres[:, np.arange(N) % 3] + 0.3 * rng.standard_normal((D, N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["kernels", "modes"], required=True)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_modes.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if args.case == "kernels":
        for D, N, Nq in ((6, 10000, 65536), (6, 2048, 2048)):
            d = kdehip.DeviceDensity(kdehip.kde(rng.standard_normal((D, N)), rng.uniform(0.3, 0.6, size=D)))
            pos = torch.from_numpy(rng.standard_normal((Nq, D))).to(dev)
            val = torch.zeros(Nq, dtype=torch.float64, device=dev)
            grad = torch.zeros((Nq, D), dtype=torch.float64, device=dev)
            st = torch.cuda.current_stream(dev)
            sp = _lib.addr(st.cuda_stream)

            def log_call():
                _lib.check(_lib.lib.kdehip_evaluate_log_device(d._h, _lib.addr(pos), Nq, 0, _lib.addr(val), sp, None))

            def grad_call():
                _lib.check(_lib.lib.kdehip_evaluate_grad_device(d._h, _lib.addr(pos), Nq, 1, _lib.addr(val), _lib.addr(grad),
                                                                None, sp))

            times = {"evaluate_log": [], "evaluate_grad": []}
            for rnd in range(args.rounds + 3):  # three warm-up rounds
                for name, call in (("evaluate_log", log_call), ("evaluate_grad", grad_call)):
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
            say(f"kernels D={D} N={N} Nq={Nq} ratio evaluate_grad / evaluate_log = {med['evaluate_grad'] / med['evaluate_log']:.3f}")
            d.close()
    else:
        D, N, many = 6, 2048, 64
        dens = [kdehip.DeviceDensity(kdehip.kde(clusters(rng, D, N), [0.4])) for _ in range(many)]
        single = []
        for rnd in range(args.rounds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            modes, logp, mass, labels = kdehip.modes(dens[0])
            if rnd >= 2:
                single.append((time.perf_counter() - t0) * 1e3)
        x, lp, iters = kdehip.meanshift(dens[0])
        niter = int(np.max(np.abs(iters)))
        say(f"modes D={D} N={N}: {modes.shape[1]} modes, the slowest start took {niter} steps, unconverged {int(np.sum(iters < 0))}")
        say(f"modes single: one kdehip.modes call, median {np.median(single):.2f} ms wall over {len(single)} "
            f"(min {min(single):.2f}, max {max(single):.2f})")
        t0 = time.perf_counter()
        kdehip.meanshift(dens[0])
        say(f"modes single: of which kdehip.meanshift {1e3 * (time.perf_counter() - t0):.2f} ms (the rest is the merge on the host)")
        items = [dict(density=d, x=torch.zeros((N, D), dtype=torch.float64, device=dev),
                      logp=torch.zeros(N, dtype=torch.float64, device=dev),
                      iters=torch.zeros(N, dtype=torch.int32, device=dev)) for d in dens]
        st = torch.cuda.current_stream(dev)
        batch = []
        for rnd in range(args.rounds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kdehip.meanshift_device_batch(items, 1e-9, niter, stream=st.cuda_stream)
            st.synchronize()
            if rnd >= 2:
                batch.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(items[0]["x"].cpu().numpy().T, x)
        say(f"modes batch: {many} densities in one meanshift_device_batch of {niter} sweeps, median {np.median(batch):.2f} ms wall "
            f"over {len(batch)} (min {min(batch):.2f}, max {max(batch):.2f}); per density {np.median(batch) / many:.3f} ms")
        for d in dens:
            d.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
