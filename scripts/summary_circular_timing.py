"""Timing of `summary_device_batch` with and without circular dimensions (csrc/summary.hip, include/kdehip.h section 5e).

One batch of 64 resident densities (D = 3, N = 1000, Ngrid = 200, every output asked for), enqueued and synchronised:
  --mode euclid     no manifold: the plain instantiations (this mode uses nothing but the call the parent commit has, so
                    the same file times the parent's library)
  --mode circular   the third dimension circular (angles straddling +-pi): the CIRC instantiations
Prints the host wall clock per call (median and min of --reps calls after a warm-up); under `rocprofv3 --kernel-trace
--stats` the stats give the kernel times.  Nothing is gated on the figures.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kdehip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("euclid", "circular"), default="euclid")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    n, D, N, Ng = 64, 3, 1000, 200
    dev = torch.device("cuda", 0)
    items = []
    for k in range(n):
        rng = np.random.default_rng(500 + k)
        pts = rng.standard_normal((D, N))
        th = np.pi + 0.2 * rng.standard_normal(N)
        pts[2] = th - 2 * np.pi * np.floor((th + np.pi) / (2 * np.pi))
        d = kdehip.DeviceDensity(kdehip.kde(pts, rng.uniform(0.2, 0.5, size=D)))
        items.append({"density": d, "Ngrid": Ng,
                      "range": torch.empty(2 * D, dtype=torch.float64, device=dev),
                      "mean": torch.empty(D, dtype=torch.float64, device=dev),
                      "cov": torch.empty(D * D, dtype=torch.float64, device=dev),
                      "argmax": torch.empty(D, dtype=torch.float64, device=dev),
                      "values": torch.empty(D * Ng, dtype=torch.float64, device=dev)})
    st = torch.cuda.current_stream(dev)
    kw = {"manifold": ["euclid", "euclid", "circular"]} if a.mode == "circular" else {}

    def run():
        kdehip.summary_device_batch(items, stream=st.cuda_stream, **kw)
        st.synchronize()

    for _ in range(10):
        run()
    for r in range(a.rounds):   # the spread between rounds of one process is part of the result
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            run()
            t.append((time.perf_counter() - t0) * 1e6)
        print(f"summary_device_batch x{n} (D={D}, N={N}, Ngrid={Ng}) {a.mode} round {r}: median {np.median(t):.1f} us, "
              f"min {np.min(t):.1f} us per enqueue + synchronise", flush=True)


if __name__ == "__main__":
    main()
