"""Device-event timings of the draw kernels of csrc/sample.hip (`sample` / `rand` / `resample`, include/kdehip.h 2f).

  1. 2^20 draws from a 6-D, 1000-point resident density (kdehip_sample_device, table already built)
  2. 64 draws of 200 samples from 2-D, 200-point densities: one kdehip_sample_device_batch call against 64 single calls
  3. the first call on a handle (the blocking table build plus its draw) at N = 10^3 and 10^5, against a later call

Bound of the draw kernel: it writes 8 (D + 1) bytes per sample (56 MB for line 1: ~9 us at 6.3 TB/s) and spends one
Philox4x32-10 block on the uniform, (D + 1) / 2 blocks plus a log, a sqrt and a sin/cos pair (fp64) on the normals, and a
binary search of ~log2(N) dependent loads.  Prints one line per measurement; nothing is gated on them.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kdehip  # noqa: E402


def dens(seed, D, N):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), rng.uniform(0.1, 0.5, size=D), rng.uniform(0.1, 1.0, size=N))


def timed(st, fn, reps):
    """median of `reps` event-timed runs of fn() on stream st, in microseconds"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out)), float(np.min(out))


def main():
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    s = st.cuda_stream
    # 1
    D, Npts = 6, 1 << 20
    d = kdehip.DeviceDensity(dens(1, D, 1000))
    P = torch.empty(D * Npts, dtype=torch.float64, device=dev)
    I = torch.empty(Npts, dtype=torch.int64, device=dev)
    d.sample_device(P, I, Npts, seed=1, stream=s)  # (table build)
    torch.cuda.synchronize()
    med, mn = timed(st, lambda: d.sample_device(P, I, Npts, seed=2, stream=s), 20)
    gb = 8 * (D + 1) * Npts / 1e9
    print(f"draw 2^20 x 6-D from N=1000: median {med:.1f} us, min {mn:.1f} us, {gb * 1e3:.0f} MB written "
          f"-> {gb / (mn * 1e-6) / 1e3:.2f} TB/s at the min")
    # 2
    ds = [kdehip.DeviceDensity(dens(100 + k, 2, 200)) for k in range(64)]
    bufs = [(torch.empty(2 * 200, dtype=torch.float64, device=dev), torch.empty(200, dtype=torch.int64, device=dev))
            for _ in range(64)]
    items = [{"density": ds[k], "Npts": 200, "seed": k, "d_pts": bufs[k][0], "d_ind": bufs[k][1]} for k in range(64)]
    kdehip.sample_device_batch(items, stream=s)  # (table builds)
    torch.cuda.synchronize()

    def singles():
        for k in range(64):
            ds[k].sample_device(bufs[k][0], bufs[k][1], 200, seed=k, stream=s)
    bmed, bmin = timed(st, lambda: kdehip.sample_device_batch(items, stream=s), 20)
    smed, smin = timed(st, singles, 20)
    print(f"64 x 200 draws, 2-D N=200: batch median {bmed:.1f} us (min {bmin:.1f}), 64 single calls median {smed:.1f} us "
          f"(min {smin:.1f})")
    # 3
    for N in (1000, 100000):
        p = dens(7, 3, N)
        firsts, laters = [], []
        P3 = torch.empty(3 * 1024, dtype=torch.float64, device=dev)
        I3 = torch.empty(1024, dtype=torch.int64, device=dev)
        for rep in range(3):
            h = kdehip.DeviceDensity(p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.sample_device(P3, I3, 1024, seed=rep, stream=s)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            h.sample_device(P3, I3, 1024, seed=rep, stream=s)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            firsts.append((t1 - t0) * 1e6)
            laters.append((t2 - t1) * 1e6)
            h.close()
        print(f"first call (table build + 1024 draws), N={N}: {min(firsts):.0f} us host wall; a later call {min(laters):.0f} us")


if __name__ == "__main__":
    main()
