"""Timings of evalAvgLogL / kld / entropy (csrc/evaluate.hip, include/kdehip.h section 5b).

  1. 64 kld of densities shaped like bench config 2 (2-D, 200 points each), resident: one kld_batch call (128 items,
     one synchronisation) against 64 single kld calls (two blocking evalAvgLogL calls each); host wall clock around work
     that ends in a device synchronise, median of 20
  2. entropy of a 6-D resident density at 2048 and at 10,000 points: host wall clock of one blocking call (median of 50)
     and the kernel-time inputs of the fp64 vector-peak share: N^2 kernel values at (4 D + 3) flops each, as
     `bench.py --frow evaluate` counts them

`--profile-entropy N`: only part 2's call at 6-D, N points (20 of them), for a run under `rocprofv3 --kernel-trace --stats` whose stats give
the kernel times.  Prints one line per measurement; nothing is gated on them.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import kdehip  # noqa: E402

VALU_PEAK_FP64_TFLOPS = 78.6  # as bench.py: 256 CU x 4 SIMD x 16 lanes x 2 flop x 2.4 GHz


def dens(seed, D, N):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))
    return kdehip.kde(pts, rng.uniform(0.2, 0.5, size=D))


def wall(fn, reps):
    """median and min of `reps` host-clock runs of a blocking fn(), in microseconds"""
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(np.min(out))


def entropy_sizes():
    return [(6, 2048), (6, 10000)]


def main():
    if "--profile-entropy" in sys.argv:  # --profile-entropy N: 20 calls at that size only
        N = int(sys.argv[sys.argv.index("--profile-entropy") + 1])
        d = kdehip.DeviceDensity(dens(N, 6, N))
        for _ in range(20):
            kdehip.entropy(d)
        return
    # 1
    ps = [kdehip.DeviceDensity(dens(100 + k, 2, 200)) for k in range(64)]
    qs = [kdehip.DeviceDensity(dens(300 + k, 2, 200)) for k in range(64)]
    pairs = list(zip(ps, qs))
    batch = kdehip.kld_batch(pairs)
    singles = np.array([kdehip.kld(p, q) for p, q in pairs])
    assert np.array_equal(batch, singles)
    bmed, bmin = wall(lambda: kdehip.kld_batch(pairs), 20)
    smed, smin = wall(lambda: [kdehip.kld(p, q) for p, q in pairs], 20)
    print(f"64 kld, 2-D N=200 resident pairs: kld_batch median {bmed:.0f} us (min {bmin:.0f}); 64 single kld calls median "
          f"{smed:.0f} us (min {smin:.0f}); {smed / bmed:.1f}x")
    # 2
    for D, N in entropy_sizes():
        d = kdehip.DeviceDensity(dens(N, D, N))
        kdehip.entropy(d)
        med, mn = wall(lambda: kdehip.entropy(d), 50)
        flops = float(N) * N * (4 * D + 3)
        print(f"entropy {D}-D N={N}: one blocking call median {med:.0f} us (min {mn:.0f}); {flops / 1e9:.3f} GFLOP "
              f"-> {flops / (mn * 1e-6) / 1e12:.2f} TFLOP/s over the call's min wall time "
              f"({flops / (mn * 1e-6) / 1e12 / VALU_PEAK_FP64_TFLOPS:.3f} of the fp64 vector peak)")


if __name__ == "__main__":
    main()
