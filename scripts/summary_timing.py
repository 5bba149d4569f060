"""Timings of getKDEMax and the other summaries (csrc/summary.hip, include/kdehip.h section 5c).

  1. getKDEMax of one 6-D, 2048-point resident density (N = 200): one summary_device_batch call of one item, enqueued and
     synchronised; host wall clock, median of 50
  2. getKDEMax of 256 such densities: one summary_device_batch call of 256 items against 256 single calls (each one
     enqueued and synchronised), and against the host composition (marginal -> 1-D density on the grid -> first argmax) in
     numpy on this machine's cores, timed on 8 of the densities and scaled to 256
  3. getKDEMax of one 6-D density of 50,000 points (the leaf split over many groups)

`--profile`: only the device calls of 1-3 (20 of each), for a run under `rocprofv3 --kernel-trace --stats` whose stats give the
kernel times.  Prints one line per measurement; nothing is gated on them.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kdehip  # noqa: E402
from kdehip.summary import grid  # noqa: E402

VALU_PEAK_FP64_TFLOPS = 78.6  # as bench.py: 256 CU x 4 SIMD x 16 lanes x 2 flop x 2.4 GHz
FLOPS_PER_EVAL = 25  # one 1-D kernel value: subtract, square, scale, exp_nonpos (~20), weight, add


def dens(seed, D, N):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))
    return kdehip.kde(pts, rng.uniform(0.2, 0.5, size=D))


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(np.min(out))


def batch_fn(ds, Ngrid=200):
    dev = torch.device("cuda", 0)
    outs = [torch.empty(d.dims, dtype=torch.float64, device=dev) for d in ds]
    items = [{"density": d, "Ngrid": Ngrid, "argmax": o} for d, o in zip(ds, outs)]
    st = torch.cuda.current_stream(dev)

    def run():
        kdehip.summary_device_batch(items, stream=st.cuda_stream)
        st.synchronize()
    return run, outs


def host_kde_max(p, Ngrid=200):
    """the composition in numpy: marginal weights / variance of original point 0, the grid, the direct sum, first argmax"""
    pts, w = kdehip.getPoints(p), kdehip.getWeights(p)
    w = w / np.cumsum(w)[-1]
    v = kdehip.getBW(p)[:, 0] ** 2
    out = np.empty(p.bt.dims)
    for i in range(p.bt.dims):
        lo, hi = pts[i].min(), pts[i].max()
        dr = 0.1 * (hi - lo)
        x = grid(lo - dr, hi + dr, Ngrid)
        d = x[:, None] - pts[i][None, :]
        y = (np.exp(d * d * (-0.5 / v[i])) * w[None, :]).sum(axis=1) / np.sqrt(2 * np.pi * v[i])
        out[i] = x[int(np.argmax(y))]
    return out


def main():
    hosts = [dens(1000 + k, 6, 2048) for k in range(256)]
    ds = [kdehip.DeviceDensity(h) for h in hosts]
    big = kdehip.DeviceDensity(dens(7, 6, 50000))
    one, _ = batch_fn(ds[:1])
    many, outs = batch_fn(ds)
    bigrun, _ = batch_fn([big])
    singles = [batch_fn([d])[0] for d in ds]
    if "--profile" in sys.argv:
        for fn in (one, many, bigrun):
            for _ in range(20):
                fn()
        return
    many()
    ref = np.stack([kdehip.getKDEMax(h) for h in hosts[:8]])
    assert np.array_equal(np.stack([o.cpu().numpy() for o in outs[:8]]), ref)
    med, mn = wall(one, 50)
    print(f"getKDEMax 6-D N=2048 resident, one item: median {med:.0f} us (min {mn:.0f}) per enqueue + synchronise")
    bmed, bmin = wall(many, 20)
    smed, smin = wall(lambda: [f() for f in singles], 5)
    hmed, hmin = wall(lambda: [host_kde_max(h) for h in hosts[:8]], 3)
    evals = 256 * 6 * 200 * 2048
    print(f"getKDEMax x256 (6-D N=2048): one batch median {bmed:.0f} us (min {bmin:.0f}); 256 single calls median {smed:.0f} us "
          f"(min {smin:.0f}); host numpy composition {hmed * 32 / 1e3:.0f} ms (8 timed, x32); {evals / 1e6:.0f} M evaluations "
          f"-> {evals * FLOPS_PER_EVAL / (bmin * 1e-6) / 1e12:.2f} TFLOP/s over the batch's min wall time")
    gmed, gmin = wall(bigrun, 20)
    print(f"getKDEMax 6-D N=50000 resident: median {gmed:.0f} us (min {gmin:.0f}); {6 * 200 * 50000 / 1e6:.0f} M evaluations")


if __name__ == "__main__":
    main()
