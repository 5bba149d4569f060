"""Timings of the refit of a resident density (csrc/refit.hip, include/kdehip.h section 5r) beside the route that existed
before it and beside the other half of a filter step, all in one run.

Shapes: 6-D x 2048, 3-D x 65,536, and 64 densities of 2-D x 200 (one batch against 64 single calls).  Per shape:
  refit      `changeWeights` with device weights: whole-call host time (the call blocks) and the device time of its passes,
             bracketed inside the library (kdehip_profile_phase_read, which = 9)
  bayes      `bayes_update` with device log-likelihoods, likewise
  rebuild    today's route for the same result: download the points, `kde(points, bw, w)`, `DeviceDensity(...)`
  evaluate   `evaluate_log` of the density at its own points (leave-one-out form): the other half of a filter step
Medians of `REPS` runs after a warm-up; prints one line per measurement, nothing is gated on them."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kdehip  # noqa: E402
from kdehip import _lib  # noqa: E402

REPS = 15


def wall(fn):
    """(median, min) host microseconds of fn(), which blocks; the device is idle before each run"""
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(np.min(out))


def device_us(fn):
    """mean device microseconds per call of the refit passes over REPS runs of fn()"""
    ms, n = C.c_double(0.0), C.c_int64(0)
    _lib.lib.kdehip_profile_sampler(1)
    _lib.lib.kdehip_profile_phase_read(9, C.byref(ms), C.byref(n))  # (reset)
    for _ in range(REPS):
        fn()
    _lib.lib.kdehip_profile_phase_read(9, C.byref(ms), C.byref(n))
    _lib.lib.kdehip_profile_sampler(0)
    return ms.value * 1e3 / max(1, n.value), n.value


def source(seed, D, N, dev):
    rng = np.random.default_rng(seed)
    pts = torch.from_numpy(np.ascontiguousarray((rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))).T)).to(dev)
    torch.cuda.synchronize()
    return kdehip.DeviceDensity.from_device_points(pts, D, N), rng


def rebuild(dd, w):
    """today's route: the points come down, the host builder runs, the block goes back up"""
    hp = dd.download()
    return kdehip.DeviceDensity(kdehip.kde(kdehip.getPoints(hp), kdehip.getBW(hp)[:, 0], w))


def main():
    dev = torch.device("cuda", 0)
    for D, N in ((6, 2048), (3, 65536)):
        dd, rng = source(D + N, D, N, dev)
        w = rng.uniform(0.1, 1.0, size=N)
        d_w = torch.from_numpy(w).to(dev)
        d_l = torch.from_numpy(rng.uniform(-30.0, 0.0, size=N)).to(dev)
        for fn in (lambda: dd.changeWeights(d_w), lambda: dd.bayes_update(d_l), lambda: rebuild(dd, w),
                   lambda: dd.evaluate_log(lvFlag=True)):
            fn()  # warm-up: the handle's table, the allocation cache
        for name, fn in (("refit (changeWeights)", lambda: dd.changeWeights(d_w)), ("bayes_update", lambda: dd.bayes_update(d_l))):
            med, mn = wall(fn)
            dus, cnt = device_us(fn)
            print(f"{D}-D x {N}: {name}: whole call median {med:.0f} us (min {mn:.0f}), device passes {dus:.1f} us (mean of {cnt})")
        med, mn = wall(lambda: rebuild(dd, w))
        print(f"{D}-D x {N}: today's route (download, kde, upload): median {med:.0f} us (min {mn:.0f})")
        med, mn = wall(lambda: dd.evaluate_log(lvFlag=True))
        print(f"{D}-D x {N}: evaluate_log at its own points: median {med:.0f} us (min {mn:.0f})")
    # 64 densities of 2-D x 200
    srcs = [source(1000 + k, 2, 200, dev) for k in range(64)]
    dds = [s[0] for s in srcs]
    ws = [s[1].uniform(0.1, 1.0, size=200) for s in srcs]
    d_ws = [torch.from_numpy(w).to(dev) for w in ws]
    items = [{"density": dd, "weights": dw} for dd, dw in zip(dds, d_ws)]

    def singles():
        return [dd.changeWeights(dw) for dd, dw in zip(dds, d_ws)]

    def rebuilds():
        return [rebuild(dd, w) for dd, w in zip(dds, ws)]

    def evaluates():
        return [dd.evaluate_log(lvFlag=True) for dd in dds]
    for fn in (lambda: kdehip.DeviceDensity.refit_batch(items), singles, rebuilds, evaluates):
        fn()
    for name, fn in (("one batch", lambda: kdehip.DeviceDensity.refit_batch(items)), ("64 single calls", singles)):
        med, mn = wall(fn)
        dus, cnt = device_us(fn)
        print(f"64 x (2-D x 200): refit, {name}: whole median {med:.0f} us (min {mn:.0f}), device passes {dus:.1f} us per call "
              f"(mean of {cnt})")
    med, mn = wall(rebuilds)
    print(f"64 x (2-D x 200): today's route, 64 times: median {med:.0f} us (min {mn:.0f})")
    med, mn = wall(evaluates)
    print(f"64 x (2-D x 200): evaluate_log at own points, 64 calls: median {med:.0f} us (min {mn:.0f})")


if __name__ == "__main__":
    main()
