"""Circular against Euclidean form of the same binary and shape (include/kdehip.h section 5d; CIRC instantiations of
csrc/evaluate.hip, csrc/loocv.hip): evaluation 6-D 10,000 x 65,536 with eeeccc, bandwidth search 6 x 2048 with eeeccc, kld_batch of 64
pairs of 200 points.  Host wall clock around blocking calls (median and min of the repetitions), the two forms interleaved.
`--profile evaluate|loocv|kld [euclid|circular]`: only that call, 10 times, for a run under
`rocprofv3 --kernel-trace --stats`, whose stats give the kernel times.  Prints one line per measurement; nothing is gated."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import kdehip  # noqa: E402

MAN6 = [0, 0, 0, 1, 1, 1]


def angles(rng, shape):
    a = math.pi + 0.8 * rng.standard_normal(shape)
    return np.where(a >= math.pi, a - 2.0 * math.pi, a)


def pts6(rng, N):
    return np.vstack([rng.standard_normal((3, N)), angles(rng, (3, N))])


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def cases():
    rng = np.random.default_rng(0)
    p = kdehip.kde(pts6(rng, 10000), [0.3])
    pos = pts6(rng, 65536)
    lo = pts6(rng, 2048)
    ps = [kdehip.DeviceDensity(kdehip.kde(np.vstack([rng.standard_normal(200), angles(rng, 200)]), [0.3])) for _ in range(64)]
    qs = [kdehip.DeviceDensity(kdehip.kde(np.vstack([rng.standard_normal(200), angles(rng, 200)]), [0.3])) for _ in range(64)]
    pairs = list(zip(ps, qs))
    return {"evaluate": (lambda m: kdehip.evaluateDualTree(p, pos, manifold=m), MAN6),
            "loocv": (lambda m: kdehip.auto_bandwidth(lo, manifold=m), MAN6),
            "kld": (lambda m: kdehip.kld_batch(pairs, manifold=m), [0, 1])}


def main():
    cs = cases()
    if "--profile" in sys.argv:
        i = sys.argv.index("--profile")
        fn, man = cs[sys.argv[i + 1]]
        m = man if (len(sys.argv) > i + 2 and sys.argv[i + 2] == "circular") else None
        for _ in range(10):
            fn(m)
        return
    for name, (fn, man) in cs.items():
        fn(None), fn(man)
        e, c = [], []
        for _ in range(5):  # interleaved
            e += wall(lambda: fn(None), 4)
            c += wall(lambda: fn(man), 4)
        print(f"{name}: euclidean median {np.median(e):.0f} us (min {min(e):.0f}, max {max(e):.0f}); circular median "
              f"{np.median(c):.0f} us (min {min(c):.0f}, max {max(c):.0f}); ratio of medians {np.median(c) / np.median(e):.2f}")


if __name__ == "__main__":
    main()
