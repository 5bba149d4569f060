"""Wall time of circular products through the batched launch, a resident plan and the one-shot entries.

Three comparisons, each alternating its two sides within one process, wall time of the blocking call:

  batch:  64 config-2-shaped products (2-D, 3 x 200 points, 256 chains, Niter 5, dimension 1 circular) in one
          prodAppxMSGibbsS_batch(manifold=...) call, against the same 64 as single prodAppxMSGibbsS_device(manifold=...) calls;
  mul:    the same 64 as mul_device_batch(manifold=...).  Its baseline -- circular items sampled one by one inside the call,
          the route before the batched instantiation existed -- is a process of its own (the switch is read once):
              KDEHIP_BATCH_CIRC=0 python scripts/circular_batch_timing.py --only mul
  plan:   a circular config-3 plan (6-D eeeccc, 4 x 1000 points, 2048 chains, Niter 10) sampled repeatedly, against
          prodAppxMSGibbsS_device(manifold=...) per call on the same densities resident in HBM.

The two sides of `batch` and of `plan` must return the same bytes (checked).  One JSON line per comparison: medians and
the spread (max - min) / median over the repetitions after warm-up.

    python scripts/circular_batch_timing.py [--reps 15] [--warmup 3] [--only batch|mul|plan]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kdehip  # noqa: E402


def wrap(t):
    return t - 2.0 * np.pi * np.floor((t + np.pi) / (2.0 * np.pi))


def densities(seed, D, Ns, circ):
    rng = np.random.default_rng(seed)
    out = []
    for n in Ns:
        p = rng.standard_normal((D, n)) * 0.7
        for d in range(D):
            if circ[d]:   # two clusters either side of the cut: the wrap is at work
                p[d] = wrap(np.where(rng.random(n) < 0.5, 3.0, -3.0) + 0.3 * rng.standard_normal(n))
        out.append(kdehip.kde(p, [0.3 if c else 0.25 for c in circ]))
    return out


def stats(x):
    x = np.asarray(x)
    med = float(np.median(x))
    return {"median": med, "min": float(x.min()), "max": float(x.max()), "spread": float((x.max() - x.min()) / med)}


def config2_sets(nprod):
    circ = [0, 1]
    return circ, [[kdehip.DeviceDensity(t) for t in densities(100 + k, 2, [200] * 3, circ)] for k in range(nprod)]


def run_batch(reps, warmup, nprod=64):
    import torch
    D, M, Np, Niter = 2, 3, 256, 5
    circ, sets = config2_sets(nprod)
    Pb = [torch.zeros(D * Np, dtype=torch.float64, device="cuda:0") for _ in range(nprod)]
    Ib = [torch.zeros(M * Np, dtype=torch.int64, device="cuda:0") for _ in range(nprod)]
    Ps = [torch.zeros(D * Np, dtype=torch.float64, device="cuda:0") for _ in range(nprod)]
    Is = [torch.zeros(M * Np, dtype=torch.int64, device="cuda:0") for _ in range(nprod)]
    st = torch.cuda.Stream()
    batch = kdehip.ProductBatch([dict(trees=sets[k], d_points=Pb[k], d_indices=Ib[k], Np=Np, Niter=Niter, seed=500 + k)
                                 for k in range(nprod)], manifold=circ)
    tb, ts = [], []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.enqueue(st.cuda_stream)
        st.synchronize()
        t1 = time.perf_counter()
        for k in range(nprod):
            kdehip.prodAppxMSGibbsS_device(sets[k], Ps[k], Is[k], Np=Np, Niter=Niter, seed=500 + k, manifold=circ,
                                           stream=st.cuda_stream)
        st.synchronize()
        t2 = time.perf_counter()
        if r >= warmup:
            tb.append((t1 - t0) * 1e3)
            ts.append((t2 - t1) * 1e3)
    same = all(torch.equal(Pb[k], Ps[k]) and torch.equal(Ib[k], Is[k]) for k in range(nprod))
    out = {"comparison": "batch", "products": nprod, "shape": "2-D, 3 x 200, 256 chains, Niter 5, [euclid, circular]",
           "reps": reps, "same_bytes": bool(same), "batched_ms": stats(tb), "single_calls_ms": stats(ts)}
    out["single_over_batched"] = out["single_calls_ms"]["median"] / out["batched_ms"]["median"]
    print(json.dumps(out), flush=True)


def run_mul(reps, warmup, nprod=64):
    circ, sets = config2_sets(nprod)
    seeds = list(range(700, 700 + nprod))
    t = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        outs = kdehip.mul_device_batch(sets, seeds=seeds, manifold=circ)
        t1 = time.perf_counter()
        for o in outs:
            o.close()
        if r >= warmup:
            t.append((t1 - t0) * 1e3)
    route = "one by one" if os.environ.get("KDEHIP_BATCH_CIRC", "1")[:1] == "0" else "batched circular launch"
    print(json.dumps({"comparison": "mul", "products": nprod, "sampling_route": route, "reps": reps,
                      "mul_device_batch_ms": stats(t)}), flush=True)


def run_plan(reps, warmup):
    import torch
    D, Ns, Np, Niter, circ = 6, [1000] * 4, 2048, 10, [0, 0, 0, 1, 1, 1]
    M = len(Ns)
    trees = densities(17, D, Ns, circ)
    dd = [kdehip.DeviceDensity(t) for t in trees]
    Pp = torch.zeros(D * Np, dtype=torch.float64, device="cuda:0")
    Ip = torch.zeros(M * Np, dtype=torch.int64, device="cuda:0")
    Po, Io = torch.zeros_like(Pp), torch.zeros_like(Ip)
    st = torch.cuda.Stream()
    tp, to = [], []
    with kdehip.ProductPlan(trees, manifold=circ) as plan:
        for r in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan.sample_philox_device(Np, Niter, 2024 + r, 0, True, Pp, Ip, None, st.cuda_stream)
            st.synchronize()
            t1 = time.perf_counter()
            kdehip.prodAppxMSGibbsS_device(dd, Po, Io, Np=Np, Niter=Niter, seed=2024 + r, manifold=circ, stream=st.cuda_stream)
            st.synchronize()
            t2 = time.perf_counter()
            assert torch.equal(Pp, Po) and torch.equal(Ip, Io), "plan and one-shot entry disagree"
            if r >= warmup:
                tp.append((t1 - t0) * 1e3)
                to.append((t2 - t1) * 1e3)
        fast = bool(plan.fast_math_path)
    out = {"comparison": "plan", "shape": "6-D eeeccc, 4 x 1000, 2048 chains, Niter 10", "reps": reps, "fast_math_path": fast,
           "plan_ms": stats(tp), "one_shot_device_ms": stats(to)}
    out["one_shot_over_plan"] = out["one_shot_device_ms"]["median"] / out["plan_ms"]["median"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["batch", "mul", "plan"], default=None)
    a = ap.parse_args()
    for name, fn in (("batch", run_batch), ("mul", run_mul), ("plan", run_plan)):
        if a.only in (None, name):
            fn(a.reps, a.warmup)


if __name__ == "__main__":
    main()
