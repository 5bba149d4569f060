"""Kernel time of the circular product: the generic arithmetic against the circular fast mode, same inputs, same run.

For one product in two shapes -- BASELINE config 3's (6-D, 4 x 1000 points, 2048 chains, Niter 10) with dimensions 3..5
circular, and config 2's (2-D, 3 x 200 points) with dimension 1 circular -- the sampling kernel alone is timed through
kdehip_profile_sampler / kdehip_profile_sampler_read, alternating

  generic: kdehip_gibbs1_manifold (host trees, the host twin of the Philox streams uploaded, generic arithmetic), and
  fast:    kdehip_prod_philox_device_manifold (resident densities, device Philox, the circular fast mode),

and the wall time of each complete call is recorded beside it.  Both consume the same random numbers, so their labels must
be identical (checked).  Prints one JSON line per shape: medians, the fast / generic ratio and the run-to-run spread
((max - min) / median over the repetitions after warm-up) of each.

    python scripts/circular_mode_timing.py [--reps 15] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kdehip  # noqa: E402

PER_THREAD_STREAM = 2   # hipStreamPerThread: where the blocking one-shot entries run


def wrap(t):
    return t - 2.0 * np.pi * np.floor((t + np.pi) / (2.0 * np.pi))


def densities(seed, D, Ns, circ):
    rng = np.random.default_rng(seed)
    out = []
    for n in Ns:
        p = rng.standard_normal((D, n)) * 0.7
        for d in range(D):
            if circ[d]:
                p[d] = wrap(np.pi + rng.standard_normal(n))   # centred at the cut: the wrap is at work
        out.append(kdehip.kde(p, rng.uniform(0.15, 0.5, D)))
    return out


def read_kernel_ms(stream):
    ms, n = C.c_double(0.0), C.c_int64(0)
    kdehip._clib.kdehip_profile_sampler_read(0, C.c_void_p(stream), C.byref(ms), C.byref(n))
    return ms.value, n.value


def stats(x):
    x = np.asarray(x)
    med = float(np.median(x))
    return {"median": med, "min": float(x.min()), "max": float(x.max()), "spread": float((x.max() - x.min()) / med)}


def run_shape(name, D, Ns, Np, Niter, circ, reps, warmup):
    import torch
    trees = densities(17, D, Ns, circ)
    M = len(Ns)
    L = kdehip.nlevels(max(Ns))
    seed = 2024
    randU, randN = kdehip.philox_streams(seed, 0, Np, M * (1 + L * (Niter + 1)), D * (L + 1))
    dd = [kdehip.DeviceDensity(t) for t in trees]
    P = torch.zeros(D * Np, dtype=torch.float64, device="cuda:0")
    I = torch.zeros(M * Np, dtype=torch.int64, device="cuda:0")
    st = torch.cuda.Stream()
    gen_k, gen_w, fast_k, fast_w = [], [], [], []
    gi = fi = None
    for r in range(warmup + reps):
        kdehip._clib.kdehip_profile_sampler(1)   # (also resets the sums)
        t0 = time.perf_counter()
        _, gi = kdehip.prodAppxMSGibbsS(None, trees, None, None, Niter=Niter, Np=Np, randU=randU, randN=randN, manifold=circ)
        tw = time.perf_counter() - t0
        ms, n = read_kernel_ms(PER_THREAD_STREAM)
        assert n == 1, n
        kdehip._clib.kdehip_profile_sampler(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=Niter, seed=seed, manifold=circ, stream=st.cuda_stream)
        st.synchronize()
        tf = time.perf_counter() - t0
        ms2, n2 = read_kernel_ms(st.cuda_stream)
        assert n2 == 1, n2
        fi = I.cpu().numpy().reshape(Np, M).T
        if r >= warmup:
            gen_k.append(ms); gen_w.append(tw * 1e3); fast_k.append(ms2); fast_w.append(tf * 1e3)
    kdehip._clib.kdehip_profile_sampler(0)
    out = {"shape": name, "D": D, "N": Ns, "Np": Np, "Niter": Niter, "circular": circ, "reps": reps,
           "labels_identical": bool(np.array_equal(gi, fi)),
           "generic_kernel_ms": stats(gen_k), "fast_kernel_ms": stats(fast_k),
           "generic_call_ms": stats(gen_w), "fast_call_ms": stats(fast_w)}
    out["kernel_ratio_fast_over_generic"] = out["fast_kernel_ms"]["median"] / out["generic_kernel_ms"]["median"]
    print(json.dumps(out), flush=True)
    for d in dd:
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    run_shape("config 3 (6-D, 4 x 1000, 2048 chains, Niter 10), dimensions 3..5 circular", 6, [1000] * 4, 2048, 10,
              [0, 0, 0, 1, 1, 1], a.reps, a.warmup)
    run_shape("config 2 (2-D, 3 x 200, 256 chains, Niter 5), dimension 1 circular", 2, [200] * 3, 256, 5, [0, 1], a.reps, a.warmup)


if __name__ == "__main__":
    main()
