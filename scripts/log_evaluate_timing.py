#!/usr/bin/env python3
"""Timings of log-domain evaluation (csrc/evaluate.hip eval_partial_log_kernel, include/kdehip.h section 5f) against the
direct path, and of the direct path against another build of the library (the parent commit's), interleaved in ONE
process on ONE device: a difference is read against the run-to-run spread of the same code, never across invocations.

  f2       6-D, 10,000 sources x 65,536 queries, the host entries kdehip_evaluate_manifold / kdehip_evaluate_log: kernel
           time = the events the library puts around its launches (kdehip_profile_phase_read(1): partial + finish kernels)
  serving  2-D, 200 x 200, 64 resident pairs in one kdehip_eval_avg_logl(_log)_device_batch(_manifold) call: device time
           of the call's three launches between two events on the launch stream

Each round runs `--steps` calls per variant, the variants in turn; per variant the script prints the median over the rounds
of the per-call time and the spread (max - min over the rounds) / median, then the ratios.  Nothing is gated on them.

Every step on the GPU runs under its own time limit, the steps chained:

    timeout -k 10 300 python scripts/log_evaluate_timing.py --shape f2 --parent-lib PARENT.so --out profiles/log_evaluate_timing.md &&
    timeout -k 10 120 python scripts/log_evaluate_timing.py --shape serving --parent-lib PARENT.so --out profiles/log_evaluate_timing.md

`--out` appends a markdown table of what was printed."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def load(path, _lib):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, at) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype = res
            getattr(lib, name).argtypes = at
    return lib


def check(lib, rc):
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {lib.kdehip_last_error().decode()}")


def dens(kdehip, seed, D, N):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((D, N)) * rng.uniform(0.5, 2.0, size=(D, 1))
    return kdehip.kde(pts, rng.uniform(0.2, 0.5, size=D)), pts


def phase(lib):
    ms, n = C.c_double(0.0), C.c_int64(0)
    lib.kdehip_profile_phase_read(1, C.byref(ms), C.byref(n))
    return ms.value, n.value


def f2_variants(libs, kdehip, _lib, D, N, Nq):
    """name -> fn(steps) returning the kernel time per call in us"""
    p, _ = dens(kdehip, 1, D, N)
    rng = np.random.default_rng(2)
    pos = np.ascontiguousarray((rng.standard_normal((D, Nq)) * 1.2).T).ravel()
    out = np.zeros(Nq)
    cd = p._cstruct()
    outs = {}

    def make(lib, entry):
        fn = getattr(lib, entry)

        def run(steps):
            lib.kdehip_profile_sampler(1)
            phase(lib)
            for _ in range(steps):
                check(lib, fn(C.byref(cd), _lib.ptr(pos, _lib.f64p), Nq, 0, _lib.ptr(out, _lib.f64p), 0, None))
            ms, n = phase(lib)
            lib.kdehip_profile_sampler(0)
            assert n == steps, (n, steps)
            outs[(id(lib), entry)] = out.copy()
            return ms * 1e3 / steps
        return run
    v = {}
    for name, lib in libs:
        v[f"direct ({name})"] = make(lib, "kdehip_evaluate_manifold")
        if hasattr(lib, "kdehip_evaluate_log"):
            v[f"log ({name})"] = make(lib, "kdehip_evaluate_log")
    return v, outs, p


def serving_variants(libs, kdehip, _lib, torch, D, N, items):
    hosts = [(dens(kdehip, 100 + 2 * k, D, N)[0], dens(kdehip, 101 + 2 * k, D, N)[0]) for k in range(items)]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    keep, results = [], {}

    def make(lib, entry):
        arr = (_lib.CLoglManifoldItem * items)()
        for k, (a, b) in enumerate(hosts):
            ha, hb = C.c_void_p(), C.c_void_p()
            ca, cb = a._cstruct(), b._cstruct()
            check(lib, lib.kdehip_density_upload(C.byref(ha), C.byref(ca), 0))
            check(lib, lib.kdehip_density_upload(C.byref(hb), C.byref(cb), 0))
            keep.append((lib, ha, hb))
            arr[k].bd, arr[k].at, arr[k].leave_one_out, arr[k].circular_mask = ha, hb, 0, 0
        d_out = torch.zeros(items, dtype=torch.float64, device=dev)
        fn = getattr(lib, entry)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def run(steps):
            st.synchronize()
            e0.record(st)
            for _ in range(steps):
                check(lib, fn(items, arr, d_out.data_ptr(), st.cuda_stream))
            e1.record(st)
            st.synchronize()
            results[(id(lib), entry)] = d_out.cpu().numpy().copy()
            return e0.elapsed_time(e1) * 1e3 / steps
        return run
    v = {}
    for name, lib in libs:
        v[f"direct ({name})"] = make(lib, "kdehip_eval_avg_logl_device_batch_manifold")
        if hasattr(lib, "kdehip_eval_avg_logl_log_device_batch"):
            v[f"log ({name})"] = make(lib, "kdehip_eval_avg_logl_log_device_batch")
    return v, results, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["f2", "serving"], required=True)
    ap.add_argument("--parent-lib", default=None, help="another build of libkdehip.so whose direct path is timed alongside")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=0, help="calls per variant and round (default: 10 for f2, 50 for serving)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("log_evaluate_timing.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    libs = [("this build", _lib.lib)]
    if args.parent_lib:
        libs.append(("parent", load(args.parent_lib, _lib)))
    if args.shape == "f2":
        D, N, Nq = 6, 10000, 65536
        steps = args.steps or 10
        variants, outs, _ = f2_variants(libs, kdehip, _lib, D, N, Nq)
        title = f"f-2 shape: {D}-D, {N} sources x {Nq} queries, host entry, kernel time per call (partial + finish)"
    else:
        D, N, items = 2, 200, 64
        steps = args.steps or 50
        variants, outs, keep = serving_variants(libs, kdehip, _lib, torch, D, N, items)
        title = f"serving shape: {D}-D, {N} x {N}, {items} resident pairs in one batch call, device time per call"
    for fn in variants.values():  # warm-up: code objects, pools
        fn(3)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(fn(steps))
    # what the variants computed: the direct builds bit for bit, the log path to the log of the direct one
    vals = list(outs.items())
    direct = [v for (_, e), v in vals if "log" not in e.replace("logl", "")]
    logs = [v for (_, e), v in vals if "log" in e.replace("logl", "")]
    for d in direct[1:]:
        assert np.array_equal(d, direct[0]), "the direct path of the two builds differs"
    for lg in logs:
        ref = np.log(direct[0]) if args.shape == "f2" else direct[0]
        ok = np.isfinite(ref)
        assert np.all(np.abs(lg[ok] - ref[ok]) <= 1e-12 * np.maximum(1.0, np.abs(ref[ok]))), "log path off the direct one"
    lines = [f"### {title}", "", f"{args.rounds} rounds of {steps} calls per variant, the variants in turn within a round.", "",
             "| variant | median us | min us | max us | spread (max - min) / median |", "|---|---|---|---|---|"]
    med = {}
    for k, ts in times.items():
        m = float(np.median(ts))
        med[k] = m
        lines.append(f"| {k} | {m:.1f} | {min(ts):.1f} | {max(ts):.1f} | {(max(ts) - min(ts)) / m * 100:.1f} % |")
    lines.append("")
    base = med["direct (this build)"]
    if "log (this build)" in med:
        lines.append(f"log / direct (this build): {med['log (this build)'] / base:.3f}")
    if "direct (parent)" in med:
        lines.append(f"direct (this build) / direct (parent): {base / med['direct (parent)']:.3f}")
        if "log (this build)" in med:
            lines.append(f"log (this build) / direct (parent): {med['log (this build)'] / med['direct (parent)']:.3f}")
    lines.append("")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if args.shape == "serving":
        for lib, ha, hb in keep:
            lib.kdehip_density_free(ha)
            lib.kdehip_density_free(hb)


if __name__ == "__main__":
    main()
