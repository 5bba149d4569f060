#!/usr/bin/env python3
"""Timings of the conditional sweeps (csrc/conditional.hip, include/kdehip.h section 5i).  Nothing is gated on them.

One resident 6-D density of 10,000 leaves, 65,536 queries, the first three dimensions given (ng = 3), enqueue-only calls,
device time per call between two events on the launch stream, the median over `--rounds` warm rounds:

  logz            kdehip_conditional_device asking for logz alone     (expand, partial sweep without moments, finish)
  logz+moments    ... for logz, mean and var                          (the partial sweep carries the moments)
  full            ... for logz, mean, var and the draw                (the select sweep as well)
  evaluate_log    kdehip_evaluate_log_device at the same shape in the same session (eval_partial_log_kernel, which this
                  feature does not touch): the yardstick of the ratios

The step on the GPU runs under its own time limit:

    timeout -k 10 300 python scripts/time_conditional.py --out profiles/conditional_timing.txt

`--out` appends what was printed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import kdehip
    from kdehip import _lib
    if kdehip.device_count() < 1:
        raise SystemExit("time_conditional.py needs a GPU: a timing taken anywhere else says nothing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    D, N, Nq, ng = 6, 10000, 65536, 3
    nf, mask = D - ng, (1 << ng) - 1
    d = kdehip.DeviceDensity(kdehip.kde(rng.standard_normal((D, N)), rng.uniform(0.3, 0.6, size=D)))
    f64 = dict(dtype=torch.float64, device=dev)
    pos = torch.from_numpy(rng.standard_normal((Nq, D))).to(dev)
    given = pos[:, :ng].contiguous()
    val, logz = torch.zeros(Nq, **f64), torch.zeros(Nq, **f64)
    mean, var, pts = (torch.zeros((Nq, nf), **f64) for _ in range(3))
    ind = torch.zeros(Nq, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    sp, a = _lib.addr(st.cuda_stream), _lib.addr

    def log_call():
        _lib.check(_lib.lib.kdehip_evaluate_log_device(d._h, a(pos), Nq, 0, a(val), sp, None))

    def cond(*outs):
        def call():
            _lib.check(_lib.lib.kdehip_conditional_device(d._h, mask, a(given), Nq, _lib.u64(11), 0, *[a(o) for o in outs], None, sp))
        return call

    calls = (("evaluate_log", log_call), ("logz", cond(logz, None, None, None, None)),
             ("logz+moments", cond(logz, mean, var, None, None)), ("full", cond(logz, mean, var, pts, ind)))
    times = {name: [] for name, _ in calls}
    for rnd in range(args.rounds + 3):  # three warm-up rounds
        for name, call in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            if rnd >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        say(f"conditional D={D} ng={ng} N={N} Nq={Nq} {k}: median {med[k]:.1f} us over {len(v)} calls "
            f"(min {min(v):.1f}, max {max(v):.1f})")
    for k in ("logz", "logz+moments", "full"):
        say(f"conditional D={D} ng={ng} N={N} Nq={Nq} ratio {k} / evaluate_log = {med[k] / med['evaluate_log']:.3f}")
    d.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
