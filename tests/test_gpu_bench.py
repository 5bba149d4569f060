"""bench.py contract checks on a GPU box: one JSON line with the required keys, and the N>1 code path
(process group "nccl" = RCCL, all-gather of the samples) exercised with a 1-rank group."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"}


def _run(cmd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    # the JSON line is the ONLY thing on stdout (library banners -- RCCL prints one -- go to stderr)
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout
    return json.loads(lines[0])


def test_bench_single_gpu_json_contract():
    d = _run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1"])
    assert REQUIRED <= set(d) and "cpu_baseline" in d
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "f64" and d["scaling"] == "weak"
    assert d["config"]["workload"].startswith("c3")
    r = d["roofline"]
    # the binding resource is vector issue: a physical fraction (< 1) of the fp64 vector peak
    assert r["bound"] == "valu" and r["peak"] == 78.6 and r["unit"] == "TFLOP/s"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.0 < r["frac"] < 1.0
    assert d["normalised_hbm"]["peak_GBps"] == 8000.0 and d["julia"] in ("absent", "present")
    # the physical floor of the vector pipe (committed instruction mix x measured issue costs): below the measured time
    vf = r["valu_floor"]
    assert 0.2 < vf["frac"] < 1.0 and abs(vf["frac"] - vf["ms"] / r["kernel_ms"]) < 1e-12
    ci = d["call_inclusive"]
    assert ci["ms"] > d["roofline"]["kernel_ms"] and ci["gibbs1_caller_streams_ms"] > ci["ms"] * 0.8
    # `value` is a complete prodAppxMSGibbsS-equivalent call from HBM-resident densities (re-layout + tables + sampling
    # every step): slower than re-sampling one resident plan, faster than the same call through host buffers
    assert "prodAppxMSGibbsS-equivalent call" in d["value_is"]
    assert d["roofline"]["kernel_ms"] < d["ms_per_step"] < ci["ms"] * 1.1
    assert d["resident_plan"]["ms_per_launch"] < d["ms_per_step"]
    cs = d["cold_start"]
    assert cs is not None and cs["cold_start_ms"] > cs["second_call_ms"] and cs["libkdehip_bytes"] < 40e6
    assert d["parity"]["label_mismatches"] == 0 and d["parity"]["moment_mean_diff"] < 1e-6
    assert d["parity"]["moment_var_diff"] < 1e-6 and d["parity"]["ks_max"] <= 2.0 / d["parity"]["samples_checked"]
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR` writes the product of the last timed step as its caller receives it (points [D, Nout], labels
    [M, Nout], float64): the same files from run to run, equal to the same call made on its own at that step's offset."""
    import numpy as np
    import torch

    import bench
    import kdehip
    W, K = 2, 3
    runs = []
    for name in ("a", "b"):
        d = _run([sys.executable, "bench.py", "--config", "c2", "--steps", str(K), "--warmup", str(W), "--no-cpu-baseline",
                  "--dump-outputs", str(tmp_path / name)])
        assert d["steps"] == K and d["ms_per_step"] > 0
        assert d["dump_outputs"]["files"] == ["labels.npy", "points.npy"] and d["dump_outputs"]["samples"] == 256
        runs.append({k: np.load(tmp_path / name / f"{k}.npy") for k in ("points", "labels")})
    assert all(a.dtype == np.float64 for r in runs for a in r.values())
    assert np.array_equal(runs[0]["points"], runs[1]["points"]) and np.array_equal(runs[0]["labels"], runs[1]["labels"])
    D, M, N, Nout, Niter, prec, cid = bench.CONFIGS["c2"]
    pts, bws = bench.synth_inputs(kdehip, D, M, N, cid)
    dd = [kdehip.DeviceDensity(kdehip.kde(p, b)) for p, b in zip(pts, bws)]
    P = torch.zeros(D * Nout, dtype=torch.float64, device="cuda:0")
    I = torch.zeros(M * Nout, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    # (bench.py's seed; step i of the timed pass draws chains [i * Nout, (i + 1) * Nout) of its stream)
    kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Nout, Niter=Niter, seed=20260101, sample_offset=(W + K - 1) * Nout,
                                   precision=prec)
    torch.cuda.synchronize()
    assert np.array_equal(runs[0]["points"], P.cpu().numpy().reshape(Nout, D).T)
    assert np.array_equal(runs[0]["labels"], I.cpu().numpy().reshape(Nout, M).T)
    for x in dd:
        x.close()


def test_bench_distributed_path_one_rank():
    d = _run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
             env={"KDEHIP_FORCE_DIST": "1", "MASTER_PORT": "29533"})
    assert d["n_gpus"] == 1 and d["value"] > 0
    d = _run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--strong", "--config", "c4"])
    assert d["scaling"] == "strong" and d["config"]["nout_total"] == 16384   # config 4 as BASELINE.json states it
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
              "--master-addr", "127.0.0.1", "--master-port", "29534", "bench.py", "--gpus", "1", "--steps", "2",
              "--warmup", "1", "--no-cpu-baseline"])
    assert d["n_gpus"] == 1 and d["value"] > 0


def test_bench_frow_lines_and_batched_star():
    """The callers either side of the product at the measurement bar (`--frow`): each line carries `roofline`
    with a kernel time measured INSIDE the library (kdehip_profile_phase_read) and `cpu_baseline`; and `--batch B --mul`
    (many `*` in one call) reports its parity with the single calls."""
    d = _run([sys.executable, "bench.py", "--frow", "loocv", "--nout", "512", "--steps", "3", "--warmup", "1"])
    assert REQUIRED <= set(d) and d["cpu_baseline"]["kind"] == "port"
    r = d["roofline"]
    assert 0.0 < r["kernel_ms"] < d["ms_per_step"] * 1.05 and 0.0 < r["frac"] < 1.0
    assert d["parity"]["bandwidths_equal_oracle_1e-9"] and d["parity"]["evaluation_counts_equal"]
    d = _run([sys.executable, "bench.py", "--frow", "evaluate", "--config", "c2", "--steps", "3", "--warmup", "1"])
    assert REQUIRED <= set(d) and d["parity"]["max_rel_err_vs_oracle"] < 1e-11
    assert 0.0 < d["roofline"]["kernel_ms"] < d["ms_per_step"]
    d = _run([sys.executable, "bench.py", "--frow", "tree", "--nout", "512", "--steps", "3", "--warmup", "1"])
    assert REQUIRED <= set(d) and d["gpu_builder"]["arrays_identical_to_host_builder"]
    d = _run([sys.executable, "bench.py", "--config", "c2", "--batch", "6", "--mul", "--steps", "3", "--warmup", "1"])
    assert d["batched_equals_single_calls_bit_for_bit"] and d["config"]["batch"] == 6
    assert d["ms_per_step"] < d["back_to_back"]["ms_per_step"]
