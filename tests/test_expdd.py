"""The double-double exp that the fp64 fast exponentials are measured against on the device (csrc/expdd.hpp, used by
csrc/selftest.hip kdehip_selftest_exp64), held to its own accuracy on the host: a stand-alone program built from the header
prints exp_dd for about 2e4 arguments -- random ones over [-745.2, -2^-60], the table boundaries of the functions under
test, the reference's own reduction boundaries, the ends of the sweep's zones, -0.0 and the tiny negatives -- and every
(hi + lo) 2^k is compared with mpmath at 200 bits.  The bound is a relative error of 2^-80: at that accuracy the reference adds
less than 2^-27 ulp to any figure the sweep reports."""
import os
import shutil
import subprocess

import mpmath as mp
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2.0 ** -80


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_exp_dd_is_within_2_to_the_minus_80_of_mpmath(tmp_path):
    exe = str(tmp_path / "expdd_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "kerneldensityestimate.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "expdd_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) >= 20000
    worst, at = 0.0, None
    with mp.workprec(200):
        for line in lines:
            xs, his, los, ks = line.split()
            x, hi, lo, k = float.fromhex(xs), float.fromhex(his), float.fromhex(los), int(ks)
            assert 0.70 <= hi + lo <= 1.42, line  # unscaled: the accuracy holds where exp(x) is subnormal or 0 in fp64
            ref = mp.exp(mp.mpf(x))
            got = mp.ldexp(mp.mpf(hi) + mp.mpf(lo), k)
            err = float(abs(got - ref) / ref)
            if err > worst:
                worst, at = err, x
    print(f"exp_dd: {len(lines)} arguments, largest relative error {worst:.3e} (2^-80 = {BOUND:.3e}) at x = {at!r}")
    assert worst <= BOUND, (worst, at)
