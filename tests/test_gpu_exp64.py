"""The premise of every fp64 density kernel, measured: csrc/fastexp.hpp's exp_nonpos (32-entry table, degree 6) and
exp256_nonpos (256-entry table, degree 4) against the double-double exp of csrc/expdd.hpp (relative error <= 2^-80,
tests/test_expdd.py), on the device, over inputs generated there (csrc/selftest.hip kdehip_selftest_exp64; the families are
described in include/kdehip.h).  Every GPU test file holds its kernel to 1e-12 "because exp is ~1 ulp"; that bound cannot see
a 50-ulp defect at a reduction boundary, in the subnormal zone or at the clamp.  This file can.

The unit is |got - ref| / ulp(ref), ulp(ref) = 2^(e-52) for 2^e <= ref < 2^(e+1), floored at 2^-1074.

THE BOUND, derived from the algorithm (nothing below is taken from a measurement).  Both functions write
x = (T k + j) c + r, c = ln2 / T (T = 32 or 256 table entries), and return 2^k fl(t + t p): t the table's 2^(j/T), p the
polynomial for e^r - 1 of degree n (6 or 4).  With u = 2^-53, rmax = ln2 / (2 T) (1 + 2^-30) (the product x / c is rounded
before it is rounded to an integer, which can carry r past ln2 / (2 T) by a relative 2^-33 at most) and y = 2^(j/T) e^r the
exact result without its power of two:
  * j >= 1: y lies in [2^(1/(2T)), 2^(1 - 1/(2T))], inside [1, 2): ulp(y) = 2 u and a relative error rho costs rho y / (2 u)
    < rho / u ulp.  j = 0: t = 1 exactly and y may lie below 1, where ulp(y) = u and again rho y / u < rho / u.
  * final     the one rounding of the fma t + t p: 1/2 ulp.  (If y < 1 <= the unrounded value, the fma returns 1 or more and
              is no further from y than the unrounded value was.)
  * table     t is 2^(j/T) correctly rounded in [1, 2): off by u at most; times e^r <= 2^(1/(2T)); in ulp(y) = 2 u:
              1/2 * 2^(1/(2T)).   (j = 0 has none.)
  * series    the terms left out, sum_{m > n} r^m / m! <= rmax^(n+1) / (n+1)! / (1 - rmax / (n+2)), relative to e^r >=
              e^-rmax, times 1 / u.
  * Horner    p = fl(q r), q = fl(1 + r (..)) in [0.98, 1.02]: u for the product, u for q's last fma, and the earlier fmas and
              the rounded coefficients, each below u and entering times r or less: (2 + 4 rmax) u relative to |p| <=
              e^rmax - 1; relative to e^r and in ulp: (2 + 4 rmax) (e^rmax - 1) e^rmax.
  * reduction r = fma(k', -c_lo, fma(k', -c_hi, x)), k' = T k + j: c_hi holds 32 bits and k' < 2^19, so k' c_hi is exact and
              the inner fma's result, a multiple of ulp(x) >= 2^-62 below 2^-6, is exact too; the outer fma rounds once, by
              half an ulp of r (2^-60 for T = 32, 2^-63 for T = 256), and c_lo is off by u |c_lo| <= u c 2^-32, times k':
              u 2^-32 |x|.  An error dr of r is a relative error dr of e^r: (2^(floor(log2 rmax) - 53) + u 2^-32 xmax) / u.
  normal results:     exp_nonpos    0.5 + 0.5054 + 0.0316 + 0.0225 + 0.0078 = 1.0674 ulp
                      exp256_nonpos 0.5 + 0.5007 + 0.3419 + 0.0027 + 0.0010 = 1.3463 ulp
  subnormal results:  the value before ldexp is within B ulp of ITS OWN precision, which below 2^-1022 is at most half a
                      spacing of the subnormal grid; ldexp then rounds once more, by half a spacing: B / 2 + 1/2, that is
                      1.0337 and 1.1731 spacings.  (The same holds for results that round to 0.)
  near zero (|x| <= 2^-30): k' = 0, r = x, j = 0: no table and no reduction error, the series ends below 2^-200, Horner's
                      error is (2 + 4 |x|) u |x|: 1/2 + 2^-28 ulp; for |x| < 2^-54 the result is 1.0 exactly.
The figures are computed below from these formulas (BOUND), not typed in.

Each sweep's worst input is evaluated again on the host with mpmath at 200 bits: the error recomputed there must equal the
device's figure to 1e-3, which ties the device's measurement to an independent reference at the point that decides it.

NaN: both functions begin with fmax(x, clamp), which returns the clamp for a NaN: they return +0.  That is pinned here as it
is (fastexp.hpp says so; the entries that take positions from a caller answer NaN on their own, tests/test_gpu_nonfinite.py)."""
import ctypes as C
import math
import struct
from fractions import Fraction

import mpmath as mp
import pytest

import kdehip
from kdehip import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAMES = ["exp_nonpos", "exp256_nonpos"]
DENSE, HALF, WHOLE, SUBNORMAL, ZERO, NEAR0, RAW = range(7)
FAMILY = ["dense", "half-way", "whole", "subnormal", "zero", "near zero", "raw"]
ONE = 0x3FF0000000000000


def _bound(which):
    """(normal, subnormal) from the derivation in the module's docstring"""
    T, n, xmax = (32, 6, 800.0) if which == 0 else (256, 4, 1000.0)
    rmax = math.log(2.0) / (2 * T) * (1.0 + 2.0 ** -30)
    final = 0.5
    table = 0.5 * 2.0 ** (1.0 / (2 * T))
    series = rmax ** (n + 1) / math.factorial(n + 1) / (1.0 - rmax / (n + 2)) * math.exp(rmax) / U
    horner = (2.0 + 4.0 * rmax) * math.expm1(rmax) * math.exp(rmax)
    reduction = (2.0 ** (math.floor(math.log2(rmax)) - 53) + U * 2.0 ** -32 * xmax) / U
    normal = final + table + series + horner + reduction
    return normal, 0.5 * normal + 0.5


BOUND = [_bound(0), _bound(1)]
NEAR0_BOUND = 0.5 + 2.0 ** -28


def test_the_derived_bounds_are_what_the_docstring_states():
    assert [round(b, 4) for b in BOUND[0]] == [1.0674, 1.0337] and [round(b, 4) for b in BOUND[1]] == [1.3463, 1.1731]
    assert BOUND[0][0] < 1.5


# ---- the map from (function, family, index) to an input, repeated from csrc/selftest.hip exp64_input --------------------------
M64 = (1 << 64) - 1


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _mix(i):
    z = (i + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (a Fraction becomes the nearest double: one rounding)


def family_size(which, family):
    return [(0xC0862000 - 0xBE100000 + 1) * 16, (369330 if which else 36933) * 129, (369329 if which else 36932) * 129,
            (1 << 26) + 1, (1 << 24) + 1, 994 * 8][family]


def exp64_input(which, family, i):
    if family == DENSE:
        j = i & 15
        low = 0 if j == 0 else 0xFFFFFFFF if j == 1 else _mix(i) & 0xFFFFFFFF
        return ((0xBE100000 + (i >> 4)) << 32) | low
    if family in (HALF, WHOLE):
        sc = 2.0 ** -8 if which else 2.0 ** -5
        chi, clo = float.fromhex("0x1.62e42fefa39efp-1") * sc, float.fromhex("0x1.abc9e3b39803fp-56") * sc
        n, off = divmod(i, 129)
        m = float(n) + (0.5 if family == HALF else 1.0)
        p = m * chi
        e = _fma(m, chi, -p)
        return (_bits(-(p + (e + m * clo))) + off - 64) & M64
    if family in (SUBNORMAL, ZERO):
        b0 = _bits(-708.3) if family == SUBNORMAL else _bits(-745.2)
        b1 = _bits(-745.2) if family == SUBNORMAL else _bits(-1000.0 if which else -800.0)
        lg = 26 if family == SUBNORMAL else 24
        if i >> lg:
            return b1
        step = (b1 - b0) >> lg
        return b0 + i * step + (_mix(i) % step if i else 0)
    if family == NEAR0:
        e, j, full = 993 - i // 8, i % 8, (1 << 52) - 1
        man = 0 if j == 0 else full if j == 1 else _mix(i) & full
        return (1 << 63) | (e << 52) | man
    return i


def _sweep(which, family, first, count):
    """(largest error, the worst input's bits, the device's result bits for it); the two forms of the function -- its
    _begin / _end halves and the one call -- must have agreed in every bit of every input"""
    err, wb, wr, mism = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib.kdehip_selftest_exp64(which, family, first, count, 0, C.byref(err), C.byref(wb), C.byref(wr),
                                              C.byref(mism)))
    assert mism.value == 0, f"{NAMES[which]}: the split and the one-call form differ at {mism.value} inputs"
    return err.value, wb.value, wr.value


def _probe(which, x_bits):
    """the device's result bits for ONE input (and the error it reports)"""
    err, wb, wr = _sweep(which, RAW, x_bits, 1)
    assert wb == x_bits
    return wr, err


def _host_error(x_bits, got_bits):
    """the sweep's unit for one (input, result), by mpmath at 200 bits"""
    with mp.workprec(200):
        ref = mp.exp(mp.mpf(_double(x_bits)))
        e = mp.frexp(ref)[1] - 1  # 2^e <= ref < 2^(e+1)
        ulp = mp.ldexp(mp.mpf(1), max(e, -1022) - 52)
        return float(abs(mp.mpf(_double(got_bits)) - ref) / ulp)


# ---- 1. the map is the device's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_the_index_to_input_map_is_the_devices(which):
    for family in range(RAW):
        size = family_size(which, family)
        for i in sorted({0, 1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 130, size // 3, size // 2 + 1, size - 2, size - 1}
                        | {_mix(1000 * family + k) % size for k in range(6)}):
            _, wb, _ = _sweep(which, family, i, 1)
            assert wb == exp64_input(which, family, i), (FAMILY[family], i, hex(wb))
        err, wb, wr, mism = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = _lib.lib.kdehip_selftest_exp64(which, family, size - 1, 2, 0, C.byref(err), C.byref(wb), C.byref(wr), C.byref(mism))
        assert rc == _lib.ERR_ARG  # (past the family's end)
    # the ends of the zones are where the header says
    assert _double(exp64_input(which, DENSE, 0)) == -2.0 ** -30
    assert _double(exp64_input(which, DENSE, family_size(which, DENSE) - 16)) == -708.0
    assert _double(exp64_input(which, SUBNORMAL, 0)) == -708.3 and _double(exp64_input(which, SUBNORMAL, 1 << 26)) == -745.2
    assert _double(exp64_input(which, ZERO, 0)) == -745.2 and _double(exp64_input(which, ZERO, 1 << 24)) == (-1000.0 if which else -800.0)
    c = math.log(2.0) / (256 if which else 32)
    n = family_size(which, HALF) // 129 - 1
    assert abs(_double(exp64_input(which, HALF, n * 129 + 64)) + (n + 0.5) * c) < 1e-12 and (n + 1.5) * c > (1000.0 if which else 800.0)
    assert _double(exp64_input(which, NEAR0, 0)) == -2.0 ** -30 and exp64_input(which, NEAR0, 994 * 8 - 8) == 1 << 63
    assert exp64_input(which, NEAR0, 994 * 8 - 7) == (1 << 63) | ((1 << 52) - 1)  # the largest subnormal


# ---- 2. the sweeps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [DENSE, HALF, WHOLE, SUBNORMAL, ZERO, NEAR0])
@pytest.mark.parametrize("which", [0, 1])
def test_the_measured_error_is_within_the_derived_bound(which, family):
    size = family_size(which, family)
    err, wb, wr = _sweep(which, family, 0, size)
    # families whose results are all subnormal or 0 take the subnormal figure; the others hold results of every kind and the
    # normal figure, which is the larger one
    bound = BOUND[which][1] if family in (SUBNORMAL, ZERO) else NEAR0_BOUND if family == NEAR0 else BOUND[which][0]
    host = _host_error(wb, wr)
    print(f"{NAMES[which]} {FAMILY[family]}: {size} inputs, max error {err:.4f} (bound {bound:.4f}) at x = {_double(wb).hex()} "
          f"= {_double(wb)!r}, device result {_double(wr).hex()}; mpmath says {host:.4f}")
    assert err <= bound, (NAMES[which], FAMILY[family], err, bound, hex(wb), hex(wr))
    assert abs(host - err) <= 1e-3, (NAMES[which], FAMILY[family], err, host, hex(wb), hex(wr))


# ---- 3. zero results and the clamp -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_results_beyond_the_clamp_are_plus_zero(which):
    clamp = -1000.0 if which else -800.0
    places = [_bits(clamp)]
    if which:  # where 256 k + j would leave 32 bits, and its sign bit, if the clamp did not hold
        places += [_bits(-(2.0 ** 31) * math.log(2.0) / 256), _bits(-(2.0 ** 32) * math.log(2.0) / 256), _bits(-(2.0 ** 31 + 128) * math.log(2.0) / 256)]
    else:      # where 32 k + j would leave 32 bits
        places += [_bits(-(2.0 ** 31) * math.log(2.0) / 32), _bits(-(2.0 ** 32) * math.log(2.0) / 32)]
    for b in places:
        err, wb, wr = _sweep(which, RAW, b - 64, 129)
        assert err < 2.0 ** -60 and wr == 0, (hex(b), err, hex(wb), hex(wr))  # every one within 2^-60 spacings of 0, that is 0
        for nb in (b - 64, b - 1, b, b + 1, b + 64):
            assert _probe(which, nb)[0] == 0, hex(nb)                        # and +0, not -0
    for x in (-1e300, -1.7976931348623157e308, -math.inf, -5000.0):
        assert _probe(which, _bits(x)) == (0, 0.0), x


# ---- 4. near zero ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_arguments_below_2_to_the_minus_54_give_exactly_one(which):
    for b in (0, 1 << 63, _bits(-2.0 ** -1074), _bits(-2.0 ** -1022), _bits(-2.0 ** -100), _bits(-2.0 ** -55), _bits(-2.0 ** -54) - 1):
        assert _probe(which, b)[0] == ONE, hex(b)
    assert _probe(which, 0) == (ONE, 0.0) and _probe(which, 1 << 63) == (ONE, 0.0)
    assert _probe(which, _bits(-2.0 ** -54))[0] == ONE       # the tie goes to the even neighbour: half an ulp off
    assert _probe(which, _bits(-2.0 ** -54) + 1)[0] == ONE - 1  # the first argument that leaves 1.0


# ---- 5. NaN ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_a_nan_argument_gives_plus_zero_as_fastexp_hpp_says(which):
    """fmax(NaN, clamp) = clamp, so exp(clamp) = +0 comes back -- NOT NaN.  Pinned as it is: the clamp is one instruction on
    the sampler's hottest path and nobody has measured a select in its place.  The sweep's unit counts a NaN argument as
    unbounded (2^60), whatever came back."""
    for b in (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF800000000BEEF, 0x7FFFFFFFFFFFFFFF, 0xFFFC0DE000000000):
        assert _double(b) != _double(b)
        assert _probe(which, b) == (0, 2.0 ** 60), hex(b)
