// expdd.hpp -- exp(x) for -2000 <= x <= 0 in double-double, the reference that fastexp.hpp's two functions are measured
// against on the device (selftest.hip kdehip_selftest_exp64) and that tests/test_expdd.py holds to a relative error of 2^-80
// against mpmath on the host.  It shares nothing with the code under test: ln2 is split in three parts of 40 + 53 + 53 bits,
// the reduction is to |r| <= ln2/2 with no table, the series of expm1(r / 256) is formed by repeated division (no
// coefficients) and is doubled eight times as expm1(2t) = expm1(t) (2 + expm1(t)).
// Plain IEEE arithmetic only: compile with -ffp-contract=off (the products and sums below must round where they are written).
#pragma once
#include <cmath>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KDEHIP_DD_HD __host__ __device__ inline
#else
#define KDEHIP_DD_HD inline
#endif

namespace kdehip {

struct DD { double hi, lo; };  // the value hi + lo, |lo| <= ulp(hi) / 2

KDEHIP_DD_HD DD dd_two_sum(double a, double b) {  // a + b exactly
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
KDEHIP_DD_HD DD dd_quick_sum(double a, double b) {  // a + b exactly, |a| >= |b|
  const double s = a + b;
  return {s, b - (s - a)};
}
KDEHIP_DD_HD DD dd_two_prod(double a, double b) {  // a * b exactly
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
KDEHIP_DD_HD DD dd_add(DD a, DD b) {
  DD s = dd_two_sum(a.hi, b.hi);
  const DD t = dd_two_sum(a.lo, b.lo);
  s = dd_quick_sum(s.hi, s.lo + t.hi);
  return dd_quick_sum(s.hi, s.lo + t.lo);
}
KDEHIP_DD_HD DD dd_mul(DD a, DD b) {
  const DD p = dd_two_prod(a.hi, b.hi);
  return dd_quick_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
KDEHIP_DD_HD DD dd_div(DD a, double n) {  // three quotient digits
  const double q1 = a.hi / n;
  DD p = dd_two_prod(q1, n);
  DD r = dd_add(a, {-p.hi, -p.lo});
  const double q2 = r.hi / n;
  p = dd_two_prod(q2, n);
  r = dd_add(r, {-p.hi, -p.lo});
  const double q3 = r.hi / n;
  const DD q = dd_quick_sum(q1, q2);
  return dd_quick_sum(q.hi, q.lo + q3);
}

// exp(x) = (hi + lo) * 2^k with hi + lo in [2^-1/2, 2^1/2] (up to the rounding of k): unscaled, so that the relative accuracy
// holds where exp(x) itself is subnormal or 0 in fp64
struct ExpDD { double hi, lo; int k; };

KDEHIP_DD_HD ExpDD exp_dd(double x) {
  constexpr double kLn2a = 0x1.62e42fefa2000p-1;    // ln2, the leading 40 bits: kf * kLn2a is exact for |kf| < 2^12
  constexpr double kLn2b = 0x1.9ef35793c7673p-41;   // the next 53
  constexpr double kLn2c = 0x1.f97b57a079a19p-103;  // and the next: together ln2 (1 + 7e-48)
  const double kf = rint(x * 0x1.71547652b82fep+0);
  // r = x - kf ln2: the first difference and the product kf * kLn2b are formed exactly
  DD r = dd_two_sum(x, -(kf * kLn2a));
  const DD m = dd_two_prod(kf, kLn2b);
  r = dd_add(r, {-m.hi, -m.lo});
  r = dd_add(r, {-(kf * kLn2c), 0.0});
  const DD t = {r.hi * 0x1p-8, r.lo * 0x1p-8};  // |t| <= ln2 / 512: the term t^11 / 11! left out is below 2^-120 |t|
  DD term = t, sum = t;
  for (int n = 2; n <= 10; ++n) {
    term = dd_div(dd_mul(term, t), static_cast<double>(n));
    sum = dd_add(sum, term);
  }
  for (int s = 0; s < 8; ++s) sum = dd_mul(sum, dd_add({2.0, 0.0}, sum));  // expm1 of twice the argument
  const DD y = dd_add({1.0, 0.0}, sum);
  return {y.hi, y.lo, static_cast<int>(kf)};
}

}  // namespace kdehip
