// Prints "x hi lo k" (hexadecimal floats) of csrc/expdd.hpp's exp_dd for about 2e4 arguments; tests/test_expdd.py compares
// (hi + lo) 2^k with mpmath.  The arguments: random ones over [-745.2, -2^-60], uniform and log-uniform; n c and (n + 1/2) c
// for c = ln2/32 and ln2/256 (where the functions under test switch table entries), the ends of the sweep's zones, -0.0 and
// the tiny negatives.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "expdd.hpp"

static uint64_t state = 0x853c49e6748fea9bull;
static double unit() {  // splitmix64 -> [0, 1)
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return static_cast<double>(z >> 11) * 0x1p-53;
}

static void show(double x) {
  const kdehip::ExpDD e = kdehip::exp_dd(x);
  std::printf("%a %a %a %d\n", x, e.hi, e.lo, e.k);
}

int main() {
  const double lo = 0x1p-60, hi = 745.2;
  for (int i = 0; i < 8000; ++i) show(-(lo + (hi - lo) * unit()));
  for (int i = 0; i < 8000; ++i) show(-std::exp(std::log(lo) + (std::log(hi) - std::log(lo)) * unit()));
  const double ln2 = 0x1.62e42fefa39efp-1;
  for (int n = 0; n <= 34300; n += 86) {
    show(-(n * (ln2 / 32)));
    show(-((n + 0.5) * (ln2 / 32)));
    show(std::nextafter(-((n + 0.5) * (ln2 / 32)), 0.0));
    show(std::nextafter(-((n + 0.5) * (ln2 / 32)), -1e9));
  }
  for (int n = 0; n <= 275000; n += 688) {
    show(-(n * (ln2 / 256)));
    show(-((n + 0.5) * (ln2 / 256)));
  }
  for (int n = 0; n <= 1075; ++n) {  // where the reference's own reduction flips
    show(-((n + 0.5) * ln2));
    show(std::nextafter(-((n + 0.5) * ln2), 0.0));
  }
  const double ends[] = {-0.0, -0x1p-1074, -0x1p-1022, -0x1p-100, -0x1p-60, -0x1p-54, -0x1p-53, -0x1p-30, -0x1p-29, -1.0, -708.0,
                         -708.3, -708.396418532264, -744.44, -745.13, -745.2, -770.0, -800.0, -1000.0, -1999.0};
  for (double x : ends) {
    show(x);
    show(std::nextafter(x, 0.0));
    show(std::nextafter(x, -1e9));
  }
  return 0;
}
