// selftest.hip -- measures, on the device it runs on, the accuracy of the three hardware fp32 approximations the fp32
// screen's error bound takes as a premise (screen_device.hpp: v_rcp_f32, v_rsq_f32 and v_exp_f32 "within 1 ulp", i.e. a
// relative error of at most 2 u, u = 2^-24).  The reference has no counterpart (src/MSGibbs01.jl:250-351 is fp64 only):
// this is what turns the premise from documentation into a measurement -- tests/test_gpu_ulp.py sweeps every fp32 input
// of the ranges the screen can feed the instructions and asserts the budget.
// Likewise for the premise of every fp64 density kernel, fastexp.hpp's exp_nonpos and exp256_nonpos "~1 ulp": measured
// against the double-double exp of expdd.hpp over generated inputs (kdehip_selftest_exp64, tests/test_gpu_exp64.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "expdd.hpp"
#include "fastexp.hpp"
#include "kdehip_internal.hpp"

namespace kdehip {
namespace {

// hardware result for input bit pattern `b` (the builtins the screen's evaluators use: gibbs_device.hpp Num<float>,
// gibbs_lean.hip step_screen)
template <int WHICH>
__device__ __forceinline__ float hw(float x) {
  if constexpr (WHICH == 0) return __builtin_amdgcn_rcpf(x);
  else if constexpr (WHICH == 1) return __builtin_amdgcn_rsqf(x);
  else return __builtin_amdgcn_exp2f(x);
}
// the error of one input: relative, in units of u (WHICH 0..2); WHICH 3: |result - 2^x| in units of 2^-126 (the zone where
// the exact value is below the smallest normal: the bound only needs "what fp32 flushes or holds as a denormal is off by
// less than 2^-126")
template <int WHICH>
__device__ __forceinline__ float err_of(uint32_t bits) {
  const float x = __uint_as_float(bits);
  const double xd = static_cast<double>(x);
  double ref;
  if constexpr (WHICH == 0) ref = 1.0 / xd;
  else if constexpr (WHICH == 1) ref = 1.0 / sqrt(xd);
  else ref = exp2(xd);
  const double r = static_cast<double>(hw<(WHICH == 3 ? 2 : WHICH)>(x));
  double e;
  if constexpr (WHICH == 3) e = fabs(r - ref) * 0x1p126;
  else e = fabs(r - ref) / fabs(ref) * 0x1p24;
  if (!(e == e)) e = 0x1p60;  // a NaN where a number was due is an unbounded error
  return static_cast<float>(e);
}

template <int WHICH>
__global__ __launch_bounds__(256) void ulp_sweep_kernel(uint32_t first, uint64_t count, unsigned long long *best) {
  unsigned long long key = 0ull;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < count; i += 256ull * gridDim.x) {
    const uint32_t b = first + static_cast<uint32_t>(i);
    const float e = err_of<WHICH>(b);
    const unsigned long long k = (static_cast<unsigned long long>(__float_as_uint(e)) << 32) | b;  // (e >= 0: bits are monotone)
    key = k > key ? k : key;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(key, s);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(best, key);
}
template <int WHICH>
__global__ void ulp_one_kernel(uint32_t bits, uint32_t *out) {
  out[0] = __float_as_uint(hw<(WHICH == 3 ? 2 : WHICH)>(__uint_as_float(bits)));
}

template <int WHICH>
hipError_t run(uint32_t first, uint64_t count, unsigned long long *d_best, uint32_t *d_res, unsigned long long *h_best,
               uint32_t *h_res) {
  hipError_t e = hipMemsetAsync(d_best, 0, sizeof(unsigned long long), nullptr);
  if (e != hipSuccess) return e;
  const int blocks = count < (1u << 20) ? 64 : 256 * 8;
  ulp_sweep_kernel<WHICH><<<blocks, 256, 0, nullptr>>>(first, count, d_best);
  e = hipMemcpy(h_best, d_best, sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  ulp_one_kernel<WHICH><<<1, 1, 0, nullptr>>>(static_cast<uint32_t>(*h_best & 0xffffffffull), d_res);
  return hipMemcpy(h_res, d_res, sizeof(uint32_t), hipMemcpyDeviceToHost);
}

}  // namespace
}  // namespace kdehip

extern "C" int kdehip_selftest_fp32(int which, uint32_t first_bits, uint64_t count, int device, double *max_err,
                                    uint32_t *worst_bits, uint32_t *worst_result_bits) {
  using namespace kdehip;
  if (which < 0 || which > 3 || count == 0 || count > (1ull << 32) || !max_err)
    return set_error(KDEHIP_ERR_ARG, "kdehip_selftest_fp32: which in 0..3, 1 <= count <= 2^32, max_err required");
  DeviceGuard guard;
  if (int rc = guard.enter(device)) return rc;
  void *blk = nullptr;
  hipError_t e = cached_malloc(&blk, 64);
  if (e != hipSuccess) return set_error(KDEHIP_ERR_ALLOC, std::string("kdehip_selftest_fp32: ") + hipGetErrorString(e));
  auto *d_best = static_cast<unsigned long long *>(blk);
  auto *d_res = reinterpret_cast<uint32_t *>(d_best + 1);
  unsigned long long best = 0;
  uint32_t res = 0;
  switch (which) {
    case 0: e = run<0>(first_bits, count, d_best, d_res, &best, &res); break;
    case 1: e = run<1>(first_bits, count, d_best, d_res, &best, &res); break;
    case 2: e = run<2>(first_bits, count, d_best, d_res, &best, &res); break;
    default: e = run<3>(first_bits, count, d_best, d_res, &best, &res); break;
  }
  cached_free(blk, 64);
  if (e != hipSuccess) return set_error(KDEHIP_ERR_HIP, std::string("kdehip_selftest_fp32: ") + hipGetErrorString(e));
  const uint32_t ebits = static_cast<uint32_t>(best >> 32);
  float ef;
  __builtin_memcpy(&ef, &ebits, sizeof ef);
  *max_err = static_cast<double>(ef);
  if (worst_bits) *worst_bits = static_cast<uint32_t>(best & 0xffffffffull);
  if (worst_result_bits) *worst_result_bits = res;
  return KDEHIP_OK;
}

// ---- the fp64 exponentials -------------------------------------------------------------------------------------------------
namespace kdehip {

__host__ __device__ inline uint64_t exp64_mix(uint64_t i) {  // splitmix64's finaliser of i + its increment
  uint64_t z = i + 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

constexpr uint64_t kExp64DenseFirst = 0xBE100000ull, kExp64DenseLast = 0xC0862000ull;  // upper words of -2^-30 and -708.0
constexpr uint64_t kBitsM708_3 = 0xC086226666666666ull, kBitsM745_2 = 0xC08749999999999Aull;  // -708.3, -745.2
constexpr uint64_t kBitsM800 = 0xC089000000000000ull, kBitsM1000 = 0xC08F400000000000ull;

// the number of inputs of a family (include/kdehip.h); 0: no such family
__host__ __device__ inline uint64_t exp64_family_size(int which, int family) {
  switch (family) {
    case 0: return (kExp64DenseLast - kExp64DenseFirst + 1) * 16;
    case 1: return (which ? 369330ull : 36933ull) * 129;  // (n + 1/2) c <= 1000 (800), n from 0
    case 2: return (which ? 369329ull : 36932ull) * 129;  // (n + 1) c   <= 1000 (800)
    case 3: return (1ull << 26) + 1;
    case 4: return (1ull << 24) + 1;
    case 5: return 994ull * 8;
    case 6: return ~0ull;
    default: return 0;
  }
}

// THE map from (function, family, index) to the 64 bits of an input: a pure function (tests/test_gpu_exp64.py repeats it)
__host__ __device__ inline uint64_t exp64_input(int which, int family, uint64_t i) {
  switch (family) {
    case 0: {
      const uint64_t j = i & 15;
      const uint64_t low = j == 0 ? 0ull : j == 1 ? 0xFFFFFFFFull : (exp64_mix(i) & 0xFFFFFFFFull);
      return ((kExp64DenseFirst + (i >> 4)) << 32) | low;
    }
    case 1:
    case 2: {
      // ln2 = hi + lo to 107 bits; c = ln2/32 or ln2/256 (exact scalings); m c rounded once from the double-double product
      const double sc = which ? 0x1p-8 : 0x1p-5;
      const double chi = 0x1.62e42fefa39efp-1 * sc, clo = 0x1.abc9e3b39803fp-56 * sc;
      const uint64_t n = i / 129;
      const int64_t off = static_cast<int64_t>(i % 129) - 64;
      const double m = static_cast<double>(n) + (family == 1 ? 0.5 : 1.0);
      const double p = m * chi, e = fma(m, chi, -p);
      const double x = -(p + (e + m * clo));
      uint64_t b;
      __builtin_memcpy(&b, &x, sizeof b);
      return b + static_cast<uint64_t>(off);  // (negative doubles: the next pattern is the next one away from 0)
    }
    case 3:
    case 4: {
      const uint64_t b0 = family == 3 ? kBitsM708_3 : kBitsM745_2;
      const uint64_t b1 = family == 3 ? kBitsM745_2 : (which ? kBitsM1000 : kBitsM800);
      const int lg = family == 3 ? 26 : 24;
      if (i >> lg) return b1;
      const uint64_t step = (b1 - b0) >> lg;
      return b0 + i * step + (i ? exp64_mix(i) % step : 0ull);
    }
    case 5: {
      const uint64_t e = 993 - i / 8, j = i % 8, full = (1ull << 52) - 1;
      const uint64_t man = j == 0 ? 0ull : j == 1 ? full : (exp64_mix(i) & full);
      return (1ull << 63) | (e << 52) | man;
    }
    default: return i;
  }
}

// |got - exp(x)| / ulp(exp(x)), include/kdehip.h's unit; a NaN on either side (or x > 0): 2^60
__host__ __device__ inline double exp64_err(double x, double got) {
  if (!(x <= 0.0) || !(got == got)) return 0x1p60;
  if (x < -770.0) return ldexp(fabs(got), 1074);  // exp(x) < 2^-1110: the reference is 0 to 2^-36 of a spacing
  const ExpDD r = exp_dd(x);
  const int es = (r.hi < 1.0 || (r.hi == 1.0 && r.lo < 0.0)) ? -1 : 0;  // 2^es <= hi + lo < 2^(es+1)
  int ex = es + r.k;
  if (ex < -1022) ex = -1022;
  const double diff = (ldexp(got, -r.k) - r.hi) - r.lo;  // the scaling and the first difference are exact
  return fabs(diff) * ldexp(1.0, 52 - ex + r.k);
}

namespace {

struct Exp64Rec { double err; uint64_t idx, res, pad; };

template <int WHICH>
__device__ __forceinline__ double exp64_both(double x, const double *tab, bool &same) {
  double split, one;
  if constexpr (WHICH == 0) {
    const ExpSplit s = exp_nonpos_begin(x, tab);  // the halves, as the sampler calls them
    split = exp_nonpos_end(s);
    one = exp_nonpos(x, tab);
  } else {
    const ExpSplit256 s = exp256_nonpos_begin(x, tab);
    split = exp256_nonpos_end(s);
    one = exp256_nonpos(x, tab);
  }
  same = __double_as_longlong(split) == __double_as_longlong(one);
  return split;
}

template <int WHICH>
__global__ __launch_bounds__(256) void exp64_sweep_kernel(int family, uint64_t first, uint64_t count, Exp64Rec *recs,
                                                          unsigned long long *mismatches) {
  constexpr int kTab = WHICH ? 256 : 32;
  __shared__ double sExpTab[kTab];
  if (threadIdx.x < kTab) sExpTab[threadIdx.x] = WHICH ? kExp2Tab256[threadIdx.x] : kExp2Tab[threadIdx.x];
  __syncthreads();
  double best = -1.0;
  uint64_t bidx = 0, bres = 0;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < count; i += 256ull * gridDim.x) {
    const uint64_t bits = exp64_input(WHICH, family, first + i);
    const double x = __longlong_as_double(static_cast<long long>(bits));
    bool same;
    const double got = exp64_both<WHICH>(x, sExpTab, same);
    if (!same) atomicAdd(mismatches, 1ull);
    const double e = exp64_err(x, got);
    if (e > best) {  // (ascending i: the first of equals stays)
      best = e;
      bidx = first + i;
      bres = static_cast<uint64_t>(__double_as_longlong(got));
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double oe = __shfl_xor(best, s);
    const unsigned long long oi = __shfl_xor(static_cast<unsigned long long>(bidx), s);
    const unsigned long long orr = __shfl_xor(static_cast<unsigned long long>(bres), s);
    if (oe > best || (oe == best && oi < bidx)) {
      best = oe;
      bidx = oi;
      bres = orr;
    }
  }
  if ((threadIdx.x & 63) == 0) recs[blockIdx.x * 4 + (threadIdx.x >> 6)] = Exp64Rec{best, bidx, bres, 0};
}

}  // namespace
}  // namespace kdehip

extern "C" int kdehip_selftest_exp64(int which, int family, uint64_t first, uint64_t count, int device, double *max_err,
                                     uint64_t *worst_bits, uint64_t *worst_result_bits, uint64_t *form_mismatches) {
  using namespace kdehip;
  const uint64_t size = (which == 0 || which == 1) ? exp64_family_size(which, family) : 0;
  if (size == 0 || count == 0 || count > (1ull << 40) || first > size - 1 || count - 1 > size - 1 - first || !max_err)
    return set_error(KDEHIP_ERR_ARG, "kdehip_selftest_exp64: which in 0..1, family in 0..6, the inputs [first, first + count) "
                                     "inside the family, 1 <= count <= 2^40, max_err required");
  DeviceGuard guard;
  if (int rc = guard.enter(device)) return rc;
  const int blocks = count < (1u << 20) ? 64 : 256 * 8;
  const size_t nrec = static_cast<size_t>(blocks) * 4, bytes = sizeof(Exp64Rec) * nrec + 64;
  void *blk = nullptr;
  hipError_t e = cached_malloc(&blk, bytes);
  if (e != hipSuccess) return set_error(KDEHIP_ERR_ALLOC, std::string("kdehip_selftest_exp64: ") + hipGetErrorString(e));
  auto *d_recs = static_cast<Exp64Rec *>(blk);
  auto *d_mism = reinterpret_cast<unsigned long long *>(d_recs + nrec);
  std::vector<Exp64Rec> recs;
  unsigned long long mism = 0;
  try {
    recs.resize(nrec);
  } catch (const std::exception &) {
    cached_free(blk, bytes);
    return set_error(KDEHIP_ERR_ALLOC, "kdehip_selftest_exp64: out of host memory");
  }
  e = hipMemsetAsync(d_mism, 0, sizeof(unsigned long long), nullptr);
  if (e == hipSuccess) {
    if (which == 0) exp64_sweep_kernel<0><<<blocks, 256, 0, nullptr>>>(family, first, count, d_recs, d_mism);
    else exp64_sweep_kernel<1><<<blocks, 256, 0, nullptr>>>(family, first, count, d_recs, d_mism);
    e = hipMemcpy(recs.data(), d_recs, sizeof(Exp64Rec) * nrec, hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess) e = hipMemcpy(&mism, d_mism, sizeof mism, hipMemcpyDeviceToHost);
  cached_free(blk, bytes);
  if (e != hipSuccess) return set_error(KDEHIP_ERR_HIP, std::string("kdehip_selftest_exp64: ") + hipGetErrorString(e));
  const Exp64Rec *w = nullptr;
  for (const Exp64Rec &r : recs)
    if (r.err >= 0.0 && (!w || r.err > w->err || (r.err == w->err && r.idx < w->idx))) w = &r;
  if (!w) return set_error(KDEHIP_ERR_HIP, "kdehip_selftest_exp64: the sweep returned nothing");
  *max_err = w->err;
  if (worst_bits) *worst_bits = exp64_input(which, family, w->idx);
  if (worst_result_bits) *worst_result_bits = w->res;
  if (form_mismatches) *form_mismatches = mism;
  return KDEHIP_OK;
}
