// circ_wrap.hpp -- the circular (2 pi) member of the enumerated manifolds (include/kdehip.h "manifolds"; no reference
// counterpart -- the reference takes its operators as callbacks, src/MSGibbs01.jl:650-653): wrap to [-pi, pi).  ONE
// expression for the sampler (gibbs_device.hpp) and for evaluation, log-likelihood and the bandwidth search (evaluate.hip):
// same expression, same constants as oracle/kde_oracle.c circ_wrap (fp64: bit for bit).  Tree construction on a manifold
// (treebuild.hip on the device, balltree.cpp on the host -- a plain C++ translation unit, hence the macro) uses it too.
#pragma once
#include <cmath>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KDEHIP_CIRC_HD __host__ __device__
#else
#define KDEHIP_CIRC_HD
#endif

namespace kdehip {

template <typename T>
KDEHIP_CIRC_HD inline __attribute__((always_inline)) T circ_wrap(T t) {
  constexpr double kTwoPi = 6.283185307179586476925286766559, kPi = 3.141592653589793238462643383279;
  return t - T(kTwoPi) * std::floor((t + T(kPi)) / T(kTwoPi));
}

}  // namespace kdehip
