// manifold_arg.hpp -- the ONE reading of a `manifold` / `tree_manifold` argument of the C ABI (include/kdehip.h "manifolds":
// NULL, or one byte per dimension, KDEHIP_MANIFOLD_EUCLIDEAN or KDEHIP_MANIFOLD_CIRCULAR), for every entry that takes one.
// What differs between entries is named in ManifoldRule; the loop over the bytes is here and nowhere else.  Host code only:
// no sampler translation unit includes it.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/kdehip.h"
#include "kdehip_internal.hpp"

namespace kdehip {

// What a non-NULL argument means when D lies outside 1..KDEHIP_MAX_DIMS:
enum class ManifoldDims {
  kDefer,        // nothing is read: the entry's own dimension check refuses D
  kUnsupported,  // KDEHIP_ERR_UNSUPPORTED (the product and `*` entries)
  kClamp,        // the first min(D, KDEHIP_MAX_DIMS) bytes are read; the entry's own check refuses D afterwards
  kUnbounded,    // all D bytes are read: the host tree builder has no dimension limit (mask: the first 32 dimensions)
};

struct ManifoldRule {
  const char *name = "manifold";              // the argument's name in the message
  ManifoldDims dims = ManifoldDims::kDefer;
  int precision = 64;                         // 32: a circular dimension is KDEHIP_ERR_UNSUPPORTED (the product entries)
};
constexpr ManifoldRule kTreeManifold{"tree_manifold", ManifoldDims::kClamp, 64};
constexpr ManifoldRule kHostTreeManifold{"tree_manifold", ManifoldDims::kUnbounded, 64};
inline ManifoldRule product_manifold(int precision) { return {"manifold", ManifoldDims::kUnsupported, precision}; }

// *mask (optional): bit k = dimension k is circular; 0 for NULL.  A byte other than 0 / 1 is KDEHIP_ERR_ARG.  Touches no device.
inline int manifold_arg(const uint8_t *arg, int64_t D, uint32_t *mask, const ManifoldRule &rule = {}) {
  if (mask) *mask = 0;
  if (!arg) return KDEHIP_OK;
  if (D < 1 || D > KDEHIP_MAX_DIMS) {
    if (rule.dims == ManifoldDims::kDefer) return KDEHIP_OK;
    if (rule.dims == ManifoldDims::kUnsupported) return set_error(KDEHIP_ERR_UNSUPPORTED, "ndims outside 1..KDEHIP_MAX_DIMS");
    if (rule.dims == ManifoldDims::kClamp && D > KDEHIP_MAX_DIMS) D = KDEHIP_MAX_DIMS;
  }
  uint32_t bits = 0;
  for (int64_t k = 0; k < D; ++k) {
    if (arg[k] == KDEHIP_MANIFOLD_CIRCULAR) bits |= k < 32 ? 1u << k : 0u;
    else if (arg[k] != KDEHIP_MANIFOLD_EUCLIDEAN)
      return set_error(KDEHIP_ERR_ARG, std::string(rule.name) + ": every entry is KDEHIP_MANIFOLD_EUCLIDEAN or KDEHIP_MANIFOLD_CIRCULAR");
  }
  if (bits != 0u && rule.precision == 32) return set_error(KDEHIP_ERR_UNSUPPORTED, "circular dimensions need precision 64");
  if (mask) *mask = bits;
  return KDEHIP_OK;
}

// ... for the callers that hand the pointer on: all zeros becomes NULL (the Euclidean path)
inline int manifold_arg_or_null(const uint8_t *&arg, int64_t D, uint32_t *mask, const ManifoldRule &rule = {}) {
  uint32_t bits = 0;
  const int rc = manifold_arg(arg, D, &bits, rule);
  if (rc == KDEHIP_OK && bits == 0u) arg = nullptr;
  if (mask) *mask = bits;
  return rc;
}

}  // namespace kdehip
