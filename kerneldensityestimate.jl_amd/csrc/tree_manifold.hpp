// tree_manifold.hpp -- the ONE check of a `tree_manifold` argument (include/kdehip.h section 4, "tree construction on a
// manifold"), shared by the entries that take it: balltree.cpp, treebuild.hip, loocv.hip, pack_device.hip.
#pragma once
#include <cstdint>

#include "../../include/kdehip.h"
#include "kdehip_internal.hpp"

namespace kdehip {

// Every one of the D bytes is KDEHIP_MANIFOLD_EUCLIDEAN or KDEHIP_MANIFOLD_CIRCULAR (KDEHIP_ERR_ARG otherwise; NULL is all
// Euclidean).  *mask (optional): bit k set for a circular dimension k < 32; the return of a valid call is KDEHIP_OK, and
// *mask == 0 for D <= 32 says "the Euclidean builder".
inline int tree_manifold_mask(const uint8_t *tree_manifold, int64_t D, uint32_t *mask) {
  if (mask) *mask = 0;
  for (int64_t k = 0; tree_manifold && k < D; ++k) {
    if (tree_manifold[k] > KDEHIP_MANIFOLD_CIRCULAR)
      return set_error(KDEHIP_ERR_ARG, "tree_manifold: every entry is KDEHIP_MANIFOLD_EUCLIDEAN or KDEHIP_MANIFOLD_CIRCULAR");
    if (mask && k < 32 && tree_manifold[k] == KDEHIP_MANIFOLD_CIRCULAR) *mask |= 1u << k;
  }
  return KDEHIP_OK;
}

}  // namespace kdehip
