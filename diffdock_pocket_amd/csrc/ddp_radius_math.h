// ddp_radius_math.h - the distance arithmetic of the neighbour searches, shared by csrc/ddp_graph.hip and
// csrc/ddp_front_lists.hip: both must select exactly the same pairs, so there is one copy of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

__device__ __forceinline__ float sqdist(const float* __restrict__ a, const float* __restrict__ b) {
  // contraction off: with it hipcc fuses some instances of this expression into FMAs and not others, so the SAME pair
  // evaluates to values one ulp apart in the counting and the selecting loop (seen as off-by-one cuts), and no instance
  // matches the separately rounded products of the dense formulation
#pragma clang fp contract(off)
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// point j of `p`, divided by `div` when the search runs on per-graph scaled coordinates (the reference's dynamic cross
// cutoff divides both point sets by 3 sigma + 20 and searches with r = 1, models/all_atom_score_model.py:548-556: the same
// correctly rounded divisions, so the strict comparison sees the same values)
__device__ __forceinline__ void load_pt(const float* __restrict__ p, size_t j, bool scaled, float div, float out[3]) {
  out[0] = p[3 * j];
  out[1] = p[3 * j + 1];
  out[2] = p[3 * j + 2];
  if (scaled) {
    out[0] = __fdiv_rn(out[0], div);
    out[1] = __fdiv_rn(out[1], div);
    out[2] = __fdiv_rn(out[2], div);
  }
}

__device__ __forceinline__ float sqdist_to(const float* __restrict__ yq, const float* __restrict__ x, size_t j, bool scaled, float div) {
  float xj[3];
  load_pt(x, j, scaled, div, xj);
  return sqdist(yq, xj);
}
