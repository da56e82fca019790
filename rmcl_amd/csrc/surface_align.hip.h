// surface_align.hip.h -- step 5 of the surface constraint (include/rmclhip.h, "surface-constrained motion"): the shortest arc that takes a
// body's z onto a unit normal.  ONE text for the constraint (surface.hip.h) and the surface sampler's draw (surface_sample.hip.h), which
// needs nothing else of the constraint.  Device code only; every float operation in the order tests/surface_ref.py performs it.
#pragma once
#include "devmath.h"

namespace rmclhip {
namespace {

__device__ __forceinline__ quat surface_qnormalise(quat q) {
  const float nrm = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
  quat r; r.x = q.x / nrm; r.y = q.y / nrm; r.z = q.z / nrm; r.w = q.w / nrm;
  return r;
}

// R turned by the shortest arc that takes its body z onto the unit vector n
__device__ __forceinline__ quat surface_align(quat R, f3 n) {
  const f3 zb = qrot(R, mk3(0.0f, 0.0f, 1.0f));
  quat q;
  q.w = 1.0f + ((zb.x * n.x + zb.y * n.y) + zb.z * n.z);
  if (q.w < 1e-6f) {
    const f3 xb = qrot(R, mk3(1.0f, 0.0f, 0.0f));   // upside down: the half turn about the body's x
    q.x = xb.x; q.y = xb.y; q.z = xb.z; q.w = 0.0f;
  } else {
    q.x = zb.y * n.z - zb.z * n.y; q.y = zb.z * n.x - zb.x * n.z; q.z = zb.x * n.y - zb.y * n.x;
  }
  return surface_qnormalise(qmul(surface_qnormalise(q), R));
}

}  // namespace
}  // namespace rmclhip
