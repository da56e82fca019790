// deskew_pose.h -- the pose of one point of a scan taken in motion (include/rmclhip.h, MOTION-COMPENSATED INPUT), shared by the
// device kernel (deskew.hip) and the host beam sampler (capi_deskew.cpp).  Every step is one IEEE operation in a stated order (the
// library is built with -ffp-contract=off and correctly rounded float divide / sqrt): tests/deskew_ref.py restates it in numpy and
// reproduces the bytes.  No transcendental: the interpolation is nlerp, the caller subdivides the knots (rmclhip.h gives the bound).
#pragma once
#include "devmath.h"

namespace rmclhip {

constexpr uint32_t kDeskewMaxKnots = 64u;
constexpr uint32_t kTimeU32 = 6u, kTimeF32 = 7u, kTimeF64 = 8u;   // sensor_msgs/PointField datatypes of a time field

// std::isfinite for a double: neither NaN nor +-inf
RM_HD bool deskew_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// the largest k with times[k] <= t, limited to [0, K - 2] (K in [2, 64]): six halvings of [0, K - 1] at the most
RM_HD uint32_t deskew_segment(const double* times, uint32_t K, double t) {
  uint32_t lo = 0u, hi = K - 1u;
#pragma unroll
  for (int it = 0; it < 6; ++it) {
    if (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (times[mid] <= t) lo = mid; else hi = mid;
    }
  }
  return lo;
}

// s of t in [t0, t1]: the quotient in double, cast to float, clamped to [0, 1]; *clamped: it left that interval
RM_HD float deskew_fraction(double t, double t0, double t1, bool* clamped) {
  const float s = static_cast<float>((t - t0) / (t1 - t0));
  *clamped = (s < 0.0f) || (s > 1.0f);
  return (s < 0.0f) ? 0.0f : ((s > 1.0f) ? 1.0f : s);
}

// nlerp of the rotations on the shorter arc, lerp of the translations
RM_HD void deskew_interp(quat q0, f3 t0, quat q1, f3 t1, float s, quat* q_out, f3* t_out) {
  const float a = 1.0f - s;
  const float d = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
  if (d < 0.0f) { q1.x = -q1.x; q1.y = -q1.y; q1.z = -q1.z; q1.w = -q1.w; }
  quat q;
  q.x = a * q0.x + s * q1.x; q.y = a * q0.y + s * q1.y; q.z = a * q0.z + s * q1.z; q.w = a * q0.w + s * q1.w;
  const float n = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
  q.x = q.x / n; q.y = q.y / n; q.z = q.z / n; q.w = q.w / n;
  *q_out = q;
  *t_out = mk3(a * t0.x + s * t1.x, a * t0.y + s * t1.y, a * t0.z + s * t1.z);
}

}  // namespace rmclhip
