// surface_sample.hip.h -- THE DRAW of the surface sampler (include/rmclhip.h, SURFACE SAMPLER): one pose from two Philox blocks, shared by
// the initialisation on the surface and the recovery injection (particles.hip), so that a pose drawn by either is the same function of
// (seed, counter).  Device code only.  Every operation is the one tests/surface_sample_ref.py performs, in its order
// (-ffp-contract=off).  No floating-point value chooses the face: position, prefix sums and the search are integers.
#pragma once
#include "pf_random.hip.h"
#include "kernels.h"
#include "surface_align.hip.h"

namespace rmclhip {
namespace {

// the first f with incl[f] > pos (pos < T = incl[n_faces - 1]: it exists).  ~log2(n_faces) dependent 8-byte loads.
__device__ __forceinline__ uint32_t surface_sample_face(const SurfaceSampleView& sv, unsigned long long pos) {
  uint32_t lo = 0u, hi = sv.n_faces - 1u;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (sv.incl[mid] > pos) hi = mid; else lo = mid + 1u;
  }
  return lo;
}

__device__ __forceinline__ xform surface_sample_pose(const SurfaceSampleView& sv, const uint32_t (&A)[4], const uint32_t (&B)[4]) {
  const unsigned long long r = (static_cast<unsigned long long>(A[0]) << 32) | A[1];
  const uint32_t f = surface_sample_face(sv, __umul64hi(r, sv.T));
  const uint4* rec = reinterpret_cast<const uint4*>(sv.tris) + static_cast<size_t>(sv.rec_of_face[f]) * 4u;
  const uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];   // v0.xyz e1.x | e1.yz e2.xy | e2.z Ng.xyz | n.xyz face
  const float v0[3] = {__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z)};
  const float e1[3] = {__uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)};
  const float e2[3] = {__uint_as_float(q1.z), __uint_as_float(q1.w), __uint_as_float(q2.x)};
  double u = (static_cast<double>(A[2]) + 0.5) * (1.0 / 4294967296.0);
  double v = (static_cast<double>(A[3]) + 0.5) * (1.0 / 4294967296.0);
  if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
  float p[3];
#pragma unroll
  for (int d = 0; d < 3; ++d)
    p[d] = static_cast<float>((static_cast<double>(v0[d]) - u * static_cast<double>(e1[d])) + v * static_cast<double>(e2[d]));
  const float yaw = uniform_in(sv.yaw_min, sv.yaw_max, B[0]);
  f3 n = mk3(__uint_as_float(q3.x), __uint_as_float(q3.y), __uint_as_float(q3.z));
  if (n.z < 0.0f) n = neg3(n);   // no consistent winding in a map
  xform T;
  T.R = euler_to_quat(0.0f, 0.0f, yaw);
  f3 a = mk3(0.0f, 0.0f, 1.0f);
  if (sv.align != 0u) { T.R = surface_align(T.R, n); a = n; }
  T.t = mk3(p[0] + sv.height * a.x, p[1] + sv.height * a.y, p[2] + sv.height * a.z);
  T.stamp = 0u;
  return T;
}

}  // namespace
}  // namespace rmclhip
