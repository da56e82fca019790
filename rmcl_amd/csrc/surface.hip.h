// surface.hip.h -- the surface constraint of one particle (include/rmclhip.h, "surface-constrained motion"): device code shared by the
// standalone pass (surface.hip: k_surface_constrain) and the fused case of the motion kernel (kernels.hip: k_pf_motion<., true>).
//
// One lane per particle, one short ray per lane along -a from probe_up above the contact point; the ray goes through trace_lane_bf on the
// quantised nodes WITH the guard: with axis 0 every ray of the cloud is exactly axis-parallel (D = (-0, -0, -1), inv = -1e30 on x and y),
// the case make_ray_slab_guarded exists for once the particle or the map lies far out (traverse.hip.h).  Every float operation below is
// the one tests/surface_ref.py performs, in its order (-ffp-contract=off: no contraction).
#pragma once
#include "pf_common.hip.h"
#include "surface_align.hip.h"

namespace rmclhip {
namespace {

constexpr uint32_t kSurfSnap = 0u, kSurfMiss = 1u, kSurfSteep = 2u;

__device__ __forceinline__ bool surface_pose_finite(const xform& T) {
  return isfinite(T.t.x) && isfinite(T.t.y) && isfinite(T.t.z) && isfinite(T.R.x) && isfinite(T.R.y) && isfinite(T.R.z) && isfinite(T.R.w);
}

// a: map +z, or the particle's own body z
__device__ __forceinline__ f3 surface_axis(const SurfaceKernelParams& sp, const xform& T) {
  return (sp.axis == 0u) ? mk3(0.0f, 0.0f, 1.0f) : qrot(T.R, mk3(0.0f, 0.0f, 1.0f));
}

// O = (t - height a) + probe_up a: the probe's origin, and the end point of the lifted collision segment
__device__ __forceinline__ f3 surface_origin(const SurfaceKernelParams& sp, const xform& T, f3 a) {
  const f3 c = mk3(T.t.x - sp.height * a.x, T.t.y - sp.height * a.y, T.t.z - sp.height * a.z);
  return mk3(c.x + sp.probe_up * a.x, c.y + sp.probe_up * a.y, c.z + sp.probe_up * a.z);
}

// The probe of one particle.  `live`: the lane has a particle; every lane of the wave must call (the traversal votes).  pose is
// rewritten for class snap only; a = surface_axis(pose), O = surface_origin(pose, a).  Returns the class.  face_out (nullable): this
// lane's word for the face the probe hit (kInvalidFace: none).
__device__ __forceinline__ uint32_t surface_constrain_lane(const uint32_t* __restrict__ qnodes, const uint32_t* __restrict__ tris,
                                                           const SurfaceKernelParams& sp, xform& pose, f3 a, f3 O, bool live,
                                                           uint32_t* __restrict__ lds_col, uint32_t* face_out = nullptr) {
  const f3 D = neg3(a);
  const float tfar = sp.probe_up + sp.probe_down;
  RayHit h;
  trace_lane_bf<16, true, false, false, true>(qnodes, tris, O, D, (live && surface_pose_finite(pose)) ? tfar : -1.0f, lds_col, h);
  if (h.rec == kNone) {
    if (face_out && live) *face_out = kInvalidFace;
    return kSurfMiss;
  }
  // the record's last 16 B: unit normal + the original face id
  const uint4 nrec = reinterpret_cast<const uint4*>(tris)[static_cast<size_t>(h.rec) * 4u + 3u];
  if (face_out) *face_out = nrec.w;   // (test output, rmclhip_debug_surface_faces; a lane without a particle has no ray and no hit)
  f3 n = mk3(asf(nrec.x), asf(nrec.y), asf(nrec.z));
  float d = (n.x * a.x + n.y * a.y) + n.z * a.z;
  if (d < 0.0f) { n = neg3(n); d = -d; }   // no consistent winding in a map
  if (!(d >= sp.min_up_cos)) return kSurfSteep;
  const f3 p = mk3(O.x + D.x * h.t, O.y + D.y * h.t, O.z + D.z * h.t);
  pose.t = mk3(p.x + sp.height * a.x, p.y + sp.height * a.y, p.z + sp.height * a.z);
  if (sp.align != 0u) pose.R = surface_align(pose.R, n);
  return kSurfSnap;
}

// class counts: one atomic per wave and class after a ballot.  stats: {particles, snapped, missed, steep}
__device__ __forceinline__ void surface_count(uint32_t* __restrict__ stats, bool live, uint32_t cls) {
  const uint64_t m_live = __ballot(live);
  const uint64_t m_snap = __ballot(live && cls == kSurfSnap), m_miss = __ballot(live && cls == kSurfMiss), m_steep = __ballot(live && cls == kSurfSteep);
  if ((threadIdx.x & 63u) == 0u) {   // (blocks are 256 lanes, all of them reach this point)
    if (m_live) atomicAdd(stats + 0, static_cast<uint32_t>(__popcll(m_live)));
    if (m_snap) atomicAdd(stats + 1, static_cast<uint32_t>(__popcll(m_snap)));
    if (m_miss) atomicAdd(stats + 2, static_cast<uint32_t>(__popcll(m_miss)));
    if (m_steep) atomicAdd(stats + 3, static_cast<uint32_t>(__popcll(m_steep)));
  }
}

}  // namespace
}  // namespace rmclhip
