// surface.hip -- the surface constraint as a pass of its own: k_surface_constrain snaps every particle of a cloud to the mesh below it
// (after an initialisation, or after a resampler's noise).  The rule, its float32 operation order and the classes snap / miss / steep
// are stated in include/rmclhip.h and implemented once, in surface.hip.h; the motion update runs the same code in its own launch
// (kernels.hip: k_pf_motion<., true>).
//
// One lane per particle, 256 per workgroup, 16 LDS stack rows per lane ([row][lane], the layout of trace_lane_bf); a pose is two 16-B
// loads, and two 16-B stores for a snapped particle only; the likelihood (12 B) is stored only where on_miss rewrites it.
#include "surface.hip.h"

namespace rmclhip {
namespace {

__global__ void __launch_bounds__(256) k_surface_constrain(const uint32_t* __restrict__ qnodes, const uint32_t* __restrict__ tris,
                                                           xform* __restrict__ poses, pattrs* __restrict__ attrs, uint32_t n,
                                                           SurfaceKernelParams sp, uint32_t max_n_meas, uint32_t* __restrict__ stats,
                                                           uint32_t* __restrict__ faces) {
  extern __shared__ uint32_t lds_dyn[];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const uint32_t ii = live ? i : 0u;
  const float4* src = reinterpret_cast<const float4*>(poses + ii);
  const float4 r = src[0], t = src[1];
  xform pose;
  pose.R.x = r.x; pose.R.y = r.y; pose.R.z = r.z; pose.R.w = r.w;
  pose.t = mk3(t.x, t.y, t.z);
  pose.stamp = __float_as_uint(t.w);
  const f3 a = surface_axis(sp, pose);
  const f3 O = surface_origin(sp, pose, a);
  const uint32_t cls = surface_constrain_lane(qnodes, tris, sp, pose, a, O, live, lds_dyn + threadIdx.x, faces ? faces + ii : nullptr);
  surface_count(stats, live, cls);
  if (!live) return;
  if (cls == kSurfSnap) {
    float4* dst = reinterpret_cast<float4*>(poses + i);
    dst[0] = make_float4(pose.R.x, pose.R.y, pose.R.z, pose.R.w);
    dst[1] = make_float4(pose.t.x, pose.t.y, pose.t.z, __uint_as_float(pose.stamp));
  } else if (sp.on_miss != 0u) {
    g1d L; L.mean = 0.0f; L.sigma = 0.0f; L.n_meas = max_n_meas;
    attrs[i].likelihood = L;
  }
}

}  // namespace

hipError_t launch_surface_constrain(const uint32_t* qnodes, const uint32_t* tris, xform* poses, void* attrs, uint32_t n,
                                    const SurfaceKernelParams& sp, uint32_t max_n_meas, uint32_t* stats, uint32_t* faces, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!stats || (reinterpret_cast<uintptr_t>(poses) & 15u) || (reinterpret_cast<uintptr_t>(attrs) & 3u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_surface_constrain, dim3((n + 255u) / 256u), dim3(256), 16u * 256u * sizeof(uint32_t), s, qnodes, tris, poses,
                     reinterpret_cast<pattrs*>(attrs), n, sp, max_n_meas, stats, faces);
  return hipGetLastError();
}

}  // namespace rmclhip
