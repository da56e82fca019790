// capi_surface.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- the surface constraint of the motion update (include/rmclhip.h states the rule; surface.hip.h implements it) ----
void rmclhip_surface_params_default(rmclhip_surface_params* out) {
  if (!out) return;
  out->axis = 0u;
  out->height = 0.0f;
  out->probe_up = 0.3f;
  out->probe_down = 1.0f;
  out->min_up_cos = 0.7f;
  out->align = 0u;
  out->on_miss = 0u;
}

RMCL_INTERNAL rmclhip_status surface_params_check(const char* who_, const rmclhip_surface_params* p) {
  const std::string who(who_);
  if (!p) return fail(RMCLHIP_ERR_INVALID, who + ": null surface parameters");
  const float len[3] = {p->height, p->probe_up, p->probe_down};
  for (float v : len)
    if (!std::isfinite(v) || v < 0.0f) return fail(RMCLHIP_ERR_INVALID, who + ": height, probe_up and probe_down must be finite and >= 0");
  if (!(p->min_up_cos >= 0.0f && p->min_up_cos <= 1.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": min_up_cos outside [0, 1] (or NaN)");
  if (p->axis > 1u) return fail(RMCLHIP_ERR_INVALID, who + ": axis must be 0 (map +z) or 1 (body z)");
  if (p->align > 1u) return fail(RMCLHIP_ERR_INVALID, who + ": align must be 0 or 1");
  if (p->on_miss > 1u) return fail(RMCLHIP_ERR_INVALID, who + ": on_miss must be 0 or 1");
  return RMCLHIP_OK;
}

static SurfaceKernelParams surface_kernel_params(const rmclhip_surface_params& p) {
  SurfaceKernelParams k;
  k.axis = p.axis; k.align = p.align; k.on_miss = p.on_miss;
  k.height = p.height; k.probe_up = p.probe_up; k.probe_down = p.probe_down; k.min_up_cos = p.min_up_cos;
  return k;
}

// the 4-word count block on the device and its pinned landing place (once per handle)
static rmclhip_status pf_surface_buffers(rmclhip_pf* f) {
  HIPCHK(f->d_surf.reserve(4));
  if (!f->h_surf.p) {
    HIPCHK(f->h_surf.reserve(4));
    std::memset(f->h_surf.p, 0, 4 * sizeof(uint32_t));
  }
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status pf_motion_enqueue(rmclhip_pf* f, xform* poses, void* attrs, uint32_t n, const xform& T_bnew_bold, double forget_rate,
                                               uint32_t max_n_meas, bool collision, const MotionNoiseKernelParams* noise) {
  if (!f->surface_on) {
    HIPCHK(launch_pf_motion(f->map->d_qnodes.p, f->map->d_tris.p, poses, attrs, n, T_bnew_bold, forget_rate, max_n_meas, collision, f->stream, nullptr, nullptr,
                            nullptr, noise));
    return RMCLHIP_OK;
  }
  if (rmclhip_status st = pf_surface_buffers(f)) return st;
  const SurfaceKernelParams k = surface_kernel_params(f->surface);
  HIPCHK(hipMemsetAsync(f->d_surf.p, 0, 4 * sizeof(uint32_t), f->stream));
  HIPCHK(launch_pf_motion(f->map->d_qnodes.p, f->map->d_tris.p, poses, attrs, n, T_bnew_bold, forget_rate, max_n_meas, collision, f->stream, &k, f->d_surf.p, f->surf_faces,
                          noise));
  HIPCHK(hipMemcpyAsync(f->h_surf.p, f->d_surf.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status pf_surface_enqueue(rmclhip_pf* f, xform* poses, void* attrs, uint32_t n, const rmclhip_surface_params& sp, uint32_t max_n_meas) {
  if (rmclhip_status st = pf_surface_buffers(f)) return st;
  HIPCHK(hipMemsetAsync(f->d_surf.p, 0, 4 * sizeof(uint32_t), f->stream));
  HIPCHK(launch_surface_constrain(f->map->d_qnodes.p, f->map->d_tris.p, poses, attrs, n, surface_kernel_params(sp), max_n_meas, f->d_surf.p, f->surf_faces, f->stream));
  HIPCHK(hipMemcpyAsync(f->h_surf.p, f->d_surf.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, f->stream));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_set_surface(rmclhip_pf* f, const rmclhip_surface_params* params) {
  ApiGuard guard_("rmclhip_pf_set_surface");
  if (!f) return fail(RMCLHIP_ERR_INVALID, "pf_set_surface: null");
  if (!params) { f->surface_on = false; return RMCLHIP_OK; }
  if (rmclhip_status st = surface_params_check("pf_set_surface", params)) return st;
  f->surface = *params;
  f->surface_on = true;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_get_surface_stats(rmclhip_pf* f, rmclhip_surface_stats* out) {
  ApiGuard guard_("rmclhip_pf_get_surface_stats");
  if (!f || !out) return fail(RMCLHIP_ERR_INVALID, "pf_get_surface_stats: null");
  std::memset(out, 0, sizeof(*out));
  if (!f->h_surf.p) return RMCLHIP_OK;
  out->n_particles = f->h_surf.p[0]; out->n_snapped = f->h_surf.p[1]; out->n_missed = f->h_surf.p[2]; out->n_steep = f->h_surf.p[3];
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_constrain_to_surface(rmclhip_pf* f, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev, uint32_t n,
                                               const rmclhip_surface_params* params, rmclhip_surface_stats* stats_out) {
  ApiGuard guard_("rmclhip_pf_constrain_to_surface");
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!f) return fail(RMCLHIP_ERR_INVALID, "pf_constrain_to_surface: null");
  if (rmclhip_status st = surface_params_check("pf_constrain_to_surface", params)) return st;
  if (n == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, "pf_constrain_to_surface: null buffers");
  HIPCHK(hipSetDevice(f->ctx->device));
  if (rmclhip_status st = pf_surface_enqueue(f, reinterpret_cast<xform*>(poses_dev), attrs_dev, n, *params, f->params.max_n_meas)) return st;
  HIPCHK(f->tag.wait_chain_end(f->ctx, f->stream));
  if (stats_out) return rmclhip_pf_get_surface_stats(f, stats_out);
  return RMCLHIP_OK;
}

// include/rmclhip_lab.h
rmclhip_status rmclhip_debug_surface_faces(rmclhip_pf* f, uint32_t* faces_dev) {
  ApiGuard guard_("rmclhip_debug_surface_faces");
  if (!f) return fail(RMCLHIP_ERR_INVALID, "debug_surface_faces: null");
  f->surf_faces = faces_dev;
  return RMCLHIP_OK;
}
