// capi_motion_noise.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- the sampled odometry model of the motion update (include/rmclhip.h, MOTION NOISE, states the rule; pf_random.hip.h draws) ----
void rmclhip_motion_noise_params_default(rmclhip_motion_noise_params* out) {
  if (!out) return;
  for (int k = 0; k < 3; ++k) {   // AMCL's alpha1..4
    out->alpha_trans_trans[k] = 0.2f;
    out->alpha_trans_rot[k] = 0.2f;
    out->alpha_rot_trans[k] = 0.2f;
    out->alpha_rot_rot[k] = 0.2f;
  }
}

RMCL_INTERNAL rmclhip_status motion_noise_params_check(const char* who_, const rmclhip_motion_noise_params* p) {
  const std::string who(who_);
  if (!p) return fail(RMCLHIP_ERR_INVALID, who + ": null motion noise parameters");
  const float* rows[4] = {p->alpha_trans_trans, p->alpha_trans_rot, p->alpha_rot_trans, p->alpha_rot_rot};
  for (const float* row : rows)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(row[k]) || row[k] < 0.0f) return fail(RMCLHIP_ERR_INVALID, who + ": every alpha must be finite and >= 0");
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status motion_noise_sigma(const char* who_, const rmclhip_motion_noise_params* p, const rmclhip_transform* T, float* sigma_out) {
  const std::string who(who_);
  if (rmclhip_status st = motion_noise_params_check(who_, p)) return st;
  if (!T || !sigma_out) return fail(RMCLHIP_ERR_INVALID, who + ": null");
  const xform x = to_x(T);
  const float step[7] = {x.R.x, x.R.y, x.R.z, x.R.w, x.t.x, x.t.y, x.t.z};
  for (float v : step)
    if (!std::isfinite(v)) return fail(RMCLHIP_ERR_INVALID, who + ": T_bnew_bold has a non-finite component");
  const double dx = x.t.x, dy = x.t.y, dz = x.t.z, qx = x.R.x, qy = x.R.y, qz = x.R.z, qw = x.R.w;
  const double s_t = std::sqrt((dx * dx + dy * dy) + dz * dz);
  const double s_r = 2.0 * std::atan2(std::sqrt((qx * qx + qy * qy) + qz * qz), std::fabs(qw));
  for (int k = 0; k < 3; ++k) {
    const double tt = static_cast<double>(p->alpha_trans_trans[k]) * s_t, tr = static_cast<double>(p->alpha_trans_rot[k]) * s_r;
    const double rt = static_cast<double>(p->alpha_rot_trans[k]) * s_t, rr = static_cast<double>(p->alpha_rot_rot[k]) * s_r;
    sigma_out[k] = static_cast<float>(std::sqrt(tt * tt + tr * tr));
    sigma_out[3 + k] = static_cast<float>(std::sqrt(rt * rt + rr * rr));
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_motion_noise_sigma_host(const rmclhip_motion_noise_params* params, const rmclhip_transform* T_bnew_bold, float* sigma_out) {
  ApiGuard guard_("rmclhip_motion_noise_sigma_host");
  return motion_noise_sigma("motion_noise_sigma_host", params, T_bnew_bold, sigma_out);
}

// the refusals of a noisy call's sigma, and the kernel's view of it; *on = false when all six are zero (the deterministic launch)
RMCL_INTERNAL rmclhip_status motion_noise_kernel_params(const char* who_, const float* sigma, uint64_t seed, uint32_t step, uint32_t first,
                                                        MotionNoiseKernelParams* out, bool* on) {
  const std::string who(who_);
  if (!sigma) return fail(RMCLHIP_ERR_INVALID, who + ": null sigma");
  *on = false;
  for (int k = 0; k < 6; ++k) {
    if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f) return fail(RMCLHIP_ERR_INVALID, who + ": every sigma must be finite and >= 0");
    out->sigma[k] = sigma[k];
    if (sigma[k] != 0.0f) *on = true;
  }
  out->key0 = static_cast<uint32_t>(seed);
  out->key1 = static_cast<uint32_t>(seed >> 32);
  out->step = step;
  out->first = first;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_motion_update_noisy(rmclhip_pf* f, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev, uint32_t n,
                                              const rmclhip_transform* T_bnew_bold, double forget_rate, int check_collision, const float* sigma,
                                              uint64_t seed, uint32_t step, uint32_t first_index) {
  ApiGuard guard_("rmclhip_pf_motion_update_noisy");
  if (!f || !T_bnew_bold) return fail(RMCLHIP_ERR_INVALID, "pf_motion_update_noisy: null");
  MotionNoiseKernelParams nz{};
  bool noisy = false;
  if (rmclhip_status st = motion_noise_kernel_params("pf_motion_update_noisy", sigma, seed, step, first_index, &nz, &noisy)) return st;
  if (!(forget_rate >= 0.0 && forget_rate <= 1.0)) return fail(RMCLHIP_ERR_INVALID, "pf_motion_update_noisy: forget_rate outside [0, 1] (or NaN)");
  if (static_cast<uint64_t>(first_index) + n > (1ull << 32))
    return fail(RMCLHIP_ERR_INVALID, "pf_motion_update_noisy: first_index + n exceeds 2^32 (the particle index is a 32-bit counter word)");
  if (n == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, "pf_motion_update_noisy: null buffers");
  HIPCHK(hipSetDevice(f->ctx->device));
  if (rmclhip_status st = pf_motion_enqueue(f, reinterpret_cast<xform*>(poses_dev), attrs_dev, n, to_x(T_bnew_bold), forget_rate,
                                            f->params.max_n_meas, check_collision != 0, noisy ? &nz : nullptr))
    return st;
  HIPCHK(f->tag.wait_chain_end(f->ctx, f->stream));
  return RMCLHIP_OK;
}
