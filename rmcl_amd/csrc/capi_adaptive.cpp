// capi_adaptive.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- a particle count that follows the posterior (include/rmclhip.h states the rules; adaptive.hip and resample.hip implement them) ----
void rmclhip_kld_params_default(rmclhip_kld_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  for (int d = 0; d < 3; ++d) { out->bin_xyz[d] = 0.5f; out->bin_rpy[d] = 0.17453292f; }
  out->min_likelihood_rel = 0.01f;
  out->epsilon = 0.01;
  out->z = 2.3263479;
  out->n_min = 500u;
  out->n_max = 0xFFFFFFFFu;
}

rmclhip_status rmclhip_kld_bound_host(uint32_t k, double epsilon, double z, uint32_t n_min, uint32_t n_max, uint32_t* n_out) {
  ApiGuard guard_("rmclhip_kld_bound_host");
  if (!n_out) return fail(RMCLHIP_ERR_INVALID, "kld_bound_host: n_out is null");
  *n_out = 0;
  if (!std::isfinite(epsilon) || !std::isfinite(z) || !(epsilon > 0.0)) return fail(RMCLHIP_ERR_INVALID, "kld_bound_host: epsilon must be finite and > 0, z finite");
  if (n_min == 0u || n_min > n_max) return fail(RMCLHIP_ERR_INVALID, "kld_bound_host: 1 <= n_min <= n_max required");
  if (k < 2u) { *n_out = n_min; return RMCLHIP_OK; }
  const double km1 = static_cast<double>(k - 1u);
  const double a = 2.0 / (9.0 * km1);
  const double x = (1.0 - a) + std::sqrt(a) * z;
  const double n = std::ceil((km1 / (2.0 * epsilon)) * ((x * x) * x));   // finite: every factor is
  uint32_t r;
  if (!(n > static_cast<double>(n_min))) r = n_min;            // (a negative x: the quantile of a delta > 1/2 on few bins)
  else if (n >= static_cast<double>(n_max)) r = n_max;         // saturates at 2^32 - 1 with it
  else r = static_cast<uint32_t>(n);
  *n_out = r;
  return RMCLHIP_OK;
}

rmclhip_status kld_bins_check(const char* who_, const rmclhip_kld_params* p) {
  const std::string who(who_);
  if (!p) return fail(RMCLHIP_ERR_INVALID, who + ": null KLD parameters");
  for (int d = 0; d < 3; ++d) {
    if (!std::isfinite(p->bin_xyz[d]) || p->bin_xyz[d] < 0.0f) return fail(RMCLHIP_ERR_INVALID, who + ": bin_xyz must be finite and >= 0");
    if (!std::isfinite(p->bin_rpy[d]) || (p->bin_rpy[d] != 0.0f && p->bin_rpy[d] < 0.05f))
      return fail(RMCLHIP_ERR_INVALID, who + ": bin_rpy must be 0 or a finite angle >= 0.05 rad");
  }
  if (!(p->min_likelihood_rel >= 0.0f && p->min_likelihood_rel <= 1.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": min_likelihood_rel outside [0, 1] (or NaN)");
  return RMCLHIP_OK;
}

// {sum, max} of the likelihoods on the resampler's stream, landed on the host
rmclhip_status resampler_stats(rmclhip_resampler* r, const rmclhip_particle_attributes* attrs_dev, uint32_t n, float* max_out) {
  HIPCHK(launch_likelihood_stats(attrs_dev, n, r->d_psum.p, r->d_pmax.p, r->d_out.p, r->stream));
  HIPCHK(hipMemcpyAsync(r->h_out.p, r->d_out.p, 2 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  *max_out = r->h_out.p[1];
  return RMCLHIP_OK;
}

// the arguments are checked; max_l: the statistics' maximum
rmclhip_status count_bins_run(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                     uint32_t n, const rmclhip_kld_params* p, float max_l, uint32_t* k_out, uint32_t* n_counted_out) {
  const uint64_t words = kld_table_words(n);
  HIPCHK(r->d_kld_table.reserve(words));
  HIPCHK(r->d_kld_cnt.reserve(2));
  HIPCHK(hipMemsetAsync(r->d_kld_table.p, 0xFF, words * sizeof(unsigned long long), r->stream));
  HIPCHK(hipMemsetAsync(r->d_kld_cnt.p, 0, 2 * sizeof(uint32_t), r->stream));
  const float floor_l = p->min_likelihood_rel * max_l;
  HIPCHK(launch_kld_count_bins(reinterpret_cast<const xform*>(poses_dev), attrs_dev, n, p->bin_xyz, p->bin_rpy, floor_l, r->d_kld_table.p, words,
                               r->d_kld_cnt.p, r->stream));
  uint32_t* h_cnt = reinterpret_cast<uint32_t*>(&r->h_res.p[5]);
  HIPCHK(hipMemcpyAsync(h_cnt, r->d_kld_cnt.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  *k_out = h_cnt[0];
  if (n_counted_out) *n_counted_out = h_cnt[1];
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_particles_count_bins(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                            uint32_t n, const rmclhip_kld_params* p, uint32_t* k_out, uint32_t* n_counted_out) {
  ApiGuard guard_("rmclhip_particles_count_bins");
  if (k_out) *k_out = 0;
  if (n_counted_out) *n_counted_out = 0;
  if (!r || !k_out) return fail(RMCLHIP_ERR_INVALID, "particles_count_bins: null");
  if (rmclhip_status st = kld_bins_check("particles_count_bins", p)) return st;
  if (n == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, "particles_count_bins: null particle buffers");
  HIPCHK(hipSetDevice(r->ctx->device));
  float max_l = 0.0f;
  if (rmclhip_status st = resampler_stats(r, attrs_dev, n, &max_l)) return st;
  return count_bins_run(r, poses_dev, attrs_dev, n, p, max_l, k_out, n_counted_out);
}

static rmclhip_status systematic_check(const char* who_, rmclhip_resampler* r, const rmclhip_transform* poses_dev,
                                       const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles, rmclhip_transform* poses_new_dev,
                                       rmclhip_particle_attributes* attrs_new_dev, uint32_t n_new, uint32_t first, uint32_t count,
                                       const rmclhip_gladiator_config* cfg) {
  const std::string who(who_);
  if (!r || !cfg) return fail(RMCLHIP_ERR_INVALID, who + ": null");
  if (rmclhip_status cs = resampler_config_check(who_, cfg)) return cs;
  if (n_new == 0) return fail(RMCLHIP_ERR_INVALID, who + ": a new cloud of 0 particles");
  if (static_cast<uint64_t>(first) + count > n_new) return fail(RMCLHIP_ERR_INVALID, who + ": slot range exceeds the new cloud");
  if (count == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev || !poses_new_dev || !attrs_new_dev || n_particles == 0) return fail(RMCLHIP_ERR_INVALID, who + ": null particle buffers");
  if (poses_new_dev == poses_dev || attrs_new_dev == attrs_dev) return fail(RMCLHIP_ERR_INVALID, who + ": out of place (double buffers)");
  return RMCLHIP_OK;
}

static rmclhip_status systematic_run(const char* who_, rmclhip_resampler* r, const rmclhip_transform* poses_dev,
                                     const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles, rmclhip_transform* poses_new_dev,
                                     rmclhip_particle_attributes* attrs_new_dev, uint32_t n_new, uint32_t first, uint32_t count,
                                     const rmclhip_gladiator_config* cfg, uint64_t seed, uint32_t step, float max_l) {
  if (!(max_l > 0.0f) || !std::isfinite(max_l))
    return fail(RMCLHIP_ERR_INVALID, std::string(who_) + ": the largest likelihood is zero, negative or not finite: nothing to resample from");
  HIPCHK(r->d_sys_incl.reserve(n_particles));
  HIPCHK(r->d_sys_btot.reserve((static_cast<size_t>(n_particles) + 1023u) / 1024u));
  HIPCHK(launch_sys_scan(attrs_dev, n_particles, static_cast<double>(max_l), r->d_sys_incl.p, r->d_sys_btot.p, r->stream));
  const float c8[8] = {cfg->min_noise_tx, cfg->min_noise_ty, cfg->min_noise_tz, cfg->min_noise_roll,
                       cfg->min_noise_pitch, cfg->min_noise_yaw, cfg->likelihood_forget_per_meter,
                       cfg->likelihood_forget_per_radian};
  HIPCHK(launch_sys_fill(reinterpret_cast<const xform*>(poses_dev), attrs_dev, r->d_sys_incl.p, n_particles, reinterpret_cast<xform*>(poses_new_dev),
                         attrs_new_dev, n_new, first, count, c8, cfg->trans_dist_metric, seed, step, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_resampler_systematic(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                            uint32_t n_particles, rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev,
                                            uint32_t n_new, uint32_t first, uint32_t count, const rmclhip_gladiator_config* cfg, uint64_t seed,
                                            uint32_t step) {
  ApiGuard guard_("rmclhip_resampler_systematic");
  if (rmclhip_status st = systematic_check("resampler_systematic", r, poses_dev, attrs_dev, n_particles, poses_new_dev, attrs_new_dev, n_new, first,
                                           count, cfg))
    return st;
  if (count == 0) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  float max_l = 0.0f;
  if (rmclhip_status st = resampler_stats(r, attrs_dev, n_particles, &max_l)) return st;
  return systematic_run("resampler_systematic", r, poses_dev, attrs_dev, n_particles, poses_new_dev, attrs_new_dev, n_new, first, count, cfg, seed,
                        step, max_l);
}

rmclhip_status rmclhip_resampler_adaptive(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                          uint32_t n_particles, rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev,
                                          uint32_t capacity_new, const rmclhip_kld_params* p, const rmclhip_gladiator_config* cfg, uint64_t seed,
                                          uint32_t step, uint32_t* n_new_out, uint32_t* k_out) {
  ApiGuard guard_("rmclhip_resampler_adaptive");
  if (n_new_out) *n_new_out = 0;
  if (k_out) *k_out = 0;
  if (!r || !n_new_out) return fail(RMCLHIP_ERR_INVALID, "resampler_adaptive: null");
  if (rmclhip_status st = kld_bins_check("resampler_adaptive", p)) return st;
  if (capacity_new == 0) return fail(RMCLHIP_ERR_INVALID, "resampler_adaptive: a new cloud of 0 particles");
  // (the buffers, with the smallest count the bound can give: a count of 0 would let null buffers pass)
  if (rmclhip_status st = systematic_check("resampler_adaptive", r, poses_dev, attrs_dev, n_particles, poses_new_dev, attrs_new_dev, capacity_new, 0u,
                                           1u, cfg))
    return st;
  if (p->n_min == 0u || p->n_min > p->n_max) return fail(RMCLHIP_ERR_INVALID, "resampler_adaptive: 1 <= n_min <= n_max required");
  const uint32_t n_max = std::min(p->n_max, capacity_new), n_min = std::min(p->n_min, n_max);
  uint32_t n_new = 0;
  if (rmclhip_status st = rmclhip_kld_bound_host(2u, p->epsilon, p->z, n_min, n_max, &n_new)) return st;   // the parameters, before any work
  HIPCHK(hipSetDevice(r->ctx->device));
  float max_l = 0.0f;
  if (rmclhip_status st = resampler_stats(r, attrs_dev, n_particles, &max_l)) return st;
  uint32_t k = 0;
  if (rmclhip_status st = count_bins_run(r, poses_dev, attrs_dev, n_particles, p, max_l, &k, nullptr)) return st;
  if (rmclhip_status st = rmclhip_kld_bound_host(k, p->epsilon, p->z, n_min, n_max, &n_new)) return st;
  if (rmclhip_status st = systematic_run("resampler_adaptive", r, poses_dev, attrs_dev, n_particles, poses_new_dev, attrs_new_dev, n_new, 0u, n_new, cfg,
                                         seed, step, max_l))
    return st;
  *n_new_out = n_new;
  if (k_out) *k_out = k;
  return RMCLHIP_OK;
}
