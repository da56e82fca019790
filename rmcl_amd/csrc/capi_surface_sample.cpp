// capi_surface_sample.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- parameters ----------------------------------------------------------------------------------------------
void rmclhip_surface_sample_params_default(rmclhip_surface_sample_params* out) {
  if (!out) return;
  const float inf = std::numeric_limits<float>::infinity(), pi_f = 3.14159265358979323846f;
  *out = rmclhip_surface_sample_params{0.7f, 0.0f, 0, {-inf, -inf, -inf}, {inf, inf, inf}, -pi_f, pi_f};
}

RMCL_INTERNAL rmclhip_status surface_sample_params_check(const std::string& who, const rmclhip_surface_sample_params* p) {
  if (!(p->min_up_cos >= 0.0f && p->min_up_cos <= 1.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": min_up_cos outside [0, 1]");
  if (!std::isfinite(p->height)) return fail(RMCLHIP_ERR_INVALID, who + ": height is not finite");
  if (p->align != 0 && p->align != 1) return fail(RMCLHIP_ERR_INVALID, who + ": align must be 0 or 1");
  for (int d = 0; d < 3; ++d)
    if (!(p->region_min[d] <= p->region_max[d])) return fail(RMCLHIP_ERR_INVALID, who + ": region_min > region_max, or a NaN bound");
  if (!std::isfinite(p->yaw_min) || !std::isfinite(p->yaw_max) || p->yaw_min > p->yaw_max)
    return fail(RMCLHIP_ERR_INVALID, who + ": yaw_min > yaw_max, or a yaw bound that is not finite");
  return RMCLHIP_OK;
}

RMCL_INTERNAL SurfaceSampleView surface_sample_view(const rmclhip_surface_sampler* sm) {
  SurfaceSampleView v;
  v.tris = sm->map->d_tris.p; v.rec_of_face = sm->d_rec.p; v.incl = sm->d_incl.p;
  v.n_faces = sm->info.n_faces; v.T = sm->info.weight_total;
  v.height = sm->params.height; v.yaw_min = sm->params.yaw_min; v.yaw_max = sm->params.yaw_max;
  v.align = static_cast<uint32_t>(sm->params.align);
  return v;
}

// ---- the handle ------------------------------------------------------------------------------------------------
void rmclhip_surface_sampler_destroy(rmclhip_surface_sampler* sm) {
  if (!sm) return;
  if (sm->ctx) (void)hipSetDevice(sm->ctx->device);
  if (sm->map) rmclhip_map_release(sm->map);
  ctx_release(sm->ctx);
  delete sm;
}

// the build: lowest record per face id -> areas and their maximum -> the weights' prefix sums, one chain on the context's particle
// stream; then the areas and the sums come to the host once for the info (a sequential sum in face order: the same bits every time)
static rmclhip_status surface_sampler_build(rmclhip_surface_sampler* sm) {
  const std::string who = "surface_sampler_create";
  rmclhip_ctx* ctx = sm->ctx;
  const uint32_t nf = sm->info.n_faces, nrec = sm->map->info.n_records;
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (rmclhip_status st = particles_stream(ctx)) return st;
  hipStream_t s = ctx->part_stream;
  HIPCHK_AS(who, sm->d_rec.reserve(std::max(nf, 1u)));
  HIPCHK_AS(who, sm->d_incl.reserve(std::max(nf, 1u)));
  HIPCHK_AS(who, sm->d_count.reserve(1));
  HIPCHK_AS(who, sm->h_count.reserve(1));
  *sm->h_count.p = 0u;
  BuildScratch tmp;
  double* d_area = nullptr;
  unsigned long long *d_amax = nullptr, *d_btot = nullptr;
  HIPCHK_AS(who, tmp.alloc(&d_area, nf));
  HIPCHK_AS(who, tmp.alloc(&d_amax, 1));
  HIPCHK_AS(who, tmp.alloc(&d_btot, (static_cast<size_t>(nf) + 1023u) / 1024u));
  HIPCHK_AS(who, hipMemsetAsync(sm->d_rec.p, 0xFF, static_cast<size_t>(nf) * sizeof(uint32_t), s));
  HIPCHK_AS(who, hipMemsetAsync(d_amax, 0, sizeof(unsigned long long), s));
  SurfaceSampleRule rule;
  rule.min_up_cos = sm->params.min_up_cos;
  for (int d = 0; d < 3; ++d) { rule.region_min[d] = sm->params.region_min[d]; rule.region_max[d] = sm->params.region_max[d]; }
  HIPCHK_AS(who, launch_surface_sample_records(sm->map->d_tris.p, nrec, nf, sm->d_rec.p, s));
  HIPCHK_AS(who, launch_surface_sample_areas(sm->map->d_tris.p, sm->d_rec.p, nf, rule, d_area, d_amax, s));
  HIPCHK_AS(who, launch_surface_sample_scan(d_area, d_amax, nf, sm->d_incl.p, d_btot, s));
  std::vector<double> area(nf);
  std::vector<unsigned long long> incl(nf);
  HIPCHK_AS(who, hipMemcpyAsync(area.data(), d_area, static_cast<size_t>(nf) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK_AS(who, hipMemcpyAsync(incl.data(), sm->d_incl.p, static_cast<size_t>(nf) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK_AS(who, hipStreamSynchronize(s));
  double sum = 0.0;
  uint32_t n_eligible = 0, n_weighted = 0;
  for (uint32_t f = 0; f < nf; ++f) {
    if (!(area[f] < 0.0)) {   // -1: not eligible (a NaN area belongs to an eligible face)
      ++n_eligible;
      if (std::isfinite(area[f])) sum = sum + area[f];
    }
    if (incl[f] != (f ? incl[f - 1u] : 0ull)) ++n_weighted;
  }
  sm->info.n_eligible = n_eligible;
  sm->info.n_weighted = n_weighted;
  sm->info.area_eligible = sum;
  sm->info.weight_total = incl[nf - 1u];
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_surface_sampler_create(rmclhip_map* map, const rmclhip_surface_sample_params* params, rmclhip_surface_sampler** out) {
  ApiGuard guard_("rmclhip_surface_sampler_create");
  if (!out) return fail(RMCLHIP_ERR_INVALID, "surface_sampler_create: out is null");
  *out = nullptr;
  if (!map) return fail(RMCLHIP_ERR_INVALID, "surface_sampler_create: null map");
  rmclhip_surface_sample_params p;
  rmclhip_surface_sample_params_default(&p);
  if (params) p = *params;
  if (rmclhip_status st = surface_sample_params_check("surface_sampler_create", &p)) return st;
  if (map->info.n_faces == 0 || map->info.n_records == 0 || !map->d_tris.p) return fail(RMCLHIP_ERR_INVALID, "surface_sampler_create: the map has no faces");
  HIPCHK(hipSetDevice(map->ctx->device));
  rmclhip_surface_sampler* sm = new rmclhip_surface_sampler();
  sm->ctx = map->ctx;
  ctx_retain(sm->ctx);
  sm->map = map;
  (void)rmclhip_map_retain(map);
  sm->params = p;
  sm->info.n_faces = map->info.n_faces;
  rmclhip_status st = surface_sampler_build(sm);
  if (st == RMCLHIP_OK && sm->info.weight_total == 0ull)
    st = fail(RMCLHIP_ERR_INVALID, "surface_sampler_create: no face of the map is eligible with a positive area (min_up_cos, region)");
  if (st != RMCLHIP_OK) {
    const std::string msg = g_err;
    rmclhip_surface_sampler_destroy(sm);
    return fail(st, msg);
  }
  *out = sm;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_surface_sampler_get_info(const rmclhip_surface_sampler* sm, rmclhip_surface_sample_info* out) {
  if (!sm || !out) return fail(RMCLHIP_ERR_INVALID, "surface_sampler_get_info: null");
  *out = sm->info;
  return RMCLHIP_OK;
}

// ---- the injection's launch ---------------------------------------------------------------------------------------
RMCL_INTERNAL rmclhip_status surface_inject_threshold(const std::string& who, double p_inject, unsigned long long* out) {
  if (!(p_inject >= 0.0 && p_inject <= 1.0)) return fail(RMCLHIP_ERR_INVALID, who + ": p_inject outside [0, 1]");
  *out = static_cast<unsigned long long>(std::floor(p_inject * 4294967296.0));
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status surface_inject_enqueue(rmclhip_surface_sampler* sm, xform* poses, void* attrs, uint32_t first, uint32_t count,
                                                    unsigned long long threshold, uint64_t seed, uint32_t step, hipStream_t s) {
  *sm->h_count.p = 0u;
  if (count == 0 || threshold == 0ull) return RMCLHIP_OK;
  HIPCHK(hipMemsetAsync(sm->d_count.p, 0, sizeof(uint32_t), s));
  HIPCHK(launch_particles_inject_surface(poses, attrs, first, count, surface_sample_view(sm), threshold, seed, step, sm->d_count.p, s));
  HIPCHK(hipMemcpyAsync(sm->h_count.p, sm->d_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  return RMCLHIP_OK;
}

// ---- the recovery averages (host, double) ------------------------------------------------------------------------
void rmclhip_recovery_params_default(rmclhip_recovery_params* out) {
  if (out) *out = rmclhip_recovery_params{0.001, 0.1, 1.0};
}

rmclhip_status rmclhip_recovery_update_host(rmclhip_recovery_state* state, const rmclhip_recovery_params* params, double likelihood_sum, uint32_t n,
                                            double* p_inject_out) {
  if (p_inject_out) *p_inject_out = 0.0;
  if (!state || !params) return fail(RMCLHIP_ERR_INVALID, "recovery_update_host: null");
  const double as = params->alpha_slow, af = params->alpha_fast;
  if (!(as > 0.0 && as <= 1.0) || !(af > 0.0 && af <= 1.0)) return fail(RMCLHIP_ERR_INVALID, "recovery_update_host: an alpha outside (0, 1]");
  if (as > af) return fail(RMCLHIP_ERR_INVALID, "recovery_update_host: alpha_slow > alpha_fast");
  if (!(params->p_max >= 0.0 && params->p_max <= 1.0)) return fail(RMCLHIP_ERR_INVALID, "recovery_update_host: p_max outside [0, 1]");
  if (n == 0) return fail(RMCLHIP_ERR_INVALID, "recovery_update_host: no particles");
  if (!std::isfinite(likelihood_sum) || likelihood_sum < 0.0) return fail(RMCLHIP_ERR_INVALID, "recovery_update_host: the likelihood sum is negative or not finite");
  const double avg = likelihood_sum / static_cast<double>(n);
  state->w_slow = (state->w_slow == 0.0) ? avg : state->w_slow + as * (avg - state->w_slow);
  state->w_fast = (state->w_fast == 0.0) ? avg : state->w_fast + af * (avg - state->w_fast);
  double p = 0.0;
  if (state->w_slow > 0.0) {
    p = 1.0 - state->w_fast / state->w_slow;
    if (!(p > 0.0)) p = 0.0;
    if (p > params->p_max) p = params->p_max;
  }
  if (p_inject_out) *p_inject_out = p;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_recovery_reset_host(rmclhip_recovery_state* state) {
  if (!state) return fail(RMCLHIP_ERR_INVALID, "recovery_reset_host: null");
  state->w_slow = 0.0;
  state->w_fast = 0.0;
  return RMCLHIP_OK;
}
