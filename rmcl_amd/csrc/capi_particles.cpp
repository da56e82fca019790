// capi_particles.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- the covariance factor of the pose initialisation (host) ------------------------------------------
// rm::chol as RmclNode::initSamples uses it (rmcl_localization.cpp:187-195), made total on what callers send: RViz's /initialpose
// covariance has zero rows for z, roll and pitch, so a positive SEMIdefinite matrix is the normal input.  Column by column
// (Cholesky-Banachiewicz) in double on the symmetrised matrix; a pivot within +-tol of zero gives a zero column, one below -tol is
// refused.  Every operation in the order tests/particle_init_ref.py restates.
rmclhip_status rmclhip_chol6_host(const double* C, float* L_out, double* err_out) {
  ApiGuard guard_("rmclhip_chol6_host");
  if (err_out) *err_out = 0.0;
  if (!C || !L_out) return fail(RMCLHIP_ERR_INVALID, "chol6_host: null");
  for (int k = 0; k < 36; ++k)
    if (!std::isfinite(C[k])) return fail(RMCLHIP_ERR_INVALID, "chol6_host: covariance has a non-finite entry");
  double A[6][6], L[6][6];
  double max_diag = 0.0;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) { A[r][c] = (C[6 * r + c] + C[6 * c + r]) / 2.0; L[r][c] = 0.0; }
  for (int j = 0; j < 6; ++j) max_diag = std::max(max_diag, std::fabs(A[j][j]));
  const double tol = (36.0 / 16777216.0) * max_diag;   // 36 * 2^-24 * max |C_jj|: the factor leaves as float
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (d < -tol) return fail(RMCLHIP_ERR_INVALID, "chol6_host: covariance is not positive semidefinite");
    if (d <= tol) continue;   // a direction without variance: column j stays zero
    const double ljj = std::sqrt(d);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / ljj;
    }
  }
  float Lf[36];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      Lf[6 * r + c] = static_cast<float>(L[r][c]);
      if (!std::isfinite(Lf[6 * r + c])) return fail(RMCLHIP_ERR_INVALID, "chol6_host: the factor does not fit float");
    }
  // "Cholesky Err" (:195): abssum(L L^T - C) / 36 of the float factor the kernel uses
  double err = 0.0;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s = s + static_cast<double>(Lf[6 * r + k]) * static_cast<double>(Lf[6 * c + k]);
      err = err + std::fabs(s - A[r][c]);
    }
  std::memcpy(L_out, Lf, sizeof(Lf));
  if (err_out) *err_out = err / 36.0;
  return RMCLHIP_OK;
}

// ---- argument checks shared with the sharded entry points (capi_pf_sharded.cpp) -------------------------
RMCL_INTERNAL rmclhip_status particles_range_check(const std::string& who, uint32_t first, uint32_t count) {
  if (static_cast<uint64_t>(first) + count > (1ull << 32)) return fail(RMCLHIP_ERR_INVALID, who + ": first + count exceeds 2^32 (the particle index is a 32-bit counter word)");
  if (count > kMaxInitCount) return fail(RMCLHIP_ERR_UNSUPPORTED, who + ": more than 2^32 / 9 particles in one call");
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status particles_uniform_check(const char* who_, uint32_t first, uint32_t count, const float* bb_min, const float* bb_max) {
  const std::string who(who_);
  if (!bb_min || !bb_max) return fail(RMCLHIP_ERR_INVALID, who + ": null bounds");
  for (int d = 0; d < 6; ++d) {
    if (!std::isfinite(bb_min[d]) || !std::isfinite(bb_max[d])) return fail(RMCLHIP_ERR_INVALID, who + ": non-finite bound");
    if (bb_min[d] > bb_max[d]) return fail(RMCLHIP_ERR_INVALID, who + ": bb_min > bb_max");
  }
  return particles_range_check(who, first, count);
}

RMCL_INTERNAL rmclhip_status particles_pose_check(const char* who_, uint32_t first, uint32_t count, const rmclhip_transform* Tlm, const double* covariance,
                                                  ParticlesPoseJob* job) {
  const std::string who(who_);
  if (!Tlm || !covariance) return fail(RMCLHIP_ERR_INVALID, who + ": null pose or covariance");
  const float p7[7] = {Tlm->R.x, Tlm->R.y, Tlm->R.z, Tlm->R.w, Tlm->t.x, Tlm->t.y, Tlm->t.z};
  for (float v : p7)
    if (!std::isfinite(v)) return fail(RMCLHIP_ERR_INVALID, who + ": non-finite pose");
  if (rmclhip_status st = particles_range_check(who, first, count)) return st;
  if (rmclhip_status st = rmclhip_chol6_host(covariance, job->L, &job->chol_err)) return fail(st, who + ": " + g_err);
  job->Tlm = to_x(Tlm);
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status particles_stream(rmclhip_ctx* ctx) {   // under ctx->part_mtx
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->part_stream == nullptr) HIPCHK(hipStreamCreateWithFlags(&ctx->part_stream, hipStreamNonBlocking));
  return RMCLHIP_OK;
}

// rmclhip_debug_particles_timing: the two events around what a call enqueues (under ctx->part_mtx, after particles_stream)
static hipError_t bracket_begin(rmclhip_ctx* ctx) { return ctx->part_timing ? hipEventRecord(ctx->part_ev0, ctx->part_stream) : hipSuccess; }
static hipError_t bracket_end_and_wait(rmclhip_ctx* ctx) {
  if (!ctx->part_timing) return hipStreamSynchronize(ctx->part_stream);
  hipError_t e = hipEventRecord(ctx->part_ev1, ctx->part_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->part_stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&ctx->part_last_ms, ctx->part_ev0, ctx->part_ev1);
  return e;
}

rmclhip_status rmclhip_debug_particles_timing(rmclhip_ctx* ctx, int on, float* last_ms) {
  ApiGuard guard_("rmclhip_debug_particles_timing");
  if (!ctx) return fail(RMCLHIP_ERR_INVALID, "debug_particles_timing: null context");
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (last_ms) *last_ms = ctx->part_last_ms;
  if (on && !ctx->part_ev0) {
    if (rmclhip_status st = particles_stream(ctx)) return st;
    HIPCHK(hipEventCreate(&ctx->part_ev0));
    HIPCHK(hipEventCreate(&ctx->part_ev1));
  }
  ctx->part_timing = on != 0 && ctx->part_ev0 && ctx->part_ev1;
  return RMCLHIP_OK;
}

// ---- RmclNode::initSamplesUniform ------------------------------------------------------------------------
rmclhip_status rmclhip_particles_init_uniform(rmclhip_ctx* ctx, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                              uint32_t first, uint32_t count, const float* bb_min, const float* bb_max, uint64_t seed,
                                              uint32_t epoch) {
  ApiGuard guard_("rmclhip_particles_init_uniform");
  if (!ctx) return fail(RMCLHIP_ERR_INVALID, "particles_init_uniform: null context");
  if (count == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, "particles_init_uniform: null particle buffers");
  if (rmclhip_status st = particles_uniform_check("particles_init_uniform", first, count, bb_min, bb_max)) return st;
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (rmclhip_status st = particles_stream(ctx)) return st;
  HIPCHK(bracket_begin(ctx));
  HIPCHK(launch_particles_init_uniform(reinterpret_cast<xform*>(poses_dev), attrs_dev, first, count, bb_min, bb_max, seed, epoch, ctx->part_stream));
  HIPCHK(bracket_end_and_wait(ctx));
  return RMCLHIP_OK;
}

// ---- RmclNode::initSamples(PoseWithCovarianceStamped) --------------------------------------------------
rmclhip_status rmclhip_particles_init_pose(rmclhip_ctx* ctx, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                           uint32_t first, uint32_t count, const rmclhip_transform* Tlm, const double* covariance,
                                           uint64_t seed, uint32_t epoch, double* chol_err_out) {
  ApiGuard guard_("rmclhip_particles_init_pose");
  if (chol_err_out) *chol_err_out = 0.0;
  if (!ctx) return fail(RMCLHIP_ERR_INVALID, "particles_init_pose: null context");
  if (count == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, "particles_init_pose: null particle buffers");
  ParticlesPoseJob job;
  if (rmclhip_status st = particles_pose_check("particles_init_pose", first, count, Tlm, covariance, &job)) return st;
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (rmclhip_status st = particles_stream(ctx)) return st;
  HIPCHK(bracket_begin(ctx));
  HIPCHK(launch_particles_init_pose(reinterpret_cast<xform*>(poses_dev), attrs_dev, first, count, job.Tlm, job.L, seed, epoch, ctx->part_stream));
  HIPCHK(bracket_end_and_wait(ctx));
  if (chol_err_out) *chol_err_out = job.chol_err;
  return RMCLHIP_OK;
}

// ---- on the surface: the initialisation and the recovery injection (the sampler: capi_surface_sample.cpp) ----
static rmclhip_status surface_call_check(const std::string& who, const void* poses_dev, const void* attrs_dev, uint32_t first, uint32_t count) {
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, who + ": null particle buffers");
  return particles_range_check(who, first, count);
}

rmclhip_status rmclhip_particles_init_surface(rmclhip_surface_sampler* sm, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                              uint32_t first, uint32_t count, uint64_t seed, uint32_t epoch) {
  ApiGuard guard_("rmclhip_particles_init_surface");
  if (!sm) return fail(RMCLHIP_ERR_INVALID, "particles_init_surface: null sampler");
  if (count == 0) return RMCLHIP_OK;
  if (rmclhip_status st = surface_call_check("particles_init_surface", poses_dev, attrs_dev, first, count)) return st;
  rmclhip_ctx* ctx = sm->ctx;
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (rmclhip_status st = particles_stream(ctx)) return st;
  HIPCHK(bracket_begin(ctx));
  HIPCHK(launch_particles_init_surface(reinterpret_cast<xform*>(poses_dev), attrs_dev, first, count, surface_sample_view(sm), seed, epoch,
                                       ctx->part_stream));
  HIPCHK(bracket_end_and_wait(ctx));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_particles_inject_surface(rmclhip_surface_sampler* sm, rmclhip_transform* poses_dev, rmclhip_particle_attributes* attrs_dev,
                                                uint32_t first, uint32_t count, double p_inject, uint64_t seed, uint32_t step,
                                                uint32_t* n_injected_out) {
  ApiGuard guard_("rmclhip_particles_inject_surface");
  if (n_injected_out) *n_injected_out = 0u;
  if (!sm) return fail(RMCLHIP_ERR_INVALID, "particles_inject_surface: null sampler");
  unsigned long long threshold = 0ull;
  if (rmclhip_status st = surface_inject_threshold("particles_inject_surface", p_inject, &threshold)) return st;
  if (count == 0) return RMCLHIP_OK;
  if (rmclhip_status st = surface_call_check("particles_inject_surface", poses_dev, attrs_dev, first, count)) return st;
  if (threshold == 0ull) return RMCLHIP_OK;
  rmclhip_ctx* ctx = sm->ctx;
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (rmclhip_status st = particles_stream(ctx)) return st;
  HIPCHK(bracket_begin(ctx));
  if (rmclhip_status st = surface_inject_enqueue(sm, reinterpret_cast<xform*>(poses_dev), attrs_dev, first, count, threshold, seed, step, ctx->part_stream))
    return st;
  HIPCHK(bracket_end_and_wait(ctx));
  if (n_injected_out) *n_injected_out = *sm->h_count.p;
  return RMCLHIP_OK;
}

// ---- RmclNode::visualize -----------------------------------------------------------------------------------
rmclhip_status rmclhip_particles_pack_visualization(rmclhip_ctx* ctx, const rmclhip_transform* poses_dev,
                                                    const rmclhip_particle_attributes* attrs_dev, uint32_t n, uint32_t max_n_meas, float* out,
                                                    int out_is_device) {
  ApiGuard guard_("rmclhip_particles_pack_visualization");
  if (!ctx) return fail(RMCLHIP_ERR_INVALID, "particles_pack_visualization: null context");
  if (max_n_meas == 0) return fail(RMCLHIP_ERR_INVALID, "particles_pack_visualization: max_n_meas must be > 0");
  if (n == 0) return RMCLHIP_OK;
  if (!poses_dev || !attrs_dev || !out) return fail(RMCLHIP_ERR_INVALID, "particles_pack_visualization: null buffers");
  std::lock_guard<std::mutex> lock(ctx->part_mtx);
  if (rmclhip_status st = particles_stream(ctx)) return st;
  const size_t nf = static_cast<size_t>(n) * 7u;
  float* dst = out;
  if (!out_is_device) {
    const hipError_t re = ctx->part_viz.reserve(nf);
    if (re == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(RMCLHIP_ERR_NOMEM, "particles_pack_visualization: no device memory for the staging buffer"); }
    HIPCHK(re);
    dst = ctx->part_viz.p;
  }
  HIPCHK(bracket_begin(ctx));
  HIPCHK(launch_particles_pack_visualization(reinterpret_cast<const xform*>(poses_dev), attrs_dev, n, max_n_meas, dst, ctx->part_stream));
  if (!out_is_device) HIPCHK(hipMemcpyAsync(out, dst, nf * sizeof(float), hipMemcpyDeviceToHost, ctx->part_stream));
  HIPCHK(bracket_end_and_wait(ctx));
  return RMCLHIP_OK;
}
