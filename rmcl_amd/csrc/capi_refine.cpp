// capi_refine.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- refinement of particles on the distance field (include/rmclhip.h, REFINE ON THE FIELD, states the arithmetic; kernel: refine.hip) ----
void rmclhip_refine_params_default(rmclhip_refine_params* out) {
  if (!out) return;
  out->iterations = 8u;
  out->dof_mask = 0x3Fu;
  out->max_dist = 0.5f;
  out->max_step_trans = 0.5f;
  out->max_step_rot = 0.25f;
  out->lambda0 = 1e-3f;
}

RMCL_INTERNAL rmclhip_status refine_check(const std::string& who, const void* poses_dev, uint32_t n, const rmclhip_range_measurement* beams, uint32_t n_beams,
                                          const rmclhip_transform* Tsb, const rmclhip_refine_params* params, rmclhip_refine_params* out) {
  rmclhip_refine_params_default(out);
  if (params) *out = *params;
  if (out->iterations > kRefineMaxIterations) return fail(RMCLHIP_ERR_INVALID, who + ": iterations must be at most 64");
  if (out->dof_mask > 0x3Fu) return fail(RMCLHIP_ERR_INVALID, who + ": dof_mask has bits beyond the six degrees of freedom");
  const float positive[4] = {out->max_dist, out->max_step_trans, out->max_step_rot, out->lambda0};
  const char* names[4] = {"max_dist", "max_step_trans", "max_step_rot", "lambda0"};
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(positive[k]) || !(positive[k] > 0.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": " + names[k] + " must be finite and > 0");
  if (n == 0u) return RMCLHIP_OK;
  if (!poses_dev || !beams || !Tsb) return fail(RMCLHIP_ERR_INVALID, who + ": null buffers");
  if (n_beams == 0u || n_beams > kRefineMaxBeams) return fail(RMCLHIP_ERR_INVALID, who + ": n_beams must be 1..8192");
  return RMCLHIP_OK;
}

RMCL_INTERNAL RefineKernelParams refine_kernel_params(const rmclhip_field* field, rmclhip_transform* poses_dev, uint32_t n, const float* beams_dev,
                                                      uint32_t n_beams, const rmclhip_transform* Tsb, const rmclhip_refine_params& params) {
  RefineKernelParams p;
  std::memset(&p, 0, sizeof(p));
  p.fv = field_view(field);
  p.poses = reinterpret_cast<xform*>(poses_dev);
  p.n_particles = n;
  p.beams = beams_dev;
  p.n_beams = n_beams;
  p.Tsb = to_x(Tsb);
  p.iterations = params.iterations;
  p.dof_mask = params.dof_mask;
  p.max_dist = params.max_dist;
  p.max_step_trans = params.max_step_trans;
  p.max_step_rot = params.max_step_rot;
  p.lambda0 = params.lambda0;
  return p;
}

RMCL_INTERNAL rmclhip_status refine_enqueue(const rmclhip_field* field, hipStream_t stream, RefineScratch& sc, rmclhip_transform* poses_dev, uint32_t n,
                                            const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                            const rmclhip_refine_params& params, rmclhip_refine_result* results_dev, bool want_stats) {
  static_assert(sizeof(rmclhip_range_measurement) == 16 * sizeof(float), "a beam record is 16 floats");
  static_assert(sizeof(rmclhip_refine_result) == 16, "a result row is 16 bytes");
  const size_t nf = static_cast<size_t>(n_beams) * 16u;
  HIPCHK(sc.beams.reserve(nf));
  HIPCHK(sc.counters.reserve(4u));
  uint32_t* rows = reinterpret_cast<uint32_t*>(results_dev);
  if (!rows && want_stats) {
    HIPCHK(sc.rows.reserve(4u * static_cast<size_t>(n)));
    rows = sc.rows.p;
  }
  sc.rows_src = rows;
  // the beams come from pageable host memory: wait for the copy, the caller may reuse them when this returns
  HIPCHK(upload_on(stream, sc.beams.p, beams, nf * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(sc.counters.p, 0, 4u * sizeof(uint32_t), stream));
  RefineKernelParams p = refine_kernel_params(field, poses_dev, n, sc.beams.p, n_beams, Tsb, params);
  p.rows = rows;
  p.counters = sc.counters.p;
  HIPCHK(launch_field_refine(p, stream));
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status refine_finish(hipStream_t stream, RefineScratch& sc, uint32_t n, rmclhip_refine_stats* stats) {
  if (!stats) {
    HIPCHK(hipStreamSynchronize(stream));
    return RMCLHIP_OK;
  }
  uint32_t counts[4] = {0u, 0u, 0u, 0u};
  std::vector<rmclhip_refine_result> rows(n);
  HIPCHK(hipMemcpyAsync(counts, sc.counters.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
  HIPCHK(upload_on(stream, rows.data(), sc.rows_src, static_cast<size_t>(n) * sizeof(rmclhip_refine_result), hipMemcpyDeviceToHost));
  stats->n_particles += n;
  stats->n_moved += counts[0];
  stats->n_no_beams += counts[1];
  stats->n_not_finite += counts[2];
  double before = 0.0, after = 0.0;
  for (uint32_t i = 0; i < n; ++i) { before += static_cast<double>(rows[i].cost_before); after += static_cast<double>(rows[i].cost_after); }
  stats->cost_before_sum += before;
  stats->cost_after_sum += after;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_refine(rmclhip_field* field, rmclhip_transform* poses_dev, uint32_t n_particles,
                                    const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                    const rmclhip_refine_params* params, rmclhip_refine_result* results_dev, rmclhip_refine_stats* stats_out) {
  ApiGuard guard_("rmclhip_field_refine");
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!field) return fail(RMCLHIP_ERR_INVALID, "field_refine: null");
  rmclhip_refine_params p;
  if (rmclhip_status st = refine_check("field_refine", poses_dev, n_particles, beams, n_beams, Tsb, params, &p)) return st;
  if (rmclhip_status st = field_band_check("field_refine", field, p.max_dist)) return st;
  if (n_particles == 0u) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(field->ctx->device));
  std::lock_guard<std::mutex> lock(field->mtx);
  if (rmclhip_status st = refine_enqueue(field, field->stream, field->refine, poses_dev, n_particles, beams, n_beams, Tsb, p, results_dev, stats_out != nullptr))
    return st;
  return refine_finish(field->stream, field->refine, n_particles, stats_out);
}

rmclhip_status rmclhip_pf_refine(rmclhip_pf* f, rmclhip_transform* poses_dev, uint32_t n_particles, const rmclhip_range_measurement* beams,
                                 uint32_t n_beams, const rmclhip_transform* Tsb, const rmclhip_refine_params* params,
                                 rmclhip_refine_result* results_dev, rmclhip_refine_stats* stats_out) {
  ApiGuard guard_("rmclhip_pf_refine");
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!f) return fail(RMCLHIP_ERR_INVALID, "pf_refine: null");
  if (!f->field) return fail(RMCLHIP_ERR_INVALID, "pf_refine: no distance field is set (rmclhip_pf_set_field)");
  rmclhip_refine_params p;
  if (rmclhip_status st = refine_check("pf_refine", poses_dev, n_particles, beams, n_beams, Tsb, params, &p)) return st;
  if (rmclhip_status st = field_band_check("pf_refine", f->field, p.max_dist)) return st;
  if (n_particles == 0u) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(f->ctx->device));
  if (rmclhip_status st = refine_enqueue(f->field, f->stream, f->refine, poses_dev, n_particles, beams, n_beams, Tsb, p, results_dev, stats_out != nullptr))
    return st;
  return refine_finish(f->stream, f->refine, n_particles, stats_out);
}
