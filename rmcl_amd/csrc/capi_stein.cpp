// capi_stein.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- the Stein variational step on a filter handle's field (include/rmclhip.h, STEIN STEP ON THE FIELD, states the arithmetic; kernels: stein.hip) ----
void rmclhip_stein_params_default(rmclhip_stein_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  rmclhip_refine_params r;
  rmclhip_refine_params_default(&r);
  out->iterations = 1u;
  out->dof_mask = r.dof_mask;
  out->max_dist = r.max_dist;
  out->max_step_trans = r.max_step_trans;
  out->max_step_rot = r.max_step_rot;
  out->lambda0 = r.lambda0;
  out->h_trans = 0.25f;
  out->h_rot = 0.2f;
  out->repulsion = 0.25f;
  out->max_per_bin = 256u;
}

static rmclhip_status stein_check(const rmclhip_stein_params& p, uint32_t n) {
  const std::string who = "pf_stein_step";
  if (!(p.max_step_trans <= 16.0f) || !(p.max_step_rot <= 16.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": max_step_trans and max_step_rot must be at most 16");
  if (!std::isfinite(p.h_trans) || !(p.h_trans > 0.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": h_trans must be finite and > 0");
  if (!std::isfinite(p.h_rot) || !(p.h_rot > 0.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": h_rot must be finite and > 0");
  if (!std::isfinite(p.repulsion) || !(p.repulsion >= 0.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": repulsion must be finite and >= 0");
  if (p.max_per_bin == 0u) return fail(RMCLHIP_ERR_INVALID, who + ": max_per_bin must be at least 1");
  if (n > kSteinMaxParticles) return fail(RMCLHIP_ERR_INVALID, who + ": at most 2^26 particles");
  return RMCLHIP_OK;
}

static rmclhip_status stein_timing_events(rmclhip_pf* f) {
  for (hipEvent_t& e : f->stein.events)
    if (!e) HIPCHK(hipEventCreate(&e));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_stein_step(rmclhip_pf* f, rmclhip_transform* poses_dev, uint32_t n, const rmclhip_range_measurement* beams, uint32_t n_beams,
                                     const rmclhip_transform* Tsb, const rmclhip_stein_params* params, rmclhip_stein_result* results_dev,
                                     rmclhip_stein_stats* stats_out) {
  ApiGuard guard_("rmclhip_pf_stein_step");
  static_assert(sizeof(rmclhip_stein_result) == 16, "a result row is 16 bytes");
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!f) return fail(RMCLHIP_ERR_INVALID, "pf_stein_step: null");
  if (!f->field) return fail(RMCLHIP_ERR_INVALID, "pf_stein_step: no distance field is set (rmclhip_pf_set_field)");
  rmclhip_stein_params p;
  rmclhip_stein_params_default(&p);
  if (params) p = *params;
  const rmclhip_refine_params as_refine = {p.iterations, p.dof_mask, p.max_dist, p.max_step_trans, p.max_step_rot, p.lambda0};
  rmclhip_refine_params rp;
  // the parameters refine has too, then this call's own, then (n > 0) the buffers and the beams
  if (rmclhip_status st = refine_check("pf_stein_step", nullptr, 0u, nullptr, 0u, nullptr, &as_refine, &rp)) return st;
  if (rmclhip_status st = stein_check(p, n)) return st;
  if (rmclhip_status st = field_band_check("pf_stein_step", f->field, p.max_dist)) return st;
  if (rmclhip_status st = refine_check("pf_stein_step", poses_dev, n, beams, n_beams, Tsb, &as_refine, &rp)) return st;
  if (n == 0u) return RMCLHIP_OK;
  if (stats_out) stats_out->n_particles = n;
  if (p.iterations == 0u) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(f->ctx->device));
  SteinScratch& sc = f->stein;
  const uint64_t words = kld_table_words(n);
  const size_t nf = static_cast<size_t>(n_beams) * 16u;
  HIPCHK(f->refine.beams.reserve(nf));
  HIPCHK(sc.table.reserve(words));
  HIPCHK(sc.incl.reserve(words));
  HIPCHK(sc.block_tot.reserve((words + 1023u) / 1024u));
  HIPCHK(sc.words3.reserve(3u * words));
  HIPCHK(sc.slot_of.reserve(n));
  HIPCHK(sc.records.reserve(static_cast<size_t>(kSteinRecordWords) * n));
  HIPCHK(sc.drive.reserve(static_cast<size_t>(kSteinDriveStride) * n));
  HIPCHK(sc.counters.reserve(kSteinCounters));
  uint32_t* rows = reinterpret_cast<uint32_t*>(results_dev);
  if (!rows && stats_out) {
    HIPCHK(sc.rows.reserve(4u * static_cast<size_t>(n)));
    rows = sc.rows.p;
  }
  if (sc.timing) { if (rmclhip_status st = stein_timing_events(f)) return st; }
  // the beams come from pageable host memory: wait for the copy, the caller may reuse them when this returns
  HIPCHK(upload_on(f->stream, f->refine.beams.p, beams, nf * sizeof(float), hipMemcpyHostToDevice));
  SteinKernelParams k;
  std::memset(&k, 0, sizeof(k));
  k.r = refine_kernel_params(f->field, poses_dev, n, f->refine.beams.p, n_beams, Tsb, rp);
  k.r.iterations = 1u;   // of the refinement's arithmetic per launch; p.iterations is the loop below
  k.h_trans = p.h_trans;
  k.h_rot = p.h_rot;
  k.repulsion = p.repulsion;
  k.max_per_bin = p.max_per_bin;
  k.key0 = static_cast<uint32_t>(p.seed);
  k.key1 = static_cast<uint32_t>(p.seed >> 32);
  k.table = sc.table.p;
  k.table_words = words;
  k.incl = sc.incl.p;
  k.block_tot = sc.block_tot.p;
  k.count = sc.words3.p;
  k.listed = sc.words3.p + words;
  k.cursor = sc.words3.p + 2u * words;
  k.slot_of = sc.slot_of.p;
  k.drive = sc.drive.p;
  k.records = sc.records.p;
  k.counters = sc.counters.p;
  k.rows = rows;
  for (uint32_t it = 0; it < p.iterations; ++it) {
    k.step = p.step + it;
    // the events bracket the phases of the last iteration
    HIPCHK(launch_stein_iteration(k, f->stream, (sc.timing && it + 1u == p.iterations) ? sc.events : nullptr));
  }
  if (!stats_out) {
    HIPCHK(hipStreamSynchronize(f->stream));
  } else {
    uint32_t counts[kSteinCounters] = {0u, 0u, 0u, 0u};
    std::vector<rmclhip_stein_result> host_rows(n);
    HIPCHK(hipMemcpyAsync(counts, sc.counters.p, sizeof(counts), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(upload_on(f->stream, host_rows.data(), rows, static_cast<size_t>(n) * sizeof(rmclhip_stein_result), hipMemcpyDeviceToHost));
    stats_out->n_not_finite = counts[0];
    stats_out->n_no_beams = counts[1];
    stats_out->n_bins = counts[2];
    stats_out->n_thinned_bins = counts[3];
    double sum = 0.0;
    for (uint32_t i = 0; i < n; ++i) sum += static_cast<double>(host_rows[i].cost);
    stats_out->cost_sum = sum;
  }
  if (sc.timing)
    for (uint32_t ph = 0; ph + 1u < kSteinEvents; ++ph) HIPCHK(hipEventElapsedTime(&sc.last_ms[ph], sc.events[ph], sc.events[ph + 1u]));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_debug_stein_timing(rmclhip_pf* f, int on, float* last_ms3) {
  ApiGuard guard_("rmclhip_debug_stein_timing");
  if (!f) return fail(RMCLHIP_ERR_INVALID, "debug_stein_timing: null");
  if (last_ms3)
    for (uint32_t ph = 0; ph + 1u < kSteinEvents; ++ph) last_ms3[ph] = f->stein.last_ms[ph];
  f->stein.timing = on != 0;
  return RMCLHIP_OK;
}
