// capi_robust.cpp -- ROBUST MICP of include/rmclhip.h: M-estimator weights in the point-to-plane reduction (kernels: robust.hip; the
// weight, the defaults and the parameter check: robust_host.h) as a free function on caller-owned views, over an operator's last find,
// and as the device-resident IRLS correction of one sensor.  The forms that only read a find's buffers (statistics, weights, scale) touch
// neither the operator's published moments nor its ccs_info; the correction runs a find, which drops the moment set as every find does.
// The same for a rig of up to 8 sensors (rmclhip_micp_correct_once_robust) and the pose information with the weights.
#include "capi_internal.h"
#include "robust_host.h"

static_assert(sizeof(rmclhip_robust_params) == 24, "RobustParams layout");
static_assert(sizeof(rmclhip_robust_statistics) == 96 && sizeof(RobustStats) == sizeof(rmclhip_robust_statistics), "RobustStatistics layout");

namespace {

std::atomic<int> g_select_recompute{0};   // rmclhip_debug_robust_select_recompute

rmclhip_status params_check(const char* who, const rmclhip_robust_params* p) {
  if (!p) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": null params");
  if (const char* msg = robust_params_error(p)) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": " + msg);
  return RMCLHIP_OK;
}

RobustScaleParams scale_params(const rmclhip_robust_params* p) {
  RobustScaleParams sp;
  sp.mode = p->scale_mode; sp.scale = p->scale; sp.tuning = p->tuning; sp.scale_min = p->scale_min;
  return sp;
}

void identity_statistics(const rmclhip_robust_params* p, rmclhip_robust_statistics* out) {
  std::memset(out, 0, sizeof(*out));
  from_cs(cs_identity(), &out->stats);
  out->scale = (p->scale_mode == RMCLHIP_ROBUST_SCALE_MAD) ? p->scale_min : p->scale;
}

rmclhip_status reserve(RobustScratch& sc, uint32_t n, uint32_t nb) {
  HIPCHK(sc.partials.reserve(2u * static_cast<size_t>(nb) * kRobustRow));
  HIPCHK(sc.sel.reserve(kRobustSelWords));
  HIPCHK(sc.keys.reserve(n));
  HIPCHK(sc.dev.reserve(1));
  HIPCHK(sc.out.reserve(1));
  return RMCLHIP_OK;
}

// the scale of `params` at Tpre into the scratch's device block: a selection (MAD, or whoever wants the count m), else c by value
rmclhip_status scale_enqueue(RobustScratch& sc, const RobustView& v, const xform& Tpre, const rmclhip_robust_params* params, bool want_m,
                             hipStream_t stream) {
  if (params->scale_mode == RMCLHIP_ROBUST_SCALE_MAD || want_m)
    HIPCHK(launch_robust_scale(v, Tpre, scale_params(params), sc.sel.p, g_select_recompute.load() ? nullptr : sc.keys.p, &sc.dev.p->scale,
                               want_m ? &sc.out.d->scale : nullptr, stream));
  else
    HIPCHK(launch_robust_fixed_scale(params->scale, &sc.dev.p->scale, stream));
  return RMCLHIP_OK;
}

// scale + one weighted reduction on `stream`, which the call waits for: the last launch wrote the result into host-mapped memory
rmclhip_status run_statistics(RobustScratch& sc, hipStream_t stream, const RobustView& v, const xform& Tpre, const rmclhip_robust_params* params,
                              float* weights_dev, rmclhip_robust_statistics* out) {
  const uint32_t nb = reduce_num_blocks(v.n, 1);
  if (rmclhip_status st = reserve(sc, v.n, nb)) return st;
  if (rmclhip_status st = scale_enqueue(sc, v, Tpre, params, false, stream)) return st;
  HIPCHK(launch_robust_statistics(v, Tpre, &sc.dev.p->scale, sc.partials.p, nb, weights_dev, &sc.out.d->stats, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (out) std::memcpy(out, &sc.out.h->stats, sizeof(*out));
  return RMCLHIP_OK;
}

// what the operator forms check, and the view of the last find's correspondences at max_dist'
rmclhip_status rcc_view(const char* who, rmclhip_rcc* r, double convergence_progress, const rmclhip_robust_params* params, RobustView* v) {
  if (r->nposes_last == 0 || r->n_model == 0) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": no find has run");
  if (r->nposes_last > 1) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": last find was a batch");
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  const uint32_t n = nred_of(r);
  if (n == 0) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": empty dataset");
  v->dataset_points = r->ds_pts;
  v->dataset_mask = r->ds_has_mask ? r->ds_msk : nullptr;
  v->model_points = r->d_points.p;
  v->model_normals = r->d_normals.p;
  v->model_mask = r->d_hits.p;
  v->n = n;
  v->max_dist = adaptive_max_dist(r, convergence_progress);
  v->kernel = params->kernel;
  return RMCLHIP_OK;
}

// rmclhip_rcc_correct_once_robust behind its checks (the rig call with one sensor runs it as well)
rmclhip_status correct_once_robust_run(rmclhip_rcc* r, const rmclhip_transform* Tom_, const rmclhip_transform* Tbo_, uint32_t n_iter,
                                       double convergence_progress, const rmclhip_robust_params* params, rmclhip_transform* T_out,
                                       rmclhip_robust_statistics* stats_out) {
  HIPCHK(hipSetDevice(r->ctx->device));
  const xform Tbo = to_x(Tbo_);
  // (1) the find at Tom * Tbo, a plain one: no moment epilogue, no speculation, ccs_info untouched.  ensure_model_buffers drops the
  // published moment set, as for every find: it described the buffers this find rewrites
  const size_t nm = static_cast<size_t>(r->W) * r->H;
  r->n_model = static_cast<uint32_t>(nm);
  r->nposes_last = 1;
  if (rmclhip_status st = ensure_model_buffers(r, nm)) return st;
  RobustView v;
  if (rmclhip_status st = rcc_view("correct_once_robust", r, convergence_progress, params, &v)) return st;
  const uint32_t nb = reduce_num_blocks(v.n, 1);
  if (rmclhip_status st = reserve(r->robust, v.n, nb)) return st;
  FindParams fp;
  fill_find_params(r, fp, 1);
  fp.Tsm = xmul(xmul(to_x(Tom_), Tbo), r->Tsb);
  fp.Tms = xinv(fp.Tsm);
  HIPCHK(launch_find(fp, r->kind, find_variant(r, 1), r->stream));
  if (n_iter == 0) {
    HIPCHK(hipStreamSynchronize(r->stream));
    from_x(xidentity(), T_out);
    if (stats_out) identity_statistics(params, stats_out);
    return RMCLHIP_OK;
  }
  // (2) the scale, once, at the identity pre-transform; (3) the iterations; one synchronisation
  if (rmclhip_status st = scale_enqueue(r->robust, v, xidentity(), params, false, r->stream)) return st;
  RobustDevBlock* d = r->robust.dev.p;
  HIPCHK(launch_robust_loop(v, &d->scale, r->robust.partials.p, nb, d->state, n_iter, r->Tsb, Tbo, &r->robust.out.d->loop, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  from_x(r->robust.out.h->loop.T_onew_oold, T_out);
  if (stats_out) std::memcpy(stats_out, &r->robust.out.h->loop.stats, sizeof(*stats_out));
  return RMCLHIP_OK;
}

}  // namespace

extern "C" {

void rmclhip_robust_params_default(int kernel, rmclhip_robust_params* out) {
  if (out) robust_params_default(kernel, out);
}

rmclhip_status rmclhip_robust_params_check(const rmclhip_robust_params* params) { return params_check("robust_params_check", params); }

float rmclhip_robust_weight_host(int kernel, float c, float r) { return robust_weight(kernel, c, r); }

rmclhip_status rmclhip_debug_robust_select_recompute(int on) {
  g_select_recompute.store(on != 0 ? 1 : 0);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_statistics_p2l_robust(rmclhip_ctx* ctx, const rmclhip_transform* Tpre, const float* dataset_points,
                                             const uint8_t* dataset_mask, const float* model_points, const float* model_normals,
                                             const uint8_t* model_mask, uint32_t n, float max_dist, const rmclhip_robust_params* params,
                                             float* weights_out_dev, rmclhip_robust_statistics* out) {
  ApiGuard guard_("rmclhip_statistics_p2l_robust");
  if (!ctx || !Tpre || !out) return fail(RMCLHIP_ERR_INVALID, "statistics_p2l_robust: null");
  if (rmclhip_status st = params_check("statistics_p2l_robust", params)) return st;
  if (n == 0) { identity_statistics(params, out); return RMCLHIP_OK; }
  if (!dataset_points || !model_points || !model_normals) return fail(RMCLHIP_ERR_INVALID, "statistics_p2l_robust: null view");
  std::lock_guard<std::mutex> lock(ctx->p2l_mtx);
  HIPCHK(hipSetDevice(ctx->device));
  if (rmclhip_status st = ctx_p2l_ensure(ctx)) return st;
  RobustView v;
  v.dataset_points = dataset_points; v.dataset_mask = dataset_mask;
  v.model_points = model_points; v.model_normals = model_normals; v.model_mask = model_mask;
  v.n = n; v.max_dist = max_dist; v.kernel = params->kernel;
  return run_statistics(ctx->robust, ctx->p2l_stream, v, to_x(Tpre), params, weights_out_dev, out);
}

rmclhip_status rmclhip_rcc_compute_robust_statistics(rmclhip_rcc* r, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                                     const rmclhip_robust_params* params, rmclhip_robust_statistics* out) {
  ApiGuard guard_("rmclhip_rcc_compute_robust_statistics");
  if (!r || !T_snew_sold || !out) return fail(RMCLHIP_ERR_INVALID, "rcc_compute_robust_statistics: null");
  if (rmclhip_status st = params_check("rcc_compute_robust_statistics", params)) return st;
  RobustView v;
  if (rmclhip_status st = rcc_view("rcc_compute_robust_statistics", r, convergence_progress, params, &v)) return st;
  HIPCHK(hipSetDevice(r->ctx->device));
  return run_statistics(r->robust, r->stream, v, to_x(T_snew_sold), params, nullptr, out);
}

rmclhip_status rmclhip_rcc_robust_weights(rmclhip_rcc* r, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                          const rmclhip_robust_params* params, float* weights_out, int on_device) {
  ApiGuard guard_("rmclhip_rcc_robust_weights");
  if (!r || !T_snew_sold || !weights_out) return fail(RMCLHIP_ERR_INVALID, "rcc_robust_weights: null");
  if (rmclhip_status st = params_check("rcc_robust_weights", params)) return st;
  RobustView v;
  if (rmclhip_status st = rcc_view("rcc_robust_weights", r, convergence_progress, params, &v)) return st;
  HIPCHK(hipSetDevice(r->ctx->device));
  float* dst = weights_out;
  if (!on_device) {
    HIPCHK(r->robust.weights.reserve(v.n));
    dst = r->robust.weights.p;
  }
  if (rmclhip_status st = run_statistics(r->robust, r->stream, v, to_x(T_snew_sold), params, dst, nullptr)) return st;
  if (!on_device) HIPCHK(upload_on(r->stream, weights_out, dst, static_cast<size_t>(v.n) * sizeof(float), hipMemcpyDeviceToHost));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_residual_scale(rmclhip_rcc* r, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                          const rmclhip_robust_params* params, float* c_out, float* median_out, uint32_t* m_out) {
  ApiGuard guard_("rmclhip_rcc_residual_scale");
  if (!r || !T_snew_sold) return fail(RMCLHIP_ERR_INVALID, "rcc_residual_scale: null");
  if (rmclhip_status st = params_check("rcc_residual_scale", params)) return st;
  RobustView v;
  if (rmclhip_status st = rcc_view("rcc_residual_scale", r, convergence_progress, params, &v)) return st;
  HIPCHK(hipSetDevice(r->ctx->device));
  if (rmclhip_status st = reserve(r->robust, v.n, reduce_num_blocks(v.n, 1))) return st;
  if (rmclhip_status st = scale_enqueue(r->robust, v, to_x(T_snew_sold), params, true, r->stream)) return st;
  HIPCHK(hipStreamSynchronize(r->stream));
  const RobustScale s = r->robust.out.h->scale;
  if (c_out) *c_out = s.c;
  if (median_out) *median_out = s.median;
  if (m_out) *m_out = s.m;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_correct_once_robust(rmclhip_rcc* r, const rmclhip_transform* Tom_, const rmclhip_transform* Tbo_, uint32_t n_iter,
                                               double convergence_progress, const rmclhip_robust_params* params, rmclhip_transform* T_out,
                                               rmclhip_robust_statistics* stats_out) {
  ApiGuard guard_("rmclhip_rcc_correct_once_robust");
  if (!r || !Tom_ || !Tbo_ || !T_out) return fail(RMCLHIP_ERR_INVALID, "correct_once_robust: null");
  if (rmclhip_status st = params_check("correct_once_robust", params)) return st;
  if (r->kind == kModelNone || r->W == 0 || r->H == 0) return fail(RMCLHIP_ERR_INVALID, "correct_once_robust: no sensor model");
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  return correct_once_robust_run(r, Tom_, Tbo_, n_iter, convergence_progress, params, T_out, stats_out);
}

// ---- the rig -------------------------------------------------------------------------------------------------------
// N sensors on one device: every sensor's find and scale selection on ITS stream (as rmclhip_micp_correct_once's finds), then the loop
// on sensor 0's stream behind the others' events -- per iteration one streaming launch over all sensors and one one-wave step --, a
// closing launch into host-mapped memory and one synchronisation.  Not captured into a graph.
rmclhip_status rmclhip_micp_correct_once_robust(rmclhip_rcc* const* sensors, uint32_t n_sensors, const rmclhip_transform* Tom_,
                                                const rmclhip_transform* Tbo_, const double* merge_weight_multiplier,
                                                const rmclhip_robust_params* params, uint32_t n_iter, double convergence_progress,
                                                rmclhip_transform* T_out, rmclhip_cross_statistics* merged_out, double* merged_weight_out,
                                                rmclhip_robust_statistics* stats_s_out) {
  ApiGuard guard_("rmclhip_micp_correct_once_robust");
  const std::string who = "micp_correct_once_robust: ";
  // every refusal of an argument, before any launch or change of state (what can still fail afterwards is an allocation or a HIP
  // call: the operators prepared until then keep their new n_model / nposes_last, as after a failed find)
  if (!sensors || !Tom_ || !Tbo_ || !params || !T_out || n_sensors == 0) return fail(RMCLHIP_ERR_INVALID, who + "null");
  if (n_sensors > kMaxMicpSensors)
    return fail(RMCLHIP_ERR_UNSUPPORTED, who + "at most 8 sensors, sensor " + std::to_string(kMaxMicpSensors) + " is one too many");
  for (uint32_t s = 0; s < n_sensors; ++s) {
    const rmclhip_rcc* r = sensors[s];
    const std::string me = who + "sensor " + std::to_string(s) + ": ";
    if (!r) return fail(RMCLHIP_ERR_INVALID, me + "null");
    if (r->ctx->device != sensors[0]->ctx->device) return fail(RMCLHIP_ERR_INVALID, me + "lives on another device than sensor 0");
    if (r->kind == kModelNone || r->W == 0 || r->H == 0) return fail(RMCLHIP_ERR_INVALID, me + "no sensor model");
    if (r->n_dataset == 0) return fail(RMCLHIP_ERR_INVALID, me + "no dataset");
    if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, me + kNeedMicpOutputs);
    if (merge_weight_multiplier && !(std::isfinite(merge_weight_multiplier[s]) && merge_weight_multiplier[s] >= 0.0))
      return fail(RMCLHIP_ERR_INVALID, me + "merge_weight_multiplier is negative or not finite");
    if (const char* msg = robust_params_error(params + s)) return fail(RMCLHIP_ERR_INVALID, me + msg);
    for (uint32_t k = 0; k < s; ++k)
      if (sensors[k] == r) return fail(RMCLHIP_ERR_INVALID, me + "the same operator as sensor " + std::to_string(k));
  }
  rmclhip_rcc* r0 = sensors[0];
  const xform Tom = to_x(Tom_);
  if (n_sensors == 1u && (!merge_weight_multiplier || merge_weight_multiplier[0] > 0.0)) {
    // one sensor that counts: the single-sensor loop -- the same algebra in the sensor frame, carried over once at the end
    rmclhip_robust_statistics st_s;
    if (rmclhip_status st = correct_once_robust_run(r0, Tom_, Tbo_, n_iter, convergence_progress, params, T_out, &st_s)) return st;
    double W = 0.0;
    const cstats Cs_o = cs_transform(to_x(Tbo_), cs_transform(r0->Tsb, to_cs(&st_s.stats)));
    const cstats merged = (n_iter == 0) ? cs_identity() : cs_merge_weighted(cs_identity(), 0.0, Cs_o, st_s.weight_sum, &W);
    if (merged_out) from_cs(merged, merged_out);
    if (merged_weight_out) *merged_weight_out = W;
    if (stats_s_out) *stats_s_out = st_s;
    return RMCLHIP_OK;
  }
  HIPCHK(hipSetDevice(r0->ctx->device));
  static thread_local RobustRigCall call;
  std::memset(&call, 0, sizeof(call));
  call.n_sensors = n_sensors;
  for (uint32_t s = 0; s < n_sensors; ++s) {
    rmclhip_rcc* r = sensors[s];
    RobustRigSensor& me = call.s[s];
    const size_t nm = static_cast<size_t>(r->W) * r->H;
    r->n_model = static_cast<uint32_t>(nm);
    r->nposes_last = 1;
    if (rmclhip_status st = ensure_model_buffers(r, nm)) return st;
    if (rmclhip_status st = rcc_view("micp_correct_once_robust", r, convergence_progress, params + s, &me.v)) return st;
    me.nblocks = reduce_num_blocks(me.v.n, 1);
    me.block0 = call.total_blocks;
    call.total_blocks += me.nblocks;
    if (rmclhip_status st = reserve(r->robust, me.v.n, me.nblocks)) return st;
    me.scale = &r->robust.dev.p->scale;
    me.partials = r->robust.partials.p;
    me.Tsb = r->Tsb;
    me.Tbo = to_x(Tbo_ + s);
    me.weight = merge_weight_multiplier ? merge_weight_multiplier[s] : 1.0;
  }
  HIPCHK(r0->robust.rig.reserve(1));
  HIPCHK(r0->robust.rig_out.reserve(1));
  // From here on work is in flight on the sensors' streams: an error (allocation or HIP alone reach these paths) drains every stream
  // before it is returned, so that the caller never gets its operators back with launches still running on them.
  // Every find before any selection: the host needs a few microseconds per launch, and the second sensor's scan should not wait behind
  // the first sensor's histograms being enqueued (micp_multi_enqueue_finds)
  const auto enqueue = [&]() -> rmclhip_status {
    for (uint32_t s = 0; s < n_sensors; ++s) {
      rmclhip_rcc* r = sensors[s];
      FindParams fp;
      fill_find_params(r, fp, 1);
      fp.Tsm = xmul(xmul(Tom, call.s[s].Tbo), r->Tsb);
      fp.Tms = xinv(fp.Tsm);
      HIPCHK(launch_find(fp, r->kind, find_variant(r, 1), r->stream));
    }
    if (n_iter == 0) return RMCLHIP_OK;
    for (uint32_t s = 0; s < n_sensors; ++s) {
      rmclhip_rcc* r = sensors[s];
      if (rmclhip_status st = scale_enqueue(r->robust, call.s[s].v, xidentity(), params + s, false, r->stream)) return st;
      if (s == 0u) continue;
      if (!r->ev_join) HIPCHK(hipEventCreateWithFlags(&r->ev_join, hipEventDisableTiming));
      HIPCHK(hipEventRecord(r->ev_join, r->stream));
      HIPCHK(hipStreamWaitEvent(r0->stream, r->ev_join, 0));
    }
    HIPCHK(launch_robust_rig_loop(call, r0->robust.rig.p, n_iter, r0->robust.rig_out.d, r0->stream));
    return RMCLHIP_OK;
  };
  const rmclhip_status enq = enqueue();
  if (enq != RMCLHIP_OK || n_iter == 0) {
    // (no loop ran behind the other sensors' events: every stream is waited for on its own)
    hipError_t first = hipSuccess;
    for (uint32_t s = 0; s < n_sensors; ++s) {
      const hipError_t e = hipStreamSynchronize(sensors[s]->stream);
      if (first == hipSuccess) first = e;
    }
    if (enq != RMCLHIP_OK) return enq;
    HIPCHK(first);
    from_x(xidentity(), T_out);
    if (merged_out) from_cs(cs_identity(), merged_out);
    if (merged_weight_out) *merged_weight_out = 0.0;
    for (uint32_t s = 0; s < n_sensors && stats_s_out; ++s) identity_statistics(params + s, stats_s_out + s);
    return RMCLHIP_OK;
  }
  HIPCHK(hipStreamSynchronize(r0->stream));
  const RobustRigState& res = *r0->robust.rig_out.h;
  from_x(res.T_onew_oold, T_out);
  if (merged_out) from_cs(res.merged_o, merged_out);
  if (merged_weight_out) *merged_weight_out = res.merged_weight;
  for (uint32_t s = 0; s < n_sensors && stats_s_out; ++s) std::memcpy(stats_s_out + s, &res.stats_s[s], sizeof(*stats_s_out));
  return RMCLHIP_OK;
}

// rmclhip_rcc_pose_information with the weights: the scale as rmclhip_rcc_residual_scale selects it at this pre-transform, then the
// weighted pass on the rows of the plain call (d_pinfo_partials / d_pinfo_rows); reads the last find's buffers, changes nothing else
rmclhip_status rmclhip_rcc_pose_information_robust(rmclhip_rcc* r, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                                   const rmclhip_robust_params* params, rmclhip_pose_information_robust* out) {
  ApiGuard guard_("rmclhip_rcc_pose_information_robust");
  if (!r || !T_snew_sold || !out) return fail(RMCLHIP_ERR_INVALID, "rcc_pose_information_robust: null");
  if (rmclhip_status st = params_check("rcc_pose_information_robust", params)) return st;
  RobustView v;
  if (rmclhip_status st = rcc_view("rcc_pose_information_robust", r, convergence_progress, params, &v)) return st;
  HIPCHK(hipSetDevice(r->ctx->device));
  ReduceParams p;
  std::memset(&p, 0, sizeof(p));
  p.dataset_points = v.dataset_points; p.dataset_mask = v.dataset_mask;
  p.model_points = v.model_points; p.model_normals = v.model_normals; p.model_mask = v.model_mask;
  p.n = v.n; p.nposes = 1; p.max_dist = v.max_dist;
  p.Tpre = to_x(T_snew_sold);
  p.nblocks = reduce_num_blocks(v.n, 1);
  if (rmclhip_status st = reserve(r->robust, v.n, p.nblocks)) return st;
  HIPCHK(r->d_pinfo_partials.reserve(static_cast<size_t>(p.nblocks) * kPoseInfoRow));
  HIPCHK(r->d_pinfo_rows.reserve(kPoseInfoRow));
  p.partials = r->d_pinfo_partials.p;
  if (rmclhip_status st = scale_enqueue(r->robust, v, p.Tpre, params, true, r->stream)) return st;
  HIPCHK(launch_pose_information_robust(p, params->kernel, &r->robust.dev.p->scale, r->d_pinfo_rows.p, r->stream));
  double row[kPoseInfoRow];
  HIPCHK(hipMemcpyAsync(row, r->d_pinfo_rows.p, sizeof(row), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  pose_information_unpack_row(row, &out->info);
  out->weight_sum = row[29];
  out->rss_unweighted = row[30];
  out->scale = r->robust.out.h->scale.c;
  out->median_abs_residual = r->robust.out.h->scale.median;
  return RMCLHIP_OK;
}

}  // extern "C"
