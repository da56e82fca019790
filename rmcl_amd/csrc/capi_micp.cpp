// capi_micp.cpp -- see capi_internal.h
// The MICP corrections of the correspondence operator, schedule (R) of micp_localization.cpp:900-964 (1 find, n_iter x (reduce + solve)):
// rmclhip_rcc_correct_once for one sensor, rmclhip_micp_correct_once for N.  Each is a dispatcher over its loop forms -- the moments
// with the iterations on the host, the moments with the loop on the device, one launch per iteration -- and the small things both need
// are written once, up front.
#include "capi_internal.h"

// what a correction sets up on an operator before its find: the model's size, the model buffers, the partial rows of the per-iteration
// form (two sets of them: k_micp_iter alternates).  *nred: the elements its reductions cover
static rmclhip_status micp_prepare_operator(rmclhip_rcc* r, uint32_t* nred) {
  const size_t n = static_cast<size_t>(r->W) * r->H;
  r->n_model = static_cast<uint32_t>(n);
  r->nposes_last = 1;
  if (rmclhip_status st = ensure_model_buffers(r, n)) return st;
  *nred = nred_of(r);
  if (*nred == 0) return fail(RMCLHIP_ERR_INVALID, "correct_once: empty dataset");
  HIPCHK(r->d_partials.reserve(std::max<size_t>(static_cast<size_t>(reduce_num_blocks(*nred, 1)) * 32, 2u * 256u * 16u)));
  return RMCLHIP_OK;
}

// per-call data of the moment kernels, BY VALUE (no H2D copy node per sensor: 4.4 us each in the kernel trace of round 2's chain): the
// frames, one max_dist as the whole gate band, the caps the operator's own corrections learnt
static MicpCallLite micp_call_lite(const rmclhip_rcc* r, const xform& Tbo, float max_dist, uint32_t seq) {
  MicpCallLite cl;
  cl.Tsb = r->Tsb; cl.Tbo = Tbo; cl.max_dist = max_dist; cl.rho_cap = r->fast_rho_cap; cl.tau_cap = r->fast_tau_cap;
  cl.gate_lo = max_dist; cl.gate_hi = max_dist; cl.seq = seq;
  return cl;
}

// the outcome of one moment-form attempt in the handle's fast_info (code 0 done: the caps follow what it met; 1 a pre-transform left
// the caps; 2 too many undecided correspondences)
static void micp_record_attempt(rmclhip_rcc* r, uint32_t code, uint32_t n_uncertain, float max_rho, float max_tau) {
  rmclhip_micp_fast_info& fi = r->fast_info;
  fi.attempts++;
  fi.last_code = code;
  fi.last_uncertain = n_uncertain;
  fi.last_rho = max_rho;
  fi.last_tau = max_tau;
  if (code == 0u) {
    fi.done++;
    learn_caps(r, max_rho, max_tau);
  } else if (code == 1u) {
    fi.cap_exits++;
  } else if (code == 2u) {
    fi.overflows++;
  }
}

// caps of the next attempt after one the per-iteration form had to finish: the pre-transform the correction ended with (sensor frame,
// Ts) bounds the next attempt (iterates approach it monotonically in the usual case; an attempt that still leaves the caps costs one
// more fallback and doubles them).  After an overflow (too many undecided correspondences) the caps tighten instead.
static void micp_caps_after_fallback(rmclhip_rcc* r, const xform& Ts, bool overflow, float prev_max_rho, float prev_max_tau) {
  const float rho = 2.0f * std::sqrt(Ts.R.x * Ts.R.x + Ts.R.y * Ts.R.y + Ts.R.z * Ts.R.z);
  const float tau = std::sqrt(Ts.t.x * Ts.t.x + Ts.t.y * Ts.t.y + Ts.t.z * Ts.t.z);
  if (overflow) {
    r->fast_rho_cap = std::max(0.002f, 1.25f * rho);
    r->fast_tau_cap = std::max(0.005f, 1.25f * tau);
  } else {
    r->fast_rho_cap = std::max(0.002f, std::max(2.0f * rho, 2.0f * prev_max_rho));
    r->fast_tau_cap = std::max(0.005f, std::max(2.0f * tau, 2.0f * prev_max_tau));
  }
  r->fast_info.rho_cap = r->fast_rho_cap;
  r->fast_info.tau_cap = r->fast_tau_cap;
}

// ---- one sensor: rmclhip_rcc_correct_once -------------------------------------------------------------------------------------

// the device's moment loop on the handle's stream: over the rows a find's epilogue left (`tiled`: nb rows and wpb mask words per
// workgroup, in the tile order of `fp`), or with a moment pass of its own over the find's outputs
static hipError_t launch_moment_loop(rmclhip_rcc* r, bool tiled, const FindParams& fp, uint32_t nb, uint32_t wpb, uint32_t nred,
                                     uint32_t n_iter, const MicpCallLite& cl) {
  const uint8_t* dmask = r->ds_has_mask ? r->ds_msk : nullptr;
  if (tiled)
    return launch_micp_fast_loop_tiled(r->ds_pts, dmask, r->d_points.p, r->d_normals.p, r->d_hits.p, nred, nb, r->d_fast_partials.p,
                                       r->d_fast_mask.p, r->W, fp.tiles_x, fp.tile_w_log2, wpb, n_iter, r->h_state.d,
                                       r->h_fast_status.d, r->h_done.d, r->stream, cl, r->d_fold_rows.p, r->d_fold_flags);
  return launch_micp_fast(r->ds_pts, dmask, r->d_points.p, r->d_normals.p, r->d_hits.p, nred, nullptr, r->d_fast_partials.p,
                          r->d_fast_mask.p, n_iter, r->h_state.d, r->h_fast_status.d, r->h_done.d, r->stream, &cl);
}

// Moment form (micp.hip "gate-stable moment form"), fast modes 1, 3 and 4, launched directly with the per-call data BY VALUE -- no
// H2D copy node, no graph launch (a graph replay costs the host 10-16 us whatever it holds).  *out: code 0 = served, the correction
// is in r->h_state.h; 1 / 2 = the caller runs the per-iteration form, which recomputes the correction from scratch.
static rmclhip_status micp_try_moment_form(rmclhip_rcc* r, const xform& Tbo, uint32_t n_iter, float maxd, uint32_t nred,
                                           MicpFastStatus* out) {
  HIPCHK(r->d_fast_partials.reserve(static_cast<size_t>(micp_fast_blocks(nred)) * kMicpFastMoments));
  HIPCHK(r->d_fast_mask.reserve((static_cast<size_t>(nred) + 63u) / 64u));
  MicpFastStatus fs{};
  bool fs_ready = false;     // the host ran the iterations: `fs` (and r->h_state.h) are final, nothing to wait for
  FindParams fp;
  fill_find_params(r, fp, 1);
  fp.Tsm = r->h_call.p->Tsm;
  fp.Tms = r->h_call.p->Tms;
  MicpCallLite cl = micp_call_lite(r, Tbo, maxd, r->h_call.p->seq);
  const int fv = find_variant(r, 1);
  const bool tiled = r->fast_mode != 3 && find_kind(fv).moments;   // the find forms the moments in its epilogue
  if (r->fast_mode == 1) {
    // ---- round 4 default: TWO launches (find with the moment epilogue; fold + publish), the iterations on the HOST from the 82
    // moments + the undecided correspondences (micp_host.h): ~0.5 us per iteration instead of ~2.7 us of one lane's f64 chain
    if (rmclhip_status st = enqueue_find_with_moments(r, r->h_call.p->Tsm, maxd, maxd, r->fast_rho_cap, r->fast_tau_cap, cl.seq, true)) return st;
    HIPCHK(wait_moments(r, cl.seq, maxd, maxd, r->fast_rho_cap, r->fast_tau_cap));
    if (r->mset.valid) {
      xform T_s = xidentity();
      cstats last = cs_identity();
      fs.code = 0u; fs.n_uncertain = r->mset.n_unc;
      for (uint32_t it = 0; it < n_iter; ++it) {
        const float rho = micp_rho(T_s), tau = micp_tau(T_s);
        fs.max_rho = std::max(fs.max_rho, rho);
        fs.max_tau = std::max(fs.max_tau, tau);
        if (!(rho <= r->mset.rho_cap) || !(tau <= r->mset.tau_cap)) { fs.code = 1u; fs.iter = it; break; }
        last = micp_statistics_from_set(r->mset, T_s, maxd);
        T_s = xmul(T_s, umeyama(last));   // micp.hip micp_advance_sensor
      }
      if (fs.code == 0u) {
        // micp.hip micp_close_sensor
        fs.iter = n_iter;
        const xform Tso = xmul(Tbo, r->Tsb);
        r->h_state.h->T_snew_sold = T_s;
        r->h_state.h->T_onew_oold = xmul(xmul(Tso, T_s), xinv(Tso));
        r->h_state.h->stats_o = cs_merge(cs_identity(), cs_transform(Tbo, cs_transform(r->Tsb, last)));
      }
      fs_ready = true;
    } else {
      // more undecided correspondences than the host takes: the device loop on the rows the find left (a sequence number of its own:
      // the publish launch used this one for its hand-over flags and its tag)
      cl.seq = r->h_call.p->seq = next_seq(r);
      // kind and row layout are the ones enqueue_find_with_moments actually ran (it replaces kind 24 by 23 to get the epilogue):
      // the loop folds THOSE rows instead of paying a moment pass of its own
      const int ufv = r->last_moment_find_kind;
      FindParams ufp;
      fill_find_params(r, ufp, 1, ufv);
      HIPCHK(launch_moment_loop(r, r->last_moment_find_tiled, ufp, find_launch_shape(ufp, ufv, true).grid_x, find_kind(ufv).tiles_per_block(), nred, n_iter, cl));
    }
  } else {
    // (fast_mode 4, round 3's default) TWO kernels: the find forms the moments in its epilogue (find_kernel.hip.h: the 10 x 10 factor
    // products of its 64 correspondences per wave through f64 MFMA), one partial row per workgroup; the loop launch folds them and runs
    // every iteration on the device.  Mode 3, or a find kind without the epilogue: a plain find, and the loop's own moment pass
    uint32_t nb = 0, wpb = 0;
    if (tiled) {
      if (rmclhip_status st = arm_moment_epilogue(r, fp, fv, nred, maxd, maxd, r->fast_rho_cap, r->fast_tau_cap, &nb, &wpb)) return st;
      HIPCHK(launch_find_moments(fp, r->kind, fv, r->stream));
    } else {
      r->last_fast_rows = micp_fast_blocks(nred); r->last_fast_words = (nred + 63u) / 64u;
      HIPCHK(launch_find(fp, r->kind, fv, r->stream));
    }
    HIPCHK(launch_moment_loop(r, tiled, fp, nb, wpb, nred, n_iter, cl));
  }
  if (!fs_ready) {
    // sum of the tag: the status block, plus the state block when the loop ran to its end (code 0)
    DoneCheck chk; chk.base = r->h_fast_status.h; chk.base_bytes = sizeof(MicpFastStatus); chk.code = &r->h_fast_status.h->code;
    chk.extra[0] = r->h_state.h; chk.extra_bytes[0] = sizeof(MicpState);
    HIPCHK(wait_done(r->ctx, r->h_done.h, r->h_call.p->seq, chk, r->stream));
    fs = *r->h_fast_status.h;
  } else {
    ++r->fast_info.host_loops;
  }
  r->last_fast = fs;
  micp_record_attempt(r, fs.code, fs.n_uncertain, fs.max_rho, fs.max_tau);
  r->fast_info.last_setup_clocks = fs.code == 0u ? fs.pad[0] : 0u;
  r->fast_info.last_loop_clocks = fs.code == 0u ? fs.pad[1] : 0u;
  if (fs.code > 2u) return fail(RMCLHIP_ERR_HIP, "correct_once: the moment-form loop did not report a status");
  if (fs.code == 0u) r->fast_overflows = 0;
  *out = fs;
  return RMCLHIP_OK;
}

// the per-iteration chain on the handle's stream: the call block (H2D), the find, then ONE launch per iteration (k_micp_iter solves
// the previous iteration in its prologue) + one closing solve -- n_iter + 1 launches instead of 2 * n_iter.  k_micp_close writes the
// result straight into host-mapped memory (no copy node).  Without iterations: k_micp_init + a copy of that state.
static rmclhip_status enqueue_micp_chain(rmclhip_rcc* r, uint32_t n_iter, uint32_t nred) {
  HIPCHK(hipMemcpyAsync(r->d_call.p, r->h_call.p, sizeof(MicpCall), hipMemcpyHostToDevice, r->stream));
  FindParams p;
  fill_find_params(r, p, 1);
  p.Tsm_arr = &r->d_call.p->Tsm;
  p.Tms_arr = &r->d_call.p->Tms;
  HIPCHK(launch_find(p, r->kind, find_variant(r, p.nposes), r->stream));
  if (n_iter == 0) {
    HIPCHK(launch_micp_init(r->d_state.p, r->stream));
    HIPCHK(hipMemcpyAsync(r->h_state.h, r->d_state.p, sizeof(MicpState), hipMemcpyDeviceToHost, r->stream));
    return RMCLHIP_OK;
  }
  const uint8_t* dmask = r->ds_has_mask ? r->ds_msk : nullptr;
  const uint32_t nb = reduce_num_blocks(nred, 1);
  double* part[2] = {r->d_partials.p, r->d_partials.p + static_cast<size_t>(nb) * 16};
  for (uint32_t i = 0; i < n_iter; ++i)
    HIPCHK(launch_micp_iter(r->ds_pts, dmask, r->d_points.p, r->d_normals.p, r->d_hits.p, nred, nb, r->d_call.p,
                            part[(i + 1u) & 1u], part[i & 1u], r->d_state.p + (i & 1u), r->d_state.p + ((i + 1u) & 1u),
                            i == 0, r->stream));
  HIPCHK(launch_micp_close(part[(n_iter - 1u) & 1u], nb, r->d_call.p, r->d_state.p + (n_iter & 1u), r->h_state.d,
                           r->h_done.d, r->stream));
  return RMCLHIP_OK;
}

// The per-iteration form, captured ONCE into a hipGraph (the kernels read the per-call pose / frames / max_dist from d_call,
// refreshed by the graph's first node), so that a correction costs one graph launch instead of 2 + n_iter host launches (~5 us each,
// which left the GPU idle between these tiny kernels); set_variant bit 9 enqueues it directly.  Leaves the result in r->h_state.
static rmclhip_status micp_per_iteration_chain(rmclhip_rcc* r, uint32_t n_iter, uint32_t nred) {
  // k_micp_close publishes a completion tag the host polls (a fresh sequence number: a moment-form attempt may have published one
  // for this call already)
  r->h_call.p->seq = next_seq(r);
  if (r->use_graph) {
    rmclhip_rcc::MicpKey key;
    std::memset(&key, 0, sizeof(key));
    key.n_iter = n_iter; key.W = r->W; key.H = r->H; key.n_dataset = r->n_dataset;
    key.kind = static_cast<int>(r->kind); key.variant = r->variant; key.tile = r->tile_override;
    key.has_mask = r->ds_has_mask ? 1 : 0;
    key.ptrs[0] = r->d_points.p; key.ptrs[1] = r->ds_pts; key.ptrs[2] = r->d_partials.p;
    key.ptrs[3] = r->d_model_tab.p; key.ptrs[4] = r->ds_msk; key.ptrs[5] = r->d_hits.p;
    if (!r->micp_exec || r->graph_dirty || !(key == r->micp_key)) {
      // the previous call returned on its completion tag, which precedes the stream's own completion: let the last node
      // retire before its executable graph is destroyed
      HIPCHK(hipStreamSynchronize(r->stream));
      if (r->micp_exec) { (void)hipGraphExecDestroy(r->micp_exec); r->micp_exec = nullptr; }
      if (r->micp_graph) { (void)hipGraphDestroy(r->micp_graph); r->micp_graph = nullptr; }
      HIPCHK(hipStreamBeginCapture(r->stream, hipStreamCaptureModeThreadLocal));
      r->capturing = true;
      const rmclhip_status cst = enqueue_micp_chain(r, n_iter, nred);
      r->capturing = false;
      hipGraph_t g = nullptr;
      const hipError_t ce = hipStreamEndCapture(r->stream, &g);
      if (cst != RMCLHIP_OK) { if (g) (void)hipGraphDestroy(g); return cst; }
      if (ce != hipSuccess) return fail(RMCLHIP_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
      r->micp_graph = g;
      HIPCHK(hipGraphInstantiate(&r->micp_exec, g, nullptr, nullptr, 0));
      r->micp_key = key;
      r->graph_dirty = false;
    }
    HIPCHK(hipGraphLaunch(r->micp_exec, r->stream));
  } else if (rmclhip_status st = enqueue_micp_chain(r, n_iter, nred)) {
    return st;
  }
  if (n_iter == 0) {
    HIPCHK(hipStreamSynchronize(r->stream));
  } else {
    DoneCheck chk; chk.base = r->h_state.h; chk.base_bytes = sizeof(MicpState);
    HIPCHK(wait_done(r->ctx, r->h_done.h, r->h_call.p->seq, chk, r->stream));
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_correct_once(rmclhip_rcc* r, const rmclhip_transform* Tom_, const rmclhip_transform* Tbo_,
                                        uint32_t n_iter, double convergence_progress, int refind_each_iteration,
                                        rmclhip_transform* T_out, rmclhip_cross_statistics* stats_out) {
  ApiGuard guard_("rmclhip_rcc_correct_once");
  if (!r || !Tom_ || !Tbo_ || !T_out) return fail(RMCLHIP_ERR_INVALID, "correct_once: null");
  if (r->kind == kModelNone || r->W == 0 || r->H == 0) return fail(RMCLHIP_ERR_INVALID, "correct_once: no sensor model");
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  HIPCHK(hipSetDevice(r->ctx->device));
  const xform Tom = to_x(Tom_), Tbo = to_x(Tbo_);
  const float maxd = adaptive_max_dist(r, convergence_progress);
  if (!refind_each_iteration) {
    // schedule (R): nothing returns to the host until the end -- the pre-transform of iteration i+1 is produced on the device
    // (or, in the moment form of mode 1, on the host from the moments the find published)
    uint32_t nred = 0;
    if (rmclhip_status st = micp_prepare_operator(r, &nred)) return st;
    r->h_call.p->Tsm = xmul(xmul(Tom, Tbo), r->Tsb);
    r->h_call.p->Tms = xinv(r->h_call.p->Tsm);
    r->h_call.p->Tsb = r->Tsb;
    r->h_call.p->Tbo = Tbo;
    r->h_call.p->max_dist = maxd;
    r->h_call.p->gate_lo = maxd; r->h_call.p->gate_hi = maxd;
    r->h_call.p->rho_cap = r->fast_rho_cap;
    r->h_call.p->tau_cap = r->fast_tau_cap;
    r->h_call.p->seq = next_seq(r);
    // moment form first; any outcome other than "done" falls through to the per-iteration form (the device loops need >= 2
    // iterations to pay for their moment pass; the host form -- two launches, no reduction launch at all -- serves 1 as well)
    const bool fast_eligible = r->fast_mode != 0 && n_iter >= ((r->fast_mode == 1) ? 1u : 2u);
    bool fast_tried = false;
    if (fast_eligible && r->fast_holdoff > 0u) --r->fast_holdoff;
    else if (fast_eligible) {
      fast_tried = true;
      MicpFastStatus fs;
      if (rmclhip_status st = micp_try_moment_form(r, Tbo, n_iter, maxd, nred, &fs)) return st;
      if (fs.code == 0u) {
        from_x(r->h_state.h->T_onew_oold, T_out);
        if (stats_out) from_cs(r->h_state.h->stats_o, stats_out);
        return RMCLHIP_OK;
      }
    }
    if (rmclhip_status st = micp_per_iteration_chain(r, n_iter, nred)) return st;
    if (fast_tried) {
      const xform Tb = xmul(xmul(xinv(Tbo), r->h_state.h->T_onew_oold), Tbo);
      const bool overflow = r->last_fast.code == 2u;
      micp_caps_after_fallback(r, xmul(xmul(xinv(r->Tsb), Tb), r->Tsb), overflow, r->last_fast.max_rho, r->last_fast.max_tau);
      // too many uncertain correspondences twice in a row: stop trying for a while
      if (overflow && ++r->fast_overflows >= 2u) { r->fast_holdoff = 32u; r->fast_overflows = 0; }
    }
    from_x(r->h_state.h->T_onew_oold, T_out);
    if (stats_out) from_cs(r->h_state.h->stats_o, stats_out);
    return RMCLHIP_OK;
  }
  // schedule (B), lidar_corrector_embree_benchmark.cpp:127-135: re-raycast from the corrected pose every iteration
  xform T_onew_oold = xidentity();
  cstats last = cs_identity();
  for (uint32_t i = 0; i < n_iter; ++i) {
    const xform Tom_cur = xmul(Tom, T_onew_oold);
    if (rmclhip_status st = find_enqueue(r, xmul(Tom_cur, Tbo))) return st;
    ReduceTail tail;
    tail.mode = kTailStats;
    tail.stats_out = r->h_stats.d;
    tail.done = r->h_done.d;
    tail.seq = next_seq(r);
    if (rmclhip_status st = reduce_enqueue(r, xidentity(), nullptr, maxd, 1, tail)) return st;
    DoneCheck chk; chk.base = &r->h_stats.h[0]; chk.base_bytes = sizeof(cstats);
    HIPCHK(wait_done(r->ctx, r->h_done.h, tail.seq, chk, r->stream));
    const cstats Cs_o = cs_transform(Tbo, cs_transform(r->Tsb, r->h_stats.h[0]));
    last = cs_merge(cs_identity(), Cs_o);
    T_onew_oold = xmul(T_onew_oold, umeyama(last));
  }
  from_x(T_onew_oold, T_out);
  if (stats_out) from_cs(last, stats_out);
  return RMCLHIP_OK;
}

// ---- N sensors: rmclhip_micp_correct_once --------------------------------------------------------------------------------------
// MICPLocalizationNode::correctOnce inner loop for N sensors on one device (micp_localization.cpp:900-964): one find per
// sensor, then per iteration one reduction per sensor and ONE step launch that merges, solves and hands out the next
// pre-transforms; nothing returns to the host until the loop is over (the host form costs one synchronisation per sensor
// and iteration).

namespace {   // (a member function of a named struct would be exported)
// one call, as every form of it sees it.  What persists between calls lives with the FIRST sensor: the device copy of the call block
// and the loop's state (d_multi_blob), the host-mapped state and status, the loop's tag (h_done[1]), the join flags, the hold-off
struct MicpMultiJob {
  rmclhip_rcc* const* sensors;
  uint32_t n_sensors, n_iter;
  xform Tom;
  MicpMultiCall* call;                  // thread-local: frames, weights, partial rows, the call's sequence number (on sensor 0)
  float max_dist[kMaxMicpSensors];      // every sensor's adaptive_max_dist(convergence_progress)
  uint32_t nred[kMaxMicpSensors];
  // sensor->setTom(Tom); sensor->findCorrespondences()  (:900-909): Tbm = Tom * Tbo, the find's pose Tbm * Tsb
  xform Tsm(uint32_t s) const { return xmul(xmul(Tom, call->Tbo[s]), sensors[s]->Tsb); }
};
// the forms a call tries before the per-iteration one.  moment: any at all; host: the host form first (every sensor in mode 1)
struct MicpMultiRoute { bool moment, host; };
}  // namespace

// every refusal, before any state changes
static rmclhip_status micp_multi_check(rmclhip_rcc* const* sensors, uint32_t n_sensors, const rmclhip_transform* Tom, const rmclhip_transform* Tbo,
                                       const double* merge_weight_multiplier, const rmclhip_transform* T_out) {
  if (!sensors || !Tom || !Tbo || !T_out || n_sensors == 0) return fail(RMCLHIP_ERR_INVALID, "micp_correct_once: null");
  if (n_sensors > kMaxMicpSensors) return fail(RMCLHIP_ERR_UNSUPPORTED, "micp_correct_once: at most 8 sensors");
  for (uint32_t s = 0; s < n_sensors; ++s) {
    const rmclhip_rcc* r = sensors[s];
    if (!r) return fail(RMCLHIP_ERR_INVALID, "micp_correct_once: null sensor");
    if (r->ctx->device != sensors[0]->ctx->device) return fail(RMCLHIP_ERR_INVALID, "micp_correct_once: sensors live on different devices");
    if (r->kind == kModelNone || r->W == 0 || r->H == 0) return fail(RMCLHIP_ERR_INVALID, "micp_correct_once: sensor without a model");
    if (r->n_dataset == 0) return fail(RMCLHIP_ERR_INVALID, "micp_correct_once: sensor without a dataset");
    if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
    // n_meas * weight is converted to uint32 on the host in one loop form and on the device in the other two: a negative or
    // non-finite product has no defined conversion, and the forms would part
    if (merge_weight_multiplier && !(std::isfinite(merge_weight_multiplier[s]) && merge_weight_multiplier[s] >= 0.0))
      return fail(RMCLHIP_ERR_INVALID, "micp_correct_once: merge_weight_multiplier of sensor " + std::to_string(s) + " is negative or not finite");
  }
  return RMCLHIP_OK;
}

// every sensor's buffers, gate and share of the call block; the call's sequence number; sensor 0's blob and host-mapped blocks
static rmclhip_status micp_multi_prepare(MicpMultiJob& j, const rmclhip_transform* Tbo, const double* merge_weight_multiplier,
                                         double convergence_progress) {
  MicpMultiCall& c = *j.call;
  std::memset(&c, 0, sizeof(c));
  for (uint32_t s = 0; s < j.n_sensors; ++s) {
    rmclhip_rcc* r = j.sensors[s];
    // (no synchronisation with the sensor's own stream: its find is enqueued ON that stream, behind whatever it still holds, and the
    // loop touches the sensor only behind that find -- flag or event; a hipStreamSynchronize per sensor cost ~9 us each here)
    if (rmclhip_status st = micp_prepare_operator(r, &j.nred[s])) return st;
    j.max_dist[s] = adaptive_max_dist(r, convergence_progress);
    c.Tsb[s] = r->Tsb;
    c.Tbo[s] = to_x(Tbo + s);
    c.weight[s] = merge_weight_multiplier ? merge_weight_multiplier[s] : 1.0;
    c.partials[s] = r->d_partials.p;
    c.nblocks[s] = reduce_num_blocks(j.nred[s], 1);
  }
  rmclhip_rcc* r0 = j.sensors[0];
  c.n_sensors = j.n_sensors;
  c.seq = next_seq(r0);
  // call + state live with the first sensor and persist between calls (an allocation per call cost more than the loop)
  HIPCHK(r0->d_multi_blob.reserve(sizeof(MicpMultiCall) + sizeof(MicpMultiState)));
  HIPCHK(r0->h_multi_state.reserve(1));
  HIPCHK(r0->h_multi_status.reserve(1));
  return RMCLHIP_OK;
}

// The ONE place that decides which forms this call tries: the moment forms need two iterations to pay for their moment passes and
// every sensor out of mode 0; a call inside sensor 0's hold-off (two overflows in a row arm it) counts it down and tries neither.
static MicpMultiRoute micp_multi_route(const MicpMultiJob& j) {
  bool moment = j.n_iter >= 2u, host = true;
  for (uint32_t s = 0; s < j.n_sensors; ++s) {
    moment = moment && j.sensors[s]->fast_mode != 0;
    host = host && j.sensors[s]->fast_mode == 1;
  }
  if (moment && j.sensors[0]->multi_holdoff > 0u) { --j.sensors[0]->multi_holdoff; moment = false; }
  return {moment, moment && host};
}

// ---- round 4: every sensor's find forms its moments and publishes them to the host (its own stream, its own block and tag), the
// host merges and solves (micp_host.h; same frame-by-frame order as k_micp_multi_step).  *code: 0 served, the result is in *res; 2 a
// sensor with too many undecided correspondences, 1 a pre-transform outside its caps: the device forms take over, from scratch.
static rmclhip_status micp_multi_host_form(MicpMultiJob& j, uint32_t* code, MicpMultiState* res) {
  MicpMultiCall& c = *j.call;
  uint32_t seqs[kMaxMicpSensors];
  for (uint32_t s = 0; s < j.n_sensors; ++s) {
    rmclhip_rcc* r = j.sensors[s];
    seqs[s] = (s == 0u) ? c.seq : next_seq(r);
    if (rmclhip_status st = enqueue_find_with_moments(r, j.Tsm(s), j.max_dist[s], j.max_dist[s], r->fast_rho_cap, r->fast_tau_cap, seqs[s], true))
      return st;
  }
  bool all_valid = true;
  for (uint32_t s = 0; s < j.n_sensors; ++s) {
    rmclhip_rcc* r = j.sensors[s];
    HIPCHK(wait_moments(r, seqs[s], j.max_dist[s], j.max_dist[s], r->fast_rho_cap, r->fast_tau_cap));
    all_valid = all_valid && r->mset.valid;
  }
  MicpMultiFastStatus hs;
  std::memset(&hs, 0, sizeof(hs));
  hs.code = all_valid ? 0u : 2u;
  xform T_onew_oold = xidentity(), T_s[kMaxMicpSensors];
  cstats merged = cs_identity(), merged_w = cs_identity();
  for (uint32_t s = 0; s < j.n_sensors; ++s) { T_s[s] = xidentity(); hs.n_uncertain += j.sensors[s]->mset.n_unc; }
  for (uint32_t it = 0; it < j.n_iter && hs.code == 0u; ++it) {
    merged = cs_identity(); merged_w = cs_identity();
    for (uint32_t s = 0; s < j.n_sensors; ++s) {
      const rmclhip_rcc* r = j.sensors[s];
      const float rho = micp_rho(T_s[s]), tau = micp_tau(T_s[s]);
      hs.max_rho[s] = std::max(hs.max_rho[s], rho);
      hs.max_tau[s] = std::max(hs.max_tau[s], tau);
      if (!(rho <= r->mset.rho_cap) || !(tau <= r->mset.tau_cap)) { hs.code = 1u; hs.iter = it; hs.sensor = s; break; }
      // micp_localization.cpp:926-937 with MICPSensor.hpp:178-182
      const cstats stats_s = micp_statistics_from_set(r->mset, T_s[s], j.max_dist[s]);
      const cstats Cs_o = cs_transform(c.Tbo[s], cs_transform(r->Tsb, stats_s));
      cstats Cs_w = Cs_o;
      Cs_w.n_meas = static_cast<uint32_t>(static_cast<double>(Cs_w.n_meas) * c.weight[s]);
      merged = cs_merge(merged, Cs_o);
      merged_w = cs_merge(merged_w, Cs_w);
    }
    if (hs.code != 0u) break;
    T_onew_oold = xmul(T_onew_oold, umeyama(merged_w));   // :952-963
    for (uint32_t s = 0; s < j.n_sensors; ++s) {
      const xform T_bnew_bold = xmul(xmul(xinv(c.Tbo[s]), T_onew_oold), c.Tbo[s]);
      T_s[s] = xmul(xmul(xinv(j.sensors[s]->Tsb), T_bnew_bold), j.sensors[s]->Tsb);
    }
  }
  for (uint32_t s = 0; s < j.n_sensors && hs.code != 2u; ++s) {   // (code 2: the device loop is this call's attempt)
    rmclhip_rcc* r = j.sensors[s];
    micp_record_attempt(r, hs.code, hs.n_uncertain, hs.max_rho[s], hs.max_tau[s]);
    r->fast_info.last_setup_clocks = r->fast_info.last_loop_clocks = 0u;
    if (hs.code == 0u) r->fast_info.host_loops++;
  }
  *code = hs.code;
  if (hs.code == 0u) {
    j.sensors[0]->multi_overflows = 0;
    res->T_onew_oold = T_onew_oold;
    res->merged_o = merged;
    return RMCLHIP_OK;
  }
  // not served on the host (the moment sets belong to finds that are about to be redone).  A pre-transform that left its caps would
  // leave them in the device's moment loop as well: the caller goes straight to the per-iteration form, whose end learns the caps from
  // this status.  Too many undecided correspondences for the host (> kMicpHostMaxUnc = 1024 in a sensor): the device's moment loop
  // takes up to 4096.  Either way a fresh sequence number: the publish launches used the first
  if (hs.code == 1u) *j.sensors[0]->h_multi_status.h = hs;
  for (uint32_t s = 0; s < j.n_sensors; ++s) drop_moment_set(j.sensors[s]);
  c.seq = next_seq(j.sensors[0]);
  return RMCLHIP_OK;
}

// The sensors' finds (and moment passes) do not depend on each other: every sensor's go to ITS OWN stream -- sensor 0's is the stream
// the loop runs on -- one scan leaves the chip partly idle (bench.py extras.find_two_operators_in_flight_*), a second sensor's scan
// fills it (round 3: everything sat on one stream).  Every find before any moment pass: the host needs ~4 us per launch, and the
// second sensor's scan should not wait behind the first sensor's moment pass being enqueued.
static rmclhip_status micp_multi_enqueue_finds(const MicpMultiJob& j) {
  rmclhip_rcc* r0 = j.sensors[0];
  // A cross-stream EVENT takes ~10 us to reach the waiting queue (measured: the loop started 10-12 us after its last input), so in the
  // moment form the join is a flag: a one-lane kernel behind the sensor's moment pass stores the call's sequence number, the loop
  // kernel -- launched without waiting -- polls it before it touches that sensor's rows.  The per-iteration form (fallback) records
  // an event on every other sensor's stream and waits for it.
  if (j.n_sensors > 1u && !r0->d_join_flags.p) {
    HIPCHK(r0->d_join_flags.reserve(kMaxMicpSensors));
    HIPCHK(hipMemset(r0->d_join_flags.p, 0, kMaxMicpSensors * sizeof(uint32_t)));
    HIPCHK(hipDeviceSynchronize());
  }
  for (uint32_t s = 0; s < j.n_sensors; ++s) {
    rmclhip_rcc* r = j.sensors[s];
    FindParams p;
    fill_find_params(r, p, 1);
    p.Tsm = j.Tsm(s);
    p.Tms = xinv(p.Tsm);
    HIPCHK(launch_find(p, r->kind, find_variant(r, 1), r->stream));
  }
  return RMCLHIP_OK;
}

// moment form on the device (micp.hip k_micp_multi_fast_loop), behind the finds: a moment pass and a flag per sensor, ONE loop launch
// for every iteration of every sensor; every sensor's caps are the ones its own corrections learnt.  *code: as MicpMultiFastStatus
static rmclhip_status micp_multi_device_loop(const MicpMultiJob& j, uint32_t* code, MicpMultiState* res) {
  rmclhip_rcc* r0 = j.sensors[0];
  const MicpMultiCall& c = *j.call;
  MicpMultiFastParams fp;
  std::memset(&fp, 0, sizeof(fp));
  for (uint32_t s = 0; s < j.n_sensors; ++s) {
    rmclhip_rcc* r = j.sensors[s];
    const uint32_t nred = j.nred[s];
    HIPCHK(r->d_fast_partials.reserve(static_cast<size_t>(micp_fast_blocks(nred)) * kMicpFastMoments));
    HIPCHK(r->d_fast_mask.reserve((static_cast<size_t>(nred) + 63u) / 64u));
    const MicpCallLite cl = micp_call_lite(r, c.Tbo[s], j.max_dist[s], c.seq);
    HIPCHK(launch_micp_moments(r->ds_pts, r->ds_has_mask ? r->ds_msk : nullptr, r->d_points.p, r->d_normals.p, r->d_hits.p, nred,
                               nullptr, r->d_fast_partials.p, r->d_fast_mask.p, r->stream, &cl));
    fp.dataset_points[s] = r->ds_pts; fp.model_points[s] = r->d_points.p; fp.model_normals[s] = r->d_normals.p;
    fp.partials[s] = r->d_fast_partials.p; fp.unc_mask[s] = r->d_fast_mask.p;
    fp.n[s] = nred; fp.nblocks[s] = micp_fast_blocks(nred);
    fp.Tsb[s] = cl.Tsb; fp.Tbo[s] = cl.Tbo; fp.weight[s] = c.weight[s];
    fp.max_dist[s] = cl.max_dist; fp.rho_cap[s] = cl.rho_cap; fp.tau_cap[s] = cl.tau_cap;
    if (s != 0u) {
      HIPCHK(launch_signal_flag(r0->d_join_flags.p + s, c.seq, r->stream));
      fp.join_mask |= 1u << s;
    }
  }
  fp.join_flags = r0->d_join_flags.p;
  fp.n_sensors = j.n_sensors;
  fp.seq = c.seq;
  fp.n_iter = j.n_iter;
  fp.state_out = r0->h_multi_state.d;
  fp.status = r0->h_multi_status.d;
  fp.done = r0->h_done.d + 1;
  HIPCHK(launch_micp_multi_fast_loop(fp, r0->stream));
  DoneCheck chk; chk.base = r0->h_multi_status.h; chk.base_bytes = sizeof(MicpMultiFastStatus); chk.code = &r0->h_multi_status.h->code;
  chk.extra[0] = &r0->h_multi_state.h->T_onew_oold; chk.extra_bytes[0] = sizeof(xform);
  chk.extra[1] = &r0->h_multi_state.h->merged_o; chk.extra_bytes[1] = sizeof(cstats);
  chk.extra[2] = &r0->h_multi_state.h->merged_weighted_o; chk.extra_bytes[2] = sizeof(cstats);
  HIPCHK(wait_done(r0->ctx, r0->h_done.h + 1, c.seq, chk, r0->stream));
  const MicpMultiFastStatus fs = *r0->h_multi_status.h;
  for (uint32_t s = 0; s < j.n_sensors; ++s) micp_record_attempt(j.sensors[s], fs.code, fs.n_uncertain, fs.max_rho[s], fs.max_tau[s]);
  *code = fs.code;
  if (fs.code > 2u) return fail(RMCLHIP_ERR_HIP, "micp_correct_once: the moment-form loop did not report a status");
  if (fs.code == 0u) {
    r0->multi_overflows = 0;
    res->T_onew_oold = r0->h_multi_state.h->T_onew_oold;
    res->merged_o = r0->h_multi_state.h->merged_o;
  }
  return RMCLHIP_OK;
}

// per-iteration form (fallback, or the moment forms are off), behind the finds: the call block goes to the device, then per iteration
// one reduction per sensor and one step launch.  The other sensors' finds ran on their own streams: this stream waits for their
// events first.  The copy of the thread-local call block is asynchronous; the stream is drained before this returns.
static rmclhip_status micp_multi_per_iteration(const MicpMultiJob& j, MicpMultiState* res) {
  rmclhip_rcc* r0 = j.sensors[0];
  hipStream_t st = r0->stream;
  MicpMultiCall* d_call = reinterpret_cast<MicpMultiCall*>(r0->d_multi_blob.p);
  MicpMultiState* d_state = reinterpret_cast<MicpMultiState*>(r0->d_multi_blob.p + sizeof(MicpMultiCall));
  for (uint32_t s = 1; s < j.n_sensors; ++s) {
    rmclhip_rcc* r = j.sensors[s];
    if (!r->ev_join) HIPCHK(hipEventCreateWithFlags(&r->ev_join, hipEventDisableTiming));
    HIPCHK(hipEventRecord(r->ev_join, r->stream));   // (recorded here, not per call: the moment form never needs it)
    HIPCHK(hipStreamWaitEvent(st, r->ev_join, 0));
  }
  HIPCHK(hipMemcpyAsync(d_call, j.call, sizeof(MicpMultiCall), hipMemcpyHostToDevice, st));
  HIPCHK(launch_micp_multi_init(d_call, d_state, st));
  for (uint32_t it = 0; it < j.n_iter; ++it) {
    for (uint32_t s = 0; s < j.n_sensors; ++s) {
      ReduceParams rp = reduce_params(j.sensors[s], j.nred[s], j.max_dist[s], j.call->nblocks[s]);
      rp.Tpre_dev = &d_state->T_snew_sold[s];
      HIPCHK(launch_reduce_partials(rp, st));
    }
    HIPCHK(launch_micp_multi_step(d_call, d_state, st));
  }
  HIPCHK(hipMemcpyAsync(res, d_state, sizeof(MicpMultiState), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_micp_correct_once(rmclhip_rcc* const* sensors, uint32_t n_sensors, const rmclhip_transform* Tom_,
                                         const rmclhip_transform* Tbo_, const double* merge_weight_multiplier, uint32_t n_iter,
                                         double convergence_progress, rmclhip_transform* T_out,
                                         rmclhip_cross_statistics* merged_out) {
  ApiGuard guard_("rmclhip_micp_correct_once");
  if (rmclhip_status st = micp_multi_check(sensors, n_sensors, Tom_, Tbo_, merge_weight_multiplier, T_out)) return st;
  rmclhip_rcc* r0 = sensors[0];
  HIPCHK(hipSetDevice(r0->ctx->device));
  static thread_local MicpMultiCall h_call;
  MicpMultiJob j{sensors, n_sensors, n_iter, to_x(Tom_), &h_call, {}, {}};
  if (rmclhip_status st = micp_multi_prepare(j, Tbo_, merge_weight_multiplier, convergence_progress)) return st;
  const MicpMultiRoute route = micp_multi_route(j);
  // how the last moment form that ran ended: 0 it served the call, 1 a pre-transform left its caps (the device loop would meet the
  // same), 2 too many undecided correspondences -- or none has run yet
  uint32_t code = 2u;
  MicpMultiState res;   // T_onew_oold and merged_o of the form that served the call (the per-iteration form: the whole state)
  if (route.host)
    if (rmclhip_status st = micp_multi_host_form(j, &code, &res)) return st;
  if (code != 0u) {
    if (rmclhip_status st = micp_multi_enqueue_finds(j)) return st;
    if (route.moment && code == 2u)
      if (rmclhip_status st = micp_multi_device_loop(j, &code, &res)) return st;
  }
  if (code != 0u) {
    if (rmclhip_status st = micp_multi_per_iteration(j, &res)) return st;
    if (route.moment) {
      // caps for the next attempt from the pre-transforms this correction ended with (see rmclhip_rcc_correct_once); too many
      // undecided correspondences twice in a row: stop trying for a while
      const MicpMultiFastStatus& ms = *r0->h_multi_status.h;
      for (uint32_t s = 0; s < n_sensors; ++s)
        micp_caps_after_fallback(sensors[s], res.T_snew_sold[s], code == 2u, ms.max_rho[s], ms.max_tau[s]);
      if (code == 2u && ++r0->multi_overflows >= 2u) { r0->multi_holdoff = 32u; r0->multi_overflows = 0; }
    }
  }
  from_x(res.T_onew_oold, T_out);
  if (merged_out) from_cs(res.merged_o, merged_out);
  return RMCLHIP_OK;
}
