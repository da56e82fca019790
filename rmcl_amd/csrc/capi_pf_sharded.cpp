// capi_pf_sharded.cpp -- see capi_internal.h
#include "multi_internal.h"
#include "pose_estimate_host.h"

// ---- the particle filter sharded over the devices of a communicator: one filter replica per rank over ONE host BVH build, the
// cloud block-partitioned (shard_bounds).  A phase ENQUEUES every rank's part before the host waits for any rank. ----
struct PfRank {
  rmclhip_ctx* ctx = nullptr;
  rmclhip_map* map = nullptr;
  rmclhip_pf* pf = nullptr;
  rmclhip_resampler* rs = nullptr;
  rmclhip_surface_sampler* sampler = nullptr;   // rmclhip_pf_sharded_set_surface_sampler: this replica's
  uint32_t lo = 0, hi = 0;
  // sized by pf_sharded_reserve, with cap = shard_cap(n_total, world), at least 1:
  DevBuf<xform> d_poses;                               // this rank's shard (cap)
  DevBuf<rmclhip_particle_attributes> d_attrs;
  DevBuf<xform> d_poses_new;                           // the resamplers' output (cap), swapped with the shard
  DevBuf<rmclhip_particle_attributes> d_attrs_new;
  DevBuf<xform> d_poses_all;                           // the gathered cloud, dense (cap * world)
  DevBuf<rmclhip_particle_attributes> d_attrs_all;
  DevBuf<xform> d_poses_pad;                           // ragged partitions only (pf_sharded_gather_records): the padded all-gather
  DevBuf<rmclhip_particle_attributes> d_attrs_pad;     // lands here (cap * world), *_all is its dense form
  DevBuf<float> d_w_send;                              // cap
  DevBuf<float> d_w_pad;                               // cap * world (all-gather layout)
  DevBuf<float> d_w_all;                               // cap * world: the dense weights of the n_total <= cap * world particles
  DevBuf<double> d_mom_part, d_mom;                    // 256 * 32; 32 (+ 32 reduced)
  PinnedBuf<double> h_mom;                             // 32 (+ 32)
};

struct rmclhip_pf_sharded {
  rmclhip_comm* comm = nullptr;
  uint32_t n_total = 0;
  std::vector<PfRank> ranks;
  rmclhip_pf_params params{2.0f, 100.0f, 100.0f, 0.0f, {0.05f, 80.0f}, 10000u, 0u};
  bool weights_fresh = false;   // every rank's d_w_all holds the likelihoods of the cloud as it is (set by the all-gather, cleared by whatever rewrites attributes)
  bool noise_on = false;        // rmclhip_pf_sharded_set_motion_noise: a step's motion update draws the sampled odometry model's noise
  rmclhip_motion_noise_params noise{};
};

// the C ABI speaks of rmclhip_transform, the kernels of xform: one layout (capi_internal.h)
static rmclhip_transform* api_poses(const DevBuf<xform>& b) { return reinterpret_cast<rmclhip_transform*>(b.p); }

void rmclhip_shard_bounds(uint32_t n, uint32_t rank, uint32_t world, uint32_t* lo, uint32_t* hi) {
  if (world == 0 || !lo || !hi) return;
  shard_bounds(n, rank, world, lo, hi);
}

void rmclhip_pf_sharded_destroy(rmclhip_pf_sharded* h) {
  if (!h) return;
  for (PfRank& R : h->ranks) {
    if (R.ctx) (void)hipSetDevice(R.ctx->device);
    if (R.rs) rmclhip_resampler_destroy(R.rs);
    if (R.sampler) rmclhip_surface_sampler_destroy(R.sampler);
    if (R.pf) rmclhip_pf_destroy(R.pf);
    if (R.map) rmclhip_map_release(R.map);
    if (R.ctx) rmclhip_ctx_destroy(R.ctx);
    R = PfRank();   // the rank's buffers go while its device is current
  }
  delete h;
}

rmclhip_status rmclhip_pf_sharded_create(rmclhip_comm* comm, const float* v, uint32_t nv, const uint32_t* f, uint32_t nf,
                                         rmclhip_pf_sharded** out) {
  ApiGuard guard_("rmclhip_pf_sharded_create");
  if (!out) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_create: out is null");
  *out = nullptr;
  if (!comm) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_create: null communicator");
  BvhHost bvh;   // built ONCE, uploaded to every device (mesh + BVH replicated)
  const std::string err = build_bvh(v, nv, f, nf, bvh);
  if (!err.empty()) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_create: " + err);
  rmclhip_pf_sharded* h = new rmclhip_pf_sharded();
  h->comm = comm;
  h->ranks.resize(comm->devices.size());
  for (uint32_t r = 0; r < h->ranks.size(); ++r) {
    PfRank& R = h->ranks[r];
    rmclhip_status st = rmclhip_ctx_create(comm->devices[r], &R.ctx);
    if (st == RMCLHIP_OK) st = map_upload(R.ctx, bvh, &R.map);
    if (st == RMCLHIP_OK) st = rmclhip_pf_create(R.ctx, R.map, &R.pf);
    if (st == RMCLHIP_OK) st = rmclhip_resampler_create(R.ctx, &R.rs);
    hipError_t e = hipSuccess;
    if (st == RMCLHIP_OK) e = R.d_mom_part.reserve(256 * 32);
    if (st == RMCLHIP_OK && e == hipSuccess) e = R.d_mom.reserve(64);
    if (st == RMCLHIP_OK && e == hipSuccess) e = R.h_mom.reserve(64);
    if (st != RMCLHIP_OK || e != hipSuccess) {
      const std::string msg = (st != RMCLHIP_OK) ? g_err : std::string(hipGetErrorString(e));
      rmclhip_pf_sharded_destroy(h);
      return fail(st != RMCLHIP_OK ? st : RMCLHIP_ERR_HIP, "pf_sharded_create: " + msg);
    }
  }
  *out = h;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_set_params(rmclhip_pf_sharded* h, const rmclhip_pf_params* p) {
  if (!h || !p) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_params: null");
  for (PfRank& R : h->ranks)
    if (rmclhip_status st = rmclhip_pf_set_params(R.pf, p)) return st;
  h->params = *p;
  return RMCLHIP_OK;
}

// ---- a phase of the filter's ranks.  Every rank that has particles, in rank order: its device is made current, `body(R, r)` enqueues
// its part, "E<r>" is traced; the wait is for what the ranks' update streams (R.pf->stream) hold, "W<r>".  Phases of another shape --
// on every rank, without the trace, waiting for the collective streams (comm_wait_all) -- are written out where they are. ----
template <typename Body>
static rmclhip_status pf_sharded_enqueue(rmclhip_pf_sharded* h, Body&& body) {
  for (uint32_t r = 0; r < h->ranks.size(); ++r) {
    PfRank& R = h->ranks[r];
    if (R.hi == R.lo) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    if (rmclhip_status st = body(R, r)) return st;
    trace('E', r);
  }
  return RMCLHIP_OK;
}

static rmclhip_status pf_sharded_wait_updates(rmclhip_pf_sharded* h) {
  for (uint32_t r = 0; r < h->ranks.size(); ++r) {
    PfRank& R = h->ranks[r];
    if (R.hi == R.lo) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(R.pf->tag.wait_chain_end(R.ctx, R.pf->stream));
    trace('W', r);
  }
  return RMCLHIP_OK;
}

// Sizes every rank's buffers for a cloud of n_total particles (grow-only, buffer by buffer), sets its bounds and clears its shard: the
// shards are padded to `cap` records so that the collectives run on equal counts, and the all-gathers send the padding.  `who` names
// the caller in the error message.  A failed allocation leaves the EMPTY cloud behind (a buffer that grew has lost its contents): the
// handle stays usable, and no buffer is ever shorter than the cloud it is used for.
static rmclhip_status pf_sharded_reserve(rmclhip_pf_sharded* h, uint32_t n_total, const char* who_) {
  const std::string who(who_);
  const uint32_t world = static_cast<uint32_t>(h->ranks.size());
  const size_t cap = std::max(shard_cap(n_total, world), 1u), cap_all = cap * world;
  h->weights_fresh = false;
  h->n_total = 0;
  for (PfRank& R : h->ranks) R.lo = R.hi = 0;
  for (PfRank& R : h->ranks) {
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK_AS(who, R.d_poses.reserve(cap)); HIPCHK_AS(who, R.d_attrs.reserve(cap));
    HIPCHK_AS(who, R.d_poses_new.reserve(cap)); HIPCHK_AS(who, R.d_attrs_new.reserve(cap));
    HIPCHK_AS(who, R.d_poses_all.reserve(cap_all)); HIPCHK_AS(who, R.d_attrs_all.reserve(cap_all));
    HIPCHK_AS(who, R.d_w_send.reserve(cap)); HIPCHK_AS(who, R.d_w_pad.reserve(cap_all));
    // d_w_all holds the dense [n_total] weights: n_total <= cap * world for every cloud this capacity admits (sizing it
    // by the n_total of the call that allocated let a later, larger cloud of the same capacity write past its end)
    HIPCHK_AS(who, R.d_w_all.reserve(cap_all));
    HIPCHK(hipMemset(R.d_poses.p, 0, cap * sizeof(xform)));
    HIPCHK(hipMemset(R.d_attrs.p, 0, cap * sizeof(rmclhip_particle_attributes)));
    HIPCHK(hipMemset(R.d_w_send.p, 0, cap * sizeof(float)));
  }
  for (uint32_t r = 0; r < world; ++r) shard_bounds(n_total, r, world, &h->ranks[r].lo, &h->ranks[r].hi);
  h->n_total = n_total;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_set_particles(rmclhip_pf_sharded* h, const rmclhip_transform* poses,
                                                const rmclhip_particle_attributes* attrs, uint32_t n_total) {
  ApiGuard guard_("rmclhip_pf_sharded_set_particles");
  if (!h || (n_total && (!poses || !attrs))) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_particles: null");
  if (rmclhip_status st = pf_sharded_reserve(h, n_total, "pf_sharded_set_particles")) return st;
  for (PfRank& R : h->ranks) {
    if (R.hi == R.lo) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(hipMemcpy(R.d_poses.p, poses + R.lo, (R.hi - R.lo) * sizeof(xform), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.d_attrs.p, attrs + R.lo, (R.hi - R.lo) * sizeof(rmclhip_particle_attributes), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());   // consumers run on non-blocking streams (see upload_on)
  }
  return RMCLHIP_OK;
}

// (re)create the cloud in place: every device fills its own block with the values of the GLOBAL particles lo_r .. hi_r - 1 (the random
// words are a function of the global index: the single-device cloud bit for bit, no collective).  Every rank's launch is enqueued on
// its collective stream before the host waits for any.  job: the pose form (null: uniform in [bb_min, bb_max]); on_surface: every
// replica's surface sampler instead of either.
static rmclhip_status pf_sharded_init_impl(rmclhip_pf_sharded* h, uint32_t n, const float* bb_min, const float* bb_max, const ParticlesPoseJob* job,
                                           uint64_t seed, uint32_t epoch, const char* who, bool on_surface = false) {
  if (rmclhip_status st = pf_sharded_reserve(h, n, who)) return st;
  trace_mark("init:");
  if (rmclhip_status st = pf_sharded_enqueue(h, [&](PfRank& R, uint32_t r) -> rmclhip_status {
        HIPCHK(hipDeviceSynchronize());   // the clears above ran on the null stream, which the collective streams do not wait for
        hipStream_t s = h->comm->streams[r];
        if (on_surface)
          HIPCHK(launch_particles_init_surface(R.d_poses.p, R.d_attrs.p, R.lo, R.hi - R.lo, surface_sample_view(R.sampler), seed, epoch, s));
        else if (job)
          HIPCHK(launch_particles_init_pose(R.d_poses.p, R.d_attrs.p, R.lo, R.hi - R.lo, job->Tlm, job->L, seed, epoch, s));
        else
          HIPCHK(launch_particles_init_uniform(R.d_poses.p, R.d_attrs.p, R.lo, R.hi - R.lo, bb_min, bb_max, seed, epoch, s));
        return RMCLHIP_OK;
      }))
    return st;
  return comm_wait_all(h->comm);
}

rmclhip_status rmclhip_pf_sharded_init_uniform(rmclhip_pf_sharded* h, uint32_t n, const float* bb_min, const float* bb_max, uint64_t seed,
                                               uint32_t epoch) {
  ApiGuard guard_("rmclhip_pf_sharded_init_uniform");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_init_uniform: null");
  if (rmclhip_status st = particles_uniform_check("pf_sharded_init_uniform", 0u, n, bb_min, bb_max)) return st;
  return pf_sharded_init_impl(h, n, bb_min, bb_max, nullptr, seed, epoch, "pf_sharded_init_uniform");
}

rmclhip_status rmclhip_pf_sharded_init_pose(rmclhip_pf_sharded* h, uint32_t n, const rmclhip_transform* Tlm, const double* covariance,
                                            uint64_t seed, uint32_t epoch, double* chol_err_out) {
  ApiGuard guard_("rmclhip_pf_sharded_init_pose");
  if (chol_err_out) *chol_err_out = 0.0;
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_init_pose: null");
  ParticlesPoseJob job;
  if (rmclhip_status st = particles_pose_check("pf_sharded_init_pose", 0u, n, Tlm, covariance, &job)) return st;
  if (rmclhip_status st = pf_sharded_init_impl(h, n, nullptr, nullptr, &job, seed, epoch, "pf_sharded_init_pose")) return st;
  if (chol_err_out) *chol_err_out = job.chol_err;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_download(rmclhip_pf_sharded* h, rmclhip_transform* poses, rmclhip_particle_attributes* attrs) {
  ApiGuard guard_("rmclhip_pf_sharded_download");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_download: null");
  for (PfRank& R : h->ranks) {
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(hipDeviceSynchronize());
    if (R.hi > R.lo) {
      if (poses) HIPCHK(hipMemcpy(poses + R.lo, R.d_poses.p, (R.hi - R.lo) * sizeof(xform), hipMemcpyDeviceToHost));
      if (attrs) HIPCHK(hipMemcpy(attrs + R.lo, R.d_attrs.p, (R.hi - R.lo) * sizeof(rmclhip_particle_attributes), hipMemcpyDeviceToHost));
    }
  }
  return RMCLHIP_OK;
}

// all-gather of likelihood.mean (4 B x N; C5: 4 MB, one collective, never bucketed): afterwards EVERY device holds the dense
// weight vector of the whole cloud (consumer: the tournament / {sum, max}, resampling.cu:108-199)
rmclhip_status rmclhip_pf_allgather_weights(rmclhip_pf_sharded* h) {
  ApiGuard guard_("rmclhip_pf_allgather_weights");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_allgather_weights: null");
  if (h->n_total == 0) return RMCLHIP_OK;
  const uint32_t world = static_cast<uint32_t>(h->ranks.size()), cap = shard_cap(h->n_total, world);
  // extract, gather, compact: three steps per rank on its collective stream, all enqueued before the ONE wait per rank
  std::vector<const void*> send(world);
  std::vector<void*> recv(world);
  for (uint32_t r = 0; r < world; ++r) {
    PfRank& R = h->ranks[r];
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(launch_pf_extract_weights(R.d_attrs.p, R.hi - R.lo, R.d_w_send.p, h->comm->streams[r]));
    send[r] = R.d_w_send.p; recv[r] = R.d_w_pad.p;
  }
  if (rmclhip_status st = comm_allgather(h->comm, send.data(), recv.data(), cap * sizeof(float))) return st;
  for (uint32_t r = 0; r < world; ++r) {
    PfRank& R = h->ranks[r];
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(launch_compact_shards(R.d_w_pad.p, R.d_w_all.p, h->n_total, world, cap, h->comm->streams[r]));
    trace('E', r);
  }
  if (rmclhip_status st = comm_wait_all(h->comm)) return st;
  h->weights_fresh = true;
  return RMCLHIP_OK;
}

// PCDSensorUpdater*::update on every device's block of the particles (concurrently: one stream per device), then the
// weight all-gather
rmclhip_status rmclhip_pf_update_sharded(rmclhip_pf_sharded* h, const rmclhip_range_measurement* beams, uint32_t n_beams,
                                         const rmclhip_transform* Tsb) {
  ApiGuard guard_("rmclhip_pf_update_sharded");
  if (!h || !Tsb || (n_beams && !beams)) return fail(RMCLHIP_ERR_INVALID, "pf_update_sharded: null");
  h->weights_fresh = false;
  trace_mark("update:");
  if (rmclhip_status st = pf_sharded_enqueue(h, [&](PfRank& R, uint32_t r) -> rmclhip_status {
        if (rmclhip_status us = rmclhip_pf_update_async(R.pf, api_poses(R.d_poses), R.d_attrs.p, R.hi - R.lo, beams, n_beams, Tsb)) return us;
        // the gather runs on the communicator's stream of this device: it waits for the update on the DEVICE (an event), not on the host
        HIPCHK(hipEventRecord(R.pf->ev1, R.pf->stream));
        HIPCHK(hipStreamWaitEvent(h->comm->streams[r], R.pf->ev1, 0));
        return RMCLHIP_OK;
      }))
    return st;
  trace_mark("gather:");
  return rmclhip_pf_allgather_weights(h);
}

// MotionUpdater<MemT>::update on every device's block (particle_motion.cu:11-46 + the collision ray of TFMotionUpdaterCPU.cpp:17-50,
// 207-221): one k_pf_motion per rank on that rank's update stream.  The launches are left in flight -- the sensor update of the same
// cycle is enqueued behind them on the same streams (rmclhip_pf_sharded_step).
// noise: null = the deterministic update; else every rank draws for the GLOBAL indices of its block (first = R.lo)
static rmclhip_status pf_sharded_motion_enqueue(rmclhip_pf_sharded* h, const rmclhip_transform* T_bnew_bold, double forget_rate, int check_collision,
                                                const MotionNoiseKernelParams* noise = nullptr) {
  h->weights_fresh = false;   // (a particle that crosses a wall gets likelihood {0, 0, MAX})
  return pf_sharded_enqueue(h, [&](PfRank& R, uint32_t) {
    MotionNoiseKernelParams nz{};
    if (noise) { nz = *noise; nz.first = R.lo; }
    return pf_motion_enqueue(R.pf, R.d_poses.p, R.d_attrs.p, R.hi - R.lo, to_x(T_bnew_bold), forget_rate, h->params.max_n_meas, check_collision != 0,
                             noise ? &nz : nullptr);
  });
}

rmclhip_status rmclhip_pf_sharded_motion_update_noisy(rmclhip_pf_sharded* h, const rmclhip_transform* T_bnew_bold, double forget_rate,
                                                      int check_collision, const float* sigma, uint64_t seed, uint32_t step) {
  ApiGuard guard_("rmclhip_pf_sharded_motion_update_noisy");
  if (!h || !T_bnew_bold) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_motion_update_noisy: null");
  MotionNoiseKernelParams nz{};
  bool noisy = false;
  if (rmclhip_status st = motion_noise_kernel_params("pf_sharded_motion_update_noisy", sigma, seed, step, 0u, &nz, &noisy)) return st;
  if (!(forget_rate >= 0.0 && forget_rate <= 1.0)) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_motion_update_noisy: forget_rate outside [0, 1] (or NaN)");
  if (h->n_total == 0) return RMCLHIP_OK;
  trace_mark("motion:");
  if (rmclhip_status st = pf_sharded_motion_enqueue(h, T_bnew_bold, forget_rate, check_collision, noisy ? &nz : nullptr)) return st;
  return pf_sharded_wait_updates(h);
}

rmclhip_status rmclhip_pf_sharded_set_motion_noise(rmclhip_pf_sharded* h, const rmclhip_motion_noise_params* params) {
  ApiGuard guard_("rmclhip_pf_sharded_set_motion_noise");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_motion_noise: null");
  if (!params) { h->noise_on = false; return RMCLHIP_OK; }
  if (rmclhip_status st = motion_noise_params_check("pf_sharded_set_motion_noise", params)) return st;
  h->noise = *params;
  h->noise_on = true;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_motion_update(rmclhip_pf_sharded* h, const rmclhip_transform* T_bnew_bold, double forget_rate,
                                                int check_collision) {
  ApiGuard guard_("rmclhip_pf_sharded_motion_update");
  if (!h || !T_bnew_bold) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_motion_update: null");
  if (!(forget_rate >= 0.0 && forget_rate <= 1.0)) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_motion_update: forget_rate outside [0, 1] (or NaN)");
  if (h->n_total == 0) return RMCLHIP_OK;
  trace_mark("motion:");
  if (rmclhip_status st = pf_sharded_motion_enqueue(h, T_bnew_bold, forget_rate, check_collision)) return st;
  return pf_sharded_wait_updates(h);
}

// ---- the surface constraint on the sharded cloud (capi_surface.cpp has the single-device entry points) ----
rmclhip_status rmclhip_pf_sharded_set_surface(rmclhip_pf_sharded* h, const rmclhip_surface_params* params) {
  ApiGuard guard_("rmclhip_pf_sharded_set_surface");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_surface: null");
  if (params)
    if (rmclhip_status st = surface_params_check("pf_sharded_set_surface", params)) return st;
  for (PfRank& R : h->ranks)
    if (rmclhip_status st = rmclhip_pf_set_surface(R.pf, params)) return st;
  return RMCLHIP_OK;
}

// the sum of every device's last counts (ranks without particles launched nothing: their block is skipped)
static void pf_sharded_sum_surface_stats(rmclhip_pf_sharded* h, rmclhip_surface_stats* out) {
  std::memset(out, 0, sizeof(*out));
  for (PfRank& R : h->ranks) {
    if (R.hi == R.lo || !R.pf->h_surf.p) continue;
    out->n_particles += R.pf->h_surf.p[0]; out->n_snapped += R.pf->h_surf.p[1]; out->n_missed += R.pf->h_surf.p[2]; out->n_steep += R.pf->h_surf.p[3];
  }
}

rmclhip_status rmclhip_pf_sharded_get_surface_stats(rmclhip_pf_sharded* h, rmclhip_surface_stats* out) {
  ApiGuard guard_("rmclhip_pf_sharded_get_surface_stats");
  if (!h || !out) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_get_surface_stats: null");
  for (PfRank& R : h->ranks) {   // (a step leaves the counts' copy behind the motion launch on the rank's stream)
    if (R.hi == R.lo || !R.pf->h_surf.p) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(hipStreamSynchronize(R.pf->stream));
  }
  pf_sharded_sum_surface_stats(h, out);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_constrain_to_surface(rmclhip_pf_sharded* h, const rmclhip_surface_params* params, rmclhip_surface_stats* stats_out) {
  ApiGuard guard_("rmclhip_pf_sharded_constrain_to_surface");
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_constrain_to_surface: null");
  if (rmclhip_status st = surface_params_check("pf_sharded_constrain_to_surface", params)) return st;
  if (h->n_total == 0) return RMCLHIP_OK;
  if (params->on_miss != 0u) h->weights_fresh = false;
  trace_mark("surface:");
  if (rmclhip_status st = pf_sharded_enqueue(h, [&](PfRank& R, uint32_t) {
        return pf_surface_enqueue(R.pf, R.d_poses.p, R.d_attrs.p, R.hi - R.lo, *params, h->params.max_n_meas);
      }))
    return st;
  if (rmclhip_status st = pf_sharded_wait_updates(h)) return st;
  if (stats_out) pf_sharded_sum_surface_stats(h, stats_out);
  return RMCLHIP_OK;
}

// ---- the surface sampler on the sharded cloud (capi_surface_sample.cpp / capi_particles.cpp have the single-device entry points) ----
rmclhip_status rmclhip_pf_sharded_set_surface_sampler(rmclhip_pf_sharded* h, const rmclhip_surface_sample_params* params) {
  ApiGuard guard_("rmclhip_pf_sharded_set_surface_sampler");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_surface_sampler: null");
  std::vector<rmclhip_surface_sampler*> fresh(h->ranks.size(), nullptr);
  if (params) {
    if (rmclhip_status st = surface_sample_params_check("pf_sharded_set_surface_sampler", params)) return st;
    for (size_t r = 0; r < h->ranks.size(); ++r)
      if (rmclhip_status st = rmclhip_surface_sampler_create(h->ranks[r].map, params, &fresh[r])) {   // the previous samplers stay
        const std::string msg = g_err;
        for (rmclhip_surface_sampler* sm : fresh) rmclhip_surface_sampler_destroy(sm);
        return fail(st, msg);
      }
  }
  for (size_t r = 0; r < h->ranks.size(); ++r) {
    rmclhip_surface_sampler_destroy(h->ranks[r].sampler);
    h->ranks[r].sampler = fresh[r];
  }
  return RMCLHIP_OK;
}

static rmclhip_status pf_sharded_need_samplers(rmclhip_pf_sharded* h, const std::string& who) {
  for (PfRank& R : h->ranks)
    if (!R.sampler) return fail(RMCLHIP_ERR_INVALID, who + ": no surface sampler is set (rmclhip_pf_sharded_set_surface_sampler)");
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_init_surface(rmclhip_pf_sharded* h, uint32_t n, uint64_t seed, uint32_t epoch) {
  ApiGuard guard_("rmclhip_pf_sharded_init_surface");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_init_surface: null");
  if (rmclhip_status st = pf_sharded_need_samplers(h, "pf_sharded_init_surface")) return st;
  if (rmclhip_status st = particles_range_check("pf_sharded_init_surface", 0u, n)) return st;
  return pf_sharded_init_impl(h, n, nullptr, nullptr, nullptr, seed, epoch, "pf_sharded_init_surface", true);
}

// every replica replaces slots of its own block in place; the counts land in each sampler's pinned word and are summed here
rmclhip_status rmclhip_pf_sharded_inject_surface(rmclhip_pf_sharded* h, double p_inject, uint64_t seed, uint32_t step, uint32_t* n_injected_out) {
  ApiGuard guard_("rmclhip_pf_sharded_inject_surface");
  if (n_injected_out) *n_injected_out = 0u;
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_inject_surface: null");
  if (rmclhip_status st = pf_sharded_need_samplers(h, "pf_sharded_inject_surface")) return st;
  unsigned long long threshold = 0ull;
  if (rmclhip_status st = surface_inject_threshold("pf_sharded_inject_surface", p_inject, &threshold)) return st;
  if (h->n_total == 0 || threshold == 0ull) return RMCLHIP_OK;
  h->weights_fresh = false;
  trace_mark("inject:");
  for (uint32_t r = 0; r < h->ranks.size(); ++r) {   // every rank's launch is in flight before the host waits for any
    PfRank& R = h->ranks[r];
    *R.sampler->h_count.p = 0u;   // (of a rank without particles too: the sum below reads every rank's)
    if (R.hi == R.lo) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    if (rmclhip_status st = surface_inject_enqueue(R.sampler, R.d_poses.p, R.d_attrs.p, R.lo, R.hi - R.lo, threshold, seed, step, h->comm->streams[r]))
      return st;
    trace('E', r);
  }
  if (rmclhip_status st = comm_wait_all(h->comm)) return st;
  uint32_t total = 0u;
  for (PfRank& R : h->ranks) total += *R.sampler->h_count.p;
  if (n_injected_out) *n_injected_out = total;
  return RMCLHIP_OK;
}

// ---- the distance field on the sharded cloud (capi_field.cpp has the single-device entry points) ----
// every replica builds its own field from its own copy of the map; its filter handle keeps the only reference.  dense or banded: the
// layout's parameters (at most one is given); neither: every replica's field is taken off
static rmclhip_status sharded_set_field(rmclhip_pf_sharded* h, const rmclhip_field_params* dense, const rmclhip_band_field_params* banded) {
  for (PfRank& R : h->ranks) {   // refuse before any replica is touched
    rmclhip_field_info info;
    rmclhip_band_field_info band;
    const float *lo = R.map->info.bbox_min, *hi = R.map->info.bbox_max;
    if (rmclhip_status st = banded ? rmclhip_band_field_layout_host(lo, hi, banded, &info, &band)
                            : dense ? rmclhip_field_layout_host(lo, hi, dense, &info) : RMCLHIP_OK)
      return st;
  }
  for (PfRank& R : h->ranks) {
    rmclhip_field* fd = nullptr;
    if (rmclhip_status st = banded ? rmclhip_field_create_banded(R.ctx, R.map, banded, &fd)
                            : dense ? rmclhip_field_create(R.ctx, R.map, dense, &fd) : RMCLHIP_OK)
      return st;
    const rmclhip_status st = rmclhip_pf_set_field(R.pf, fd);
    rmclhip_field_destroy(fd);
    if (st) return st;
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_set_field(rmclhip_pf_sharded* h, const rmclhip_field_params* params) {
  ApiGuard guard_("rmclhip_pf_sharded_set_field");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_field: null");
  return sharded_set_field(h, params, nullptr);
}

// the same with a banded field on every replica (capi_band_field.cpp)
rmclhip_status rmclhip_pf_sharded_set_field_banded(rmclhip_pf_sharded* h, const rmclhip_band_field_params* params) {
  ApiGuard guard_("rmclhip_pf_sharded_set_field_banded");
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_set_field_banded: null");
  return sharded_set_field(h, nullptr, params);
}

// every replica refines its own block on its own field (capi_refine.cpp); no collective, attributes and weights are not touched
rmclhip_status rmclhip_pf_sharded_refine(rmclhip_pf_sharded* h, const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                         const rmclhip_refine_params* params, rmclhip_refine_stats* stats_out) {
  ApiGuard guard_("rmclhip_pf_sharded_refine");
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_refine: null");
  for (PfRank& R : h->ranks)
    if (!R.pf->field) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_refine: no distance field is set (rmclhip_pf_sharded_set_field)");
  rmclhip_refine_params p;
  if (rmclhip_status st = refine_check("pf_sharded_refine", h, h->n_total, beams, n_beams, Tsb, params, &p)) return st;
  for (PfRank& R : h->ranks)
    if (rmclhip_status st = field_band_check("pf_sharded_refine", R.pf->field, p.max_dist)) return st;
  if (h->n_total == 0) return RMCLHIP_OK;
  for (PfRank& R : h->ranks) {   // every rank's launch is in flight before the host waits for any (not traced)
    if (R.hi == R.lo) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    if (rmclhip_status st = refine_enqueue(R.pf->field, R.pf->stream, R.pf->refine, api_poses(R.d_poses), R.hi - R.lo, beams, n_beams, Tsb, p, nullptr,
                                           stats_out != nullptr))
      return st;
  }
  for (PfRank& R : h->ranks) {
    if (R.hi == R.lo) continue;
    HIPCHK(hipSetDevice(R.ctx->device));
    if (rmclhip_status st = refine_finish(R.pf->stream, R.pf->refine, R.hi - R.lo, stats_out)) return st;
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_get_weights(rmclhip_pf_sharded* h, uint32_t rank, float* weights_host) {
  ApiGuard guard_("rmclhip_pf_sharded_get_weights");
  if (!h || !weights_host || rank >= h->ranks.size()) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_get_weights: bad arguments");
  PfRank& R = h->ranks[rank];
  HIPCHK(hipSetDevice(R.ctx->device));
  if (h->n_total) HIPCHK(hipMemcpy(weights_host, R.d_w_all.p, h->n_total * sizeof(float), hipMemcpyDeviceToHost));
  return RMCLHIP_OK;
}

// moments of one pass on every rank's overlap with [0, n_use), all-reduced (sums with ncclSum, maxima with ncclMax);
// result (identical on every rank) in out32
static rmclhip_status sharded_moments(rmclhip_pf_sharded* h, uint32_t n_use, int pass, double L_sum, const xform& Tbm, double* out32) {
  const uint32_t world = static_cast<uint32_t>(h->ranks.size());
  for (uint32_t r = 0; r < world; ++r) {
    PfRank& R = h->ranks[r];
    HIPCHK(hipSetDevice(R.ctx->device));
    const uint32_t hi = std::min(R.hi, n_use);
    const uint32_t n = (hi > R.lo) ? (hi - R.lo) : 0u;
    HIPCHK(launch_pose_moments(R.d_poses.p, R.d_attrs.p, n, pass, L_sum, Tbm, R.d_mom_part.p, R.d_mom.p, h->comm->streams[r]));
  }
  std::vector<const double*> s_sum(world), s_max(world);
  std::vector<double*> r_sum(world), r_max(world);
  for (uint32_t r = 0; r < world; ++r) {
    double* mom = h->ranks[r].d_mom.p;
    s_sum[r] = mom; r_sum[r] = mom + 32; s_max[r] = mom + 24; r_max[r] = mom + 32 + 24;
  }
  if (rmclhip_status st = comm_allreduce_f64(h->comm, s_sum.data(), r_sum.data(), 24, false)) return st;
  if (rmclhip_status st = comm_allreduce_f64(h->comm, s_max.data(), r_max.data(), 8, true)) return st;
  PfRank& R0 = h->ranks[0];
  HIPCHK(hipSetDevice(R0.ctx->device));
  HIPCHK(hipMemcpyAsync(R0.h_mom.p, R0.d_mom.p + 32, 32 * sizeof(double), hipMemcpyDeviceToHost, h->comm->streams[0]));
  if (rmclhip_status st = comm_wait_all(h->comm)) return st;
  std::memcpy(out32, R0.h_mom.p, 32 * sizeof(double));
  return RMCLHIP_OK;
}

// global {sum, max} of the likelihoods (simple_stats_kernel, resampling.cu:41-92; consumer rmcl_localization.cpp:664-689 and the residual
// resampler's size_t(L / sum * N)).  Round 6: NO collective -- after the weight all-gather every rank holds all N likelihoods, so every
// rank reduces its own copy with the single-device kernel (same blocks, same order: the value is the single-device value bit for bit
// whatever library moved the weights, and does not depend on a reduction order RCCL is free to choose).  The name is kept for the ABI.
// A cloud whose attributes changed since the last gather (set_particles, motion update, resampling) is gathered first.
rmclhip_status rmclhip_pf_allreduce_stats(rmclhip_pf_sharded* h, rmclhip_likelihood_stats* out) {
  ApiGuard guard_("rmclhip_pf_allreduce_stats");
  if (!h || !out) return fail(RMCLHIP_ERR_INVALID, "pf_allreduce_stats: null");
  if (h->n_total == 0) { out->sum = 0.f; out->max = 0.f; return RMCLHIP_OK; }
  if (!h->weights_fresh)
    if (rmclhip_status st = rmclhip_pf_allgather_weights(h)) return st;
  for (uint32_t r = 0; r < h->ranks.size(); ++r) {
    PfRank& R = h->ranks[r];
    HIPCHK(hipSetDevice(R.ctx->device));
    HIPCHK(launch_likelihood_stats_dense(R.d_w_all.p, h->n_total, R.rs->d_psum.p, R.rs->d_pmax.p, R.rs->d_out.p, h->comm->streams[r]));
    trace('E', r);
  }
  // the host needs ONE copy: rank 0's (the other ranks keep theirs on the device, ordered on their streams)
  PfRank& R0 = h->ranks[0];
  HIPCHK(hipSetDevice(R0.ctx->device));
  HIPCHK(hipMemcpyAsync(R0.rs->h_out.p, R0.rs->d_out.p, 2 * sizeof(float), hipMemcpyDeviceToHost, h->comm->streams[0]));
  HIPCHK(hipStreamSynchronize(h->comm->streams[0]));
  trace('W', 0u);
  out->sum = R0.rs->h_out.p[0];
  out->max = R0.rs->h_out.p[1];
  return RMCLHIP_OK;
}

// RmclNode::estimateStats (rmcl_localization.cpp:642-731) over the first n_induction particles of the sharded cloud (the passes'
// host side: pose_estimate_host.h)
rmclhip_status rmclhip_pf_allreduce_pose_estimate(rmclhip_pf_sharded* h, uint32_t n_induction, rmclhip_pose_estimate* out) {
  ApiGuard guard_("rmclhip_pf_allreduce_pose_estimate");
  if (!h || !out) return fail(RMCLHIP_ERR_INVALID, "pf_allreduce_pose_estimate: null");
  const uint32_t n_use = std::min(n_induction, h->n_total);
  return pose_estimate_passes("pf_allreduce_pose_estimate", n_use,
                              [&](int pass, double L_sum, const xform& Tbm, double* m) { return sharded_moments(h, n_use, pass, L_sum, Tbm, m); }, out);
}

// all-gather of the particle records (68 B per particle) on every rank's collective stream: afterwards -- in stream order, nothing
// here waits -- every rank's d_poses_all / d_attrs_all hold the dense cloud.  The shards are not touched.
static rmclhip_status pf_sharded_gather_records(rmclhip_pf_sharded* h, const char* who, const char* mark) {
  const uint32_t world = static_cast<uint32_t>(h->ranks.size()), cap = shard_cap(h->n_total, world);
  // a ragged partition (n_total not a multiple of the number of devices): the all-gather needs equal counts, so the padded shards
  // land in a second buffer and one kernel per record type squeezes the padding out (68 B x N read + written once more per rank)
  const bool ragged = (h->n_total % world) != 0u && world > 1u;
  if (ragged) {
    const size_t cap_all = static_cast<size_t>(cap) * world;
    for (PfRank& R : h->ranks) {
      if (R.d_poses_pad.cap >= cap_all && R.d_attrs_pad.cap >= cap_all) continue;
      HIPCHK(hipSetDevice(R.ctx->device));
      HIPCHK_AS(who, R.d_poses_pad.reserve(cap_all));
      HIPCHK_AS(who, R.d_attrs_pad.reserve(cap_all));
    }
  }
  // (1) the cloud (68 B per particle) is all-gathered on every rank's collective stream; (2) BEHIND it, on the same stream, every
  // rank's tournament / slot fill over its own champions -- enqueued for ALL ranks before the host waits for any (round 3 ran the N
  // tournaments one after the other, each with its own launch + wait).  The tournament reads one enemy per champion; gathering the
  // whole cloud instead of an indexed exchange of the winners costs 68 B x N x (world - 1) / world per rank: C5 = 59.5 MB per rank,
  // ~0.2 ms at the ~300 GB/s an 8-GPU RCCL all-gather reaches over xGMI (an estimate: no node to measure on) against a 2.9 ms
  // sensor update per resampling step -- accepted, stated, and the first thing to replace if a profile says otherwise.
  trace_mark(mark);
  std::vector<const void*> sp(world), sa(world);
  std::vector<void*> rp(world), ra_(world);
  for (uint32_t r = 0; r < world; ++r) {
    PfRank& R = h->ranks[r];
    sp[r] = R.d_poses.p; rp[r] = ragged ? R.d_poses_pad.p : R.d_poses_all.p;
    sa[r] = R.d_attrs.p; ra_[r] = ragged ? R.d_attrs_pad.p : R.d_attrs_all.p;
  }
  if (rmclhip_status st = comm_allgather(h->comm, sp.data(), rp.data(), cap * sizeof(xform))) return st;
  if (rmclhip_status st = comm_allgather(h->comm, sa.data(), ra_.data(), cap * sizeof(rmclhip_particle_attributes))) return st;
  if (ragged) {
    for (uint32_t r = 0; r < world; ++r) {
      PfRank& R = h->ranks[r];
      HIPCHK(hipSetDevice(R.ctx->device));
      HIPCHK(launch_compact_records(R.d_poses_pad.p, R.d_poses_all.p, h->n_total, world, cap, sizeof(xform), h->comm->streams[r]));
      HIPCHK(launch_compact_records(R.d_attrs_pad.p, R.d_attrs_all.p, h->n_total, world, cap, sizeof(rmclhip_particle_attributes), h->comm->streams[r]));
    }
  }
  return RMCLHIP_OK;
}

// distributed gladiator tournament: the enemy of a champion may live on any rank, so the cloud (68 B per
// particle) is all-gathered once, then every rank resamples its own champions against the gathered copy; the Philox
// stream is a function of the GLOBAL champion index, so the result equals the single-GPU tournament
static rmclhip_status pf_sharded_resample_impl(rmclhip_pf_sharded* h, const rmclhip_gladiator_config* cfg, uint64_t seed, uint32_t step,
                                              bool residual) {
  if (!h || !cfg) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_resample: null");
  {   // before the all-gather: a refused call leaves the cloud, and the gathered copies, alone
    rmclhip_gladiator_config c = *cfg;
    if (residual) c.trans_dist_metric = 0u;   // ignored by the residual resampler
    if (rmclhip_status cs = resampler_config_check(residual ? "pf_sharded_resample_residual" : "pf_sharded_resample", &c)) return cs;
  }
  if (h->n_total == 0) return RMCLHIP_OK;
  h->weights_fresh = false;   // the cloud is about to be replaced
  const uint32_t world = static_cast<uint32_t>(h->ranks.size());
  if (rmclhip_status st = pf_sharded_gather_records(h, "pf_sharded_resample", "resample:")) return st;
  if (!residual) {
    for (uint32_t r = 0; r < world; ++r) {   // (no device is made current here: gladiator_enqueue launches on the stream it is given)
      PfRank& R = h->ranks[r];
      if (R.hi == R.lo) continue;
      // every device resamples ITS champions against the whole gathered cloud: the random stream is a function of the global index
      if (rmclhip_status st = gladiator_enqueue(R.rs, api_poses(R.d_poses_all), R.d_attrs_all.p, h->n_total, api_poses(R.d_poses_new), R.d_attrs_new.p,
                                                R.lo, R.hi - R.lo, cfg, seed, step, h->comm->streams[r]))
        return st;
      trace('E', r);
    }
    if (rmclhip_status st = comm_wait_all(h->comm)) return st;
  } else {
    std::vector<ResidualJob> jobs(world);
    for (uint32_t r = 0; r < world; ++r) {
      PfRank& R = h->ranks[r];
      ResidualJob& j = jobs[r];
      j.r = R.rs; j.st = h->comm->streams[r];
      j.poses = api_poses(R.d_poses_all); j.attrs = R.d_attrs_all.p;
      j.poses_new = api_poses(R.d_poses_new); j.attrs_new = R.d_attrs_new.p;
      j.n_particles = h->n_total; j.n_new = h->n_total; j.first = R.lo; j.count = R.hi - R.lo; j.cfg = cfg; j.seed = seed; j.step = step;
      if (rmclhip_status st = residual_check(j)) return st;
    }
    // three phases, each enqueued on every rank before the one wait per rank (round 3: three waits per rank, rank after rank)
    for (uint32_t r = 0; r < world; ++r) { if (rmclhip_status st = residual_prepare_enqueue(jobs[r])) return st; trace('E', r); }
    if (rmclhip_status st = comm_wait_all(h->comm)) return st;
    for (bool first_try = true;; first_try = false) {
      bool any = false;
      for (uint32_t r = 0; r < world; ++r) {
        if (!jobs[r].active || jobs[r].filled) continue;
        any = true;
        if (rmclhip_status st = residual_draws_enqueue(jobs[r], first_try)) return st;
        trace('E', r);
      }
      if (!any) break;
      if (rmclhip_status st = comm_wait_all(h->comm)) return st;
      for (uint32_t r = 0; r < world; ++r) residual_draws_done(jobs[r]);
    }
    for (uint32_t r = 0; r < world; ++r) { if (rmclhip_status st = residual_fill_enqueue(jobs[r], false)) return st; trace('E', r); }
    if (rmclhip_status st = comm_wait_all(h->comm)) return st;
  }
  for (PfRank& R : h->ranks) {
    if (R.hi == R.lo) continue;
    std::swap(R.d_poses, R.d_poses_new);
    std::swap(R.d_attrs, R.d_attrs_new);
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_sharded_resample(rmclhip_pf_sharded* h, const rmclhip_gladiator_config* cfg, uint64_t seed, uint32_t step) {
  ApiGuard guard_("rmclhip_pf_sharded_resample");
  return pf_sharded_resample_impl(h, cfg, seed, step, false);
}

rmclhip_status rmclhip_pf_sharded_resample_residual(rmclhip_pf_sharded* h, const rmclhip_gladiator_config* cfg, uint64_t seed, uint32_t step) {
  ApiGuard guard_("rmclhip_pf_sharded_resample_residual");
  return pf_sharded_resample_impl(h, cfg, seed, step, true);
}

// One cycle of the filter node (rmcl_localization.cpp:84, 432-552: motionUpdate, sensorUpdate, resampling with its {sum, max}) on the
// sharded cloud: motion (nullable T_bnew_bold: skipped) -> sensor update -> weight all-gather -> {sum, max} all-reduce -> resampling
// (resample: 0 none, 1 gladiator tournament, 2 residual).  Motion and sensor update of a rank share its stream, so the host waits
// once for the gather, once for the statistics and once inside the resampler -- never between motion and update.
rmclhip_status rmclhip_pf_sharded_step(rmclhip_pf_sharded* h, const rmclhip_transform* T_bnew_bold, double forget_rate, int check_collision,
                                       const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                       int resample, const rmclhip_gladiator_config* cfg, uint64_t seed, uint32_t step,
                                       rmclhip_likelihood_stats* stats_out) {
  ApiGuard guard_("rmclhip_pf_sharded_step");
  if (!h || !Tsb || (n_beams && !beams)) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_step: null");
  if (resample < 0 || resample > 2 || (resample != 0 && !cfg)) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_step: bad resampling arguments");
  if (T_bnew_bold && !(forget_rate >= 0.0 && forget_rate <= 1.0))
    return fail(RMCLHIP_ERR_INVALID, "pf_sharded_step: forget_rate outside [0, 1] (or NaN)");
  MotionNoiseKernelParams nz{};
  bool noisy = false;
  if (T_bnew_bold && h->noise_on) {   // rmclhip_pf_sharded_set_motion_noise: sigma of THIS step, drawn with this cycle's seed and step
    float sigma[6];
    if (rmclhip_status ns = motion_noise_sigma("pf_sharded_step", &h->noise, T_bnew_bold, sigma)) return ns;
    if (rmclhip_status ns = motion_noise_kernel_params("pf_sharded_step", sigma, seed, step, 0u, &nz, &noisy)) return ns;
  }
  if (resample != 0) {   // the resampler's own rule, before the motion and sensor updates change the cloud
    rmclhip_gladiator_config c = *cfg;
    if (resample == 2) c.trans_dist_metric = 0u;
    if (rmclhip_status cs = resampler_config_check("pf_sharded_step", &c)) return cs;
  }
  if (h->n_total == 0) { if (stats_out) { stats_out->sum = 0.f; stats_out->max = 0.f; } return RMCLHIP_OK; }
  if (T_bnew_bold) {
    trace_mark("motion:");
    if (rmclhip_status st = pf_sharded_motion_enqueue(h, T_bnew_bold, forget_rate, check_collision, noisy ? &nz : nullptr)) return st;
  }
  if (rmclhip_status st = rmclhip_pf_update_sharded(h, beams, n_beams, Tsb)) return st;
  rmclhip_likelihood_stats st_local;
  trace_mark("stats:");
  if (rmclhip_status st = rmclhip_pf_allreduce_stats(h, stats_out ? stats_out : &st_local)) return st;
  if (resample != 0) {
    if (rmclhip_status st = pf_sharded_resample_impl(h, cfg, seed, step, resample == 2)) return st;
  }
  return RMCLHIP_OK;
}

// pose hypotheses of the sharded cloud: the records are gathered as the resamplers gather them, then rank 0 runs the single-device
// path (capi_hypotheses.cpp) on its gathered copy with its own resampler handle -- the single-device bytes.  The shards stay as they are.
rmclhip_status rmclhip_pf_sharded_pose_hypotheses(rmclhip_pf_sharded* h, const rmclhip_kld_params* bins, uint32_t max_hypotheses,
                                                  rmclhip_pose_hypothesis* out, uint32_t* n_out, uint32_t* n_clusters_out) {
  ApiGuard guard_("rmclhip_pf_sharded_pose_hypotheses");
  if (n_out) *n_out = 0;
  if (n_clusters_out) *n_clusters_out = 0;
  if (!h) return fail(RMCLHIP_ERR_INVALID, "pf_sharded_pose_hypotheses: null");
  if (rmclhip_status st = pose_hypotheses_check("pf_sharded_pose_hypotheses", h->ranks[0].rs, bins, max_hypotheses, out, n_out, n_clusters_out)) return st;
  if (h->n_total == 0) return RMCLHIP_OK;
  if (rmclhip_status st = pf_sharded_gather_records(h, "pf_sharded_pose_hypotheses", "hypotheses:")) return st;
  if (rmclhip_status st = comm_wait_all(h->comm)) return st;
  PfRank& R0 = h->ranks[0];
  return pose_hypotheses_run("pf_sharded_pose_hypotheses", R0.rs, api_poses(R0.d_poses_all), R0.d_attrs_all.p, h->n_total, bins, max_hypotheses, out, n_out,
                             n_clusters_out, nullptr);
}
