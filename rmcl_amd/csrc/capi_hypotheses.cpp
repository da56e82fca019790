// capi_hypotheses.cpp -- see capi_internal.h: the single-device pose estimate and the pose hypotheses (include/rmclhip.h states the
// rules; hypotheses.hip implements them; pose_estimate_host.h is the estimate's host side, shared with the sharded filter)
#include "capi_internal.h"
#include "pose_estimate_host.h"

// one pass of k_pose_moments over n particles of a cloud on the handle's stream, landed on the host; labels (nullable): the filter
static rmclhip_status resampler_moments(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                        uint32_t n, int pass, double L_sum, const xform& Tbm, double* out32, const uint32_t* labels, uint32_t want) {
  HIPCHK(r->d_hyp_mom.reserve(256 * 32 + 32));
  double* d_out = r->d_hyp_mom.p + 256 * 32;
  HIPCHK(launch_pose_moments(reinterpret_cast<const xform*>(poses_dev), attrs_dev, n, pass, L_sum, Tbm, r->d_hyp_mom.p, d_out, r->stream, labels, want));
  HIPCHK(hipMemcpyAsync(out32, d_out, 32 * sizeof(double), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_particles_pose_estimate(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                               uint32_t n, uint32_t n_induction, rmclhip_pose_estimate* out) {
  ApiGuard guard_("rmclhip_particles_pose_estimate");
  if (!r || !out) return fail(RMCLHIP_ERR_INVALID, "particles_pose_estimate: null");
  const uint32_t n_use = std::min(n_induction, n);
  if (n_use != 0 && (!poses_dev || !attrs_dev)) {
    std::memset(out, 0, sizeof(*out));
    return fail(RMCLHIP_ERR_INVALID, "particles_pose_estimate: null particle buffers");
  }
  if (n_use != 0) HIPCHK(hipSetDevice(r->ctx->device));
  return pose_estimate_passes("particles_pose_estimate", n_use,
                              [&](int pass, double L_sum, const xform& Tbm, double* m) {
                                return resampler_moments(r, poses_dev, attrs_dev, n_use, pass, L_sum, Tbm, m, nullptr, 0u);
                              },
                              out);
}

rmclhip_status pose_hypotheses_check(const char* who_, rmclhip_resampler* r, const rmclhip_kld_params* bins, uint32_t max_hypotheses,
                                     rmclhip_pose_hypothesis* out, uint32_t* n_out, uint32_t* n_clusters_out) {
  const std::string who(who_);
  if (!r || !out || !n_out || !n_clusters_out) return fail(RMCLHIP_ERR_INVALID, who + ": null");
  if (rmclhip_status st = kld_bins_check(who_, bins)) return st;
  if (max_hypotheses == 0u || max_hypotheses > kMaxHypotheses) return fail(RMCLHIP_ERR_INVALID, who + ": max_hypotheses must be in [1, 64]");
  return RMCLHIP_OK;
}

// the arguments are checked (pose_hypotheses_check) and n > 0
rmclhip_status pose_hypotheses_run(const char* who_, rmclhip_resampler* r, const rmclhip_transform* poses_dev,
                                   const rmclhip_particle_attributes* attrs_dev, uint32_t n, const rmclhip_kld_params* bins, uint32_t max_hypotheses,
                                   rmclhip_pose_hypothesis* out, uint32_t* n_out, uint32_t* n_clusters_out, uint32_t* labels_dev) {
  const std::string who(who_);
  *n_out = 0;
  *n_clusters_out = 0;
  if (!poses_dev || !attrs_dev) return fail(RMCLHIP_ERR_INVALID, who + ": null particle buffers");
  if (n > (1u << 30)) return fail(RMCLHIP_ERR_UNSUPPORTED, who + ": at most 2^30 particles");
  HIPCHK(hipSetDevice(r->ctx->device));
  // the labels are also the moment passes' filter: the handle's own when the caller wants none
  uint32_t* labels = labels_dev;
  if (!labels) { HIPCHK(r->d_hyp_labels.reserve(n)); labels = r->d_hyp_labels.p; }
  HIPCHK(hipMemsetAsync(labels, 0xFF, static_cast<size_t>(n) * sizeof(uint32_t), r->stream));
  float max_l = 0.0f;
  if (rmclhip_status st = resampler_stats(r, attrs_dev, n, &max_l)) return st;      // (waits: the labels are cleared on return)
  if (!(max_l > 0.0f) || !std::isfinite(max_l)) return RMCLHIP_OK;                  // nothing is counted
  uint32_t k = 0, n_counted = 0;
  if (rmclhip_status st = count_bins_run(r, poses_dev, attrs_dev, n, bins, max_l, &k, &n_counted)) return st;
  if (k == 0 || n_counted == 0) return RMCLHIP_OK;
  const uint64_t words = kld_table_words(n);
  HIPCHK(r->d_hyp_u32.reserve(4 * words));
  HIPCHK(r->d_hyp_u64.reserve(words + kHypCounters));
  HIPCHK(r->d_hyp_rec.reserve(4 * (static_cast<size_t>(k) + kMaxHypotheses)));
  HypScratch sc;
  sc.parent = r->d_hyp_u32.p; sc.rank = sc.parent + words; sc.n_bins = sc.rank + words; sc.n_part = sc.n_bins + words;
  sc.weight = r->d_hyp_u64.p; sc.counters = sc.weight + words;
  sc.records = r->d_hyp_rec.p; sc.hyps = reinterpret_cast<HypRecord*>(sc.records + 4 * static_cast<size_t>(k));
  const float floor_l = bins->min_likelihood_rel * max_l;                          // count_bins_run's product
  HIPCHK(launch_hypotheses(reinterpret_cast<const xform*>(poses_dev), attrs_dev, n, bins->bin_xyz, bins->bin_rpy, floor_l, static_cast<double>(max_l),
                           r->d_kld_table.p, words, k, max_hypotheses, sc, labels, r->stream));
  unsigned long long counters[kHypCounters] = {0ull, 0ull, 0ull, 0ull};
  HypRecord hyps[kMaxHypotheses];
  HIPCHK(hipMemcpyAsync(counters, sc.counters, sizeof(counters), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  const uint32_t n_clusters = static_cast<uint32_t>(counters[0]);
  const uint32_t n_hyp = std::min(n_clusters, max_hypotheses);
  if (n_clusters == 0 || n_clusters > k || counters[2] != counters[0])
    return fail(RMCLHIP_ERR_HIP, who + ": the cluster count is inconsistent with the bin table");
  HIPCHK(hipMemcpyAsync(hyps, sc.hyps, sizeof(HypRecord) * n_hyp, hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  const double total = static_cast<double>(counters[1]);
  for (uint32_t h = 0; h < n_hyp; ++h) {
    rmclhip_pose_hypothesis& o = out[h];
    const rmclhip_status st = pose_estimate_passes(who_, hyps[h].n_particles,
                                                   [&](int pass, double L_sum, const xform& Tbm, double* m) {
                                                     return resampler_moments(r, poses_dev, attrs_dev, n, pass, L_sum, Tbm, m, labels, h);
                                                   },
                                                   &o.estimate);
    if (st != RMCLHIP_OK) return st;
    o.key_min = hyps[h].key_min;
    o.weight = hyps[h].weight;
    o.weight_share = static_cast<double>(hyps[h].weight) / total;
    o.n_bins = hyps[h].n_bins;
    o.reserved = 0u;
  }
  *n_out = n_hyp;
  *n_clusters_out = n_clusters;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_particles_pose_hypotheses(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                                 uint32_t n, const rmclhip_kld_params* bins, uint32_t max_hypotheses, rmclhip_pose_hypothesis* out,
                                                 uint32_t* n_out, uint32_t* n_clusters_out, uint32_t* labels_dev) {
  ApiGuard guard_("rmclhip_particles_pose_hypotheses");
  if (n_out) *n_out = 0;
  if (n_clusters_out) *n_clusters_out = 0;
  if (rmclhip_status st = pose_hypotheses_check("particles_pose_hypotheses", r, bins, max_hypotheses, out, n_out, n_clusters_out)) return st;
  if (n == 0) return RMCLHIP_OK;
  return pose_hypotheses_run("particles_pose_hypotheses", r, poses_dev, attrs_dev, n, bins, max_hypotheses, out, n_out, n_clusters_out, labels_dev);
}
