// kernels.h -- launch interface between the C ABI (capi_*.cpp) and the HIP kernels (kernels.hip, micp.hip and the other *.hip files).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "devmath.h"
#include "find_kinds.h"
#include "layout.h"
#include "micp_host.h"

namespace rmclhip {

// what a launcher returns for a kernel variant that lives in librmclhip_lab.so while that library is not loaded: a value of its own,
// NOT hipErrorNotSupported -- the runtime reports that for real failures (graph capture, host-allocation flags), which must stay
// visible as what they are
constexpr hipError_t kLabMissing = static_cast<hipError_t>(2040);

enum ModelKind : uint32_t { kModelNone = 0, kModelSpherical = 1, kModelO1Dn = 2, kModelPinhole = 3, kModelOnDn = 4 };

// one find() launch: every ray of (nposes x H x W)
struct FindParams {
  const uint32_t* nodes;   // Node4[]
  const uint32_t* qnodes;  // Node4Q[] (quantised twins)
  const uint32_t* cnodes;  // Node4C[] (child-major twins)
  const uint32_t* cnodes16;  // Node16C[] (a node's grandchildren, child-major; kind 32's two-levels-per-pass descent), nullable
  const uint32_t* tris;    // TriRec[]
  uint32_t n_nodes;        // number of Node4 (the LDS-resident top of the tree copies min(kTop, n_nodes) of them)
  // spherical: [cos(phi_v) (H) | sin(phi_v) (H) | cos(theta_h) (W) | sin(theta_h) (W)], host libm values
  // o1dn:      dirs xyz (W*H*3)
  // ondn:      [origs xyz (W*H*3) | dirs xyz (W*H*3)]
  // pinhole:   none (procedural from pin_f = {fx, fy}, pin_c = {cx, cy})
  const float* model_tab;
  float pin_f[2], pin_c[2];
  uint32_t W, H;
  uint32_t tile_w_log2;    // wave = 2^tile_w_log2 x (64 >> tile_w_log2) rays of the scan image
  uint32_t tiles_x, tiles_y;
  float tfar;              // model.range.max
  f3 orig_s;               // sensor-frame ray origin (0 for spherical)
  // pose(s): Tsm = Tbm * Tsb. Single pose: by value; batch: device arrays (pose = blockIdx.y)
  xform Tsm, Tms;
  const xform* Tsm_arr;
  const xform* Tms_arr;
  uint32_t nposes;
  // outputs (nullable), sensor frame, index = pose*W*H + vid*W + hid
  uint8_t* hits;
  float* ranges;
  float* points;
  float* normals;
  uint32_t* face_ids;
  // frontier start (find_kinds.h FindKind::frontier()): the map's frontier table and what bounds a hit's distance from any origin
  const uint32_t* frontier;      // n_frontier x 8 dwords {lo.xyz hi.x | hi.yz ref pad} (layout.h kFrontierDepth)
  uint32_t n_frontier;
  f3 scene_center;
  float scene_half_diag;
  const float* tile_planes;      // per tile of the scan image: the pyramid of its rays in the sensor frame (k_tile_planes), or null
  uint32_t frontier_max_preload; // stack entries the frontier start may leave per lane: 64 - stack_need of the tree the kind walks
  // kind 32 (traverse.hip.h frontier_descent_start): the wave stops descending when a level would leave more than descent_final_cap
  // entries (<= 64) or after descent_levels levels
  uint32_t descent_final_cap, descent_levels;
  // pose batches in world order (kernels.hip launch_batch_tile_order; nullable = pose-major): entry s = pose << 16 | (first tile / tiles per workgroup) of the s-th workgroup,
  // sorted by where the tile's central ray leaves the map's bounding box -- the launch is then ONE row of blocks (gridDim.y == 1)
  const uint32_t* tile_order;
  uint32_t n_tile_order;
  uint32_t tile_order_granule;
  uint32_t xcd_mapping;    // single scans: 0 = workgroup b computes tiles 4b.. (every XCD sees all of the image), 1 = an eighth of the image per XCD, 2 = a CU's two workgroups from the image's two halves (find_kernel.hip.h)   // workgroups of consecutive slots one XCD takes before the next XCD's turn (load balance across the XCDs)
  // diagnostics (nullable): per physical wave {s_memtime at entry, at exit (low 32 bits), s_memrealtime at entry, tile | xcc << 24}
  uint32_t* wave_clock;
  // MICP moment epilogue (launch_find_moments, k_find<..., kMom = true>): the moments of the gate-stable form (micp.hip) are
  // formed while the correspondences are still in registers -- classification as in k_micp_moments, the 10 x 10 products
  // X^T Y of the factor vectors through v_mfma_f64_16x16x4_f64 -- instead of a second pass over the find's outputs
  const float* mom_dataset_points;
  const uint8_t* mom_dataset_mask;     // nullable
  uint32_t mom_n;                      // correspondences: min(n_dataset, W * H)
  float mom_gate_lo, mom_gate_hi, mom_rho_cap, mom_tau_cap;   // devmath.h micp_gate_class
  double* mom_partials;                // [gridDim.x][kMicpFastMoments]
  unsigned long long* mom_unc_mask;    // [4 * gridDim.x]: bit l of word t = lane l of (virtual) tile t holds an undecided correspondence
  // kind 32: the group boxes of `frontier` (bvh_build.h frontier_groups_of), 16 x 8 dwords in the table's format: entry g = the union of
  // table entries 16 g ... 16 g + 15; null when n_frontier <= 64.  (Last: the kernels of the other kinds keep their argument offsets.)
  const uint32_t* frontier_groups;
};

// what follows the reduction launch (capi_internal.h ReduceTail): nothing, the finalize launch or the batch solve launch
enum TailMode : uint32_t { kTailNone, kTailStats, kTailBatchSolve };

struct ReduceParams {
  const float* dataset_points;
  const uint8_t* dataset_mask;   // nullable
  const float* model_points;
  const float* model_normals;
  const uint8_t* model_mask;     // nullable (k_reduce_partials only: a caller-owned view without a mask)
  uint32_t n;                    // elements per pose
  uint32_t nposes;               // model buffers hold nposes*n elements; dataset is shared
  float max_dist;
  xform Tpre;                    // used when Tpre_dev == nullptr
  const xform* Tpre_dev;         // per-pose pre-transform (device), nullable
  double* partials;              // [nposes][nblocks][16]
  uint32_t nblocks;
};

struct PfParams {
  const uint32_t* nodes;
  const uint32_t* qnodes;         // quantised twins (Node4Q), nullable
  const uint32_t* tris;
  const xform* poses;            // Tbm per particle
  void* attrs;                   // rmclhip_particle_attributes[n]
  uint32_t n_particles;
  const float* beams;            // rmclhip_range_measurement[n_beams] (16 floats each), device
  uint32_t n_beams;
  xform Tsb;
  float dist_sigma, rhsm, rmsh, rmsm, range_min, range_max;
  uint32_t max_n_meas;
  float* errors;                 // nullable [n_particles*n_beams]
  uint32_t particles_per_block;
  uint32_t raw_ng;               // correspondence_type 2: error against Embree's un-normalised Ng
  uint32_t sim_min_range;        // sim hit requires t > sensor_range.min (Embree updater :47; the OptiX program does not)
  float ray_tfar;                // inf (Embree updater :27) or 1e4 (optixTrace tmax, BeamEvaluateProgram.cu:48)
  uint32_t beams_at_origin;      // every beam starts at (0,0,0) of the sensor frame (what PCDSensorUpdaterEmbree::update builds,
                                 // :314-327): Tsm * orig is Tsm.t, the rotation of a zero vector is skipped
  uint32_t refill_thr, tail_lanes;  // schedule of the persistent-lane kernel: refill when >= refill_thr lanes of a wave are idle;
                                 // leave the node phase when <= tail_lanes lanes still descend and a lane holds a leaf
  uint32_t nb_magic;             // floor(2^32 / n_beams) + 1: ray index / n_beams = umulhi(ray, nb_magic) for ray * n_beams < 2^32
  // Round 4 -- particle-coherent mapping (rmclhip_pf_set_mapping): the block's rays are dealt out PARTICLE-minor (ray j = beam j / np
  // of particle j % np), so the 64 lanes of a wave hold the SAME beam of 64 particles -- nearly the same ray when the cloud has
  // converged and neighbouring slots hold neighbouring particles (order: slot -> particle index, sorted by a Morton key of x, y, yaw;
  // null = identity).  Same rays, same per-particle merge order: results do not depend on the mapping.
  uint32_t particle_minor;
  const uint32_t* order;         // nullable [n_particles]
  // correspondence_type 1 (closest point): the map's near grid (kernels.h NearGrid; null: unseeded queries) and the record count
  const uint32_t* near_grid;
  uint32_t gn[3];
  float gorg[3], ginv[3];
  uint32_t n_tris;
  // k_pf_update_v3: the beam errors of a workgroup wait for the dense pass in GLOBAL scratch ([n_particles * n_beams] floats, written
  // and read back by the same workgroup: L2) instead of LDS -- 16 KB less LDS per workgroup, 7 instead of 4 workgroups per CU
  // (profiles/r04_pf_occupancy.txt).  null: the LDS form of rounds 3.
  float* evals;
  // k_pf_update_v3<..., kAccum> (round 5): g^i for i = 0 .. n_beams, g = max_n_meas / (max_n_meas + 1), and 1 / (max_n_meas + 1) -- the
  // closed-form merge weights of a particle's beams (kernels.hip "order-independent likelihood accumulation"); null: the forms of rounds 3 / 4
  const double* gpow;
  double inv_max1;
};

// per-call inputs of the device-resident MICP loop: written by ONE H2D copy so that the whole loop can be a
// static hipGraph (kernel arguments never change between replays)
struct MicpCall {
  xform Tsm, Tms;   // find pose: Tom * Tbo * Tsb and its inverse
  xform Tsb, Tbo;
  float max_dist;
  float rho_cap, tau_cap;   // moment form of the loop (launch_micp_fast): bounds on the pre-transforms it may meet
  uint32_t seq;             // sequence number of this call: echoed in the completion tag the chain's last kernel publishes
  float gate_lo, gate_hi;   // moment form: the classification holds for every max_dist in [gate_lo, gate_hi] (devmath.h micp_gate_class)
  uint32_t pad[2];
};

// the part of MicpCall the moment-form kernels read, passed BY VALUE when the chain is launched directly (no hipGraph, no H2D
// copy node: kernel arguments are fresh on every launch anyway)
struct MicpCallLite {
  xform Tsb, Tbo;
  float max_dist, rho_cap, tau_cap;
  uint32_t seq;
  float gate_lo, gate_hi;   // see MicpCall
};

// MICP-L inner-loop state kept on the device between launches (correct_once)
struct MicpState {
  xform T_onew_oold;
  xform T_snew_sold;             // pre-transform for the next reduction
  cstats stats_o;                // last merged statistics, odom frame
};

// moment form of the schedule-(R) loop (micp.hip: "gate-stable moment form"): one streaming pass + one single-workgroup
// launch for all iterations.  status->code: 0 = done (state_out valid), 1 = a pre-transform left (rho_cap, tau_cap) at
// iteration `iter`, 2 = more than 4096 uncertain correspondences; for 1 and 2 the caller runs the per-iteration form.
struct MicpFastStatus { uint32_t code, iter, n_uncertain; float max_rho, max_tau; uint32_t pad[3]; };
constexpr uint32_t kMicpFastMoments = 96;
inline uint32_t micp_fast_blocks(uint32_t n) {
  const uint32_t b = (n + 255u) / 256u;   // one correspondence per thread for small scans, up to 128 rows
  return b < 1u ? 1u : (b > 128u ? 128u : b);
}
// partials: micp_fast_blocks(n) * 96 doubles; unc_mask: ceil(n / 64) words
hipError_t launch_micp_fast(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                            const float* model_normals, const uint8_t* model_mask, uint32_t n, const MicpCall* call,
                            double* partials, unsigned long long* unc_mask, uint32_t n_iter, MicpState* state_out,
                            MicpFastStatus* status, unsigned long long* done, hipStream_t s,
                            const MicpCallLite* call_by_value = nullptr);   // non-null: `call` is ignored

// the loop launch alone, after launch_find_moments: `nblocks` partial rows, mask words in the find's tile order (decoded with
// W / tiles_x / tile_w_log2 of that find)
hipError_t launch_micp_fast_loop_tiled(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                                       const float* model_normals, const uint8_t* model_mask, uint32_t n, uint32_t nblocks,
                                       const double* partials, const unsigned long long* unc_mask, uint32_t W, uint32_t tiles_x,
                                       uint32_t tile_w_log2, uint32_t words_per_block, uint32_t n_iter, MicpState* state_out,
                                       MicpFastStatus* status, unsigned long long* done, hipStream_t s, const MicpCallLite& call_by_value,
                                       double* fold_rows, uint32_t* fold_flags);   // [kMicpFoldBlocks][96] doubles / flags, zeroed once; null: one workgroup
constexpr uint32_t kMicpFoldBlocks = 8;
// Round 4 -- the iterations on the host (micp_host.h): fold the rows like the loop launch does, then hand {82 moments, undecided
// count, the undecided correspondences' D | I | N} to the host behind one completion tag {seq, xor of the written words}.
// _tiled: after launch_find_moments (mask words in the find's tile order); _moments_publish: the separate pass + the publish.
hipError_t launch_micp_publish_tiled(const float* dataset_points, const float* model_points, const float* model_normals, uint32_t n,
                                     uint32_t nblocks, const double* partials, const unsigned long long* unc_mask, uint32_t W,
                                     uint32_t tiles_x, uint32_t tile_w_log2, uint32_t words_per_block, MicpHostBlock* host_block,
                                     unsigned long long* done, uint32_t seq, double* fold_rows, uint32_t* fold_flags, hipStream_t s);
hipError_t launch_micp_moments_publish(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                                       const float* model_normals, const uint8_t* model_mask, uint32_t n, double* partials,
                                       unsigned long long* unc_mask, const MicpCallLite& cv, MicpHostBlock* host_block,
                                       unsigned long long* done, hipStream_t s);

// N-sensor MICP loop on the device (micp_localization.cpp:900-964): per-call frames + per-sensor partials, one step launch per
// iteration merges every sensor's statistics (weighted and unweighted), solves once and hands every sensor its next
// pre-transform
constexpr uint32_t kMaxMicpSensors = 8;
struct MicpMultiCall {
  xform Tsb[kMaxMicpSensors], Tbo[kMaxMicpSensors];
  double weight[kMaxMicpSensors];              // merge_weight_multiplier
  const double* partials[kMaxMicpSensors];     // [nblocks[s]][16]
  uint32_t nblocks[kMaxMicpSensors];
  uint32_t n_sensors, seq;                     // seq: echoed in the completion tag (see MicpCall)
};
struct MicpMultiState {
  xform T_onew_oold;
  cstats merged_o, merged_weighted_o;
  xform T_snew_sold[kMaxMicpSensors];
};
// moment form of the N-sensor loop: launch_micp_moments once per sensor (its MicpCall carries max_dist and the caps), then ONE
// single-workgroup launch for all iterations of all sensors; status->code as MicpFastStatus (0 done, 1 a pre-transform of
// sensor `sensor` left its caps, 2 more than 4096 undecided correspondences in total)
struct MicpMultiFastStatus {
  uint32_t code, iter, n_uncertain, sensor;
  float max_rho[kMaxMicpSensors], max_tau[kMaxMicpSensors];
};
struct MicpMultiFastParams {
  const float* dataset_points[kMaxMicpSensors];
  const float* model_points[kMaxMicpSensors];
  const float* model_normals[kMaxMicpSensors];
  const double* partials[kMaxMicpSensors];               // [nblocks][96] of launch_micp_moments
  const unsigned long long* unc_mask[kMaxMicpSensors];
  uint32_t n[kMaxMicpSensors], nblocks[kMaxMicpSensors];
  // per-call data BY VALUE (round 3: no H2D copy nodes in the chain, and nothing the one solving lane has to fetch from global
  // memory inside the iterations): frames, merge weights, gates and caps of the sensors
  xform Tsb[kMaxMicpSensors], Tbo[kMaxMicpSensors];
  double weight[kMaxMicpSensors];
  float max_dist[kMaxMicpSensors], rho_cap[kMaxMicpSensors], tau_cap[kMaxMicpSensors];
  uint32_t n_sensors, seq;
  uint32_t n_iter;
  MicpMultiState* state_out;                              // may be host-mapped
  MicpMultiFastStatus* status;                            // may be host-mapped
  unsigned long long* done;                               // host-mapped completion tag (see reduce_common.hip.h publish_tag)
  // sensors whose find + moment pass ran on ANOTHER stream (bit s of join_mask): the loop waits for join_flags[s] == seq before it
  // touches sensor s's rows -- an in-kernel wait of ~1 us where a cross-stream event takes ~10 us to reach the waiting queue
  const uint32_t* join_flags;
  uint32_t join_mask;
};
// one lane stores `seq` to *flag with release semantics at device scope: enqueued behind a sensor's moment pass on that sensor's stream
hipError_t launch_signal_flag(uint32_t* flag, uint32_t seq, hipStream_t s);
// {seq, 0} to a pinned completion tag, behind whatever the stream holds
hipError_t launch_host_tag(unsigned long long* done, uint32_t seq, hipStream_t s);
hipError_t launch_micp_moments(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                               const float* model_normals, const uint8_t* model_mask, uint32_t n, const MicpCall* call,
                               double* partials, unsigned long long* unc_mask, hipStream_t s, const MicpCallLite* call_by_value = nullptr);
hipError_t launch_micp_multi_fast_loop(const MicpMultiFastParams& p, hipStream_t s);
hipError_t launch_micp_multi_init(const MicpMultiCall* call, MicpMultiState* state, hipStream_t s);
hipError_t launch_micp_multi_step(const MicpMultiCall* call, MicpMultiState* state, hipStream_t s);

// pose batches in world order (kernels.hip: keys + counting sort over 4096 cells of the map's bounding box)
uint32_t batch_order_scratch_dwords(uint32_t n);
hipError_t launch_batch_tile_order(const FindParams& p, ModelKind kind, uint32_t group, f3 bb_min, f3 bb_max, uint32_t* scratch, uint32_t* order,
                                   hipStream_t s);
hipError_t launch_find(const FindParams& p, ModelKind kind, int variant, hipStream_t s);
// the kinds with the MICP moment epilogue (find_kinds.h FindKind::moments): find_launch_shape(p, variant, true).grid_x workgroups, one
// partial row per workgroup and one mask word per tile, that is find_kind(variant).tiles_per_block words per workgroup (p.mom_* set by
// the caller); followed by launch_micp_fast_loop_tiled
hipError_t launch_find_moments(const FindParams& p, ModelKind kind, int variant, hipStream_t s);
// THE launch shape of k_find, for every kind and every caller: the grid (gridDim.x % 8 == 0; the one-row grid of the world order when
// the launch has a tile order), the dynamic LDS and the size of a clocked launch's p.wave_clock.  All zero: no such kind.
struct FindLaunchShape {
  uint32_t grid_x, grid_y, lds_bytes, clock_dwords;
};
FindLaunchShape find_launch_shape(int kind, bool moments, uint32_t ntiles, uint32_t nposes, uint32_t n_tile_order, uint32_t granule);   // n_tile_order 0: pose-major
FindLaunchShape find_launch_shape(const FindParams& p, int kind, bool moments);
// the plane table of the frontier start (kinds 23 / 24): tiles_x * tiles_y * 16 floats for p's model and tiling
hipError_t launch_tile_planes(const FindParams& p, ModelKind kind, float* planes, hipStream_t s);
// diagnostics (tools/probe_find.py): per-wave step timeline of one spherical scan; probe_log: tiles x 512 dwords
hipError_t launch_find_probe(const FindParams& p, int mode, uint32_t* probe_log, hipStream_t s);
// the map's near grid (traverse.hip.h CpcParams): `cells` = one record index per cell, x fastest; org / inv = the box's corner and
// cells per metre per axis
struct NearGrid {
  const uint32_t* cells;
  uint32_t n[3];
  float org[3], inv[3];
};
// grid (nullable): seeds points without a tracking seed; cells (nullable): BUILD a grid -- the query points are the centres of cells
// [0, n) of `cells` (whose records are not read), rec_out receives their records
hipError_t launch_cpc_find(const uint32_t* nodes, const uint32_t* tris, const float* dataset_points, uint32_t n,
                           float max_dist, xform Tsm, xform Tms, uint8_t* hits, float* dists, float* points,
                           float* normals, uint32_t* face_ids, bool quad, hipStream_t s, const uint32_t* seed_rec = nullptr,
                           uint32_t* rec_out = nullptr, uint32_t n_tris = 0, float bound_d2 = 3.0e38f, const NearGrid* grid = nullptr,
                           const NearGrid* cells = nullptr, float skip_d2 = 3.0e38f);
// residual resampling (ResidualResamplerCPU.cpp:55-203) in three steps; stats: 32 bytes on the device {double sum, double max,
// u64 n * E[copies per draw], u64 draws used}
hipError_t launch_residual_prepare(const void* attrs, uint32_t n, uint32_t n_new, double* psum, float* pmax, void* stats, hipStream_t s);
hipError_t launch_residual_draws(const void* attrs, uint32_t n, uint32_t n_new, const void* stats, uint32_t n_draws, uint64_t seed,
                                 uint32_t step, uint32_t* draw_idx, uint32_t* draw_cnt, unsigned long long* incl,
                                 unsigned long long* block_tot, hipStream_t s);
hipError_t launch_residual_fill(const xform* poses, const void* attrs, const uint32_t* draw_idx, const unsigned long long* incl,
                                uint32_t n_draws, xform* poses_new, void* attrs_new, uint32_t n_new, uint32_t first, uint32_t count,
                                const float* cfg8, void* stats, uint64_t seed, uint32_t step, hipStream_t s);
hipError_t launch_gladiator_resample(const xform* poses, const void* attrs, uint32_t n, xform* poses_new, void* attrs_new,
                                     uint32_t first, uint32_t count, const float* cfg8, uint32_t trans_dist_metric,
                                     uint64_t seed, uint32_t step, hipStream_t s);
// blocks of the reductions that leave one partial per block (likelihood statistics, pose moments): 1024 particles each, 1 .. 256
inline uint32_t partial_blocks(uint32_t n) {
  const uint32_t nblocks = (n + 1023u) / 1024u;
  return nblocks < 1u ? 1u : (nblocks > 256u ? 256u : nblocks);
}
// psum / pmax: scratch of 256 entries each; out2: {sum, max} (device)
hipError_t launch_likelihood_stats(const void* attrs, uint32_t n, double* psum, float* pmax, float* out2, hipStream_t s);
// the same {sum, max} of a DENSE weight vector (the gathered likelihood.mean of a sharded cloud): bit-identical to the call above on
// attributes that hold the same n values
hipError_t launch_likelihood_stats_dense(const float* weights, uint32_t n, double* psum, float* pmax, float* out2, hipStream_t s);
hipError_t launch_pointcloud2_unpack(const uint8_t* data, uint32_t point_step, uint32_t row_step, uint32_t off_x,
                                     uint32_t off_y, uint32_t off_z, bool is_f64, uint32_t h_skip, uint32_t h_inc,
                                     uint32_t w_skip, uint32_t w_inc, uint32_t out_w, uint32_t out_h, float range_min,
                                     float range_max, float* dirs, float* points, uint8_t* mask, uint32_t* n_valid,
                                     hipStream_t s);
// the 16-wide twins of the child-major nodes (layout.h Node16C), built on the device from them: one thread per (node, entry)
hipError_t launch_build_cnodes16(const uint32_t* cnodes, uint32_t n_nodes, uint32_t* cnodes16, hipStream_t s);
hipError_t launch_compose_poses(const xform* Tbm_dev, xform Tsb, xform* Tsm_out, xform* Tms_out, uint32_t n,
                                hipStream_t s);
uint32_t reduce_num_blocks(uint32_t n, uint32_t nposes);
hipError_t launch_reduce_partials(const ReduceParams& p, hipStream_t s);
// finalize one pose's partials into CrossStatistics (writes to out, which may be host-mapped memory)
// done (nullable, host-mapped, single pose only): completion tag {seq, xor of the 16 result words}, one 8-byte store after
// `out` (reduce_common.hip.h publish_tag): the host polls the tag and VERIFIES the sum -- a flag alone is not enough, see capi_rcc.cpp wait_done
hipError_t launch_reduce_finalize(const double* partials, uint32_t nblocks, uint32_t nposes, cstats* out,
                                  unsigned long long* done, uint32_t seq, hipStream_t s);
// closing launch of the launch_micp_iter chain: solve of the last iteration + T_onew_oold / stats_o (the chain itself works in
// the sensor frame, micp.hip micp_advance_sensor)
// done (nullable, host-mapped): completion tag {call->seq, xor of the state's words}, stored after the results
hipError_t launch_micp_close(const double* partials, uint32_t nblocks, const MicpCall* call, const MicpState* state,
                             MicpState* state_out, unsigned long long* done, hipStream_t s);
// state: TWO MicpState slots (ping-pong of k_micp_iter); both initialised.  Only a correction without iterations needs it
hipError_t launch_micp_init(MicpState* state, hipStream_t s);
// one launch per MICP iteration: finishes the previous iteration (finalize + solve, redundantly in every block)
// and streams the next reduction; a final launch_micp_close closes the last iteration
hipError_t launch_micp_iter(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                            const float* model_normals, const uint8_t* model_mask, uint32_t n, uint32_t nblocks,
                            const MicpCall* call, const double* partials_prev, double* partials_out,
                            const MicpState* state_in, MicpState* state_out, bool first, hipStream_t s);
// batch: per pose finalize + umeyama -> Tdelta (sensor->base conjugated), stats
hipError_t launch_batch_solve(const double* partials, uint32_t nblocks, uint32_t nposes, xform Tsb,
                              xform* Tdelta_out, cstats* stats_out, hipStream_t s);
// rmclhip_debug_solve: out[i] = umeyama(stats[i]) (fast = 0) or umeyama_fast(stats[i]) (fast = 1), one thread per element, 64 per block
hipError_t launch_debug_solve(const cstats* stats, uint32_t n, int fast, xform* out, hipStream_t s);
hipError_t launch_dataset_from_ranges(const float* ranges, const float* model_tab, uint32_t kind, uint32_t W,
                                      uint32_t H, f3 orig, const float* pin_fc, float rmin, float rmax, float* points,
                                      uint8_t* mask, uint32_t* n_valid, hipStream_t s);
// map segmentation (segment.hip; ScanMapSegmentationEmbreeNode / O1DnMapSegmentationEmbreeNode): every ray of ONE scan is labelled from its
// measured and its simulated range, the two outlier clouds leave compacted in buffer order
constexpr uint32_t kSegBlock = 1024;     // rays per workgroup, one per lane
enum SegLabel : uint8_t { kSegNone = 0, kSegInlier = 1, kSegOutlierScan = 2, kSegOutlierMap = 3 };
struct SegmentParams {
  const float* ranges_real;      // measured, W * H
  const float* ranges_sim;       // the find's ranges (miss: range.max + 1)
  const float* normals_sim;      // the find's normals, sensor frame (miss: NaN)
  const float* model_tab;        // as FindParams::model_tab
  uint32_t kind, W, H;
  f3 orig;                       // O1Dn: the model's origin
  float pin_f[2], pin_c[2];
  float rmin, rmax;
  float min_dist_outlier_scan, min_dist_outlier_map;
  uint32_t pint_with_origin;     // RMCLHIP_SEG_PINT_WITH_ORIGIN
  uint8_t* labels;               // W * H, never null (the caller's buffer or the operator's scratch): the scatter launch reads them back
  uint32_t* block_counts;        // [ceil(W * H / kSegBlock)][2] = {scan outliers, map outliers} of a workgroup's rays
  float* outlier_scan_xyz;       // nullable
  float* outlier_map_xyz;        // nullable
  uint32_t* counts_dev;          // nullable [2]
  uint32_t* counts_host;         // nullable [2], host-mapped
};
// two launches: k_segment_classify (labels + per-workgroup counts), k_segment_scatter (offsets from the counts below a workgroup's
// index, points at offset + rank, totals); the kernel boundary between them is what orders the workgroups
hipError_t launch_segment(const SegmentParams& p, hipStream_t s);
// PointCloud2 bytes -> range image of a spherical model (pc2scan.hip; Pc2ToScanNode::convert).  The flag values are those of
// RMCLHIP_PC2SCAN_* (include/rmclhip.h).
constexpr uint32_t kPc2ScanBlock = 256;
constexpr uint32_t kPc2ScanTrueElevation = 1u, kPc2ScanFloor = 2u, kPc2ScanWrapTheta = 4u, kPc2ScanNearest = 8u;
struct Pc2ScanParams {
  const uint8_t* data;           // device; point i = row * width + col lies at row * row_step + col * point_step
  uint32_t n_points, width, point_step, row_step, off_x, off_y, off_z, is_f64;
  uint32_t has_T;
  xform T;                       // T_sensor_cloud
  float phi_min, phi_inc, theta_min, theta_inc;
  uint32_t W, H;                 // theta.size, phi.size
  double theta_period;           // 2 pi / theta.inc when PC2SCAN_WRAP_THETA is set and that is a whole number, else 0
  float rmin, rmax, range_empty; // range_empty = (float)((double)range.max + 1.0)
  uint32_t flags;
  unsigned long long* keys;      // W * H, set to "nobody" by the launcher
  uint32_t* bin_counts;          // [pc2scan_blocks(n_points)][3] = {finite, in image, in range (candidates)} of a workgroup's points
  uint32_t* cell_counts;         // [pc2scan_blocks(W * H)] = filled cells among a workgroup's cells
  float* ranges;                 // W * H out
  const float* model_tab;        // the operator form: the spherical model's trig tables (FindParams::model_tab) ...
  float* ds_points;              // ... its dataset points (null: the free function) ...
  uint8_t* ds_mask;              // ... and mask
};
inline uint32_t pc2scan_blocks(size_t n) { return static_cast<uint32_t>((n + kPc2ScanBlock - 1u) / kPc2ScanBlock); }
// the keys' memset + k_pc2scan_bin + k_pc2scan_resolve + k_pc2scan_publish ({finite, in image, in range, cells filled} to the
// host-mapped counters_host), all on s
hipError_t launch_pc2scan(const Pc2ScanParams& p, uint32_t* counters_host, hipStream_t s);
// PointCloud2 bytes + per-point times + the scan's motion -> every point from its own pose (deskew.hip; the rules: include/rmclhip.h,
// MOTION-COMPENSATED INPUT).  The knots travel BY VALUE in the launch parameters (2.3 of the 4 KB a launch may carry), so they need
// no copy of their own on the stream; every workgroup stages them in LDS.
constexpr uint32_t kDeskewBlock = 256;
struct DeskewKnots { double times[64]; quat q[64]; f3 t[64]; };   // 2 304 B
constexpr uint32_t kDeskewValid = 0u, kDeskewFinite = 1u, kDeskewClamped = 2u, kDeskewTimeNonFinite = 3u, kDeskewCounters = 4u;
constexpr uint32_t kDeskewCounterStride = 32u;   // words between two counters: a 128-byte line each
struct DeskewParams {
  const uint8_t* data;           // device; output point (ti, tj) reads row ti * h_inc + h_skip, column tj * w_inc + w_skip
  uint32_t point_step, row_step, off_x, off_y, off_z, is_f64;
  uint32_t off_t, t_type;        // the time field and its PointField datatype (6 UINT32, 7 FLOAT32, 8 FLOAT64)
  double t_scale, t_offset;      // t = t_offset + t_scale * raw
  uint32_t h_skip, h_inc, w_skip, w_inc, out_w, out_h;
  float range_min, range_max;
  DeskewKnots knots;
  uint32_t n_knots;              // in [2, 64]
  float* origs; float* dirs;     // the operator form: the OnDn model table's two halves, 3 n floats each ...
  float* points; uint8_t* mask;  // ... and the dataset.  The cloud form: points = n records of 12 bytes, NaN where the mask would be 0
  uint32_t* counters;            // counter c at word c * kDeskewCounterStride, zeroed by the caller
};
hipError_t launch_deskew(const DeskewParams& p, bool cloud_form, hipStream_t s);
hipError_t launch_pf_update(const PfParams& p, int variant, hipStream_t s);
hipError_t launch_pf_extract_weights(const void* attrs, uint32_t n, float* weights, hipStream_t s);
// rmclhip_surface_params as the kernels take it (surface.hip.h)
struct SurfaceKernelParams {
  uint32_t axis, align, on_miss;
  float height, probe_up, probe_down, min_up_cos;
};
// the motion noise as the kernel takes it (pf_random.hip.h: motion_noise_compose): the six standard deviations, the Philox key (the
// seed's low and high word), the step, and the global index of the launch's first particle
struct MotionNoiseKernelParams {
  float sigma[6];
  uint32_t key0, key1, step, first;
};
// noise: null = the deterministic update (the launches of before); else every particle's moved pose is composed with its draw first.
// surface: null = the unconstrained update; else the surface constraint runs in the same launch (move -> forget -> collision ray on the
// lifted segment -> surface ray) and surface_stats (device, 4 words {particles, snapped, missed, steep}, zeroed by the caller) counts
hipError_t launch_pf_motion(const uint32_t* nodes, const uint32_t* tris, xform* poses, void* attrs, uint32_t n,
                            xform T_bnew_bold, double forget_rate, uint32_t max_n_meas, bool collision, hipStream_t s,
                            const SurfaceKernelParams* surface = nullptr, uint32_t* surface_stats = nullptr, uint32_t* surface_faces = nullptr,
                            const MotionNoiseKernelParams* noise = nullptr);
// the standalone pass (surface.hip): qnodes = the map's quantised nodes; stats as above.  faces (both launches; nullable, n words): the
// face every particle's probe hit, kInvalidFace for none (a test output)
hipError_t launch_surface_constrain(const uint32_t* qnodes, const uint32_t* tris, xform* poses, void* attrs, uint32_t n,
                                    const SurfaceKernelParams& sp, uint32_t max_n_meas, uint32_t* stats, uint32_t* faces, hipStream_t s);

// pose-estimate moments (RmclNode::estimateStats): partials = 256 * 32 doubles of scratch, out32 = 24 sums + 8 maxima (device).
// labels (nullable, n words): only the particles with labels[i] == want take part -- the moments of one pose hypothesis
hipError_t launch_pose_moments(const xform* poses, const void* attrs, uint32_t n, int pass, double L_sum, xform Tbm,
                               double* partials, double* out32, hipStream_t s, const uint32_t* labels = nullptr, uint32_t want = 0u);
hipError_t launch_loopback_allreduce(const double* const* send, uint32_t world, double* recv, uint32_t count, bool is_max, hipStream_t s);
hipError_t launch_compact_shards(const float* padded, float* dense, uint32_t n_total, uint32_t world, uint32_t cap, hipStream_t s);
// the same for records of record_bytes (a multiple of 4): the padded all-gather layout of a ragged partition -> the dense cloud
hipError_t launch_compact_records(const void* padded, void* dense, uint32_t n_total, uint32_t world, uint32_t cap, uint32_t record_bytes,
                                  hipStream_t s);

// the particle cloud's initialisations and visualisation channels (particles.hip; RmclNode::initSamplesUniform / initSamples / visualize).
// poses / attrs: elements first .. first+count-1 of a cloud (poses 16-B aligned, attrs 4-B aligned); element k gets the values of GLOBAL
// particle first + k.  One launch writes at most kMaxInitCount records (its attribute stream is indexed in 32-bit dwords).
constexpr uint32_t kMaxInitCount = 0xFFFFFFFFu / 9u;
hipError_t launch_particles_init_uniform(xform* poses, void* attrs, uint32_t first, uint32_t count, const float* bb_min, const float* bb_max,
                                         uint64_t seed, uint32_t epoch, hipStream_t s);
hipError_t launch_particles_init_pose(xform* poses, void* attrs, uint32_t first, uint32_t count, const xform& Tlm, const float* L36, uint64_t seed,
                                      uint32_t epoch, hipStream_t s);
// out: 7 * n floats on the device: x | y | z | likelihood | likelihood_sigma | likelihood_n_meas | badness
hipError_t launch_particles_pack_visualization(const xform* poses, const void* attrs, uint32_t n, uint32_t max_n_meas, float* out, hipStream_t s);

// the surface sampler (include/rmclhip.h, SURFACE SAMPLER).  Build (surface_sample.hip, and the scan of resample.hip with a load of
// its own): rec_of_face[f] = the lowest record index that carries face id f (all-ones on entry: integer atomicMin, independent of the
// order); area[f] = a_f of an eligible face, -1 of any other; *amax_bits = the bits of the largest finite a_f > 0 (zero on entry:
// positive doubles order as their bits, integer atomicMax); incl = the inclusive prefix sums of the integer weights.
struct SurfaceSampleRule { float min_up_cos; float region_min[3], region_max[3]; };
hipError_t launch_surface_sample_records(const uint32_t* tris, uint32_t n_records, uint32_t n_faces, uint32_t* rec_of_face, hipStream_t s);
hipError_t launch_surface_sample_areas(const uint32_t* tris, const uint32_t* rec_of_face, uint32_t n_faces, const SurfaceSampleRule& rule,
                                       double* area, unsigned long long* amax_bits, hipStream_t s);
hipError_t launch_surface_sample_scan(const double* area, const unsigned long long* amax_bits, uint32_t n_faces, unsigned long long* incl,
                                      unsigned long long* block_tot, hipStream_t s);
// what a draw reads (surface_sample.hip.h); T = incl[n_faces - 1] > 0
struct SurfaceSampleView {
  const uint32_t* tris; const uint32_t* rec_of_face; const unsigned long long* incl;
  uint32_t n_faces; unsigned long long T;
  float height, yaw_min, yaw_max; uint32_t align;
};
// particles.hip: the initialisation on the surface (the contract of launch_particles_init_uniform) and the recovery injection in place:
// slot first + k is replaced iff its 32-bit word < threshold (<= 2^32); *n_injected (device, zeroed by the caller) counts them
hipError_t launch_particles_init_surface(xform* poses, void* attrs, uint32_t first, uint32_t count, const SurfaceSampleView& sv, uint64_t seed,
                                         uint32_t epoch, hipStream_t s);
hipError_t launch_particles_inject_surface(xform* poses, void* attrs, uint32_t first, uint32_t count, const SurfaceSampleView& sv,
                                           unsigned long long threshold, uint64_t seed, uint32_t step, uint32_t* n_injected, hipStream_t s);

// adaptive.hip: occupied bins of pose space (counts2 = {distinct bins, counted particles}, zeroed by the caller; table: table_words
// 64-bit words, a power of two >= 2 n, all-ones on entry); resample.hip: systematic resampling -- the integer weights' inclusive
// prefix sums (incl: n words, block_tot: ceil(n / 1024) words), then the slots [first, first + count) of the new cloud
hipError_t launch_kld_count_bins(const xform* poses, const void* attrs, uint32_t n, const float* bin_xyz, const float* bin_rpy, float floor_l,
                                 unsigned long long* table, uint64_t table_words, uint32_t* counts2, hipStream_t s);
hipError_t launch_sys_scan(const void* attrs, uint32_t n, double max_l, unsigned long long* incl, unsigned long long* block_tot, hipStream_t s);
hipError_t launch_sys_fill(const xform* poses, const void* attrs, const unsigned long long* incl, uint32_t n, xform* poses_new, void* attrs_new,
                           uint32_t n_new, uint32_t first, uint32_t count, const float* cfg8, uint32_t trans_dist_metric, uint64_t seed,
                           uint32_t step, hipStream_t s);

// hypotheses.hip: pose hypotheses = connected components of the occupied bins (include/rmclhip.h, POSE HYPOTHESES).  `table` is what
// launch_kld_count_bins left (table_words words, k of them occupied).  Scratch, all the caller's: parent / rank / n_bins / n_part:
// table_words words of 32 bits each, weight: table_words words of 64 bits, labels: n words, records: 4 * k words of 64 bits,
// counters: kHypCounters words of 64 bits, hyps: kMaxHypotheses records.  Everything is enqueued on s; nothing waits.
constexpr uint32_t kMaxHypotheses = 64u;
constexpr uint32_t kHypCounters = 4u;     // {clusters, total weight, records written, unused}
struct HypRecord { unsigned long long key_min, weight; uint32_t n_bins, n_particles, root, pad; };   // 32 B
struct HypScratch {
  uint32_t* parent; uint32_t* rank; uint32_t* n_bins; uint32_t* n_part; unsigned long long* weight;
  unsigned long long* records; unsigned long long* counters; HypRecord* hyps;
};
hipError_t launch_hypotheses(const xform* poses, const void* attrs, uint32_t n, const float* bin_xyz, const float* bin_rpy, float floor_l,
                             double max_l, const unsigned long long* table, uint64_t table_words, uint32_t k_bins, uint32_t max_hypotheses,
                             const HypScratch& sc, uint32_t* labels, hipStream_t s);


// pose_information.hip: the point-to-plane normal matrix over the correspondences of statistics_p2l (include/rmclhip.h, POSE
// COVARIANCE).  Same inputs and grid as launch_reduce_partials (p.partials: [nposes][p.nblocks][kPoseInfoRow] doubles), then one wave
// per pose folds the rows in a fixed order into rows_out[pose][kPoseInfoRow] = {the 28 entries of sum u u^T, upper triangle row by row,
// u = [N ; D x N ; r] | the count | 3 x 0}.  No atomics: the same inputs give the same bytes.
constexpr uint32_t kPoseInfoRow = 32u;
hipError_t launch_pose_information(const ReduceParams& p, double* rows_out, hipStream_t s);

// robust.hip: M-estimator weights in the point-to-plane reduction (include/rmclhip.h, ROBUST MICP).  The views and the
// grid (reduce_num_blocks(n, 1)) are those of launch_reduce_partials for one pose.
constexpr uint32_t kRobustRow = 32u;   // a partial row: the 16 weighted sums | gated-in count | sum w r^2 | sum r^2 | 13 x 0
// scratch of the scale selection, cleared by launch_robust_scale: three histograms (2048 + 2048 + 1024 bins) and the two states between the passes
constexpr uint32_t kRobustSelWords = 2048u + 2048u + 1024u + 8u;
struct RobustView {
  const float* dataset_points;
  const uint8_t* dataset_mask;   // nullable
  const float* model_points;
  const float* model_normals;
  const uint8_t* model_mask;     // nullable
  uint32_t n;
  float max_dist;
  int32_t kernel;                // RMCLHIP_ROBUST_*
};
struct RobustScaleParams { int32_t mode; float scale, tuning, scale_min; };
struct RobustScale { float c, median; uint32_t m, pad; };
struct RobustStats { cstats stats; double weight_sum, wrss, rss; float scale, median; };   // rmclhip_robust_statistics
struct RobustLoopOut { xform T_onew_oold, T_snew_sold; RobustStats stats; };
// the exact lower median of |r| over the gated-in correspondences at Tpre by three histogram passes (11 + 11 + 10 bits of the f32 pattern),
// then c by sp (FIXED: sp.scale, the median reported as 0) -> *scale_out with the count m.  keys: n words of scratch the first pass
// fills and the others read, or nullptr: every pass recomputes r.  scale_copy (nullable, may be host-mapped): a second copy for the host.
hipError_t launch_robust_scale(const RobustView& v, const xform& Tpre, const RobustScaleParams& sp, uint32_t* sel, uint32_t* keys,
                               RobustScale* scale_out, RobustScale* scale_copy, hipStream_t s);
// *scale_out = {c, 0, 0} without a pass over the data (FIXED mode where nobody asks for m)
hipError_t launch_robust_fixed_scale(float c, RobustScale* scale_out, hipStream_t s);
// one weighted reduction at Tpre with the scale in *scale_dev: partials[nblocks][kRobustRow], weights_out (nullable, n floats), *out
// (may be host-mapped, as launch_robust_loop's)
hipError_t launch_robust_statistics(const RobustView& v, const xform& Tpre, const RobustScale* scale_dev, double* partials, uint32_t nblocks,
                                    float* weights_out, RobustStats* out, hipStream_t s);
// n_iter >= 1 iterations { weighted reduction at T_snew_sold, umeyama, T_snew_sold *= U }, one launch each + a closing launch (the form
// of launch_micp_iter / launch_micp_close): partials[2][nblocks][kRobustRow] and state[2] ping-pong
hipError_t launch_robust_loop(const RobustView& v, const RobustScale* scale_dev, double* partials, uint32_t nblocks, xform* state,
                              uint32_t n_iter, const xform& Tsb, const xform& Tbo, RobustLoopOut* out, hipStream_t s);

// The robust loop of a sensor rig (rmclhip_micp_correct_once_robust).  The call block travels BY VALUE with every launch
// (no copy node); what the loop keeps between launches is RobustRigState in device memory.  A sensor's rows are the rows it would have
// alone: block0 is the first workgroup of its share of the ONE streaming launch over all sensors (grid: the sum of the nblocks).
struct RobustRigSensor {
  RobustView v;
  const RobustScale* scale;    // the sensor's own, selected once behind its find and held
  double* partials;            // [nblocks][kRobustRow]
  uint32_t nblocks, block0;
  xform Tsb, Tbo;
  double weight;               // merge_weight_multiplier: multiplies sum w in the solved merge, never truncated
};
struct RobustRigCall { RobustRigSensor s[kMaxMicpSensors]; uint32_t n_sensors, total_blocks; };
struct RobustRigState {
  xform T_onew_oold;
  cstats merged_o, merged_weighted_o;
  double merged_weight, merged_weighted_weight;   // sum over the sensors of sum w, and of sum w * multiplier
  xform T_snew_sold[kMaxMicpSensors];
  RobustStats stats_s[kMaxMicpSensors];           // the last iteration's, sensor frame
};
// identity state; then n_iter x {one streaming launch over every sensor at its T_snew_sold, one one-wave step: robust_finalize per sensor,
// Cs_o = Tbo * (Tsb * stats_s), the two weighted merges, T_onew_oold *= umeyama(merged_weighted_o) if that merge has weight, the next
// pre-transforms as k_micp_multi_step forms them}; a closing launch copies the state to *out (may be host-mapped).  n_iter >= 1
hipError_t launch_robust_rig_loop(const RobustRigCall& call, RobustRigState* state, uint32_t n_iter, RobustRigState* out, hipStream_t s);

// pose_information.hip with M-estimator weights: A = sum w u u^T by k_pose_information_partials' grid, mapping and fold, every term
// (double)w * (u[a] * u[b]); rows_out[kPoseInfoRow] = {the 28 sums | the gated-in count | sum w | sum r^2 | 0}.  *scale_dev: the scale c
hipError_t launch_pose_information_robust(const ReduceParams& p, int32_t kernel, const RobustScale* scale_dev, double* rows_out, hipStream_t s);

// field.hip: reading the map's distance field (include/rmclhip.h, DISTANCE FIELD).  lat: n[0] * n[1] * n[2] floats, x fastest, then y, then z.
// A banded field (include/rmclhip.h, BANDED DISTANCE FIELD) has lat == nullptr and the three arrays below: table,
// nb[0] * nb[1] * nb[2] words (the stored index of a brick or kBandFar), x fastest; coarse, (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1)
// floats, x fastest; bricks, kBandBrickNodes floats per stored brick, x fastest inside a brick.
constexpr uint32_t kBandFar = 0xFFFFFFFFu;
constexpr uint32_t kBandBrickNodes = 729u;     // 9 * 9 * 9: the 8 cells of a brick per axis and their shared faces
struct FieldView {
  const float* lat;
  uint32_t n[3];
  float origin[3];
  float cell, inv_cell;
  const uint32_t* table;
  const float* coarse;
  const float* bricks;
  uint32_t nb[3];
};
// the lookup alone: n points (xyz, map coordinates) -> n distances
hipError_t launch_field_query(const FieldView& fv, const float* points, size_t n, float* out, hipStream_t s);
// the sensor update of correspondence_type 1 answered from the field: k_pf_update<64, 3>'s end points, evaluation and in-order merge
struct PfFieldParams {
  FieldView fv;
  const xform* poses;
  void* attrs;
  uint32_t n_particles;
  const float* beams;
  uint32_t n_beams;
  xform Tsb;
  float dist_sigma;
  uint32_t max_n_meas;
  float* errors;                 // nullable [n_particles * n_beams]
  uint32_t particles_per_block;
};
hipError_t launch_pf_update_field(const PfFieldParams& p, hipStream_t s);

// field_build.hip: the build of a field.  All index arithmetic is size_t.
// launch_field_level: one level of a coarse-to-fine build, one lane per node: the logical nodes min(c_k * stride, n_k - 1), c_k < cn[k],
// of `fv`'s lattice (its pointers are not read).  seed_rec (nullable): the records the previous level left, pn[0] * pn[1] * pn[2] of
// them at stride pstride -- a node i starts from the record of the previous level's node min((i_k + pstride / 2) / pstride, pn[k] - 1),
// the one nearest to it; rec_out (nullable): cn[0] * cn[1] * cn[2] records, x fastest; dist_out (nullable): as many distances -- the
// dense lattice at stride 1, a banded field's coarse lattice at stride 8
struct FieldBuildParams {
  const uint32_t* nodes;
  const uint32_t* tris;
  uint32_t n_tris;
  FieldView fv;
  uint32_t stride, cn[3];
  const uint32_t* seed_rec;
  uint32_t pstride, pn[3];
  uint32_t* rec_out;
  float* dist_out;
};
hipError_t launch_field_level(const FieldBuildParams& p, hipStream_t s);
// a banded field's bricks, in the order the caller runs them.  v: the logical geometry with nb set (its pointers are not read).
//   launch_band_classify  one lane per brick: flags[b] = 1 if the minimum of its eight coarse corners is <= reach or one is NaN, else 0
//   launch_band_table     incl: the inclusive prefix sums of flags (launch_scan_counts).  table[b] = incl[b] - 1 of a stored brick,
//                         kBandFar of any other; stored[incl[b] - 1] = b
//   launch_band_fill      one workgroup per stored brick: its 729 node values, every query seeded from the record of the nearest
//                         coarse corner; NaN beyond n_k - 1
hipError_t launch_band_classify(const FieldView& v, const float* coarse, float reach, uint32_t* flags, hipStream_t s);
hipError_t launch_band_table(const FieldView& v, const uint32_t* flags, const unsigned long long* incl, uint32_t* table, uint32_t* stored,
                             hipStream_t s);
struct BandFillParams {
  const uint32_t* nodes;
  const uint32_t* tris;
  uint32_t n_tris;
  FieldView fv;
  const uint32_t* stored;        // n_stored brick numbers
  uint32_t n_stored;
  const uint32_t* coarse_rec;    // the records of the coarse lattice's queries
  float* bricks;
};
hipError_t launch_band_fill(const BandFillParams& p, hipStream_t s);

// refine.hip: the damped Gauss-Newton refinement of every particle on the field (include/rmclhip.h, REFINE ON THE FIELD), all
// iterations in one launch.  poses are rewritten in place for particles that accepted a step; rows (nullable): n_particles
// rmclhip_refine_result; counters (nullable): {n_moved, n_no_beams, n_not_finite}, added to, so zeroed by the caller.
constexpr uint32_t kRefineMaxBeams = 8192u;
constexpr uint32_t kRefineMaxIterations = 64u;
struct RefineKernelParams {
  FieldView fv;
  xform* poses;
  uint32_t n_particles;
  const float* beams;            // n_beams records of 16 floats, as the sensor update reads them
  uint32_t n_beams;
  xform Tsb;
  uint32_t iterations, dof_mask;
  float max_dist, max_step_trans, max_step_rot, lambda0;
  uint32_t* rows;
  uint32_t* counters;
};
hipError_t launch_field_refine(const RefineKernelParams& p, hipStream_t s);

// resample.hip: the inclusive 64-bit prefix sums of n 32-bit counts, by the three scan kernels of the resamplers (incl: n words,
// block_tot: ceil(n / 1024) words)
hipError_t launch_scan_counts(const uint32_t* counts, uint32_t n, unsigned long long* incl, unsigned long long* block_tot, hipStream_t s);

// stein.hip: one iteration of the Stein variational step (include/rmclhip.h, STEIN STEP ON THE FIELD): the drive of every particle, the
// cell list over the free translation axes, the pair sums and the move, all enqueued on s; nothing waits.  r carries the field, the
// poses, the beams, Tsb, dof_mask, max_dist, the step limits and lambda0 (its iterations, rows and counters are not read).  Scratch,
// all the caller's: table / incl: table_words words of 64 bits (a power of two >= 2 n), block_tot: ceil(table_words / 1024) words,
// count / listed / cursor: table_words words of 32 bits each, slot_of: n words, drive: kSteinDriveStride * n floats, records:
// kSteinRecordWords * n words, counters: kSteinCounters words.  rows (nullable): n rmclhip_stein_result.
constexpr uint32_t kSteinMaxParticles = 1u << 26;
constexpr uint32_t kSteinDriveStride = 8u;     // six floats of drive, two of padding: one particle's drive is two 16-B loads
constexpr uint32_t kSteinRecordWords = 16u;    // {t.x t.y t.z index | R.x R.y R.z R.w | drive 0..3 | drive 4 5, two words of padding}
constexpr uint32_t kSteinCounters = 4u;        // {n_not_finite, n_no_beams, n_bins, n_thinned_bins}
constexpr uint32_t kSteinEvents = 4u;          // the borders of drive | cell list | pair sums and move
struct SteinKernelParams {
  RefineKernelParams r;
  float h_trans, h_rot, repulsion;
  uint32_t max_per_bin;
  uint32_t key0, key1, step;     // the Philox key (the seed's halves) and step + iteration
  unsigned long long* table;
  uint64_t table_words;
  unsigned long long* incl;
  unsigned long long* block_tot;
  uint32_t* count;
  uint32_t* listed;
  uint32_t* cursor;
  uint32_t* slot_of;
  float* drive;
  uint32_t* records;
  uint32_t* counters;
  uint32_t* rows;
};
// events (nullable): kSteinEvents events recorded on s before the drive, before the cell list, before the pair kernel and after it
hipError_t launch_stein_iteration(const SteinKernelParams& p, hipStream_t s, hipEvent_t* events);

}  // namespace rmclhip
