// micp.hip -- the inner iterations of MICPLocalizationNode::correctOnce (rmcl_ros/src/nodes/micp_localization.cpp:915-964) +
// rm::umeyama_transform on the device, for one sensor and for a rig of up to eight.
//
//   k_micp_iter, k_micp_close, k_micp_init     one launch per iteration: the streaming reduction of k_reduce_partials (kernels.hip)
//                                              with the previous iteration's solve in its prologue
//   k_micp_moments                             the gate-stable moment form: 82 moments + a mask of the undecided correspondences
//   k_micp_fast_loop                           ... every iteration in one launch, from the moments and the undecided correspondences
//   k_micp_publish                             ... or the moments handed to the host, which iterates itself (micp_host.h)
//   k_micp_multi_init, k_micp_multi_step       N sensors, one launch per iteration
//   k_micp_multi_fast_loop                     N sensors, the moment form
//   k_signal_flag                              the join of another sensor's stream with the N-sensor loop
//   k_debug_solve                              umeyama() / umeyama_fast() on caller-supplied statistics (include/rmclhip_lab.h)
//
// The three kernels that consume moment rows share ONE text for each step of their set-up: the fold hand-over between workgroups
// (fold_hand_over_row / fold_gather_rows), the count and scan of the mask words (mask_count_scan, wave_offsets), the index list
// (mask_list_append), the re-evaluation of the undecided correspondences (undecided_row_sums) and what a pre-transform needs
// (micp_rho, micp_tau, micp_rotation_f64 of micp_host.h: the host's iterations use the same).  Every workgroup barrier stands in the
// kernel bodies, never in a helper.  The loop forms measured slower (a persistent grid-barrier kernel, reduce + solve launches, a
// reduction tail fused into the last block) are gone; profiles/r03_micp_loop_forms.txt holds their measurements.
#include "kernels.h"
#include "reduce_common.hip.h"
#include "wave_sum.hip.h"

namespace rmclhip {

namespace {

// One MICP inner iteration for ONE sensor, micp_localization.cpp:915-964 (merge_weight_multiplier == 1) frame by frame:
//   Cs_o = Tbo * (Tsb * stats_s); T_inner = umeyama(Cs_o); T_onew_oold = T_onew_oold * T_inner;
//   next T_snew_sold = ~Tsb * (~Tbo * T_onew_oold * Tbo) * Tsb
// written here in the sensor frame.  umeyama is equivariant under a rigid change of frame
// (umeyama(T * C) = T o umeyama(C) o T^-1 for a transform T applied to both means and the covariance), so with
// Tso = Tbo * Tsb:  T_inner = Tso U Tso^-1 with U = umeyama(stats_s), and
//   T_snew_sold' = Tso^-1 (T_onew_oold T_inner) Tso = T_snew_sold * U.
// The loop therefore only needs U and one product per iteration; T_onew_oold = Tso T_snew_sold Tso^-1 and
// stats_o = Tbo * (Tsb * stats_s) are formed once, after the last iteration (micp_close_sensor).  Same mathematics as
// the frame-by-frame order, ~700 instead of ~2500 dependent operations per iteration for the lone lane that runs it; the rounding
// differs from the frame-by-frame order at the 1e-7 level (tests: 1e-5 against the oracle's frame-by-frame loop).
__device__ __forceinline__ void micp_advance_sensor(const cstats& stats_s, xform* T_snew_sold) {
  *T_snew_sold = xmul(*T_snew_sold, umeyama(stats_s));
}
__device__ __forceinline__ void micp_close_sensor(const cstats& stats_s_last, const xform& T_snew_sold, const xform& Tsb,
                                                  const xform& Tbo, MicpState* st) {
  const xform Tso = xmul(Tbo, Tsb);
  st->T_snew_sold = T_snew_sold;
  st->T_onew_oold = xmul(xmul(Tso, T_snew_sold), xinv(Tso));
  st->stats_o = cs_merge(cs_identity(), cs_transform(Tbo, cs_transform(Tsb, stats_s_last)));
}

// One MICP iteration per launch (instead of reduce + solve = two): the launch of iteration i first finishes
// iteration i-1 -- wave 0 of EVERY block sums the previous partials and solves redundantly (same inputs, same
// order => the same pre-transform in every block; block 0 records the advanced state) -- and then streams the
// correspondences with that pre-transform.  Partials and state ping-pong between two buffers so that no block
// reads what another block of the same launch writes.
struct MicpIterParams {
  const float* dataset_points;
  const uint8_t* dataset_mask;  // nullable
  const float* model_points;
  const float* model_normals;
  const uint8_t* model_mask;
  uint32_t n, nblocks;
  const MicpCall* call;
  const double* partials_prev;  // of the previous launch (unused when first)
  double* partials_out;
  const MicpState* state_in;    // state before finishing the previous iteration
  MicpState* state_out;
  uint32_t first;
};

__global__ void __launch_bounds__(256) k_micp_iter(const MicpIterParams p) {
  __shared__ double red[4][kAcc];
  __shared__ double s_wsum[4][64 * 17];
  __shared__ xform s_Tpre;
  // The correspondences of this thread do not depend on the pre-transform the prologue is about to compute: request the
  // first two elements (all a thread gets at reduce_num_blocks' 512 elements per block) BEFORE the prologue, so that
  // their load latency hides behind the finalize + solve of wave 0 instead of following it.
  constexpr int kPre = 2;
  float pd[kPre][3], pm[kPre][3], pn[kPre][3];
  bool pok[kPre];
#pragma unroll
  for (int u = 0; u < kPre; ++u) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x + static_cast<uint32_t>(u) * gridDim.x * 256u;
    pok[u] = false;
    if (i < p.n) {
      const bool dok = (p.dataset_mask == nullptr) || (p.dataset_mask[i] > 0);
      pok[u] = dok && p.model_mask[i] > 0;
      const float* dp = p.dataset_points + 3 * static_cast<size_t>(i);
      const float* mp = p.model_points + 3 * static_cast<size_t>(i);
      const float* mn = p.model_normals + 3 * static_cast<size_t>(i);
#pragma unroll
      for (int k = 0; k < 3; ++k) { pd[u][k] = dp[k]; pm[u][k] = mp[k]; pn[u][k] = mn[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { pd[u][k] = 0.f; pm[u][k] = 0.f; pn[u][k] = 0.f; }
    }
  }
  if (threadIdx.x < 64u) {
    if (p.first) {
      if (threadIdx.x == 0) {
        s_Tpre = xidentity();
        if (blockIdx.x == 0) {  // the state before any iteration (replaces a separate init launch)
          MicpState init;
          init.T_onew_oold = xidentity();
          init.T_snew_sold = xidentity();
          init.stats_o = cs_identity();
          *p.state_out = init;
        }
      }
    } else {
      const cstats st = finalize_pose(p.partials_prev, p.nblocks);
      if (threadIdx.x == 0) {
        // sensor-frame form of the iteration (micp_advance_sensor): the odom-frame quantities are formed by the closing
        // launch (k_micp_close); between launches the state carries T_snew_sold only
        xform T_s = p.state_in->T_snew_sold;
        micp_advance_sensor(st, &T_s);
        s_Tpre = T_s;
        if (blockIdx.x == 0) p.state_out->T_snew_sold = T_s;
      }
    }
  }
  __syncthreads();
  const xform Tpre = s_Tpre;
  const float max_dist = p.call->max_dist;
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
#pragma unroll
  for (int u = 0; u < kPre; ++u)
    if (pok[u])
      p2l_accumulate(Tpre, mk3(pd[u][0], pd[u][1], pd[u][2]), mk3(pm[u][0], pm[u][1], pm[u][2]), mk3(pn[u][0], pn[u][1], pn[u][2]), max_dist, acc);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x + static_cast<uint32_t>(kPre) * gridDim.x * 256u; i < p.n; i += gridDim.x * 256u) {
    const bool dok = (p.dataset_mask == nullptr) || (p.dataset_mask[i] > 0);
    if (dok && p.model_mask[i] > 0) p2l_accumulate(Tpre, p.dataset_points, p.model_points, p.model_normals, i, max_dist, acc);
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  {
    const double wsum = wave_sum16_lds(acc, &s_wsum[wave][0], lane);
    if (lane < 16u) red[wave][lane] = wsum;
  }
  __syncthreads();
  if (threadIdx.x < kAcc)
    p.partials_out[static_cast<size_t>(blockIdx.x) * kAcc + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the state of a correction without iterations (k_micp_iter initialises itself)
__global__ void k_micp_init(MicpState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->T_onew_oold = xidentity();
    st->T_snew_sold = xidentity();
    st->stats_o = cs_identity();
    st[1] = st[0];  // the state ping-pongs between two slots (k_micp_iter)
  }
}

// closing launch of the one-launch-per-iteration form: the last iteration's solve + the odom-frame results.  st_out may point
// to host-mapped memory: the correction then delivers its result without a device-to-host copy node
__global__ void __launch_bounds__(64) k_micp_close(const double* __restrict__ partials, uint32_t nblocks, const MicpCall* call,
                                                   const MicpState* st, MicpState* st_out, unsigned long long* done) {
  const cstats stats_s = finalize_pose(partials, nblocks);
  if (threadIdx.x == 0) {
    xform T_s = st->T_snew_sold;
    micp_advance_sensor(stats_s, &T_s);
    MicpState out;
    micp_close_sensor(stats_s, T_s, call->Tsb, call->Tbo, &out);
    *st_out = out;
    if (done) publish_tag(done, call->seq, xor_words(out));   // the caller polls the tag instead of waiting for the stream's signal
  }
}

// ---------------------------------------------------------------------------------------------
// Gate-stable moment form of the MICP-L inner loop, schedule (R) (micp_localization.cpp:900-964: ONE find, then n_iter x
// (statistics_p2l + umeyama) over the SAME correspondences).  Between iterations only the pre-transform T = (R, t) changes:
//   D' = R D + t,  dist = N.I - N.D',  M = D' + N dist,  gate |dist| < max_dist           (MICPSensorCPU.cpp:70-84)
// so for a FIXED set of gated-in correspondences the 16 raw sums of the reduction (sum D', sum M, sum M D'^T, n) are
// polynomials in (R, t) whose coefficients are 82 moments of (D, N, s = N.I):
//   sum D, sum D D^T, sum s N, sum s N D^T, sum N N^T, sum N_a N_b D_j, sum N_a N_b D_j D_k.
// The gate is the only non-polynomial part.  A correspondence whose |dist| at the first pre-transform (identity) is
// farther from max_dist than the farthest its point can move, |D' - D| <= rho |D| + tau (rho = 2 sin(theta/2), tau = |t|),
// keeps its gate decision for every iteration whose pre-transform stays within (rho_cap, tau_cap): its contribution comes
// from the moments.  The others ("uncertain", normally a few hundred) are re-evaluated every iteration with the reduction's
// own f32 arithmetic.  One streaming pass (k_micp_moments) + ONE single-workgroup launch for all iterations
// (k_micp_fast_loop) replace n_iter streaming launches.  If a pre-transform leaves the caps or more than
// kFastMaxUncertain correspondences are uncertain, the loop reports it and the caller runs the per-iteration form instead:
// the result never depends on the caps.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kFastMaxUncertain = 4096;
// Bound of the device-side polls below (fold flags of sibling workgroups, join flags of another stream's signal kernel): a poll is
// one L2 round trip (~1 us), so ~2 s.  A producer that never arrives ends the launch with status code 2 -- the host then takes the
// per-iteration form, which joins with stream events -- instead of a kernel the 20 ms host fallback could never get past.
constexpr uint32_t kDevicePollBound = 1u << 21;
constexpr uint32_t kFastThreads = 256;   // 1 wave per SIMD: the one-lane solve may use up to 512 VGPRs (no scratch)

// ---- cheaper reciprocals for the ONE lane that solves (moment-form loops): a lone lane retires one instruction per ~5-8 cycles,
// so the solve costs what its instruction count costs, and an IEEE f64 division is ~25 instructions, a square root + division
// ~50.  v_rcp_f64 / v_rsq_f64 with two Newton-Raphson refinements give 1/x and 1/sqrt(x) to ~1 ulp in 5 / 9 instructions.  Used
// where the consumer is itself an iteration (Newton's step of the quartic) or is rounded to f32 afterwards (quaternion
// normalisation, 1/n of the statistics); the generic umeyama() of devmath.h -- shared with the host and the oracle-facing
// entry points -- keeps IEEE divisions.
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ double rsq_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * fma(-0.5 * x, y * y, 1.5);
  y = y * fma(-0.5 * x, y * y, 1.5);
  return y;
}

// horn_quaternion (devmath.h) with rcp_nr / rsq_nr; same formulas, same return codes (anything but kHornSolved -> the caller takes umeyama())
__device__ __forceinline__ int horn_quaternion_fast(const double* C, double* q) {
  const double Sxx = C[0], Sxy = C[3], Sxz = C[6], Syx = C[1], Syy = C[4], Syz = C[7], Szx = C[2], Szy = C[5], Szz = C[8];
  sym4 K;
  K.k00 = Sxx + Syy + Szz; K.k01 = Syz - Szy; K.k02 = Szx - Sxz; K.k03 = Sxy - Syx;
  K.k11 = Sxx - Syy - Szz; K.k12 = Sxy + Syx; K.k13 = Szx + Sxz;
  K.k22 = -Sxx + Syy - Szz; K.k23 = Syz + Szy;
  K.k33 = -Sxx - Syy + Szz;
  const double ss = ((Sxx * Sxx + Sxy * Sxy + Sxz * Sxz) + (Syx * Syx + Syy * Syy + Syz * Syz)) + (Szx * Szx + Szy * Szy + Szz * Szz);
  if (!(ss > 0.0)) return kHornRankLe1;   // the zero matrix
  const double c2 = -2.0 * ss;
  const double c1 = -8.0 * det3(C);
  const double c0 = sym4_det(sym4_sub(K));
  if (horn_rank_le1(ss, c0)) return kHornRankLe1;   // decided before anything is solved: the eigenvector of such a K is noise
  const double lam0 = sqrt(3.0 * ss) * (1.0 + 1e-12);
  double lam = lam0;
  {
    const double a = K.k00, a2 = a * a;
    const double Pa = (a2 + c2) * a2 + c1 * a + c0, dPa = (4.0 * a2 + 2.0 * c2) * a + c1;
    if (a > 0.0 && 3.0 * a2 > ss && dPa > 0.0 && Pa <= 0.0) {
      const double a1 = a - Pa * rcp_nr(dPa);
      if (a1 < lam0) lam = a1;
    }
  }
  bool converged = false;
  for (int it = 0; it < 60; ++it) {
    const double l2 = lam * lam;
    const double P = (l2 + c2) * l2 + c1 * lam + c0;
    const double dP = (4.0 * l2 + 2.0 * c2) * lam + c1;
    if (!(dP > 0.0)) break;
    const double step = P * rcp_nr(dP);
    lam -= step;
    if (step <= 1e-14 * lam0) { converged = true; break; }
  }
  if (!converged) return kHornDeclined;
  K.k00 -= lam; K.k11 -= lam; K.k22 -= lam; K.k33 -= lam;
  const sym4_minors m = sym4_sub(K);
  const double a00 = K.k11 * m.c5 - K.k12 * m.c4 + K.k13 * m.c3;
  const double a11 = K.k00 * m.c5 - K.k02 * m.c2 + K.k03 * m.c1;
  const double a22 = K.k03 * m.s4 - K.k13 * m.s2 + K.k33 * m.s0;
  const double a33 = K.k02 * m.s3 - K.k12 * m.s1 + K.k22 * m.s0;
  const double a01 = -K.k01 * m.c5 + K.k02 * m.c4 - K.k03 * m.c3;
  const double a02 = K.k13 * m.s5 - K.k23 * m.s4 + K.k33 * m.s3;
  const double a03 = -K.k12 * m.s5 + K.k22 * m.s4 - K.k23 * m.s3;
  const double a12 = -K.k03 * m.s5 + K.k23 * m.s2 - K.k33 * m.s1;
  const double a13 = K.k02 * m.s5 - K.k22 * m.s2 + K.k23 * m.s1;
  const double a23 = -K.k02 * m.s4 + K.k12 * m.s2 - K.k23 * m.s0;
  double v0 = a00, v1 = a01, v2 = a02, v3 = a03, dbest = fabs(a00);
  if (fabs(a11) > dbest) { v0 = a01; v1 = a11; v2 = a12; v3 = a13; dbest = fabs(a11); }
  if (fabs(a22) > dbest) { v0 = a02; v1 = a12; v2 = a22; v3 = a23; dbest = fabs(a22); }
  if (fabs(a33) > dbest) { v0 = a03; v1 = a13; v2 = a23; v3 = a33; dbest = fabs(a33); }
  if (!(dbest > 1e-10 * lam0 * lam0 * lam0)) return kHornDeclined;  // repeated largest eigenvalue
  const double n2 = (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
  if (!(n2 > 0.0)) return kHornDeclined;
  const double rn = rsq_nr(n2);
  double w = v0 * rn, x = v1 * rn, y = v2 * rn, z = v3 * rn;
  double lead = w;
  if (!(fabs(w) > 0.5)) {
    if (x * x > y * y && x * x > z * z) lead = x;
    else if (y * y > z * z) lead = y;
    else lead = z;
  }
  if (lead < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
  return kHornSolved;
}

// umeyama() for the moment-form loops' one solving lane; degenerate inputs take the generic path
__device__ __forceinline__ xform umeyama_fast(const cstats& s) {
  if (s.n_meas == 0) return xidentity();
  double C[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) C[i] = static_cast<double>(s.covariance[i]);
  double q[4];
  // rank <= 1 (devmath.h: the rank-one rule) and what Horn declines go to umeyama()
  if (horn_quaternion_fast(C, q) != kHornSolved) return umeyama(s);
  xform T = xidentity();
  T.R.x = static_cast<float>(q[0]); T.R.y = static_cast<float>(q[1]);
  T.R.z = static_cast<float>(q[2]); T.R.w = static_cast<float>(q[3]);
  T.t = sub3(s.model_mean, qrot(T.R, s.dataset_mean));
  return T;
}

// raw sums of the reduction (sd[3] sm[3] smd[9] n) -> CrossStatistics, as finalize_pose does but with one refined reciprocal
__device__ __forceinline__ cstats cstats_from_sums(const double* acc) {
  cstats s = cs_identity();
  const double n = acc[15];
  if (n > 0.0) {
    const double rn = rcp_nr(n);   // (finalize_pose divides 15 times: same values to the last bit or two)
    const double md[3] = {acc[0] * rn, acc[1] * rn, acc[2] * rn};
    const double mm[3] = {acc[3] * rn, acc[4] * rn, acc[5] * rn};
    s.dataset_mean = mk3(static_cast<float>(md[0]), static_cast<float>(md[1]), static_cast<float>(md[2]));
    s.model_mean = mk3(static_cast<float>(mm[0]), static_cast<float>(mm[1]), static_cast<float>(mm[2]));
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) s.covariance[3 * r + c] = static_cast<float>(acc[6 + 3 * r + c] * rn - mm[r] * md[c]);
    // ONE correspondence has no covariance.  The streaming sums give exactly that; sums evaluated from the moments leave their own
    // rounding (~1e-15) instead, a matrix of noise the solve would turn into an arbitrary rotation
    if (n == 1.0)
      for (int k = 0; k < 9; ++k) s.covariance[k] = 0.0f;
    s.n_meas = static_cast<uint32_t>(n);
  }
  return s;
}

struct MicpFastParams {
  const float* dataset_points;
  const uint8_t* dataset_mask;  // nullable
  const float* model_points;
  const float* model_normals;
  const uint8_t* model_mask;
  uint32_t n, nblocks;          // nblocks: grid of k_micp_moments
  const MicpCall* call;
  double* partials;             // [nblocks][kMom]
  unsigned long long* unc_mask; // [ceil(n / 64)]: bit i%64 of word i/64 = correspondence i is uncertain
  uint32_t n_iter;
  MicpState* state_out;         // may be host-mapped
  MicpFastStatus* status;       // may be host-mapped
  unsigned long long* done;     // host-mapped completion tag
  MicpCallLite cv;              // used when call == nullptr (direct launches)
  // mask words in the tile order of the find that produced them (launch_find_moments): word t = (virtual) tile t, bit l = lane l
  uint32_t mask_tiled, mask_W, mask_tiles_x, mask_tile_w_log2, mask_nwords;
  // k_micp_fast_loop launched as gridDim.x > 1 workgroups: workgroup b folds its share of the partial rows; b > 0 hands its 82 sums to
  // workgroup 0 through fold_rows[b] / fold_flags[b] (= this call's sequence number) and leaves
  double* fold_rows;            // [kMicpFoldBlocks][kMom]
  uint32_t* fold_flags;         // [kMicpFoldBlocks]
  MicpHostBlock* host_block;    // k_micp_publish: pinned, host-mapped
};
// correspondence index of bit `b` of mask word `w`
__device__ __forceinline__ uint32_t micp_mask_index(const MicpFastParams& p, uint32_t w, uint32_t b) {
  if (p.mask_tiled == 0u) return (w << 6) + b;
  const uint32_t ty = w / p.mask_tiles_x, tx = w - ty * p.mask_tiles_x, twl = p.mask_tile_w_log2;
  const uint32_t vid = (ty << (6u - twl)) + (b >> twl), hid = (tx << twl) + (b & ((1u << twl) - 1u));
  return vid * p.mask_W + hid;
}
__device__ __forceinline__ uint32_t micp_mask_words(const MicpFastParams& p) { return (p.mask_tiled != 0u) ? p.mask_nwords : ((p.n + 63u) >> 6); }
#define RMCL_FCALL(p, field) ((p).call != nullptr ? (p).call->field : (p).cv.field)

// Status blocks live in pinned host memory: the block is written whole, then the completion tag (publish_tag) with the sum of
// the block and of whatever else this exit wrote for the host (`extra`: the xor of the state block, 0 for the early exits).
__device__ __forceinline__ void publish_status(MicpFastStatus* dst, const MicpFastStatus& st, unsigned long long* tag, uint32_t seq,
                                               uint32_t extra) {
  MicpFastStatus body = st;
  body.pad[2] = 0u;
  *dst = body;                      // two 16-B stores
  publish_tag(tag, seq, xor_words(body) ^ extra);
}
__device__ __forceinline__ void publish_status(MicpMultiFastStatus* dst, const MicpMultiFastStatus& st, unsigned long long* tag,
                                               uint32_t seq, uint32_t extra) {
  *dst = st;
  publish_tag(tag, seq, xor_words(st) ^ extra);
}

__global__ void __launch_bounds__(256) k_micp_moments(const MicpFastParams p) {
  __shared__ double red[4][kMom];
  __shared__ double s_scratch[4][2][64 * 17];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const float gate_lo = RMCL_FCALL(p, gate_lo), gate_hi = RMCL_FCALL(p, gate_hi), rho_cap = RMCL_FCALL(p, rho_cap), tau_cap = RMCL_FCALL(p, tau_cap);
  double m[kMom];
#pragma unroll
  for (int k = 0; k < kMom; ++k) m[k] = 0.0;
  // a wave takes 64 consecutive correspondences per step (one mask word); two steps are requested before the first is used
  const uint32_t stride = gridDim.x * 256u;
  const uint32_t nceil = (p.n + 63u) & ~63u;
  for (uint32_t base = (blockIdx.x * 4u + wave) * 64u; base < nceil; base += 2u * stride) {
    float d[2][3], q[2][3], nn[2][3];
    bool ok[2], live[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t i = base + static_cast<uint32_t>(u) * stride + lane;
      live[u] = (base + static_cast<uint32_t>(u) * stride) < nceil;
      ok[u] = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) { d[u][k] = 0.f; q[u][k] = 0.f; nn[u][k] = 0.f; }
      if (i < p.n) {
        const bool dok = (p.dataset_mask == nullptr) || (p.dataset_mask[i] > 0);
        ok[u] = dok && p.model_mask[i] > 0;
        const float* dp = p.dataset_points + 3 * static_cast<size_t>(i);
        const float* mp = p.model_points + 3 * static_cast<size_t>(i);
        const float* mn = p.model_normals + 3 * static_cast<size_t>(i);
#pragma unroll
        for (int k = 0; k < 3; ++k) { d[u][k] = dp[k]; q[u][k] = mp[k]; nn[u][k] = mn[k]; }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!live[u]) continue;   // wave-uniform
      const f3 Di = mk3(d[u][0], d[u][1], d[u][2]), Ii = mk3(q[u][0], q[u][1], q[u][2]), Ni = mk3(nn[u][0], nn[u][1], nn[u][2]);
      // the reduction's own gate value at the identity pre-transform
      const float spd0 = dot_plain(sub3(Ii, Di), Ni);
      const float nd = sqrtf(dot_plain(Di, Di));
      // (a NaN gate value -- a NaN / inf dataset point without a mask -- is NaN under every pre-transform: gated out for good)
      const int cls = micp_gate_class(spd0, nd, gate_lo, gate_hi, rho_cap, tau_cap);
      const bool uncertain = ok[u] && cls == 2;
      const unsigned long long word = __ballot(uncertain);
      if (lane == 0u) p.unc_mask[(base + static_cast<uint32_t>(u) * stride) >> 6] = word;
      if (ok[u] && cls == 1) {
        const double D[3] = {Di.x, Di.y, Di.z}, N[3] = {Ni.x, Ni.y, Ni.z};
        const double sI = (N[0] * static_cast<double>(Ii.x) + N[1] * static_cast<double>(Ii.y)) + N[2] * static_cast<double>(Ii.z);
        const double DD[6] = {D[0] * D[0], D[0] * D[1], D[0] * D[2], D[1] * D[1], D[1] * D[2], D[2] * D[2]};
        const double NN[6] = {N[0] * N[0], N[0] * N[1], N[0] * N[2], N[1] * N[1], N[1] * N[2], N[2] * N[2]};
        m[0] += 1.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) m[1 + j] += D[j];
#pragma unroll
        for (int k = 0; k < 6; ++k) m[4 + k] += DD[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double sn = sI * N[a];
          m[10 + a] += sn;
#pragma unroll
          for (int j = 0; j < 3; ++j) m[13 + 3 * a + j] += sn * D[j];
        }
#pragma unroll
        for (int pq = 0; pq < 6; ++pq) {
          m[22 + pq] += NN[pq];
#pragma unroll
          for (int j = 0; j < 3; ++j) m[28 + 3 * pq + j] += NN[pq] * D[j];
#pragma unroll
          for (int k = 0; k < 6; ++k) m[46 + 6 * pq + k] += NN[pq] * DD[k];
        }
      }
    }
  }
  // six chunks of 16 moments, each with its own scratch area so that the chunks overlap
#pragma unroll
  for (int c = 0; c < kMom / 16; ++c) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = m[16 * c + k];
    const double t = wave_sum16_lds(v, &s_scratch[wave][c & 1][0], lane);
    if (lane < 16u) red[wave][16 * c + lane] = t;
  }
  __syncthreads();
  if (threadIdx.x < kMom)
    p.partials[static_cast<size_t>(blockIdx.x) * kMom + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// The 16 raw sums of the reduction over the CERTAIN correspondences at pre-transform (R row-major, t) from the moments, by
// one wave.  With X ranging over the ten per-correspondence factors  N_aN_b (6, symmetric pairs) | 1 | s N_a (3)  the moments
// are W(X) = sum X, P(X)_j = sum X D_j, Q(X)_jk = sum X D_j D_k, and every sum below is one of
//   rP(X)_b = sum_j R_bj P(X)_j,   H(X)_bc = sum_jk R_bj R_ck Q(X)_jk   (X = "1": sum D'_b, sum D'_b D'_c up to the t terms).
// Stage A (63 lanes) G(X)_cj = sum_k Q(X)_jk R_ck; stage B (63 + 30 lanes) H and rP; stage C (16 lanes) the outputs.
// All operands live in LDS; LDS operations of one wave complete in order (no barrier between the stages).
__device__ __forceinline__ int sym3(int a, int b) {
  const int lo = min(a, b), hi = max(a, b);
  return lo == 0 ? hi : (lo == 1 ? hi + 2 : 5);
}
__device__ __forceinline__ const double* mom_Q(const double* mom, int x) { return x < 6 ? mom + 46 + 6 * x : mom + 4; }
__device__ __forceinline__ const double* mom_P(const double* mom, int x) { return x < 6 ? mom + 28 + 3 * x : (x == 6 ? mom + 1 : mom + 13 + 3 * (x - 7)); }
__device__ __forceinline__ double mom_W(const double* mom, int x) { return x < 6 ? mom[22 + x] : (x == 6 ? mom[0] : mom[10 + (x - 7)]); }

struct MomentScratch { double G[64], H[64], rP[32]; };

__device__ __forceinline__ void micp_moment_sums_wave(uint32_t lane, const double* mom, const double* R, const double* t,
                                                      MomentScratch* ws, double* tot) {
  // stage A: lane = 9 x + 3 c + j, x = 0..6
  if (lane < 63u) {
    const int x = static_cast<int>(lane) / 9, c = (static_cast<int>(lane) % 9) / 3, j = static_cast<int>(lane) % 3;
    const double* Q = mom_Q(mom, x);
    ws->G[lane] = (Q[sym3(j, 0)] * R[3 * c] + Q[sym3(j, 1)] * R[3 * c + 1]) + Q[sym3(j, 2)] * R[3 * c + 2];
  }
  // stage B: lane = 9 x + 3 b + c -> H(x)_bc; lanes 0..29 also rP(x)_b with lane = 3 x + b, x = 0..9
  if (lane < 63u) {
    const int x = static_cast<int>(lane) / 9, b = (static_cast<int>(lane) % 9) / 3, c = static_cast<int>(lane) % 3;
    const double* Gx = ws->G + 9 * x + 3 * c;
    ws->H[lane] = (R[3 * b] * Gx[0] + R[3 * b + 1] * Gx[1]) + R[3 * b + 2] * Gx[2];
  }
  if (lane < 30u) {
    const int x = static_cast<int>(lane) / 3, b = static_cast<int>(lane) % 3;
    const double* P = mom_P(mom, x);
    ws->rP[lane] = (R[3 * b] * P[0] + R[3 * b + 1] * P[1]) + R[3 * b + 2] * P[2];
  }
  // stage C
  if (lane < 16u) {
    const double n = mom[0];
    double out;
    if (lane == 15u) {
      out = n;
    } else if (lane < 3u) {
      const int c = static_cast<int>(lane);
      out = ws->rP[18 + c] + n * t[c];
    } else if (lane < 6u) {
      const int a = static_cast<int>(lane) - 3;
      double ndp = 0.0;   // sum N_a (N . D')
      for (int b = 0; b < 3; ++b) {
        const int x = sym3(a, b);
        ndp += ws->rP[3 * x + b] + t[b] * mom_W(mom, x);
      }
      out = (ws->rP[18 + a] + n * t[a]) + mom[10 + a] - ndp;
    } else {
      const int a = (static_cast<int>(lane) - 6) / 3, c = (static_cast<int>(lane) - 6) % 3;
      const double ddp = ws->H[54 + 3 * a + c] + ws->rP[18 + a] * t[c] + t[a] * ws->rP[18 + c] + n * t[a] * t[c];   // sum D'_a D'_c
      const double sndp = ws->rP[3 * (7 + a) + c] + mom[10 + a] * t[c];                                            // sum s N_a D'_c
      double nndd = 0.0;                                                                                           // sum N_a (N . D') D'_c
      for (int b = 0; b < 3; ++b) {
        const int x = sym3(a, b);
        nndd += ws->H[9 * x + 3 * b + c] + t[c] * ws->rP[3 * x + b] + t[b] * ws->rP[3 * x + c] + t[b] * t[c] * mom_W(mom, x);
      }
      out = ddp + sndp - nndd;
    }
    tot[lane] = out;
  }
}

// Sum of the per-block moment partials [nblocks][kMom] into s_part[kFoldGroups][kMom] (the caller adds the groups after a barrier):
// five groups of 48 threads, TWO moments (one 16-B load) per thread and row, 13 rows in flight -- 128 rows are two round trips
// (round 2: two groups of 96 threads, one moment each, 16 in flight: four round trips, ~2 us of the loop kernel's set-up).
// Six groups of 41 lanes: a lane owns one 16-B column pair and every sixth row, 22 rows requested per round -- a fold is bound by what
// ONE compute unit can pull from L2 (64 B per clock), so only the 82 used columns are read and enough requests are in flight to
// keep that path busy: 128 rows (k_micp_moments) are one round, the 512 rows of a find with the moment epilogue four.
constexpr uint32_t kFoldGroups = 6, kFoldLanes = kMomUsed / 2, kFoldBatch = 22;
static_assert(kFoldGroups * kFoldLanes <= kFastThreads, "fold lanes");
__device__ __forceinline__ void fold_moment_partials(const double* __restrict__ partials, uint32_t nblocks, double (*s_part)[kMom], uint32_t tid) {
  const uint32_t k2 = tid % kFoldLanes, g = tid / kFoldLanes;
  if (g >= kFoldGroups) return;
  const double2* base = reinterpret_cast<const double2*>(partials) + k2;
  double a0 = 0.0, a1 = 0.0;
  for (uint32_t b0 = g; b0 < nblocks; b0 += kFoldBatch * kFoldGroups) {
    double2 v[kFoldBatch];
#pragma unroll
    for (uint32_t u = 0; u < kFoldBatch; ++u) {
      const uint32_t b = b0 + u * kFoldGroups;
      v[u] = (b < nblocks) ? base[static_cast<size_t>(b) * (kMom / 2)] : double2{0.0, 0.0};
    }
#pragma unroll
    for (uint32_t u = 0; u < kFoldBatch; ++u) { a0 += v[u].x; a1 += v[u].y; }
  }
  s_part[g][2u * k2] = a0;
  s_part[g][2u * k2 + 1u] = a1;
  if (k2 < (kMom - kMomUsed) / 2u) { s_part[g][kMomUsed + 2u * k2] = 0.0; s_part[g][kMomUsed + 2u * k2 + 1u] = 0.0; }
}
// ... column k over the groups, after the caller's barrier
__device__ __forceinline__ double fold_groups_sum(const double (*s_part)[kMom], uint32_t k) {
  double a = s_part[0][k];
#pragma unroll
  for (uint32_t g = 1; g < kFoldGroups; ++g) a += s_part[g][k];
  return a;
}

// ---- the fold by several workgroups (k_micp_fast_loop, k_micp_publish behind a find with the moment epilogue).  One compute unit pulls
// 64 B per clock from L2: the 512 rows such a find leaves (336 KB) would take it 4 us, so the launch comes as gridDim.x workgroups -- each
// folds its share of the rows, the others hand their 82 sums to workgroup 0 (write-through stores, then a release of this call's sequence
// number) and leave.
__device__ __forceinline__ void fold_workgroup_share(const MicpFastParams& p, double (*s_part)[kMom], uint32_t tid) {
  const uint32_t nfold = gridDim.x;
  const uint32_t rows_per = (p.nblocks + nfold - 1u) / nfold;
  const uint32_t row0 = min(blockIdx.x * rows_per, p.nblocks), row1 = min(row0 + rows_per, p.nblocks);
  fold_moment_partials(p.partials + static_cast<size_t>(row0) * kMom, row1 - row0, s_part, tid);
}
// a sibling's side, between two barriers of the caller: its sums into fold_rows[blockIdx.x] ...
__device__ __forceinline__ void fold_hand_over_row(const double (*s_part)[kMom], double* fold_rows, uint32_t tid) {
  if (tid < kMomUsed)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(fold_rows) + blockIdx.x * kMom + tid,
                       static_cast<unsigned long long>(__double_as_longlong(fold_groups_sum(s_part, tid))), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
// ... and, after the second barrier, the flag
__device__ __forceinline__ void fold_hand_over_release(uint32_t* fold_flags, uint32_t seq, uint32_t tid) {
  if (tid == 0u) __hip_atomic_store(fold_flags + blockIdx.x, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// Workgroup 0's side, thread tid < kMomUsed: the other workgroups' sums of column tid added to *a in workgroup order; every reading
// thread acquires the flags itself (all flags polled together, ONE acquire, all rows requested together: two memory round trips, not
// two per workgroup).  false: a sibling's sums did not arrive within kDevicePollBound polls (what was added is then meaningless).
__device__ __forceinline__ bool fold_gather_rows(const double* fold_rows, const uint32_t* fold_flags, uint32_t nfold, uint32_t seq,
                                                 uint32_t tid, double* a) {
  bool ready;
  uint32_t polls = 0;
  do {
    uint32_t f[kMicpFoldBlocks];
#pragma unroll
    for (uint32_t b = 1; b < kMicpFoldBlocks; ++b)
      f[b] = (b < nfold) ? __hip_atomic_load(fold_flags + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : seq;
    ready = true;
#pragma unroll
    for (uint32_t b = 1; b < kMicpFoldBlocks; ++b) ready = ready && (f[b] == seq);
  } while (!ready && ++polls < kDevicePollBound);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  unsigned long long v[kMicpFoldBlocks];
#pragma unroll
  for (uint32_t b = 1; b < kMicpFoldBlocks; ++b)
    v[b] = (b < nfold) ? __hip_atomic_load(reinterpret_cast<const unsigned long long*>(fold_rows) + b * kMom + tid, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)
                       : 0ull;
#pragma unroll
  for (uint32_t b = 1; b < kMicpFoldBlocks; ++b) *a += __longlong_as_double(static_cast<long long>(v[b]));
  return ready;
}

// ---- the undecided correspondences in index order: every thread counts the bits of a contiguous range of mask words, a scan over the
// workgroup turns the counts into list positions
struct MaskShare { uint32_t w0, w1, cnt, incl; };   // the thread's words [w0, w1), their bits, the inclusive sum over the wave's lanes
__device__ __forceinline__ MaskShare mask_count_scan(const unsigned long long* mask, uint32_t nwords, uint32_t tid) {
  const uint32_t lane = tid & 63u;
  const uint32_t wpt = (nwords + kFastThreads - 1u) / kFastThreads;
  const uint32_t w0 = min(tid * wpt, nwords), w1 = min(w0 + wpt, nwords);
  uint32_t cnt = 0;
  for (uint32_t w = w0; w < w1; w += 8u) {   // eight words requested together (a word per iteration was one round trip per word)
    unsigned long long m[8];
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) m[u] = (w + u < w1) ? mask[w + u] : 0ull;
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) cnt += static_cast<uint32_t>(__popcll(m[u]));
  }
  uint32_t incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off, 64);
    if (lane >= static_cast<uint32_t>(off)) incl += v;
  }
  return MaskShare{w0, w1, cnt, incl};
}
// s_wave_cnt[w] = lane 63's inclusive sum of wave w, read after the caller's barrier -> bits before this wave, bits in all
__device__ __forceinline__ void wave_offsets(const uint32_t* s_wave_cnt, uint32_t wave, uint32_t* wave_base, uint32_t* total) {
  *wave_base = 0;
  *total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kFastThreads / 64; ++w) {
    const uint32_t c = s_wave_cnt[w];
    if (w < wave) *wave_base += c;
    *total += c;
  }
}
// correspondence index of bit b of word w: words in index order, or in the tile order of the find that wrote them
struct PlainMaskIndex {
  __device__ __forceinline__ uint32_t operator()(uint32_t w, uint32_t b) const { return (w << 6) + b; }
};
struct TiledMaskIndex {
  const MicpFastParams& p;
  __device__ __forceinline__ uint32_t operator()(uint32_t w, uint32_t b) const { return micp_mask_index(p, w, b); }
};
// the thread's bits appended to s_list from position `pos` (= list start + wave_base + incl - cnt)
template <typename Index>
__device__ __forceinline__ void mask_list_append(const unsigned long long* mask, const MaskShare& ms, uint32_t pos, uint32_t* s_list, Index index) {
  if (ms.cnt == 0u) return;
  for (uint32_t w = ms.w0; w < ms.w1; ++w) {
    unsigned long long bits = mask[w];
    while (bits) {
      const int b = __builtin_ctzll(bits);
      bits &= bits - 1ull;
      s_list[pos++] = index(w, static_cast<uint32_t>(b));
    }
  }
}

// The undecided correspondences s_list[e0 .. e1) with the reduction's own arithmetic (p2l_accumulate); re-read every iteration (L2 hits,
// normally a few hundred elements) so that nothing of them is live across the one-lane solve.  Thread t sums elements e0 + t,
// e0 + t + 256, ... into row t; the caller adds the rows in index order: no cross-lane butterfly, deterministic.
__device__ __forceinline__ void undecided_row_sums(const xform Tpre, float max_dist, const float* dataset_points, const float* model_points,
                                                   const float* model_normals, const uint32_t* s_list, uint32_t e0, uint32_t e1, uint32_t tid,
                                                   double (*s_rows)[17]) {
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  for (uint32_t e = e0 + tid; e < e1; e += kFastThreads) p2l_accumulate(Tpre, dataset_points, model_points, model_normals, s_list[e], max_dist, acc);
#pragma unroll
  for (int k = 0; k < kAcc; ++k) s_rows[tid][k] = acc[k];
}
// the pre-transform of an iteration as the moment sums take it: rotation matrix in double from the f32 quaternion, translation
__device__ __forceinline__ void pretransform_f64(const xform& T, double* R, double* t) {
  micp_rotation_f64(T.R, R);
  t[0] = T.t.x; t[1] = T.t.y; t[2] = T.t.z;
}

__global__ void __launch_bounds__(kFastThreads) k_micp_fast_loop(const MicpFastParams p) {
  __shared__ double s_mom[kMom];
  __shared__ double s_part[kFoldGroups][kMom];
  __shared__ double s_rows[kFastThreads][17];   // per-thread raw sums of the uncertain correspondences (+1: bank spread)
  __shared__ double s_tot[16];
  __shared__ double s_R[9], s_t[3];
  __shared__ MomentScratch s_ws;
  __shared__ uint32_t s_list[kFastMaxUncertain];
  __shared__ uint32_t s_wave_cnt[kFastThreads / 64];
  __shared__ xform s_Tpre;
  __shared__ uint32_t s_flag;
  __shared__ uint32_t s_abort;   // a sibling workgroup's sums did not arrive within kDevicePollBound polls
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long clk0 = __builtin_readcyclecounter();

  // (1) moments = sum of the per-block partials; launched as several workgroups, the others hand their sums to workgroup 0 and leave
  const uint32_t nfold = gridDim.x;
  fold_workgroup_share(p, s_part, tid);
  if (blockIdx.x != 0u) {
    __syncthreads();
    fold_hand_over_row(s_part, p.fold_rows, tid);
    __syncthreads();
    fold_hand_over_release(p.fold_flags, RMCL_FCALL(p, seq), tid);
    return;
  }
  // (2) the uncertain correspondences, in index order: count per thread over a contiguous range of mask words, block scan
  const MaskShare ms = mask_count_scan(p.unc_mask, micp_mask_words(p), tid);
  if (lane == 63u) s_wave_cnt[wave] = ms.incl;
  if (tid == 0u) { s_flag = 0u; s_abort = 0u; }
  __syncthreads();
  if (tid < kMom) {
    double a = fold_groups_sum(s_part, tid);
    if (nfold > 1u && tid < kMomUsed && !fold_gather_rows(p.fold_rows, p.fold_flags, nfold, RMCL_FCALL(p, seq), tid, &a)) s_abort = 1u;
    s_mom[tid] = a;
  }
  uint32_t wave_base, total;
  wave_offsets(s_wave_cnt, wave, &wave_base, &total);
  if (nfold > 1u) {   // (launch-uniform) did every sibling's row arrive?
    __syncthreads();
    if (s_abort != 0u) total = kFastMaxUncertain + 1u;
  }
  if (total > kFastMaxUncertain) {
    if (tid == 0u) {
      MicpFastStatus st;
      st.code = 2u; st.iter = 0u; st.n_uncertain = total; st.max_rho = 0.f; st.max_tau = 0.f; st.pad[0] = st.pad[1] = st.pad[2] = 0u;
      publish_status(p.status, st, p.done, RMCL_FCALL(p, seq), 0u);
    }
    return;
  }
  mask_list_append(p.unc_mask, ms, wave_base + ms.incl - ms.cnt, s_list, TiledMaskIndex{p});
  const float max_dist = RMCL_FCALL(p, max_dist), rho_cap = RMCL_FCALL(p, rho_cap), tau_cap = RMCL_FCALL(p, tau_cap);
  const uint32_t nrows = min(total, kFastThreads);
  // No undecided correspondence (the usual case of a tracking-size correction): everything the iterations need is the 82
  // moments, and wave 0 alone runs them -- no workgroup barrier inside the loop (the LDS operations of ONE wave complete in
  // program order); the other waves leave once the moments they summed are in LDS.
  const bool lone = (total == 0u);
  if (lone) {
    __syncthreads();
    if (wave != 0u) return;
  }
  // thread 0 owns the loop state (registers): the sensor-frame pre-transform and the statistics of the last iteration
  xform T_s = xidentity();
  cstats last = cs_identity();
  float max_rho = 0.f, max_tau = 0.f;
  const unsigned long long clk1 = __builtin_readcyclecounter();
  for (uint32_t it = 0; it < p.n_iter; ++it) {
    if (tid == 0u) {
      const float rho = micp_rho(T_s), tau = micp_tau(T_s);
      max_rho = fmaxf(max_rho, rho);
      max_tau = fmaxf(max_tau, tau);
      if (!(rho <= rho_cap) || !(tau <= tau_cap)) s_flag = 1u;
      s_Tpre = T_s;
      pretransform_f64(T_s, s_R, s_t);
    }
    if (lone) __builtin_amdgcn_wave_barrier();
    else __syncthreads();   // (A) pre-transform published; also orders the previous iteration's reads of s_rows / s_tot
    if (s_flag != 0u) {
      if (tid == 0u) {
        MicpFastStatus st;
        st.code = 1u; st.iter = it; st.n_uncertain = total; st.max_rho = max_rho; st.max_tau = max_tau; st.pad[0] = st.pad[1] = st.pad[2] = 0u;
        publish_status(p.status, st, p.done, RMCL_FCALL(p, seq), 0u);
      }
      return;
    }
    if (tid < nrows) undecided_row_sums(s_Tpre, max_dist, p.dataset_points, p.model_points, p.model_normals, s_list, 0u, total, tid, s_rows);
    if (nrows > 64u) __syncthreads();   // (B) rows of other waves (block-uniform condition); wave 0's own rows are in order
    if (wave == 0u) {
      micp_moment_sums_wave(lane, s_mom, s_R, s_t, &s_ws, s_tot);
      if (lane < 16u && nrows != 0u) {
        double v = s_tot[lane];
        for (uint32_t r = 0; r < nrows; ++r) v += s_rows[r][lane];
        s_tot[lane] = v;
      }
    }
    if (tid == 0u) {
      // lanes 0..15 of this wave wrote s_tot just above (LDS operations of one wave complete in order)
      double tot[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) tot[k] = s_tot[k];
      last = cstats_from_sums(tot);
      T_s = xmul(T_s, umeyama_fast(last));   // micp_advance_sensor with the cheaper reciprocals
    }
  }
  if (tid == 0u) {
    MicpState out;
    micp_close_sensor(last, T_s, RMCL_FCALL(p, Tsb), RMCL_FCALL(p, Tbo), &out);
    *p.state_out = out;
    MicpFastStatus st;
    st.code = 0u; st.iter = p.n_iter; st.n_uncertain = total; st.max_rho = max_rho; st.max_tau = max_tau;
    st.pad[0] = static_cast<uint32_t>(clk1 - clk0);                              // diagnostics: shader clocks of the set-up
    st.pad[1] = static_cast<uint32_t>(__builtin_readcyclecounter() - clk1);      // ... and of all iterations
    st.pad[2] = 0u;
    publish_status(p.status, st, p.done, RMCL_FCALL(p, seq), xor_words(out));
  }
}

// ---------------------------------------------------------------------------------------------
// Round 4: the iterations leave the device.  k_micp_fast_loop above spends ~4.4 k cycles per iteration in ONE lane's dependent f64
// chain (Horn's quartic, the frame products) -- 34 of a correction's 60 us -- although an iteration is a closed-form function of
// the 82 moments and the few undecided correspondences.  k_micp_publish folds the per-workgroup rows exactly as the loop kernel
// does (same order, same sums) and writes {moments, undecided count, D | I | N of every undecided correspondence} into pinned
// host memory behind one completion tag; the host (micp_host.h) then runs the iterations -- rmclhip_rcc_correct_once -- or
// answers every computeCrossStatistics of the reference's unchanged caller loop (micp_localization.cpp:915-964) with no launch
// at all.  More than kMicpHostMaxUnc undecided correspondences: code 2, the caller launches the device loop on the same rows.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFastThreads) k_micp_publish(const MicpFastParams p) {
  __shared__ double s_part[kFoldGroups][kMom];
  __shared__ uint32_t s_list[kMicpHostMaxUnc];
  __shared__ float s_stage[9u * kMicpHostMaxUnc];
  __shared__ uint32_t s_wave_cnt[kFastThreads / 64];
  __shared__ uint32_t s_xor[kFastThreads / 64];
  __shared__ uint32_t s_abort;   // a sibling workgroup's sums did not arrive within kDevicePollBound polls: code 2
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nfold = gridDim.x;
  fold_workgroup_share(p, s_part, tid);
  if (blockIdx.x != 0u) {
    __syncthreads();
    fold_hand_over_row(s_part, p.fold_rows, tid);
    __syncthreads();
    fold_hand_over_release(p.fold_flags, p.cv.seq, tid);
    return;
  }
  // the undecided correspondences, in index order (as k_micp_fast_loop counts them)
  const MaskShare ms = mask_count_scan(p.unc_mask, micp_mask_words(p), tid);
  if (lane == 63u) s_wave_cnt[wave] = ms.incl;
  if (tid == 0u) s_abort = 0u;
  __syncthreads();
  uint32_t x = 0u;   // xor of the words this thread writes for the host
  if (tid < kMom) {
    double a = 0.0;
    if (tid < kMomUsed) {
      a = fold_groups_sum(s_part, tid);
      if (nfold > 1u && !fold_gather_rows(p.fold_rows, p.fold_flags, nfold, p.cv.seq, tid, &a)) s_abort = 1u;
    }
    p.host_block->mom[tid] = a;
    const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(a));
    x ^= static_cast<uint32_t>(bits) ^ static_cast<uint32_t>(bits >> 32);
  }
  uint32_t wave_base, total;
  wave_offsets(s_wave_cnt, wave, &wave_base, &total);
  const bool fits = total <= kMicpHostMaxUnc;   // block-uniform
  if (fits && total != 0u) {
    mask_list_append(p.unc_mask, ms, wave_base + ms.incl - ms.cnt, s_list, TiledMaskIndex{p});
    __syncthreads();
    // gather D | I | N of the listed correspondences into LDS, then write the block to the host in address order (consecutive lanes,
    // consecutive dwords: a thread storing its own 36-B record put nine narrow writes per correspondence on the bus)
    for (uint32_t e = tid; e < total; e += kFastThreads) {
      const uint32_t i = s_list[e];
      const float* dp = p.dataset_points + 3 * static_cast<size_t>(i);
      const float* mp = p.model_points + 3 * static_cast<size_t>(i);
      const float* mn = p.model_normals + 3 * static_cast<size_t>(i);
      const float v[9] = {dp[0], dp[1], dp[2], mp[0], mp[1], mp[2], mn[0], mn[1], mn[2]};
#pragma unroll
      for (int k = 0; k < 9; ++k) s_stage[9u * e + static_cast<uint32_t>(k)] = v[k];
    }
    __syncthreads();
    float* dst = &p.host_block->unc[0][0];
    for (uint32_t w = tid; w < 9u * total; w += kFastThreads) {
      const float v = s_stage[w];
      dst[w] = v;
      x ^= __float_as_uint(v);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x ^= __shfl_xor(x, off, 64);
  if (lane == 0u) s_xor[wave] = x;
  __threadfence_system();   // this thread's stores to the host block, before the tag below
  __syncthreads();
  if (tid == 0u) {
    const uint32_t code = (fits && s_abort == 0u) ? 0u : 2u;
    p.host_block->code = code;
    p.host_block->n_uncertain = total;
    p.host_block->pad[0] = 0u; p.host_block->pad[1] = 0u;
    publish_tag(p.done, p.cv.seq, ((s_xor[0] ^ s_xor[1]) ^ (s_xor[2] ^ s_xor[3])) ^ (code ^ total));
  }
}

// N sensors, one iteration of MICPLocalizationNode::correctOnce (micp_localization.cpp:915-964), ONE wave:
//   per sensor (in order): stats_s <- partials; Cs_b = Tsb * stats_s (MICPSensor.hpp:182); Cs_o = Tbo * Cs_b (:931);
//   Cs_weighted_o = Cs_o with n_meas *= merge_weight_multiplier (truncating, :934); Cmerged_o += Cs_o; Cmerged_weighted_o += ...
//   T_inner = umeyama(Cmerged_weighted_o) (:952); T_onew_oold *= T_inner (:963);
//   next pre-transforms: T_bnew_bold = ~Tbo * T_onew_oold * Tbo (:926), T_snew_sold = ~Tsb * T_bnew_bold * Tsb (MICPSensor.hpp:178)
__global__ void __launch_bounds__(64) k_micp_multi_step(const MicpMultiCall* __restrict__ call, MicpMultiState* __restrict__ st) {
  const uint32_t ns = call->n_sensors;
  cstats merged = cs_identity(), merged_w = cs_identity();
  for (uint32_t s = 0; s < ns; ++s) {
    const cstats stats_s = finalize_pose(call->partials[s], call->nblocks[s]);   // whole wave
    if (threadIdx.x == 0) {
      const cstats Cs_o = cs_transform(call->Tbo[s], cs_transform(call->Tsb[s], stats_s));
      cstats Cs_w = Cs_o;
      Cs_w.n_meas = static_cast<uint32_t>(static_cast<double>(Cs_w.n_meas) * call->weight[s]);
      merged = cs_merge(merged, Cs_o);
      merged_w = cs_merge(merged_w, Cs_w);
    }
  }
  if (threadIdx.x == 0) {
    const xform T_inner = umeyama(merged_w);
    const xform T_onew_oold = xmul(st->T_onew_oold, T_inner);
    st->T_onew_oold = T_onew_oold;
    st->merged_o = merged;
    st->merged_weighted_o = merged_w;
    for (uint32_t s = 0; s < ns; ++s) {
      const xform T_bnew_bold = xmul(xmul(xinv(call->Tbo[s]), T_onew_oold), call->Tbo[s]);
      st->T_snew_sold[s] = xmul(xmul(xinv(call->Tsb[s]), T_bnew_bold), call->Tsb[s]);
    }
  }
}

__global__ void k_micp_multi_init(const MicpMultiCall* __restrict__ call, MicpMultiState* __restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->T_onew_oold = xidentity();
  st->merged_o = cs_identity();
  st->merged_weighted_o = cs_identity();
  for (uint32_t s = 0; s < kMaxMicpSensors; ++s) st->T_snew_sold[s] = xidentity();
}

// rmclhip_debug_solve (include/rmclhip_lab.h): the device's solvers on caller-supplied statistics, one thread per element
__global__ void __launch_bounds__(64) k_debug_solve(const cstats* __restrict__ stats, uint32_t n, int fast, xform* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const cstats s = stats[i];
  out[i] = fast ? umeyama_fast(s) : umeyama(s);
}

}  // namespace

// Moment form of the N-sensor loop (k_micp_multi_step's iteration, micp_localization.cpp:915-964): every sensor's statistics
// come from its moments + its undecided correspondences at ITS pre-transform (see k_micp_fast_loop); the merge over the sensors
// and the solve keep the frame-by-frame order of k_micp_multi_step.
__global__ void __launch_bounds__(kFastThreads) k_micp_multi_fast_loop(const MicpMultiFastParams p) {
  __shared__ double s_mom[kMaxMicpSensors][kMom];
  __shared__ double s_part[kFoldGroups][kMom];
  __shared__ double s_rows[kFastThreads][17];
  __shared__ double s_tot[kMaxMicpSensors][16];
  __shared__ double s_R[kMaxMicpSensors][9], s_t[kMaxMicpSensors][3];
  __shared__ MomentScratch s_ws[kFastThreads / 64];   // one per wave: without undecided correspondences wave w sums sensor w
  __shared__ uint32_t s_list[kFastMaxUncertain];
  __shared__ uint32_t s_seg[kMaxMicpSensors + 1];
  __shared__ uint32_t s_wave_cnt[kFastThreads / 64];
  __shared__ xform s_Ts[kMaxMicpSensors];
  __shared__ cstats s_Cs[kMaxMicpSensors];       // sensor statistics in the odom frame
  __shared__ uint32_t s_wn[kMaxMicpSensors];     // ... and their weighted n_meas
  __shared__ xform s_Tone;                       // T_onew_oold of this iteration, for the sensors' lanes
  __shared__ float s_max_rho[kMaxMicpSensors], s_max_tau[kMaxMicpSensors];
  __shared__ uint32_t s_bad;                     // smallest index of a sensor whose pre-transform left its caps
  __shared__ uint32_t s_join_lost;               // a joined stream's signal did not arrive within kDevicePollBound polls
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t ns = p.n_sensors;

  // set-up, sensor by sensor: moments and the index-ordered list segment of its undecided correspondences
  uint32_t total = 0;
  for (uint32_t s = 0; s < ns; ++s) {
    if ((p.join_mask >> s) & 1u) {
      // this sensor's rows and mask words come from another stream: its signal kernel (behind its moment pass) stores the call's
      // sequence number; one lane acquires it, the barrier hands the visibility to the workgroup
      if (tid == 0u) {
        uint32_t polls = 0;
        while (__hip_atomic_load(p.join_flags + s, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != p.seq && ++polls < kDevicePollBound)
          __builtin_amdgcn_s_sleep(2);
        s_join_lost = (polls >= kDevicePollBound) ? 1u : 0u;
      }
      __syncthreads();
      if (s_join_lost != 0u) {   // the other stream's signal never came: code 2, the host takes the per-iteration form
        if (tid == 0u) {
          MicpMultiFastStatus st;
          st.code = 2u; st.iter = 0u; st.n_uncertain = 0xffffffffu; st.sensor = s;
          for (uint32_t q = 0; q < kMaxMicpSensors; ++q) { st.max_rho[q] = 0.f; st.max_tau[q] = 0.f; }
          publish_status(p.status, st, p.done, p.seq, 0u);
        }
        return;
      }
    }
    fold_moment_partials(p.partials[s], p.nblocks[s], s_part, tid);
    const unsigned long long* mask = p.unc_mask[s];
    const MaskShare ms = mask_count_scan(mask, (p.n[s] + 63u) >> 6, tid);
    if (lane == 63u) s_wave_cnt[wave] = ms.incl;
    __syncthreads();
    if (tid < kMom) s_mom[s][tid] = fold_groups_sum(s_part, tid);
    uint32_t wave_base, cnt_s;
    wave_offsets(s_wave_cnt, wave, &wave_base, &cnt_s);
    if (tid == 0u) s_seg[s] = total;
    if (total + cnt_s > kFastMaxUncertain) {
      if (tid == 0u) {
        MicpMultiFastStatus st;
        st.code = 2u; st.iter = 0u; st.n_uncertain = total + cnt_s; st.sensor = s;
        for (uint32_t q = 0; q < kMaxMicpSensors; ++q) { st.max_rho[q] = 0.f; st.max_tau[q] = 0.f; }
        publish_status(p.status, st, p.done, p.seq, 0u);
      }
      return;
    }
    mask_list_append(mask, ms, total + wave_base + ms.incl - ms.cnt, s_list, PlainMaskIndex{});
    total += cnt_s;
    __syncthreads();   // s_part / s_wave_cnt are reused by the next sensor
  }
  if (tid == 0u) {
    s_seg[ns] = total;
    s_bad = 0xFFFFFFFFu;
  }
  // Lane s of wave 0 OWNS sensor s (round 3): its frames, their inverses, its pre-transform and its caps live in that lane's
  // registers, and everything that is per sensor -- the pre-transform's rotation matrix, the frame changes of its statistics, its
  // next pre-transform -- runs in the ns lanes at once.  Lane 0 alone only merges and solves.  (Round 2 ran all of it on lane 0:
  // ~2000 dependent instructions per iteration for two sensors, 9.4 us.)
  const bool is_sensor = tid < ns;
  const uint32_t sx = is_sensor ? tid : 0u;
  const xform my_Tsb = p.Tsb[sx], my_Tbo = p.Tbo[sx];
  const xform my_Tsb_inv = xinv(my_Tsb), my_Tbo_inv = xinv(my_Tbo);
  const double my_weight = p.weight[sx];
  const float my_rho_cap = p.rho_cap[sx], my_tau_cap = p.tau_cap[sx];
  xform my_Ts = xidentity();
  float my_max_rho = 0.f, my_max_tau = 0.f;
  if (is_sensor) { s_Ts[tid] = my_Ts; s_max_rho[tid] = 0.f; s_max_tau[tid] = 0.f; }
  // loop state of thread 0
  xform T_onew_oold = xidentity();
  cstats merged = cs_identity(), merged_w = cs_identity();
  __syncthreads();
  for (uint32_t it = 0; it < p.n_iter; ++it) {
    if (is_sensor) {
      const xform T = my_Ts;
      const float rho = micp_rho(T), tau = micp_tau(T);
      my_max_rho = fmaxf(my_max_rho, rho);
      my_max_tau = fmaxf(my_max_tau, tau);
      s_max_rho[tid] = my_max_rho; s_max_tau[tid] = my_max_tau;
      if (!(rho <= my_rho_cap) || !(tau <= my_tau_cap)) atomicMin(&s_bad, tid);   // the FIRST sensor outside its caps is reported
      pretransform_f64(T, s_R[tid], s_t[tid]);
    }
    __syncthreads();
    if (s_bad != 0xFFFFFFFFu) {
      if (tid == 0u) {
        MicpMultiFastStatus st;
        st.code = 1u; st.iter = it; st.n_uncertain = total; st.sensor = s_bad;
        for (uint32_t q = 0; q < kMaxMicpSensors; ++q) { st.max_rho[q] = (q < ns) ? s_max_rho[q] : 0.f; st.max_tau[q] = (q < ns) ? s_max_tau[q] : 0.f; }
        publish_status(p.status, st, p.done, p.seq, 0u);
      }
      return;
    }
    if (total == 0u) {
      // nothing to re-evaluate (the usual tracking case): the sensors' 16 sums come from their moments alone, one sensor per wave
      for (uint32_t s = wave; s < ns; s += kFastThreads / 64u) micp_moment_sums_wave(lane, s_mom[s], s_R[s], s_t[s], &s_ws[wave], s_tot[s]);
      __syncthreads();
    } else
    for (uint32_t s = 0; s < ns; ++s) {
      const uint32_t seg0 = s_seg[s], seg1 = s_seg[s + 1];
      const uint32_t nrows = min(seg1 - seg0, kFastThreads);
      if (tid < nrows)
        undecided_row_sums(s_Ts[s], p.max_dist[s], p.dataset_points[s], p.model_points[s], p.model_normals[s], s_list, seg0, seg1, tid, s_rows);
      __syncthreads();
      if (wave == 0u) {
        micp_moment_sums_wave(lane, s_mom[s], s_R[s], s_t[s], &s_ws[0], s_tot[s]);
        if (lane < 16u && nrows != 0u) {
          double v = s_tot[s][lane];
          for (uint32_t r = 0; r < nrows; ++r) v += s_rows[r][lane];
          s_tot[s][lane] = v;
        }
      }
      __syncthreads();   // s_rows / s_ws are reused by the next sensor
    }
    // k_micp_multi_step's merge and solve, frame by frame: the frame changes sensor-parallel, merge + solve on lane 0, the next
    // pre-transforms sensor-parallel again.  All in wave 0, whose LDS operations complete in program order.
    if (is_sensor) {
      double tot[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) tot[k] = s_tot[tid][k];
      const cstats stats_s = cstats_from_sums(tot);
      s_Cs[tid] = cs_transform(my_Tbo, cs_transform(my_Tsb, stats_s));
      s_wn[tid] = static_cast<uint32_t>(static_cast<double>(stats_s.n_meas) * my_weight);   // n_meas *= merge_weight_multiplier (:934)
    }
    if (wave == 0u) __builtin_amdgcn_wave_barrier();
    if (tid == 0u) {
      merged = cs_identity();
      merged_w = cs_identity();
      for (uint32_t s = 0; s < ns; ++s) {
        const cstats Cs_o = s_Cs[s];
        cstats Cs_w = Cs_o;
        Cs_w.n_meas = s_wn[s];
        merged = cs_merge(merged, Cs_o);
        merged_w = cs_merge(merged_w, Cs_w);
      }
      T_onew_oold = xmul(T_onew_oold, umeyama_fast(merged_w));
      s_Tone = T_onew_oold;
    }
    if (wave == 0u) __builtin_amdgcn_wave_barrier();
    if (is_sensor) {
      const xform T1 = s_Tone;
      const xform T_bnew_bold = xmul(xmul(my_Tbo_inv, T1), my_Tbo);
      my_Ts = xmul(xmul(my_Tsb_inv, T_bnew_bold), my_Tsb);
      s_Ts[tid] = my_Ts;
    }
  }
  __syncthreads();
  if (tid == 0u) {
    MicpMultiState* out = p.state_out;
    out->T_onew_oold = T_onew_oold;
    out->merged_o = merged;
    out->merged_weighted_o = merged_w;
    for (uint32_t s = 0; s < ns; ++s) out->T_snew_sold[s] = s_Ts[s];
    MicpMultiFastStatus st;
    st.code = 0u; st.iter = p.n_iter; st.n_uncertain = total; st.sensor = 0u;
    for (uint32_t q = 0; q < kMaxMicpSensors; ++q) { st.max_rho[q] = (q < ns) ? s_max_rho[q] : 0.f; st.max_tau[q] = (q < ns) ? s_max_tau[q] : 0.f; }
    // the host reads T_onew_oold and the merged statistics of this block (rmclhip_micp_correct_once)
    publish_status(p.status, st, p.done, p.seq, xor_words(T_onew_oold) ^ xor_words(merged) ^ xor_words(merged_w));
  }
}

hipError_t launch_micp_iter(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                            const float* model_normals, const uint8_t* model_mask, uint32_t n, uint32_t nblocks,
                            const MicpCall* call, const double* partials_prev, double* partials_out,
                            const MicpState* state_in, MicpState* state_out, bool first, hipStream_t s) {
  MicpIterParams p{dataset_points, dataset_mask, model_points, model_normals, model_mask, n, nblocks, call,
                   partials_prev, partials_out, state_in, state_out, first ? 1u : 0u};
  hipLaunchKernelGGL(k_micp_iter, dim3(nblocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

namespace {
// What every launch of the one-sensor moment form passes: the correspondences, the partial rows and the mask words, the call block
// by pointer or (call_by_value non-null) by value.  Everything else starts as zero.
MicpFastParams fast_params(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points, const float* model_normals,
                           const uint8_t* model_mask, uint32_t n, uint32_t nblocks, const double* partials, const unsigned long long* unc_mask,
                           const MicpCall* call, const MicpCallLite* call_by_value) {
  MicpFastParams p{};
  p.dataset_points = dataset_points; p.dataset_mask = dataset_mask;
  p.model_points = model_points; p.model_normals = model_normals; p.model_mask = model_mask;
  p.n = n; p.nblocks = nblocks;
  p.partials = const_cast<double*>(partials);
  p.unc_mask = const_cast<unsigned long long*>(unc_mask);
  p.call = call_by_value ? nullptr : call;
  if (call_by_value) p.cv = *call_by_value;
  return p;
}
// the rows and mask words a find with the moment epilogue left (launch_find_moments), and the area the fold hands over through
void rows_of_find(MicpFastParams& p, uint32_t W, uint32_t tiles_x, uint32_t tile_w_log2, uint32_t words_per_block, double* fold_rows,
                  uint32_t* fold_flags) {
  p.mask_tiled = 1u; p.mask_W = W; p.mask_tiles_x = tiles_x; p.mask_tile_w_log2 = tile_w_log2;
  p.mask_nwords = words_per_block * p.nblocks;
  p.fold_rows = fold_rows; p.fold_flags = fold_flags;
}
// workgroups of k_micp_fast_loop / k_micp_publish: one folds up to 255 rows alone (and whenever there is no hand-over area)
uint32_t micp_fold_blocks(const MicpFastParams& p) {
  return (p.fold_rows != nullptr && p.fold_flags != nullptr && p.nblocks >= 256u) ? kMicpFoldBlocks : 1u;
}
void launch_moments_pass(const MicpFastParams& p, hipStream_t s) { hipLaunchKernelGGL(k_micp_moments, dim3(p.nblocks), dim3(256), 0, s, p); }

__global__ void k_signal_flag(uint32_t* flag, uint32_t seq) {
  if (threadIdx.x == 0u && blockIdx.x == 0u) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace

hipError_t launch_micp_moments(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                               const float* model_normals, const uint8_t* model_mask, uint32_t n, const MicpCall* call,
                               double* partials, unsigned long long* unc_mask, hipStream_t s, const MicpCallLite* call_by_value) {
  launch_moments_pass(fast_params(dataset_points, dataset_mask, model_points, model_normals, model_mask, n, micp_fast_blocks(n), partials,
                                  unc_mask, call, call_by_value), s);
  return hipGetLastError();
}

hipError_t launch_signal_flag(uint32_t* flag, uint32_t seq, hipStream_t s) {
  hipLaunchKernelGGL(k_signal_flag, dim3(1), dim3(64), 0, s, flag, seq);
  return hipGetLastError();
}

hipError_t launch_micp_multi_fast_loop(const MicpMultiFastParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_micp_multi_fast_loop, dim3(1), dim3(kFastThreads), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_micp_fast(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                            const float* model_normals, const uint8_t* model_mask, uint32_t n, const MicpCall* call,
                            double* partials, unsigned long long* unc_mask, uint32_t n_iter, MicpState* state_out,
                            MicpFastStatus* status, unsigned long long* done, hipStream_t s, const MicpCallLite* call_by_value) {
  MicpFastParams p = fast_params(dataset_points, dataset_mask, model_points, model_normals, model_mask, n, micp_fast_blocks(n), partials,
                                 unc_mask, call, call_by_value);
  p.n_iter = n_iter; p.state_out = state_out; p.status = status; p.done = done;
  launch_moments_pass(p, s);
  hipLaunchKernelGGL(k_micp_fast_loop, dim3(1), dim3(kFastThreads), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_micp_fast_loop_tiled(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                                       const float* model_normals, const uint8_t* model_mask, uint32_t n, uint32_t nblocks,
                                       const double* partials, const unsigned long long* unc_mask, uint32_t W, uint32_t tiles_x,
                                       uint32_t tile_w_log2, uint32_t words_per_block, uint32_t n_iter, MicpState* state_out,
                                       MicpFastStatus* status, unsigned long long* done, hipStream_t s, const MicpCallLite& call_by_value,
                                       double* fold_rows, uint32_t* fold_flags) {
  MicpFastParams p = fast_params(dataset_points, dataset_mask, model_points, model_normals, model_mask, n, nblocks, partials, unc_mask,
                                 nullptr, &call_by_value);
  p.n_iter = n_iter; p.state_out = state_out; p.status = status; p.done = done;
  rows_of_find(p, W, tiles_x, tile_w_log2, words_per_block, fold_rows, fold_flags);
  hipLaunchKernelGGL(k_micp_fast_loop, dim3(micp_fold_blocks(p)), dim3(kFastThreads), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_micp_publish_tiled(const float* dataset_points, const float* model_points, const float* model_normals, uint32_t n,
                                     uint32_t nblocks, const double* partials, const unsigned long long* unc_mask, uint32_t W,
                                     uint32_t tiles_x, uint32_t tile_w_log2, uint32_t words_per_block, MicpHostBlock* host_block,
                                     unsigned long long* done, uint32_t seq, double* fold_rows, uint32_t* fold_flags, hipStream_t s) {
  MicpCallLite cv{};
  cv.seq = seq;
  MicpFastParams p = fast_params(dataset_points, nullptr, model_points, model_normals, nullptr, n, nblocks, partials, unc_mask, nullptr, &cv);
  p.done = done; p.host_block = host_block;
  rows_of_find(p, W, tiles_x, tile_w_log2, words_per_block, fold_rows, fold_flags);
  hipLaunchKernelGGL(k_micp_publish, dim3(micp_fold_blocks(p)), dim3(kFastThreads), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_micp_moments_publish(const float* dataset_points, const uint8_t* dataset_mask, const float* model_points,
                                       const float* model_normals, const uint8_t* model_mask, uint32_t n, double* partials,
                                       unsigned long long* unc_mask, const MicpCallLite& cv, MicpHostBlock* host_block,
                                       unsigned long long* done, hipStream_t s) {
  MicpFastParams p = fast_params(dataset_points, dataset_mask, model_points, model_normals, model_mask, n, micp_fast_blocks(n), partials,
                                 unc_mask, nullptr, &cv);
  p.done = done; p.host_block = host_block;
  launch_moments_pass(p, s);
  hipLaunchKernelGGL(k_micp_publish, dim3(1), dim3(kFastThreads), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_micp_multi_init(const MicpMultiCall* call, MicpMultiState* state, hipStream_t s) {
  hipLaunchKernelGGL(k_micp_multi_init, dim3(1), dim3(64), 0, s, call, state);
  return hipGetLastError();
}

hipError_t launch_micp_multi_step(const MicpMultiCall* call, MicpMultiState* state, hipStream_t s) {
  hipLaunchKernelGGL(k_micp_multi_step, dim3(1), dim3(64), 0, s, call, state);
  return hipGetLastError();
}

hipError_t launch_micp_init(MicpState* state, hipStream_t s) {
  hipLaunchKernelGGL(k_micp_init, dim3(1), dim3(64), 0, s, state);
  return hipGetLastError();
}

hipError_t launch_micp_close(const double* partials, uint32_t nblocks, const MicpCall* call, const MicpState* state,
                             MicpState* state_out, unsigned long long* done, hipStream_t s) {
  hipLaunchKernelGGL(k_micp_close, dim3(1), dim3(64), 0, s, partials, nblocks, call, state, state_out, done);
  return hipGetLastError();
}

hipError_t launch_debug_solve(const cstats* stats, uint32_t n, int fast, xform* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_debug_solve, dim3((n + 63u) / 64u), dim3(64), 0, s, stats, n, fast, out);
  return hipGetLastError();
}

}  // namespace rmclhip
