// robust.hip -- ROBUST MICP (include/rmclhip.h): M-estimator weights in the point-to-plane reduction (gfx950).
//
//   k_robust_hist<pass>      the scale: exact lower median of |r| over the gated-in correspondences by radix selection on the f32 bit
//                            pattern, three histogram passes (11 + 11 + 10 bits).  LDS histogram per workgroup, one global integer add
//                            per non-empty bin; wave 0 of every workgroup picks the previous pass's bucket in its prologue (same
//                            integers in every workgroup => the same bucket), so a selection is three launches + k_robust_scale_final
//   k_robust_partials        the weighted streaming reduction: grid, element-to-thread mapping and order of additions of
//                            k_reduce_partials (kernels.hip), every term times (double)w, + the count, sum w r^2, sum r^2
//   k_robust_finalize        one wave folds the rows in finalize_pose's order (reduce_common.hip.h) and divides by sum w
//   k_robust_iter, _close    the IRLS loop, one launch per iteration: the previous iteration's fold + solve in the prologue of the next
//                            reduction (the form of k_micp_iter / k_micp_close, micp.hip)
//   k_robust_rig_partials,   the rig: ONE streaming launch over all sensors -- a workgroup finds its sensor in the call
//   _step, _init, _close     block and is one of that sensor's own rows --, then one wave finalizes every sensor, merges with real
//                            weights (cs_merge_weighted, devmath.h), solves and hands out the next pre-transforms (k_micp_multi_step's shape)
//
// The weight itself is robust_weight() of robust_host.h, the one definition host and device share: f32, IEEE division, no fused
// operation (-ffp-contract=off, hipcc's correctly rounded f32 division) -- numpy float32 reproduces every weight bit for bit; keep it so.
// Integers decide the median: no floating-point atomics anywhere, the same inputs give the same bytes on every call.
#include "kernels.h"
#include "reduce_common.hip.h"
#include "robust_host.h"
#include "wave_sum.hip.h"

namespace rmclhip {

namespace {

constexpr int kRow = static_cast<int>(kRobustRow);
constexpr int kCnt = 16, kWrss = 17, kRss = 18;   // columns behind the 16 sums
constexpr uint32_t kNoKey = 0xFFFFFFFFu;          // masked or gated out (a gated-in |r| is finite: its pattern is at most 0x7F7FFFFF)

// r = spd of p2l_accumulate (reduce_common.hip.h) by the same f32 expressions, and whether the element is gated in
struct Residual { f3 Di, Ni; float r; bool in; };
__device__ __forceinline__ Residual robust_residual(const RobustView& v, const xform& Tpre, size_t i) {
  Residual e;
  e.in = false; e.r = 0.0f; e.Di = mk3(0.f, 0.f, 0.f); e.Ni = e.Di;
  const bool dok = (v.dataset_mask == nullptr) || (v.dataset_mask[i] > 0);
  if (dok && (v.model_mask == nullptr || v.model_mask[i] > 0)) {
    const float* dp = v.dataset_points + 3 * i;
    const float* mp = v.model_points + 3 * i;
    const float* mn = v.model_normals + 3 * i;
    e.Di = xapply(Tpre, mk3(dp[0], dp[1], dp[2]));
    e.Ni = mk3(mn[0], mn[1], mn[2]);
    e.r = dot_plain(sub3(mk3(mp[0], mp[1], mp[2]), e.Di), e.Ni);
    e.in = fabsf(e.r) < v.max_dist;   // false for NaN
  }
  return e;
}

// ---- scale -------------------------------------------------------------------------------------------------------------------------
// key = bit pattern of |r| (order-preserving as uint32 for non-negative finite floats; +0 and -0 share the key 0)
struct SelState { uint32_t prefix, rank, m, pad; };   // the selected digits so far | the rank inside that bucket | the gated-in count
constexpr uint32_t sel_bits(int pass) { return pass == 2 ? 10u : 11u; }
constexpr uint32_t sel_hist_off(int pass) { return pass == 0 ? 0u : (pass == 1 ? 2048u : 4096u); }
constexpr uint32_t kSelStateOff = 2048u + 2048u + 1024u;

// One wave: the bucket of hist[1 << bits] that holds rank in.rank of the keys counted there.  first: the counts are all gated-in keys --
// m and the median's rank (m - 1) / 2 come from their total.  Nothing counted: prefix and rank stay meaningless, m == 0 says so.
template <uint32_t kBits>
__device__ __forceinline__ SelState select_pick(const uint32_t* hist, SelState in, bool first, uint32_t lane) {
  constexpr uint32_t kPer = (1u << kBits) / 64u;   // consecutive bins per lane
  uint32_t h[kPer];
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t b = 0; b < kPer; ++b) { h[b] = hist[lane * kPer + b]; sum += h[b]; }
  uint32_t incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= static_cast<uint32_t>(off)) incl += t;
  }
  const uint32_t total = __shfl(incl, 63, 64);
  if (first) { in.prefix = 0u; in.m = total; in.rank = (total != 0u) ? (total - 1u) / 2u : 0u; }
  const uint32_t excl = incl - sum;
  const bool mine = in.rank >= excl && in.rank < incl;
  const unsigned long long who = __ballot(mine);
  SelState out = in;
  out.prefix = in.prefix << kBits;
  out.rank = 0u;
  if (who != 0ull) {
    uint32_t bin = 0, before = excl, found = 0;
#pragma unroll
    for (uint32_t b = 0; b < kPer; ++b) {
      if (!found && in.rank < before + h[b]) { bin = lane * kPer + b; found = 1u; }
      if (!found) before += h[b];
    }
    const int src = __builtin_ctzll(who);
    out.prefix |= __shfl(bin, src, 64);
    out.rank = in.rank - __shfl(before, src, 64);
  }
  return out;
}

// pass 0: bits 31..21 of every gated-in key; pass 1: bits 20..10 of the keys in pass 0's bucket; pass 2: bits 9..0 of those in pass 1's.
// kKeys: pass 0 writes every element's key (kNoKey where masked or gated out), the later passes read 4 bytes per element instead of 38.
template <int kPass, bool kKeys>
__global__ void __launch_bounds__(256) k_robust_hist(const RobustView v, const xform Tpre, uint32_t* __restrict__ sel,
                                                     uint32_t* __restrict__ keys) {
  __shared__ uint32_t s_h[2048];
  __shared__ SelState s_st;
  for (uint32_t b = threadIdx.x; b < 2048u; b += 256u) s_h[b] = 0u;
  if (kPass > 0 && threadIdx.x < 64u) {
    SelState in = {0u, 0u, 0u, 0u};
    SelState* states = reinterpret_cast<SelState*>(sel + kSelStateOff);
    if (kPass == 2) in = states[0];
    const SelState st = select_pick<sel_bits(kPass - 1)>(sel + sel_hist_off(kPass - 1), in, kPass == 1, threadIdx.x);
    if (threadIdx.x == 0u) {
      s_st = st;
      if (blockIdx.x == 0u) states[kPass - 1] = st;   // (pass 1 reads nothing of it; pass 2 and the final launch do, after the kernel boundary)
    }
  }
  __syncthreads();
  const uint32_t prefix = (kPass > 0) ? s_st.prefix : 0u;
  constexpr uint32_t kShift = kPass == 0 ? 21u : (kPass == 1 ? 10u : 0u);   // the digit's position
  constexpr uint32_t kMask = (1u << sel_bits(kPass)) - 1u;
  const size_t stride = static_cast<size_t>(gridDim.x) * 256u;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < v.n; i += stride) {
    uint32_t key;
    if (kKeys && kPass > 0) {
      key = keys[i];
    } else {
      const Residual e = robust_residual(v, Tpre, i);
      key = e.in ? __float_as_uint(fabsf(e.r)) : kNoKey;
      if (kKeys) keys[i] = key;
    }
    if (key != kNoKey && (kPass == 0 || (key >> (kShift + sel_bits(kPass))) == prefix)) atomicAdd(&s_h[(key >> kShift) & kMask], 1u);
  }
  __syncthreads();
  uint32_t* hist = sel + sel_hist_off(kPass);
  for (uint32_t b = threadIdx.x; b <= kMask; b += 256u) {
    const uint32_t c = s_h[b];
    if (c != 0u) atomicAdd(hist + b, c);
  }
}

__global__ void __launch_bounds__(64) k_robust_scale_final(const uint32_t* __restrict__ sel, const RobustScaleParams sp,
                                                           RobustScale* __restrict__ out, RobustScale* __restrict__ copy) {
  const SelState* states = reinterpret_cast<const SelState*>(sel + kSelStateOff);
  const SelState st = select_pick<sel_bits(2)>(sel + sel_hist_off(2), states[1], false, threadIdx.x);
  if (threadIdx.x == 0u) {
    RobustScale r;
    r.m = st.m;
    r.pad = 0u;
    const float median = (st.m != 0u) ? __uint_as_float(st.prefix) : 0.0f;
    if (sp.mode == RMCLHIP_ROBUST_SCALE_MAD) {
      r.median = median;
      r.c = (st.m != 0u) ? robust_mad_scale(sp.tuning, median, sp.scale_min) : sp.scale_min;
    } else {
      r.median = 0.0f;
      r.c = sp.scale;
    }
    *out = r;
    if (copy != nullptr) *copy = r;
  }
}

__global__ void k_robust_fixed_scale(float c, RobustScale* out) {
  if (threadIdx.x == 0u && blockIdx.x == 0u) {
    RobustScale r;
    r.c = c; r.median = 0.0f; r.m = 0u; r.pad = 0u;
    *out = r;
  }
}

// ---- weighted reduction ----------------------------------------------------------------------------------------------------------------
// p2l_accumulate with every term times wd = (double)w, in its order of additions; w == 1 adds the very values p2l_accumulate adds
__device__ __forceinline__ float robust_accumulate(const Residual& e, int kernel, float c, double* acc) {
  if (!e.in) return 0.0f;
  const float w = robust_weight(kernel, c, e.r);
  const double wd = static_cast<double>(w);
  const f3 Mi = add3(e.Di, scale3(e.Ni, e.r));
  const double d[3] = {e.Di.x, e.Di.y, e.Di.z}, m[3] = {Mi.x, Mi.y, Mi.z};
#pragma unroll
  for (int k = 0; k < 3; ++k) { acc[k] += wd * d[k]; acc[3 + k] += wd * m[k]; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) acc[6 + 3 * r + cc] += wd * (m[r] * d[cc]);
  acc[15] += wd;
  const double rd = static_cast<double>(e.r);
  acc[kCnt] += 1.0;               // an integer in a double: exact up to 2^53
  acc[kWrss] += wd * (rd * rd);
  acc[kRss] += rd * rd;
  return w;
}

// the thread's elements in k_reduce_partials' mapping, as workgroup `row` of `nrows` (a launch of its own: blockIdx.x of gridDim.x; a
// sensor's share of the rig's launch: its row of its nblocks -- the same elements in the same order either way)
__device__ __forceinline__ void robust_stream_rows(const RobustView& v, const xform& Tpre, float c, float* weights_out, double* acc,
                                                   uint32_t row, uint32_t nrows) {
#pragma unroll
  for (int k = 0; k < kRow; ++k) acc[k] = 0.0;
  // (64-bit index: the same elements in the same order as k_reduce_partials' 32-bit one, without its wrap for n within a stride of 2^32)
  const size_t stride = static_cast<size_t>(nrows) * 256u;
  for (size_t i = static_cast<size_t>(row) * 256u + threadIdx.x; i < v.n; i += stride) {
    const float w = robust_accumulate(robust_residual(v, Tpre, i), v.kernel, c, acc);
    if (weights_out != nullptr) weights_out[i] = w;
  }
}
__device__ __forceinline__ void robust_stream(const RobustView& v, const xform& Tpre, float c, float* weights_out, double* acc) {
  robust_stream_rows(v, Tpre, c, weights_out, acc, blockIdx.x, gridDim.x);
}

// the wave's sums of the row's two halves (the first half is k_reduce_partials' wave_sum16_lds call); lanes 0..15 hold them afterwards
__device__ __forceinline__ void robust_wave_row(const double* acc, double* scratch, uint32_t lane, double* red_row) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = acc[16 * h + k];
    const double wsum = wave_sum16_lds(t, scratch, lane);   // (one scratch for both halves: LDS operations of one wave complete in order)
    if (lane < 16u) red_row[16 * h + lane] = wsum;
  }
}

// sixteen columns of the rows folded in finalize_pose's order (reduce_common.hip.h) at this row width: lane k < 16 returns column col0 + k
__device__ __forceinline__ double robust_fold16(const double* partials, uint32_t nblocks, uint32_t col0) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k0 = col0 + (lane & 15u), g = lane >> 4;
  double a = 0.0;
  uint32_t b = g;
  for (; b + 124u < nblocks; b += 128u) {
    double t[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) t[u] = partials[static_cast<size_t>(b + 4u * u) * kRobustRow + k0];
#pragma unroll
    for (int u = 0; u < 32; u += 8) a += ((t[u] + t[u + 1]) + (t[u + 2] + t[u + 3])) + ((t[u + 4] + t[u + 5]) + (t[u + 6] + t[u + 7]));
  }
  for (; b + 28u < nblocks; b += 32u) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = partials[static_cast<size_t>(b + 4u * u) * kRobustRow + k0];
    a += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  }
  for (; b < nblocks; b += 4u) a += partials[static_cast<size_t>(b) * kRobustRow + k0];
  a += __shfl_xor(a, 16, 64);
  a += __shfl_xor(a, 32, 64);
  return a;
}

// finalize_pose with sum w in place of n (one wave): the same divisions in the same order, so weight 1 throughout gives its bytes
__device__ __forceinline__ RobustStats robust_finalize(const double* partials, uint32_t nblocks, const RobustScale sc) {
  const double a0 = robust_fold16(partials, nblocks, 0u);
  const double a1 = robust_fold16(partials, nblocks, 16u);
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = __shfl(a0, k, 64);
  const double count = __shfl(a1, 0, 64);
  RobustStats out;
  out.stats = cs_identity();
  out.weight_sum = acc[15];
  out.wrss = __shfl(a1, 1, 64);
  out.rss = __shfl(a1, 2, 64);
  out.scale = sc.c;
  out.median = sc.median;
  const double n = acc[15];
  if (n > 0.0) {
    const double md[3] = {acc[0] / n, acc[1] / n, acc[2] / n};
    const double mm[3] = {acc[3] / n, acc[4] / n, acc[5] / n};
    out.stats.dataset_mean = mk3(static_cast<float>(md[0]), static_cast<float>(md[1]), static_cast<float>(md[2]));
    out.stats.model_mean = mk3(static_cast<float>(mm[0]), static_cast<float>(mm[1]), static_cast<float>(mm[2]));
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) out.stats.covariance[3 * r + c] = static_cast<float>(acc[6 + 3 * r + c] / n - mm[r] * md[c]);
    if (count == 1.0)   // ONE correspondence has no covariance (finalize_pose)
      for (int k = 0; k < 9; ++k) out.stats.covariance[k] = 0.0f;
  }
  out.stats.n_meas = static_cast<uint32_t>(count);
  return out;
}

// an iteration's step: statistics whose weights sum to zero (every correspondence at or beyond TUKEY's c) say nothing and move nothing
__device__ __forceinline__ xform robust_advance(const RobustStats& st, const xform& T_s) {
  return (st.weight_sum > 0.0) ? xmul(T_s, umeyama(st.stats)) : T_s;
}

__global__ void __launch_bounds__(256) k_robust_partials(const RobustView v, const xform Tpre, const RobustScale* __restrict__ scale,
                                                         double* __restrict__ partials, float* __restrict__ weights_out) {
  __shared__ double red[4][kRow];
  __shared__ double s_wsum[4][64 * 17];
  double acc[kRow];
  robust_stream(v, Tpre, scale->c, weights_out, acc);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  robust_wave_row(acc, &s_wsum[wave][0], lane, &red[wave][0]);
  __syncthreads();
  if (threadIdx.x < kRobustRow) {
    const double t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    // write-through store, read by the next launch after the kernel boundary (as k_reduce_partials)
    __hip_atomic_store(partials + static_cast<size_t>(blockIdx.x) * kRobustRow + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(64) k_robust_finalize(const double* __restrict__ partials, uint32_t nblocks,
                                                        const RobustScale* __restrict__ scale, RobustStats* __restrict__ out) {
  const RobustStats st = robust_finalize(partials, nblocks, *scale);
  if (threadIdx.x == 0u) *out = st;
}

// One IRLS iteration per launch: wave 0 of EVERY workgroup first finishes the previous iteration -- folds its rows and solves,
// redundantly (same inputs, same order => the same pre-transform everywhere; workgroup 0 records it) -- then all stream the
// correspondences with that pre-transform.  Rows and state ping-pong so that no workgroup reads what another of the same launch writes.
__global__ void __launch_bounds__(256) k_robust_iter(const RobustView v, const RobustScale* __restrict__ scale, uint32_t nblocks,
                                                     const double* __restrict__ partials_prev, double* __restrict__ partials_out,
                                                     const xform* __restrict__ state_in, xform* __restrict__ state_out, uint32_t first) {
  __shared__ double red[4][kRow];
  __shared__ double s_wsum[4][64 * 17];
  __shared__ xform s_Tpre;
  const RobustScale sc = *scale;
  if (threadIdx.x < 64u) {
    if (first) {
      if (threadIdx.x == 0u) {
        s_Tpre = xidentity();
        if (blockIdx.x == 0u) *state_out = xidentity();
      }
    } else {
      const RobustStats st = robust_finalize(partials_prev, nblocks, sc);
      if (threadIdx.x == 0u) {
        const xform T_s = robust_advance(st, *state_in);
        s_Tpre = T_s;
        if (blockIdx.x == 0u) *state_out = T_s;
      }
    }
  }
  __syncthreads();
  const xform Tpre = s_Tpre;
  double acc[kRow];
  robust_stream(v, Tpre, sc.c, nullptr, acc);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  robust_wave_row(acc, &s_wsum[wave][0], lane, &red[wave][0]);
  __syncthreads();
  if (threadIdx.x < kRobustRow) {
    const double t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __hip_atomic_store(partials_out + static_cast<size_t>(blockIdx.x) * kRobustRow + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// closing launch: the last iteration's fold + solve, then the odometry-frame transform as micp_close_sensor (micp.hip) forms it; the
// statistics stay in the sensor frame
__global__ void __launch_bounds__(64) k_robust_close(const double* __restrict__ partials, uint32_t nblocks,
                                                     const RobustScale* __restrict__ scale, const xform* __restrict__ state, const xform Tsb,
                                                     const xform Tbo, RobustLoopOut* __restrict__ out) {
  const RobustStats st = robust_finalize(partials, nblocks, *scale);
  if (threadIdx.x == 0u) {
    const xform T_s = robust_advance(st, *state);
    const xform Tso = xmul(Tbo, Tsb);
    RobustLoopOut o;
    o.T_snew_sold = T_s;
    o.T_onew_oold = xmul(xmul(Tso, T_s), xinv(Tso));
    o.stats = st;
    *out = o;
  }
}

// ---- the rig: N sensors, one streaming launch and one step launch per iteration ----------------------------------------
// One launch covers every sensor: a workgroup finds its sensor in the call block's table (at most 8 entries, wave-uniform scalar loads from
// the kernel arguments) and is row blockIdx.x - block0 of that sensor's nblocks -- k_robust_partials' mapping and order of additions, so
// a sensor's rows are the rows it would have alone.  Pre-transform and scale come from device memory: the step launch before this one
// (or the init launch) wrote the one, the sensor's own selection behind its find the other.
__global__ void __launch_bounds__(256) k_robust_rig_partials(const RobustRigCall call, const RobustRigState* __restrict__ st) {
  __shared__ double red[4][kRow];
  __shared__ double s_wsum[4][64 * 17];
  uint32_t s = 0;
  for (uint32_t k = 1; k < call.n_sensors; ++k)
    if (blockIdx.x >= call.s[k].block0) s = k;
  const RobustRigSensor& me = call.s[s];
  const uint32_t row = blockIdx.x - me.block0;
  if (row >= me.nblocks) return;   // (never: the grid is the sum of the nblocks)
  const xform Tpre = st->T_snew_sold[s];
  double acc[kRow];
  robust_stream_rows(me.v, Tpre, me.scale->c, nullptr, acc, row, me.nblocks);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  robust_wave_row(acc, &s_wsum[wave][0], lane, &red[wave][0]);
  __syncthreads();
  if (threadIdx.x < kRobustRow) {
    const double t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    // write-through store, read by the step launch after the kernel boundary (as k_robust_partials)
    __hip_atomic_store(me.partials + static_cast<size_t>(row) * kRobustRow + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(64) k_robust_rig_init(RobustRigState* __restrict__ st) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  st->T_onew_oold = xidentity();
  st->merged_o = cs_identity();
  st->merged_weighted_o = cs_identity();
  st->merged_weight = 0.0;
  st->merged_weighted_weight = 0.0;
  for (uint32_t s = 0; s < kMaxMicpSensors; ++s) st->T_snew_sold[s] = xidentity();
}

// One iteration's merge and solve, ONE wave -- k_micp_multi_step (micp.hip) with real weights: per sensor, in order, stats_s <- its rows
// (robust_finalize); Cs_o = Tbo * (Tsb * stats_s); merged folds the Cs_o with sum w, merged_w with sum w * merge_weight_multiplier.
// The plain loop truncates n_meas * multiplier to an integer there (micp_localization.cpp:934, a count has to be one); a weight has
// not: NO truncation here.  T_onew_oold *= umeyama(merged_w) when merged_w has weight, else nothing moves; the next pre-transforms
// exactly as k_micp_multi_step forms them.
__global__ void __launch_bounds__(64) k_robust_rig_step(const RobustRigCall call, RobustRigState* __restrict__ st) {
  cstats merged = cs_identity(), merged_w = cs_identity();
  double W = 0.0, Ww = 0.0;
  for (uint32_t s = 0; s < call.n_sensors; ++s) {
    const RobustRigSensor& me = call.s[s];
    const RobustStats rs = robust_finalize(me.partials, me.nblocks, *me.scale);   // whole wave
    if (threadIdx.x == 0u) {
      st->stats_s[s] = rs;
      const cstats Cs_o = cs_transform(me.Tbo, cs_transform(me.Tsb, rs.stats));
      merged = cs_merge_weighted(merged, W, Cs_o, rs.weight_sum, &W);
      merged_w = cs_merge_weighted(merged_w, Ww, Cs_o, rs.weight_sum * me.weight, &Ww);
    }
  }
  if (threadIdx.x == 0u) {
    xform T_onew_oold = st->T_onew_oold;
    if (Ww > 0.0) T_onew_oold = xmul(T_onew_oold, umeyama(merged_w));
    st->T_onew_oold = T_onew_oold;
    st->merged_o = merged;
    st->merged_weighted_o = merged_w;
    st->merged_weight = W;
    st->merged_weighted_weight = Ww;
    for (uint32_t s = 0; s < call.n_sensors; ++s) {
      const xform T_bnew_bold = xmul(xmul(xinv(call.s[s].Tbo), T_onew_oold), call.s[s].Tbo);
      st->T_snew_sold[s] = xmul(xmul(xinv(call.s[s].Tsb), T_bnew_bold), call.s[s].Tsb);
    }
  }
}

// closing launch: the state's way to the caller (host-mapped memory: dword stores in address order, consecutive lanes consecutive words)
__global__ void __launch_bounds__(64) k_robust_rig_close(const RobustRigState* __restrict__ st, RobustRigState* __restrict__ out) {
  static_assert(sizeof(RobustRigState) % sizeof(uint32_t) == 0, "copied by words");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(st);
  uint32_t* dst = reinterpret_cast<uint32_t*>(out);
  for (uint32_t w = threadIdx.x; w < sizeof(RobustRigState) / sizeof(uint32_t); w += 64u) dst[w] = src[w];
}

}  // namespace

hipError_t launch_robust_scale(const RobustView& v, const xform& Tpre, const RobustScaleParams& sp, uint32_t* sel, uint32_t* keys,
                               RobustScale* scale_out, RobustScale* scale_copy, hipStream_t s) {
  if (const hipError_t e = hipMemsetAsync(sel, 0, kRobustSelWords * sizeof(uint32_t), s)) return e;
  const dim3 grid(reduce_num_blocks(v.n, 1)), block(256);
  if (keys != nullptr) {
    hipLaunchKernelGGL((k_robust_hist<0, true>), grid, block, 0, s, v, Tpre, sel, keys);
    hipLaunchKernelGGL((k_robust_hist<1, true>), grid, block, 0, s, v, Tpre, sel, keys);
    hipLaunchKernelGGL((k_robust_hist<2, true>), grid, block, 0, s, v, Tpre, sel, keys);
  } else {
    hipLaunchKernelGGL((k_robust_hist<0, false>), grid, block, 0, s, v, Tpre, sel, keys);
    hipLaunchKernelGGL((k_robust_hist<1, false>), grid, block, 0, s, v, Tpre, sel, keys);
    hipLaunchKernelGGL((k_robust_hist<2, false>), grid, block, 0, s, v, Tpre, sel, keys);
  }
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_robust_scale_final, dim3(1), dim3(64), 0, s, sel, sp, scale_out, scale_copy);
  return hipGetLastError();
}

hipError_t launch_robust_fixed_scale(float c, RobustScale* scale_out, hipStream_t s) {
  hipLaunchKernelGGL(k_robust_fixed_scale, dim3(1), dim3(64), 0, s, c, scale_out);
  return hipGetLastError();
}

hipError_t launch_robust_statistics(const RobustView& v, const xform& Tpre, const RobustScale* scale_dev, double* partials, uint32_t nblocks,
                                    float* weights_out, RobustStats* out, hipStream_t s) {
  hipLaunchKernelGGL(k_robust_partials, dim3(nblocks), dim3(256), 0, s, v, Tpre, scale_dev, partials, weights_out);
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_robust_finalize, dim3(1), dim3(64), 0, s, partials, nblocks, scale_dev, out);
  return hipGetLastError();
}

hipError_t launch_robust_loop(const RobustView& v, const RobustScale* scale_dev, double* partials, uint32_t nblocks, xform* state,
                              uint32_t n_iter, const xform& Tsb, const xform& Tbo, RobustLoopOut* out, hipStream_t s) {
  double* part[2] = {partials, partials + static_cast<size_t>(nblocks) * kRobustRow};
  for (uint32_t i = 0; i < n_iter; ++i) {
    hipLaunchKernelGGL(k_robust_iter, dim3(nblocks), dim3(256), 0, s, v, scale_dev, nblocks, part[(i + 1u) & 1u], part[i & 1u],
                       state + (i & 1u), state + ((i + 1u) & 1u), (i == 0u) ? 1u : 0u);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_robust_close, dim3(1), dim3(64), 0, s, part[(n_iter - 1u) & 1u], nblocks, scale_dev, state + (n_iter & 1u), Tsb, Tbo, out);
  return hipGetLastError();
}

hipError_t launch_robust_rig_loop(const RobustRigCall& call, RobustRigState* state, uint32_t n_iter, RobustRigState* out, hipStream_t s) {
  hipLaunchKernelGGL(k_robust_rig_init, dim3(1), dim3(64), 0, s, state);
  if (const hipError_t e = hipGetLastError()) return e;
  for (uint32_t i = 0; i < n_iter; ++i) {
    hipLaunchKernelGGL(k_robust_rig_partials, dim3(call.total_blocks), dim3(256), 0, s, call, state);
    hipLaunchKernelGGL(k_robust_rig_step, dim3(1), dim3(64), 0, s, call, state);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_robust_rig_close, dim3(1), dim3(64), 0, s, state, out);
  return hipGetLastError();
}

}  // namespace rmclhip
