// kernels.hip -- PRODUCTION kernels of librmclhip.so (gfx950, MI355X, CDNA4) for the RMCL / MICP-L hot path.
//
//  k_find            (find_kernel.hip.h) ray-casting correspondences, the kinds the product can select (find_kinds.h)
//  k_cpc_find        (traverse.hip.h) closest-point correspondences, CPCEmbree::find
//  k_reduce_partials rm::statistics_p2l (CorrespondencesCPU.cpp:26-30; gate MICPSensorCPU.cpp:70-84); its 16 sums, the wave that
//                    finishes them and the completion tag are in reduce_common.hip.h, shared with the MICP iterations
//                    (k_micp_*: micp.hip)
//  k_pf_update_v3   PCDSensorUpdater{Embree,Optix}::update, all beams fused
//                    (PCDSensorUpdaterEmbree.cpp:290-342, optix/BeamEvaluateProgram.cu:15-130)
//  k_pf_motion, k_pose_moments*: the rest of a filter cycle (the resamplers and the likelihood statistics: resample.hip)
//
// Experiments (rejected traversal kinds, probes, the round-2 particle-filter kernels) live in kernels_lab.hip and ship in
// librmclhip_lab.so; launch_find / launch_pf_update hand kinds they do not own to that library when it is loaded
// (lab_hooks.h), and report kLabMissing (kernels.h) otherwise.
#include <type_traits>

#include "find_kernel.hip.h"
#include "lab_hooks.h"
#include "pc2_load.hip.h"
#include "pf_common.hip.h"
#include "pf_random.hip.h"
#include "reduce_common.hip.h"
#include "surface.hip.h"
#include "wave_sum.hip.h"

namespace rmclhip {

namespace {

// Node16C twins (layout.h): thread = (node, entry)
__global__ void __launch_bounds__(256) k_build_cnodes16(const uint4* __restrict__ cn, uint32_t n_nodes, uint4* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t node = t >> 4, e = t & 15u, c = e >> 2, g = e & 3u;
  if (node >= n_nodes) return;
  const uint4 ca = cn[static_cast<size_t>(node) * 8u + 2u * c], cb = cn[static_cast<size_t>(node) * 8u + 2u * c + 1u];
  const uint4 far_a = uint4{__float_as_uint(kFarPoint[0]), __float_as_uint(kFarPoint[1]), __float_as_uint(kFarPoint[2]), __float_as_uint(kFarPoint[0])};
  const uint4 far_b = uint4{__float_as_uint(kFarPoint[1]), __float_as_uint(kFarPoint[2]), kLeafBit, 0u};
  uint4 oa = far_a, ob = far_b;
  const bool unused = __uint_as_float(ca.x) >= 1.0e29f;
  if (!unused) {
    if (cb.z & kLeafBit) {
      if (g == 0u) { oa = ca; ob = cb; }
    } else {
      oa = cn[static_cast<size_t>(cb.z) * 8u + 2u * g];
      ob = cn[static_cast<size_t>(cb.z) * 8u + 2u * g + 1u];
    }
  }
  out[static_cast<size_t>(node) * 32u + 2u * e] = oa;
  out[static_cast<size_t>(node) * 32u + 2u * e + 1u] = ob;
}

__global__ void k_compose_poses(const xform* __restrict__ Tbm, xform Tsb, xform* __restrict__ Tsm,
                                xform* __restrict__ Tms, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xform T = xmul(Tbm[i], Tsb);
  Tsm[i] = T;
  Tms[i] = xinv(T);
}

// one partial row of 16 sums per block and pose; k_reduce_finalize / k_batch_solve turn them into results in a launch of their own
// (a last-block tail fused into this kernel measured slower: profiles/r03_micp_loop_forms.txt)
__global__ void __launch_bounds__(256) k_reduce_partials(const ReduceParams p) {
  __shared__ double red[4][kAcc];
  __shared__ double s_wsum[4][64 * 17];
  const uint32_t pose = blockIdx.y;
  const xform Tpre = (p.Tpre_dev != nullptr) ? p.Tpre_dev[pose] : p.Tpre;
  const float max_dist = p.max_dist;
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  const size_t mbase = static_cast<size_t>(pose) * p.n;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < p.n; i += gridDim.x * 256u) {
    const bool dok = (p.dataset_mask == nullptr) || (p.dataset_mask[i] > 0);
    if (dok && (p.model_mask == nullptr || p.model_mask[mbase + i] > 0)) {   // (null: rmclhip_statistics_p2l on a view without a mask)
      const float* dp = p.dataset_points + 3 * static_cast<size_t>(i);
      const float* mp = p.model_points + 3 * (mbase + i);
      const float* mn = p.model_normals + 3 * (mbase + i);
      p2l_accumulate(Tpre, mk3(dp[0], dp[1], dp[2]), mk3(mp[0], mp[1], mp[2]), mk3(mn[0], mn[1], mn[2]), max_dist, acc);
    }
  }
  // wave64 reduction of the 16 moments through LDS (wave_sum16_lds: round 1 used a halving butterfly of 17 dependent
  // double shuffles, ~3.4k clocks for the last wave of a block; the transposed sum has no dependent round trips)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  {
    const double wsum = wave_sum16_lds(acc, &s_wsum[wave][0], lane);
    if (lane < 16u) red[wave][lane] = wsum;
  }
  __syncthreads();
  if (threadIdx.x < kAcc) {
    const double v = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    // agent-scope relaxed store = write-through (sc1) 8-B store (MI355X_MICROARCH.md, hand-off forms); the finalize
    // launch reads the rows after the kernel boundary
    __hip_atomic_store(p.partials + (static_cast<size_t>(pose) * p.nblocks + blockIdx.x) * kAcc + threadIdx.x, v,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(64) k_reduce_finalize(const double* __restrict__ partials, uint32_t nblocks,
                                                       cstats* __restrict__ out, unsigned long long* done, uint32_t seq) {
  const uint32_t pose = blockIdx.x;
  const cstats s = finalize_pose(partials + static_cast<size_t>(pose) * nblocks * kAcc, nblocks);
  if (threadIdx.x == 0) {
    out[pose] = s;
    if (done) publish_tag(done, seq, xor_words(s));   // single-pose call with a host-mapped result (capi_rcc.cpp wait_done)
  }
}

// stale v1 corrector (lidar_corrector_embree_benchmark.cpp:127-135): per pose, Tdelta_b = Tsb * T_s * ~Tsb
__global__ void __launch_bounds__(64) k_batch_solve(const double* __restrict__ partials, uint32_t nblocks, xform Tsb,
                                                    xform* __restrict__ Tdelta, cstats* __restrict__ stats) {
  const uint32_t pose = blockIdx.x;
  const cstats s = finalize_pose(partials + static_cast<size_t>(pose) * nblocks * kAcc, nblocks);
  if (threadIdx.x == 0) {
    const xform Ts = umeyama(s);
    Tdelta[pose] = xmul(xmul(Tsb, Ts), xinv(Tsb));
    if (stats) stats[pose] = s;
  }
}

// MICPSphericalSensorCPU::unpackMessage / MICPO1DnSensorCPU::unpackMessage (dataset construction)
__global__ void k_dataset_from_ranges(const float* __restrict__ ranges, const float* __restrict__ tab, uint32_t kind,
                                      uint32_t W, uint32_t H, f3 orig, float fx, float fy, float cx, float cy,
                                      float rmin, float rmax, float* __restrict__ points,
                                      uint8_t* __restrict__ mask, uint32_t* __restrict__ n_valid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t vid = i / W, hid = i - vid * W;
  const float r = ranges[i];
  f3 dir, o = orig;
  if (kind == kModelSpherical) {
    const float cp = tab[vid], sp = tab[H + vid], ct = tab[2u * H + hid], st = tab[2u * H + W + hid];
    dir = mk3(cp * ct, cp * st, sp);
  } else if (kind == kModelPinhole) {
    dir = pinhole_direction(fx, fy, cx, cy, vid, hid);
  } else if (kind == kModelOnDn) {
    o = mk3(tab[3u * i], tab[3u * i + 1u], tab[3u * i + 2u]);
    const float* dr = tab + 3u * (static_cast<size_t>(W) * H + i);
    dir = mk3(dr[0], dr[1], dr[2]);
  } else {
    dir = mk3(tab[3u * i], tab[3u * i + 1u], tab[3u * i + 2u]);
  }
  // unpackMessage: spherical adds no origin (MICPSphericalSensorCPU.cpp:218), the others do (MICPO1DnSensorCPU.cpp:211-213)
  f3 pt = scale3(dir, r);
  if (kind != kModelSpherical) pt = add3(pt, o);
  points[3u * i] = pt.x; points[3u * i + 1u] = pt.y; points[3u * i + 2u] = pt.z;
  const bool out_of_range = (r < rmin) || (r > rmax);
  mask[i] = out_of_range ? 0 : 1;
  if (!out_of_range) atomicAdd(n_valid, 1u);
}

// sensor_msgs/PointCloud2 bytes -> O1Dn model (dirs) + dataset (points, mask) in one pass:
// estimateModelAndData (conversions.cpp:869-1002) + filter (scan_operations.cpp:41-116) + MICPO1DnSensorCPU::unpackMessage
struct Pc2Params {
  const uint8_t* data;
  uint32_t point_step, row_step, off_x, off_y, off_z, is_f64;
  uint32_t h_skip, h_inc, w_skip, w_inc;
  uint32_t out_w, out_h;
  float range_min, range_max;
  float* dirs;
  float* points;
  uint8_t* mask;
  uint32_t* n_valid;
};

__global__ void __launch_bounds__(256) k_pointcloud2_unpack(const Pc2Params p) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= p.out_w * p.out_h) return;
  const uint32_t ti = id / p.out_w, tj = id - ti * p.out_w;
  const size_t si = static_cast<size_t>(ti) * p.h_inc + p.h_skip, sj = static_cast<size_t>(tj) * p.w_inc + p.w_skip;
  const uint8_t* ptr = p.data + si * p.row_step + sj * p.point_step;
  const float x = pc2_load(ptr + p.off_x, p.is_f64), y = pc2_load(ptr + p.off_y, p.is_f64), z = pc2_load(ptr + p.off_z, p.is_f64);
  const bool fin = (fabsf(x) <= 3.402823466e38f) && (fabsf(y) <= 3.402823466e38f) && (fabsf(z) <= 3.402823466e38f);
  float range = 0.0f;
  f3 d = mk3(0.f, 0.f, 0.f);
  if (fin) {
    range = sqrtf((x * x + y * y) + z * z);
    d = mk3(x / range, y / range, z / range);
  }
  p.dirs[3u * id] = d.x; p.dirs[3u * id + 1u] = d.y; p.dirs[3u * id + 2u] = d.z;
  p.points[3u * id] = d.x * range + 0.0f; p.points[3u * id + 1u] = d.y * range + 0.0f; p.points[3u * id + 2u] = d.z * range + 0.0f;
  const bool out_of_range = (range < p.range_min) || (range > p.range_max);
  p.mask[id] = out_of_range ? 0 : 1;
  if (!out_of_range) atomicAdd(p.n_valid, 1u);
}

// ---------------------------------------------------------------------------------------------
// Round 3 form of the persistent-lane kernel (the default).  tools/pfsim.py -- a wave-level model of this schedule on the
// product's own BVH arrays that reproduces the round-2 PMC figures (2.0 ms, ~60 % of the lanes active) -- says the kernel is
// bound by VALU instruction ISSUES, and that what moves the issue count is (a) shorter leaves, (b) what the refill block and
// the merge tail cost, not how many lanes sit in each issue:
//   * the filter's OWN tree (bvh_build.h): leaves of <= 2 records, same record array; a leaf visit is ONE round trip for
//     both records (leaf_pair) instead of a loop over up to four;
//   * the refill block only derives the point-to-plane ERROR of a finished beam; the double-precision exp / divide of the
//     likelihood runs afterwards as a dense pass over the block's beams (every lane busy) -- same operations, same result;
//   * the in-order Gaussian1D merge (one lane per particle, sequential by the reference's semantics) no longer divides:
//     the count sequence of a particle is known up front (n0 + k, clamped), so the two weights of every (particle, beam) are
//     computed by all lanes into the LDS the traversal stacks have just vacated, and the chain is ~14 dependent flops;
//   * ray set-up takes v_rcp_f32 for the slab reciprocals (the slab test is free-form and conservative: boxes are padded
//     1000 x wider than the reciprocal's error).
// Results are those of k_pf_update / k_pf_update_persist bit for bit (tests/test_gpu_pf.py runs all of them).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float fast_inv(float d) {
  const float ad = fabsf(d);
  const float s = (ad < 1e-30f) ? copysignf(1e-30f, d) : d;
  return __builtin_amdgcn_rcpf(s);
}

// a leaf of the filter's tree (<= kPfLeafTris = 2 records) in one memory round trip; a lane whose leaf holds one record
// re-tests it (a repeated test cannot change (best_t, best_rec))
__device__ __forceinline__ void leaf_pair(const uint32_t* __restrict__ tris, uint32_t cur, f3 O, f3 D, float ray_tfar,
                                          float& best_t, uint32_t& best_rec) {
  const uint32_t first = cur & 0x0FFFFFFFu;
  const bool two = ((cur >> 28) & 7u) != 0u;
  const uint32_t second = first + (two ? 1u : 0u);
  const uint4* t0 = reinterpret_cast<const uint4*>(tris) + static_cast<size_t>(first) * 4u;
  const uint4* t1 = reinterpret_cast<const uint4*>(tris) + static_cast<size_t>(second) * 4u;
  const uint4 a0 = t0[0], b0 = t0[1], c0 = t0[2];
  const uint4 a1 = t1[0], b1 = t1[1], c1 = t1[2];
  tri_update(a0, b0, c0, first, tris, O, D, ray_tfar, best_t, best_rec);
  if (__any(two)) tri_update(a1, b1, c1, second, tris, O, D, ray_tfar, best_t, best_rec);
}

// ---------------------------------------------------------------------------------------------
// Round 5: ORDER-INDEPENDENT likelihood accumulation (kAccum).  The reference merges a particle's beams one by one,
//   likelihood += Gaussian1D{eval, 0, 1};  n_meas = min(n_meas, MAX_N_MEAS)             (PCDSensorUpdaterEmbree.cpp:232-238)
// which is a linear recurrence with weights that depend on the COUNTS alone: with S = sigma + mean^2,
//   mean' = w1 mean + w2 e,   S' = w1 S + w2 e^2,   w1 = a / (a + 1),  w2 = 1 / (a + 1),  a = the count before the beam.
// So   mean_K = P0 mean_0 + sum_k W_k e_k,   S_K = P0 S_0 + sum_k W_k e_k^2,   W_k = w2_k prod_{j > k} w1_j,  P0 = prod_j w1_j,
// and the counts are a_k = min(n0 + k, MAX) (a_0 = n0 whatever it is): W_k is the SAME for every beam merged before the clamp
// (g^(K - Kc) / (n0 + Kc), Kc = min(MAX - n0, K), g = MAX / (MAX + 1)) and g^(K - 1 - k) / (MAX + 1) for the beams after it.
// Rounds 3 / 4 kept every beam's error (LDS, then 100 MB of global scratch written and read back) for a dense pass and ONE lane per
// particle walking the chain.  Here a finished ray adds W_k e and W_k e^2 straight into its particle's accumulators and is forgotten.
// The sums must not depend on the order the rays finish in (results are compared bit for bit across schedules, shards and runs):
// the accumulators are FIXED-POINT -- per quantity a row of 64-bit integers, one per 16 binades ("bin"), a term t = m 2^e going to
// bin (e - e_min) / 16 as m shifted so that the bin's top is 2^48 units: integer adds commute, a term keeps >= 32 significant bits
// (the eval is a float: 24), 2^16 terms fit.  Final value = the bins added in ascending order in double.
// Differences to the sequential float chain: ~1e-7 relative (its own rounding).  sigma = max(S - mean^2, 0): every term keeps >= 32
// significant bits (rounded to nearest into its bin, so the error has no sign), hence S and mean^2 each carry ~2^-33 relative and a
// variance below ~1e-10 mean^2 is noise of either sign -- clamped at 0, which is what the reference's chain of non-negative terms
// (P1 + P2 >= 0 in Gaussian1D::operator+=) can reach at the least (the unclamped difference went negative for particles
// whose beams all evaluate alike, and a downstream sqrt(sigma) would have been NaN).  n_meas is the closed form as before, bit-exact.
// ---------------------------------------------------------------------------------------------
// exp(arg) * inv_den for arg <= 0 in float arithmetic: arg log2(e) split Cody-Waite style into an integer n and a residual r in
// [-0.5, 0.5] (one fused multiply-add against each half of log2 e: |error of r| ~ 1e-8), 2^r by v_exp_f32 (1 ulp), the scale before
// the exponent so that results below 2^-126 round like any other denormal.  Below 2^-149 the result is 0.  A NaN argument gives 0, not
// NaN (fmaxf is maxnum): NaN penalty parameters are rejected by rmclhip_pf_set_params, and a NaN geometric error (maps
// beyond float32's products: chain200, chain2000, nested200) is caught by the caller before the value is used.
__device__ __forceinline__ float pf_eval_fast(float arg, float inv_den) {
  const float kL2eHi = 1.44269502162933349609375f, kL2eLo = 1.925963033500011e-08f;
  const float n = fmaxf(rintf(arg * kL2eHi), -400.0f);
  float r = fmaf(arg, kL2eHi, -n);
  r = fmaf(arg, kL2eLo, r);
  return ldexpf(__builtin_amdgcn_exp2f(fmaxf(r, -2.0f)) * inv_den, static_cast<int>(n));
}

constexpr int kAccBins1 = 18, kAccEmin1 = -256;   // sum W e:   terms in [2^-256, 2^32): evals up to 4e9, i.e. dist_sigma down to 1e-10
constexpr int kAccBins2 = 30, kAccEmin2 = -416;   // sum W e^2: terms in [2^-416, 2^64)
constexpr int kAccWords = kAccBins1 + kAccBins2;  // 64-bit words per particle

// returns false when t lies above the row's range (the caller poisons the particle: NaN, as an infinite term would make the chain)
__device__ __forceinline__ bool acc_add(unsigned long long* row, int nbins, int e_min, double t) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(t));
  const int e = static_cast<int>((b >> 52) & 0x7FFull) - 1023;   // floor(log2 t) of a positive normal double
  const int j = (e - e_min) >> 4;
  if (j < 0) return true;                                         // below 2^e_min: cannot reach a float result
  if (j >= nbins) return false;
  const int shift = 4 + (e_min + 16 * (j + 1) - e);               // 5..20: the bin's top 2^E is 2^48 units
  const unsigned long long mant = (b & 0xFFFFFFFFFFFFFull) | (1ull << 52);
  atomicAdd(row + j, (mant + (1ull << (shift - 1))) >> shift);   // round to nearest: truncation biased every sum downwards
  return true;
}
__device__ __forceinline__ double acc_value(const unsigned long long* row, int nbins, int e_min) {
  double v = 0.0;
  for (int j = 0; j < nbins; ++j) v += ldexp(static_cast<double>(row[j]), e_min + 16 * (j + 1) - 48);
  return v;
}

template <int kRows, bool kLeaf2, bool kSlotOrder = false, bool kAccum = false>
// (kAccum: 72 instead of 78 registers = 7 instead of 6 waves per SIMD, which is also what the LDS admits: the C5 shard -5 %, room-100k -2 %,
//  sphere-100k unchanged -- profiles/r05_pf_forms_ab.txt; the stored forms keep the 6 they were measured with)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kAccum ? 7 : 6, kAccum ? 7 : 6))) k_pf_update_v3(const PfParams p) {
  // LDS: [ per-lane stacks kRows*256 (later: merge weights) | Tsm (PB xforms) | n0 (PB) | errors -> evals (PB*n_beams floats) ]
  // (round 4 A/B, removed: the top 85 / 341 nodes of the tree in LDS -- the TD / TA units read 94 % / 82 % busy, but those are
  // "non-idle" counters, not bandwidth: 14 % / 33 % SLOWER, profiles/r04_pf_lds_top.txt.  The kernel is VALU-issue bound at the
  // per-class issue costs of profiles/r04_valu_issue_rate.txt: DESIGN.md, particle filter.)
  extern __shared__ uint32_t lds_dyn[];
  __shared__ uint32_t s_next;
  uint32_t* lds_col = lds_dyn + threadIdx.x;   // stack rows of this lane: row r at lds_col[r * 256], row 0 = sentinel
  xform* s_Tsm = reinterpret_cast<xform*>(lds_dyn + kRows * 256);
  uint32_t* s_n0 = reinterpret_cast<uint32_t*>(s_Tsm + p.particles_per_block);

  const uint32_t PB = p.particles_per_block;
  const uint32_t p0 = blockIdx.x * PB;
  if (p0 >= p.n_particles) return;
  // the workgroup's beam errors: LDS behind n0 (rounds 3), or its slice of the global scratch (round 4: see PfParams::evals)
  const bool evals_global = p.evals != nullptr;
  float* s_eval = evals_global ? (p.evals + static_cast<size_t>(p0) * p.n_beams) : reinterpret_cast<float*>(s_n0 + p.particles_per_block);
  const uint32_t np = min(PB, p.n_particles - p0);
  pattrs* attrs = reinterpret_cast<pattrs*>(p.attrs);
  // kAccum: behind n0 (8-byte aligned) per particle { W of an unclamped beam (double) | first clamped beam | poison } and the bins
  // (the dynamic segment starts behind the 4 bytes of s_next: 8-byte alignment is taken from the ADDRESS, not from the offset -- 64-bit LDS
  // atomics fault on a misaligned word; the launcher reserves the dword this may skip)
  const uint32_t acc_dw = kRows * 256u + 8u * PB + PB;
  double* s_wu = reinterpret_cast<double*>(lds_dyn + acc_dw + (((static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_dyn)) >> 2) + acc_dw) & 1u));
  uint32_t* s_kc = reinterpret_cast<uint32_t*>(s_wu + PB);
  uint32_t* s_bad = s_kc + PB;
  unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(s_bad + PB);
  // slot j of the block = particle `mine` (identity, or the caller's spatial order)
  const uint32_t mine_p = (threadIdx.x < np) ? (p.order ? p.order[p0 + threadIdx.x] : p0 + threadIdx.x) : 0u;
  if (threadIdx.x < np) {
    s_Tsm[threadIdx.x] = xmul(p.poses[mine_p], p.Tsb);
    const uint32_t n0 = attrs[mine_p].likelihood.n_meas;
    s_n0[threadIdx.x] = n0;
    if (kAccum) {
      const uint32_t K = p.n_beams;
      // beams 0 .. kc-1 are merged before the count clamps (n0 >= MAX: beam 0 alone, with a = n0)
      const uint32_t kc = (n0 < p.max_n_meas) ? min(p.max_n_meas - n0, K) : 1u;
      s_wu[threadIdx.x] = p.gpow[K - kc] / (static_cast<double>(n0) + static_cast<double>(kc));
      s_kc[threadIdx.x] = kc;
      s_bad[threadIdx.x] = 0u;
    }
  }
  if (kAccum)
    for (uint32_t i = threadIdx.x; i < np * static_cast<uint32_t>(kAccWords); i += 256u) s_acc[i] = 0ull;
  if (threadIdx.x == 0) s_next = 0u;
  __syncthreads();

  const float sq = p.dist_sigma * p.dist_sigma;
  const float inv_den_f = static_cast<float>(1.0 / sqrt(static_cast<double>(2 * sq) * 3.14159265358979323846));
  const uint32_t nrays = np * p.n_beams;
  const uint32_t np_magic = (np == 1u) ? 0u : static_cast<uint32_t>(0x100000000ull / np) + 1u;   // ray / np (particle-minor order)
  const uint32_t lane = threadIdx.x & 63u;
  constexpr uint32_t kDone = 0x7FFFFFFFu;
  // per-lane ray state
  uint32_t rr = 0;
  bool has_ray = false, exhausted = false;
  f3 O = mk3(0.f, 0.f, 0.f), D = O;
  RaySlab rs = make_ray_slab(O, mk3(1.f, 1.f, 1.f));
  float range = 0.f, best_t = 0.f;
  uint32_t best_rec = kNone;
  uint32_t rev_mask = 0u;   // kSlotOrder: bit a = the ray runs towards negative `a`
  uint32_t priv[(kRows < 65) ? (65 - kRows) : 1];
  lds_col[0] = kDone;
  uint32_t sp = 1, cur = kDone;
#define RMCL_ROW_ST(r, v) { if ((r) < static_cast<uint32_t>(kRows)) lds_col[(r) * kBfStride] = (v); else priv[(r) - kRows] = (v); }
#define RMCL_ROW_LD(r) (((r) < static_cast<uint32_t>(kRows)) ? lds_col[(r) * kBfStride] : priv[(r) - kRows])
  for (;;) {
    const bool idle = (cur == kDone) && !exhausted;
    const uint64_t want = __ballot(idle);
    const uint64_t busy = __ballot(cur != kDone);
    if (want == 0 && busy == 0) break;
    if (want != 0 && (busy == 0 || static_cast<uint32_t>(__popcll(want)) >= p.refill_thr)) {
      if (idle && has_ray) {
        // evaluate_rcc (PCDSensorUpdaterEmbree.cpp:18-86) with unit face normals (BeamEvaluateProgram.cu:104-113): the error only
        const bool real_hit = (range >= p.range_min) && (range <= p.range_max);
        const bool sim_hit = (best_rec != kNone) && (!p.sim_min_range || best_t > p.range_min);
        float error;
        if (sim_hit) {
          if (real_hit) {
            const f3 n = pf_error_normal(p.tris, best_rec, p.raw_ng);
            const f3 preal = add3(O, scale3(D, range));
            const f3 pint = add3(O, scale3(D, best_t));
            error = fabsf(dot_plain(sub3(pint, preal), n));
          } else {
            error = p.rmsh;
          }
        } else {
          error = real_hit ? p.rhsm : p.rmsm;
        }
        if (kAccum) {
          const uint32_t pi = (p.n_beams == 1u) ? rr : __umulhi(rr, p.nb_magic), k = rr - pi * p.n_beams;
          if (p.errors) p.errors[static_cast<size_t>(p.order ? p.order[p0 + pi] : (p0 + pi)) * p.n_beams + k] = error;
          // PCDSensorUpdaterEmbree.cpp:224 evaluates exp(-e^2 / sigma^2 / 2) / sqrt(2 sigma^2 pi) with a float argument, double exp /
          // sqrt and a float result; here the same float argument through pf_eval_fast: <= 2e-7 relative from that value
          const float arg = -(error * error) / sq / 2;
          const float ev = pf_eval_fast(arg, inv_den_f);
          const double e1 = static_cast<double>(ev);
          const double w = (k < s_kc[pi]) ? s_wu[pi] : p.gpow[p.n_beams - 1u - k] * p.inv_max1;
          unsigned long long* row = s_acc + pi * static_cast<uint32_t>(kAccWords);
          // (a NaN error -- a geometric one: t = inf against a unit normal of 0 where the intersector's products leave float32, at 1e16 m
          //  on chain200 -- must poison the particle as exp(NaN) poisons the reference's chain; pf_eval_fast turns it into 0)
          bool ok = (error == error) && e1 < __builtin_inf();   // false for NaN and +inf
          if (ok && e1 > 0.0) {
            const double t1 = w * e1;
            ok = acc_add(row, kAccBins1, kAccEmin1, t1) && acc_add(row + kAccBins1, kAccBins2, kAccEmin2, t1 * e1);
          }
          if (!ok) atomicOr(&s_bad[pi], 1u);
        } else {
          s_eval[rr] = error;
        }
        has_ray = false;
      }
      // next rays for the idle lanes: one LDS atomic per wave and refill
      const uint32_t nwant = static_cast<uint32_t>(__popcll(want));
      const int leader = __builtin_ctzll(want);
      uint32_t base = 0;
      if (static_cast<int>(lane) == leader) base = atomicAdd(&s_next, nwant);
      base = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(base), leader));
      if (idle) {
        const uint32_t mine = base + static_cast<uint32_t>(__popcll(want & ((1ull << lane) - 1ull)));
        if (mine < nrays) {
          // (n_beams == 1: floor(2^32 / 1) + 1 does not fit the 32-bit magic -- every ray is its own particle)
          uint32_t pi, b;
          if (p.particle_minor) { b = (np == 1u) ? mine : __umulhi(mine, np_magic); pi = mine - b * np; }
          else { pi = (p.n_beams == 1u) ? mine : __umulhi(mine, p.nb_magic); b = mine - pi * p.n_beams; }
          rr = pi * p.n_beams + b;     // the beam's slot in s_eval (particle-major whatever the dealing order)
          const xform Tsm = s_Tsm[pi];
          const float* bm = p.beams + 16u * b;
          // meas_m = Tsm * meas_s (RangeMeasurement.hpp:28-42)
          D = qrot(Tsm.R, mk3(bm[3], bm[4], bm[5]));
          O = p.beams_at_origin ? Tsm.t : xapply(Tsm, mk3(bm[0], bm[1], bm[2]));
          range = bm[6];
          rs.inv = mk3(fast_inv(D.x), fast_inv(D.y), fast_inv(D.z));
          rs.noi = mk3(-(O.x * rs.inv.x), -(O.y * rs.inv.y), -(O.z * rs.inv.z));
          if (kSlotOrder) rev_mask = (D.x < 0.0f ? 1u : 0u) | (D.y < 0.0f ? 2u : 0u) | (D.z < 0.0f ? 4u : 0u);
          best_t = p.ray_tfar;
          best_rec = kNone;
          sp = 1;
          has_ray = true;
          const bool finite = (D.x == D.x) && (D.y == D.y) && (D.z == D.z);
          cur = finite ? 0u : kDone;  // a non-finite beam is a miss: evaluated at the next refill
        } else {
          exhausted = true;
        }
      }
    }
    // phase 1: inner nodes -- left early once at most kTailLanes lanes are still descending while others hold a leaf
    for (;;) {
      const bool inner = (cur != kDone) && !(cur & kLeafBit);
      const uint64_t m_inner = __ballot(inner);
      if (m_inner == 0) break;
      if (static_cast<uint32_t>(__popcll(m_inner)) <= p.tail_lanes && __ballot((cur != kDone) && (cur & kLeafBit)) != 0) break;
      if (inner && kSlotOrder) {
        // children in the ray's slot order (node_hits_q4_so): the first one hit is entered, the later ones wait on the stack, nearest
        // on top; three unconditional stores as in the sorted form
        bool hit[4];
        uint32_t ref[4];
        if (!__any(sp + 3u > static_cast<uint32_t>(kRows))) {
          const uint32_t top = lds_col[(sp - 1u) * kBfStride];
          node_hits_q_so(p.qnodes, cur, rs, best_t, rev_mask, hit, ref);
          const bool h01 = hit[0] || hit[1], h012 = h01 || hit[2];
          lds_col[sp * kBfStride] = ref[3]; sp += (hit[3] && h012) ? 1u : 0u;
          lds_col[sp * kBfStride] = ref[2]; sp += (hit[2] && h01) ? 1u : 0u;
          lds_col[sp * kBfStride] = ref[1]; sp += (hit[1] && hit[0]) ? 1u : 0u;
          const bool any = h012 || hit[3];
          cur = hit[0] ? ref[0] : (hit[1] ? ref[1] : (hit[2] ? ref[2] : (hit[3] ? ref[3] : top)));
          sp = any ? sp : (sp - 1u);
        } else {
          node_hits_q_so(p.qnodes, cur, rs, best_t, rev_mask, hit, ref);
          const bool h01 = hit[0] || hit[1], h012 = h01 || hit[2];
          if (hit[3] && h012) { RMCL_ROW_ST(sp, ref[3]) ++sp; }
          if (hit[2] && h01) { RMCL_ROW_ST(sp, ref[2]) ++sp; }
          if (hit[1] && hit[0]) { RMCL_ROW_ST(sp, ref[1]) ++sp; }
          if (h012 || hit[3]) cur = hit[0] ? ref[0] : (hit[1] ? ref[1] : (hit[2] ? ref[2] : ref[3]));
          else { --sp; cur = RMCL_ROW_LD(sp); }
        }
      } else if (inner) {
        uint32_t key[4], ref[4];
        if (!__any(sp + 3u > static_cast<uint32_t>(kRows))) {
          const uint32_t top = lds_col[(sp - 1u) * kBfStride];
          node_keys_q(p.qnodes, cur, rs, best_t, key, ref);
          RMCL_CSWAP(0, 1) RMCL_CSWAP(2, 3) RMCL_CSWAP(0, 2) RMCL_CSWAP(1, 3) RMCL_CSWAP(1, 2)
          lds_col[sp * kBfStride] = ref[3]; sp += (key[3] != kNone) ? 1u : 0u;
          lds_col[sp * kBfStride] = ref[2]; sp += (key[2] != kNone) ? 1u : 0u;
          lds_col[sp * kBfStride] = ref[1]; sp += (key[1] != kNone) ? 1u : 0u;
          const bool any = key[0] != kNone;
          cur = any ? ref[0] : top;
          sp = any ? sp : (sp - 1u);
        } else {
          node_keys_q(p.qnodes, cur, rs, best_t, key, ref);
          RMCL_CSWAP(0, 1) RMCL_CSWAP(2, 3) RMCL_CSWAP(0, 2) RMCL_CSWAP(1, 3) RMCL_CSWAP(1, 2)
          if (key[3] != kNone) { RMCL_ROW_ST(sp, ref[3]) ++sp; }
          if (key[2] != kNone) { RMCL_ROW_ST(sp, ref[2]) ++sp; }
          if (key[1] != kNone) { RMCL_ROW_ST(sp, ref[1]) ++sp; }
          if (key[0] != kNone) cur = ref[0];
          else { --sp; cur = RMCL_ROW_LD(sp); }
        }
      }
    }
    // phase 2: this lane's leaf (if any); tfar = infinity
    if ((cur != kDone) && (cur & kLeafBit)) {
      if (kLeaf2) leaf_pair(p.tris, cur, O, D, p.ray_tfar, best_t, best_rec);
      else leaf_loop(p.tris, cur, O, D, p.ray_tfar, best_t, best_rec);
      --sp;
      cur = RMCL_ROW_LD(sp);
    }
  }
#undef RMCL_ROW_ST
#undef RMCL_ROW_LD
  __syncthreads();  // every beam of the block has its error in s_eval; the stack rows are free from here on

  const double den = sqrt(static_cast<double>(2 * sq) * 3.14159265358979323846);
  float* s_w = reinterpret_cast<float*>(lds_dyn);
  g1d L = {0.f, 0.f, 0u};
  if (threadIdx.x < np) L = attrs[mine_p].likelihood;
  if (kAccum) {
    if (threadIdx.x < np) {
      const unsigned long long* row = s_acc + threadIdx.x * static_cast<uint32_t>(kAccWords);
      const double p0w = static_cast<double>(s_n0[threadIdx.x]) * s_wu[threadIdx.x];   // prod of every w1: the weight of the history
      const double m0 = static_cast<double>(L.mean);
      const double mean = p0w * m0 + acc_value(row, kAccBins1, kAccEmin1);
      const double S = p0w * (static_cast<double>(L.sigma) + m0 * m0) + acc_value(row + kAccBins1, kAccBins2, kAccEmin2);
      const bool bad = s_bad[threadIdx.x] != 0u;
      L.mean = bad ? __uint_as_float(0x7FC00000u) : static_cast<float>(mean);
      L.sigma = bad ? __uint_as_float(0x7FC00000u) : static_cast<float>(fmax(S - mean * mean, 0.0));   // never negative: see above
    }
  } else if (!evals_global) {
  // dense pass: error -> likelihood (PCDSensorUpdaterEmbree.cpp:224: float argument, double exp / sqrt, float result)
  for (uint32_t i = threadIdx.x; i < nrays; i += 256u) {
    const float error = s_eval[i];
    if (p.errors) {
      if (p.order) { const uint32_t pi = i / p.n_beams; p.errors[static_cast<size_t>(p.order[p0 + pi]) * p.n_beams + (i - pi * p.n_beams)] = error; }
      else p.errors[static_cast<size_t>(p0) * p.n_beams + i] = error;
    }
    const float arg = -(error * error) / sq / 2;
    s_eval[i] = static_cast<float>(exp(static_cast<double>(arg)) / den);
  }

  // in-order merge (sequential semantics of sensorUpdate, :232-238): likelihood += Gaussian1D{eval, 0, 1}; n_meas = min(n_meas, max)
  // after every beam.  The count a particle carries INTO beam k is a_k = n0 (k = 0), n0 + min(k, max - n0) (n0 < max), max
  // (otherwise): both weights of rm::Gaussian1D::operator+= for every (particle, beam) come from all lanes, chunk by chunk,
  // into the stack rows; the chain of one lane per particle is then the multiply-adds of g1d_add in g1d_add's order.
  const uint32_t chunk = min(p.n_beams, (static_cast<uint32_t>(kRows * 256) / np - 2u) / 2u);  // beams per chunk; np <= 64 => >= 39
  const uint32_t wstride = 2u * chunk + 2u;
  for (uint32_t b0 = 0; b0 < p.n_beams; b0 += chunk) {
    const uint32_t nb = min(chunk, p.n_beams - b0);
    __syncthreads();
    for (uint32_t pi = 0; pi < np; ++pi) {
      const uint32_t n0 = s_n0[pi];
      for (uint32_t j = threadIdx.x; j < nb; j += 256u) {
        const uint32_t k = b0 + j;
        const uint32_t a = (k == 0u) ? n0 : ((n0 < p.max_n_meas) ? n0 + min(k, p.max_n_meas - n0) : p.max_n_meas);
        const uint32_t n = a + 1u;
        s_w[pi * wstride + 2u * j] = static_cast<float>(a) / static_cast<float>(n);
        s_w[pi * wstride + 2u * j + 1u] = static_cast<float>(1u) / static_cast<float>(n);
      }
    }
    __syncthreads();
    if (threadIdx.x < np) {
      const float* ev = s_eval + threadIdx.x * p.n_beams + b0;
      const float* w = s_w + threadIdx.x * wstride;
      for (uint32_t j = 0; j < nb; ++j) {
        const float w1 = w[2u * j], w2 = w[2u * j + 1u], e = ev[j];
        const float mean = L.mean * w1 + e * w2;
        const float P1 = L.sigma * w1 + 0.0f * w2;
        const float P2 = ((L.mean - mean) * (L.mean - mean)) * w1 + ((e - mean) * (e - mean)) * w2;
        L.mean = mean;
        L.sigma = P1 + P2;
      }
    }
  }
  } else {
  // The same two steps with the errors in global scratch: chunk by chunk, ALL lanes turn the chunk's errors into likelihoods
  // (same operations, same result) and the two merge weights, three floats per (particle, beam) in the vacated stack rows
  // [ w1 | w2 | likelihood ]; then one lane per particle runs the chain over the chunk from LDS as before.
  const uint32_t chunk = min(p.n_beams, (static_cast<uint32_t>(kRows * 256) / np) / 3u);   // np <= 64, kRows >= 16 => >= 21
  const uint32_t cstride = 3u * chunk;
  for (uint32_t b0 = 0; b0 < p.n_beams; b0 += chunk) {
    const uint32_t nb = min(chunk, p.n_beams - b0);
    const uint32_t cells = np * nb;
    const uint32_t nb_m = (nb == 1u) ? 0u : static_cast<uint32_t>(0x100000000ull / nb) + 1u;   // cell / nb (cells < 2^16 * 2^8)
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
      const uint32_t pi = (nb == 1u) ? c : __umulhi(c, nb_m), j = c - pi * nb, k = b0 + j;
      const float error = s_eval[pi * p.n_beams + k];
      if (p.errors) {
        const uint32_t dst = p.order ? p.order[p0 + pi] : (p0 + pi);
        p.errors[static_cast<size_t>(dst) * p.n_beams + k] = error;
      }
      const float arg = -(error * error) / sq / 2;
      const uint32_t n0 = s_n0[pi];
      const uint32_t a = (k == 0u) ? n0 : ((n0 < p.max_n_meas) ? n0 + min(k, p.max_n_meas - n0) : p.max_n_meas);
      const uint32_t n = a + 1u;
      float* cell = s_w + pi * cstride + 3u * j;
      cell[0] = static_cast<float>(a) / static_cast<float>(n);
      cell[1] = static_cast<float>(1u) / static_cast<float>(n);
      cell[2] = static_cast<float>(exp(static_cast<double>(arg)) / den);
    }
    __syncthreads();
    if (threadIdx.x < np) {
      const float* w = s_w + threadIdx.x * cstride;
      for (uint32_t j = 0; j < nb; ++j) {
        const float w1 = w[3u * j], w2 = w[3u * j + 1u], e = w[3u * j + 2u];
        const float mean = L.mean * w1 + e * w2;
        const float P1 = L.sigma * w1 + 0.0f * w2;
        const float P2 = ((L.mean - mean) * (L.mean - mean)) * w1 + ((e - mean) * (e - mean)) * w2;
        L.mean = mean;
        L.sigma = P1 + P2;
      }
    }
  }
  }
  if (threadIdx.x < np) {
    const uint32_t n0 = s_n0[threadIdx.x], k = p.n_beams;
    L.n_meas = (n0 < p.max_n_meas) ? n0 + min(k, p.max_n_meas - n0) : p.max_n_meas;
    attrs[mine_p].likelihood = L;
  }
}

// particle_move_and_forget_kernel (rmcl_ros/src/rmcl/particle_motion.cu:11-34) + the wall-collision test of the
// CPU updater (collision_in_between, TFMotionUpdaterCPU.cpp:17-50,207-221): one lane per particle; the occlusion
// ray runs from the old to the new particle position with tfar = segment length.
// kSurface: the surface constraint in the same launch (surface.hip.h; include/rmclhip.h has the rule).  The collision segment is then
// LIFTED by the step height: it runs between the probe origins of the old and of the moved pose, so that what is lower than probe_up is
// climbed and what is taller is a wall; the probe runs on the moved pose whether or not the particle was killed.  The instantiations
// without it are the kernel of before (`sx` is not read).
// kNoise: the sampled odometry model (include/rmclhip.h, MOTION NOISE): the moved pose is composed with this particle's Gaussian draw
// (pf_random.hip.h: motion_noise_compose) before anything else looks at it, so the collision segment ends at the noisy position and the
// surface constraint probes the noisy pose.  The instantiations without it do not read `nz`.
struct SurfaceArgs { SurfaceKernelParams sp; uint32_t* stats; uint32_t* faces; };
template <bool kCollision, bool kSurface = false, bool kNoise = false>
__global__ void __launch_bounds__(256) k_pf_motion(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ tris,
                                                   xform* __restrict__ poses, pattrs* __restrict__ attrs, uint32_t n,
                                                   xform T_bnew_bold, double forget_rate, uint32_t max_n_meas, SurfaceArgs sx,
                                                   MotionNoiseKernelParams nz) {
  extern __shared__ uint32_t lds_dyn[];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const uint32_t ii = live ? i : 0u;
  const xform pose_old = poses[ii];
  g1d L = attrs[ii].likelihood;
  xform pose_new = xmul(pose_old, T_bnew_bold);
  if (kNoise) pose_new = motion_noise_compose(pose_new, nz.first + ii, nz.step, nz.key0, nz.key1, nz.sigma);
  // `n_meas -= forget_rate * n_meas` on a uint32: double arithmetic, truncating store
  L.n_meas = static_cast<uint32_t>(static_cast<double>(L.n_meas) - forget_rate * static_cast<double>(L.n_meas));
  f3 a_new = mk3(0.0f, 0.0f, 1.0f), O_new = pose_new.t, seg_from = pose_old.t;
  if (kSurface) {
    a_new = surface_axis(sx.sp, pose_new);
    O_new = surface_origin(sx.sp, pose_new, a_new);
    if (kCollision) seg_from = surface_origin(sx.sp, pose_old, surface_axis(sx.sp, pose_old));
  }
  if (kCollision) {
    f3 vec = sub3(kSurface ? O_new : pose_new.t, seg_from);
    const float length = sqrtf((vec.x * vec.x + vec.y * vec.y) + vec.z * vec.z);
    const bool moving = !(static_cast<double>(length) < 0.00001);
    vec = mk3(vec.x / length, vec.y / length, vec.z / length);
    RayHit h;
    // guarded slab: a centimetre step far from the origin is axis-parallel in float32 (traverse.hip.h: make_ray_slab_guarded)
    trace_lane_bf<16, true, false, false, true>(nodes, tris, seg_from, vec, (live && moving) ? length : -1.0f, lds_dyn + threadIdx.x, h);
    if (moving && h.rec != kNone) { L.mean = 0.0f; L.sigma = 0.0f; L.n_meas = max_n_meas; }
  }
  if (kSurface) {
    const uint32_t cls = surface_constrain_lane(nodes, tris, sx.sp, pose_new, a_new, O_new, live, lds_dyn + threadIdx.x, sx.faces ? sx.faces + ii : nullptr);
    if (cls != kSurfSnap && sx.sp.on_miss != 0u) { L.mean = 0.0f; L.sigma = 0.0f; L.n_meas = max_n_meas; }
    surface_count(sx.stats, live, cls);
  }
  if (live) {
    poses[i] = pose_new;
    attrs[i].likelihood = L;
  }
}

// ---------------------------------------------------------------------------------------------
// pose estimate of the particle cloud (RmclNode::estimateStats, rmcl_ros/src/nodes/rmcl_localization.cpp:642-731) as
// three linear moment passes, so that it shards: every GPU reduces its block of the particles to <= 24 doubles and the
// ranks all-reduce them ("Stats for pose estimate: all-reduce of ~32 floats").
//   pass 0: sum L, sum L^2, count | max L, -min L, bb_max xyz, -bb_min xyz (max-reduced)           (:664-689)
//   pass 1: sum w q q^T (10 unique entries, x y z w order), sum w t, with w = L / L_sum                  (:703-705)
//           -- the Markley mean is the eigenvector of the largest eigenvalue of that 4x4 matrix
//   pass 2: sum w d d^T (21 unique entries), d = (dt, roll, pitch, yaw) of ~Tbm * T_i                    (:716-718)
// Partials per block: 24 sums (double) + 8 maxima (float as double).
// ---------------------------------------------------------------------------------------------
constexpr int kMomSums = 24, kMomMax = 8;

// labels (nullable): only the particles with labels[i] == want take part (the moments of one pose hypothesis, hypotheses.hip); the
// arithmetic of a particle that takes part, and the order of the sums, do not depend on it.
__global__ void __launch_bounds__(256) k_pose_moments(const xform* __restrict__ poses, const pattrs* __restrict__ attrs, uint32_t n,
                                                      int pass, double L_sum, xform Tbm, double* __restrict__ partials,
                                                      const uint32_t* __restrict__ labels, uint32_t want) {
  __shared__ double red[4][kMomSums + kMomMax];
  double acc[kMomSums];
  float mx[kMomMax];
#pragma unroll
  for (int k = 0; k < kMomSums; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 0; k < kMomMax; ++k) mx[k] = -3.402823466e38f;
  const xform Tmb = xinv(Tbm);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (labels != nullptr && labels[i] != want) continue;
    const xform T = poses[i];
    const float Lf = attrs[i].likelihood.mean;
    const double L = static_cast<double>(Lf);
    if (pass == 0) {
      acc[0] += L; acc[1] += L * L; acc[2] += 1.0;
      mx[0] = fmaxf(mx[0], Lf); mx[1] = fmaxf(mx[1], -Lf);
      mx[2] = fmaxf(mx[2], T.t.x); mx[3] = fmaxf(mx[3], T.t.y); mx[4] = fmaxf(mx[4], T.t.z);
      mx[5] = fmaxf(mx[5], -T.t.x); mx[6] = fmaxf(mx[6], -T.t.y); mx[7] = fmaxf(mx[7], -T.t.z);
    } else if (pass == 1) {
      const double w = L / L_sum;
      const double q[4] = {T.R.x, T.R.y, T.R.z, T.R.w};
      int k = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) acc[k++] += w * q[a] * q[b];
      acc[10] += w * T.t.x; acc[11] += w * T.t.y; acc[12] += w * T.t.z;
    } else {
      const double w = L / L_sum;
      const xform Td = xmul(Tmb, T);
      double d[6] = {Td.t.x, Td.t.y, Td.t.z, 0.0, 0.0, 0.0};
      quat_to_euler_f64(Td.R, d[3], d[4], d[5]);   // the angles in double, not rounded to float (pf_random.hip.h)
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) acc[k++] += w * d[a] * d[b];
    }
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kMomSums; ++k) {
    double v = acc[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0u) red[wave][k] = v;
  }
#pragma unroll
  for (int k = 0; k < kMomMax; ++k) {
    float v = mx[k];
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if (lane == 0u) red[wave][kMomSums + k] = static_cast<double>(v);
  }
  __syncthreads();
  if (threadIdx.x < kMomSums + kMomMax) {
    const int k = static_cast<int>(threadIdx.x);
    double v;
    if (k < kMomSums) v = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    else v = fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]));
    partials[static_cast<size_t>(blockIdx.x) * (kMomSums + kMomMax) + k] = v;
  }
}

// One workgroup folds the per-block partials: thread = (moment k, group g of 8); a group takes every 8th block with four loads in
// flight, the eight group sums are folded in a fixed order through LDS (deterministic).  Round 2's version -- one 64-lane wave,
// one dependent load per block and lane -- took 23.7 us for 98 blocks, twice the streaming pass it finalizes.
__global__ void __launch_bounds__(256) k_pose_moments_final(const double* __restrict__ partials, uint32_t nblocks, double* __restrict__ out) {
  constexpr int kW = kMomSums + kMomMax;   // 32
  __shared__ double s_g[8][kW];
  const int k = static_cast<int>(threadIdx.x) & (kW - 1);
  const uint32_t g = threadIdx.x >> 5;
  const bool is_sum = k < kMomSums;
  double v = is_sum ? 0.0 : -1.7976931348623157e308;
  uint32_t b = g;
  for (; b + 24u < nblocks; b += 32u) {
    const double x0 = partials[static_cast<size_t>(b) * kW + k], x1 = partials[static_cast<size_t>(b + 8u) * kW + k];
    const double x2 = partials[static_cast<size_t>(b + 16u) * kW + k], x3 = partials[static_cast<size_t>(b + 24u) * kW + k];
    v = is_sum ? (v + ((x0 + x1) + (x2 + x3))) : fmax(fmax(v, fmax(x0, x1)), fmax(x2, x3));
  }
  for (; b < nblocks; b += 8u) {
    const double x = partials[static_cast<size_t>(b) * kW + k];
    v = is_sum ? (v + x) : fmax(v, x);
  }
  s_g[g][k] = v;
  __syncthreads();
  if (threadIdx.x < static_cast<uint32_t>(kW)) {
    double r = s_g[0][k];
#pragma unroll
    for (int q = 1; q < 8; ++q) r = is_sum ? (r + s_g[q][k]) : fmax(r, s_g[q][k]);
    out[k] = r;
  }
}

// dense weight vector from the padded all-gather layout: rank r's shard sits at r * cap
__global__ void k_compact_shards(const float* __restrict__ padded, float* __restrict__ dense, uint32_t n_total, uint32_t world, uint32_t cap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_total) return;
  const uint32_t base = n_total / world, rem = n_total % world;
  // owner of global index i under the block partition (the first `rem` ranks own base + 1)
  const uint32_t split = rem * (base + 1u);
  const uint32_t r = (i < split) ? (i / (base + 1u)) : (rem + (i - split) / max(base, 1u));
  const uint32_t lo = r * base + min(r, rem);
  dense[i] = padded[static_cast<size_t>(r) * cap + (i - lo)];
}

// the same for records of `wpr` dwords (poses: 8, attributes: 9): one thread per dword
__global__ void k_compact_records(const uint32_t* __restrict__ padded, uint32_t* __restrict__ dense, uint32_t n_total, uint32_t world, uint32_t cap,
                                  uint32_t wpr) {
  const size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= static_cast<size_t>(n_total) * wpr) return;
  const uint32_t i = static_cast<uint32_t>(g / wpr), w = static_cast<uint32_t>(g - static_cast<size_t>(i) * wpr);
  const uint32_t base = n_total / world, rem = n_total % world;
  const uint32_t split = rem * (base + 1u);
  const uint32_t r = (i < split) ? (i / (base + 1u)) : (rem + (i - split) / max(base, 1u));
  const uint32_t lo = r * base + min(r, rem);
  dense[g] = padded[(static_cast<size_t>(r) * cap + (i - lo)) * wpr + w];
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
namespace {
const LabHooks* g_lab = nullptr;

// the run-time sensor model as a compile-time constant: f(std::integral_constant<uint32_t, kModel...>); false = no such model
template <class F>
bool with_model(ModelKind kind, F&& f) {
  switch (kind) {
    case kModelSpherical: f(std::integral_constant<uint32_t, kModelSpherical>{}); return true;
    case kModelO1Dn: f(std::integral_constant<uint32_t, kModelO1Dn>{}); return true;
    case kModelPinhole: f(std::integral_constant<uint32_t, kModelPinhole>{}); return true;
    case kModelOnDn: f(std::integral_constant<uint32_t, kModelOnDn>{}); return true;
    default: return false;
  }
}
}
const LabHooks* lab_hooks() { return g_lab; }

// ---------------------------------------------------------------------------------------------
// World order of a pose batch (VERDICT r5 #7b): key of wave-tile (pose, tile) = Morton code (4 bits per axis) of the point where the
// tile's central ray leaves the map's bounding box -- for a sensor inside its map that is where the tile's rays end up, whatever pose
// they start from.  4096 cells and a counting sort (count while the keys are made, one block scans the cells, scatter): three small
// launches, ~15 us for the 228 k tiles of the reference's v1 batch; rocPRIM's radix sort of 30-bit keys took 16 launches and 100 us.
// The order inside a cell is whatever the atomics make it -- it decides which workgroup computes a tile, never what is computed.
// k_find then walks the tiles in that order (FindParams::tile_order).
// ---------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kOrderCells = 4096u;
__device__ __forceinline__ uint32_t morton_spread4(uint32_t v) {   // bits 0..3 -> bits 0, 3, 6, 9
  return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6);
}
template <uint32_t kModel>
__global__ void __launch_bounds__(256) k_batch_tile_keys(const FindParams p, uint32_t group, uint32_t ngroups, f3 bb_min, f3 bb_max,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ cell_count) {
  const uint32_t ntiles = p.tiles_x * p.tiles_y;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= ngroups * p.nposes) return;
  const uint32_t pose = i / ngroups, tile = min((i - pose * ngroups) * group + (group >> 1), ntiles - 1u);   // the middle tile of the workgroup's tiles
  const uint32_t ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const uint32_t twl = p.tile_w_log2;
  const uint32_t cv = min((ty << (6u - twl)) + (32u >> twl), p.H - 1u), ch = min((tx << twl) + ((1u << twl) >> 1), p.W - 1u);
  f3 dir_s, orig_s = p.orig_s;
  find_ray_s<kModel>(p, cv, ch, cv * p.W + ch, dir_s, orig_s);
  const xform Tsm = p.Tsm_arr[pose];
  const f3 o = xapply(Tsm, orig_s), d = qrot(Tsm.R, dir_s);
  float t = 3.0e38f;
  const float od[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, lo[3] = {bb_min.x, bb_min.y, bb_min.z}, hi[3] = {bb_max.x, bb_max.y, bb_max.z};
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (dd[a] != 0.0f) t = fminf(t, fmaxf(((dd[a] > 0.0f ? hi[a] : lo[a]) - od[a]) / dd[a], 0.0f));
  if (!(t < 3.0e38f)) t = 0.0f;   // (NaN directions, a ray without direction: the origin's cell)
  uint32_t q[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float u = (od[a] + t * dd[a] - lo[a]) / fmaxf(hi[a] - lo[a], 1e-20f);
    q[a] = static_cast<uint32_t>(fminf(fmaxf(u, 0.0f), 1.0f) * 15.0f);   // (NaN -> 0)
  }
  const uint32_t key = morton_spread4(q[0]) | (morton_spread4(q[1]) << 1) | (morton_spread4(q[2]) << 2);
  keys[i] = key;
  atomicAdd(cell_count + key, 1u);
}
// exclusive scan of the 4096 cell counts, in place (one block; the counts become the cells' first slots)
__global__ void __launch_bounds__(256) k_batch_cell_scan(uint32_t* __restrict__ cell) {
  __shared__ uint32_t s_sum[256];
  const uint32_t t = threadIdx.x;
  uint32_t v[16], run = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { v[k] = cell[t * 16u + k]; run += v[k]; }
  s_sum[t] = run;
  __syncthreads();
  for (uint32_t off = 1; off < 256u; off <<= 1) {
    const uint32_t add = (t >= off) ? s_sum[t - off] : 0u;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  uint32_t base = s_sum[t] - run;
#pragma unroll
  for (int k = 0; k < 16; ++k) { cell[t * 16u + k] = base; base += v[k]; }
}
__global__ void __launch_bounds__(256) k_batch_tile_scatter(const uint32_t* __restrict__ keys, uint32_t* __restrict__ cell_next, uint32_t ngroups,
                                                            uint32_t n, uint32_t* __restrict__ order) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t pose = i / ngroups, g = i - pose * ngroups;
  order[atomicAdd(cell_next + keys[i], 1u)] = (pose << 16) | g;
}
}  // namespace

uint32_t batch_order_scratch_dwords(uint32_t n) { return n + kOrderCells; }

// One entry per WORKGROUP of the find (its `group` = 4 consecutive tiles of one pose -- 1 for the quad kind --: neighbours in the scan image
// stay together, their waves share the CU's L1 as in the pose-major launch; sorting single tiles cost the 100 k-face map 6 %).
// scratch: n keys | 4096 cells; order: n = nposes x ceil(ntiles / group) entries pose << 16 | group index
hipError_t launch_batch_tile_order(const FindParams& p, ModelKind kind, uint32_t group, f3 bb_min, f3 bb_max, uint32_t* scratch, uint32_t* order,
                                   hipStream_t s) {
  const uint32_t ntiles = p.tiles_x * p.tiles_y, ngroups = (ntiles + group - 1u) / group, n = ngroups * p.nposes;
  uint32_t* keys = scratch;
  uint32_t* cells = scratch + n;
  hipError_t e = hipMemsetAsync(cells, 0, kOrderCells * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const dim3 grid((n + 255u) / 256u), block(256);
  const bool known = with_model(kind, [&](auto m) {
    hipLaunchKernelGGL((k_batch_tile_keys<decltype(m)::value>), grid, block, 0, s, p, group, ngroups, bb_min, bb_max, keys, cells);
  });
  if (!known) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_batch_cell_scan, dim3(1), block, 0, s, cells);
  hipLaunchKernelGGL(k_batch_tile_scatter, grid, block, 0, s, keys, cells, ngroups, n, order);
  return hipGetLastError();
}

FindLaunchShape find_launch_shape(int kind, bool moments, uint32_t ntiles, uint32_t nposes, uint32_t n_tile_order, uint32_t granule) {
  const FindKind K = find_kind(kind);
  FindLaunchShape sh = {0u, 0u, 0u, 0u};
  if (!K.exists) return sh;
  moments = moments && K.moments;
  sh.grid_x = ((ntiles + K.tiles_per_block() - 1u) / K.tiles_per_block() + 7u) & ~7u;  // the XCD remap in k_find needs gridDim.x % 8 == 0
  sh.grid_y = moments ? 1u : nposes;   // (the moment epilogue: one scan, and k_find ignores the world order under it)
  if (n_tile_order != 0u && !moments) {   // world order: one row of blocks over the sorted (pose, tile) list, one entry per workgroup
    const uint32_t turn = 8u * max(granule, 1u);
    sh.grid_x = (n_tile_order + turn - 1u) / turn * turn;   // whole turns of the eight XCDs (k_find's slot mapping)
    sh.grid_y = 1u;
  }
  sh.lds_bytes = find_lds_dwords(kind, moments) * static_cast<uint32_t>(sizeof(uint32_t));
  sh.clock_dwords = sh.grid_x * sh.grid_y * 4u * K.clock_words();
  return sh;
}
FindLaunchShape find_launch_shape(const FindParams& p, int kind, bool moments) {
  return find_launch_shape(kind, moments, p.tiles_x * p.tiles_y, p.nposes, p.tile_order != nullptr ? p.n_tile_order : 0u, p.tile_order_granule);
}

namespace {
// the product's k_find<model, kTrav, no clocks, kMoments, kCarry>
template <int kTrav, bool kMoments, bool kCarry = false>
hipError_t launch_find_one(const FindParams& p, ModelKind kind, hipStream_t s) {
  static_assert(find_kind(kTrav).in_product && (!kMoments || find_kind(kTrav).moments), "not a kernel of the product (find_kinds.h)");
  const FindLaunchShape sh = find_launch_shape(p, kTrav, kMoments);
  const bool known = with_model(kind, [&](auto m) {
    hipLaunchKernelGGL((k_find<decltype(m)::value, kTrav, false, kMoments, kCarry>), dim3(sh.grid_x, sh.grid_y, 1), dim3(256, 1, 1), sh.lds_bytes, s, p);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}
// kind 32: bit 16 of descent_levels = pending candidates in the cooperative leaf loop, a kernel of its own
template <bool kMoments>
hipError_t launch_find_32(const FindParams& p, ModelKind kind, hipStream_t s) {
  return ((p.descent_levels >> 16) & 1u) ? launch_find_one<32, kMoments, true>(p, kind, s) : launch_find_one<32, kMoments>(p, kind, s);
}
}  // namespace

// the two switches below list the product's 40 k_find kernels (x 4 models each), in the order the object file holds them
hipError_t launch_find(const FindParams& p, ModelKind kind, int variant, hipStream_t s) {
  if (!find_kind(variant).in_product || p.wave_clock != nullptr) {
    // an experiment's kind, or a clocked launch of any kind (tools/wave_timeline.py): librmclhip_lab.so
    if (g_lab && g_lab->find) return g_lab->find(p, kind, variant, p.wave_clock != nullptr, s);
    return kLabMissing;
  }
  switch (variant) {
    case 0: return launch_find_one<0, false>(p, kind, s);
    case 2: return launch_find_one<2, false>(p, kind, s);
    case 23: return launch_find_one<23, false>(p, kind, s);
    case 32: return launch_find_32<false>(p, kind, s);
    case 24: return launch_find_one<24, false>(p, kind, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_find_moments(const FindParams& p, ModelKind kind, int variant, hipStream_t s) {
  static_assert(kMomRow == kMicpFastMoments && kMomRow == static_cast<uint32_t>(kMom), "one partial-row layout");
  if (p.nposes != 1u || p.wave_clock != nullptr || p.mom_partials == nullptr || p.mom_unc_mask == nullptr) return hipErrorInvalidValue;
  switch (variant) {
    case 2: return launch_find_one<2, true>(p, kind, s);
    case 32: return launch_find_32<true>(p, kind, s);
    case 23: return launch_find_one<23, true>(p, kind, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_tile_planes(const FindParams& p, ModelKind kind, float* planes, hipStream_t s) {
  const uint32_t ntiles = p.tiles_x * p.tiles_y;
  if (ntiles == 0u) return hipSuccess;
  const dim3 grid((ntiles + 3u) / 4u), block(256);
  if (kind == kModelOnDn) return hipErrorInvalidValue;   // one origin per ray, no pyramid: no k_tile_planes<OnDn> either
  const bool known = with_model(kind, [&](auto m) {
    if constexpr (decltype(m)::value != kModelOnDn) hipLaunchKernelGGL((k_tile_planes<decltype(m)::value>), grid, block, 0, s, p, planes);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_find_probe(const FindParams& p, int mode, uint32_t* probe_log, hipStream_t s) {
  if (g_lab && g_lab->find_probe) return g_lab->find_probe(p, mode, probe_log, s);
  return kLabMissing;
}

hipError_t launch_cpc_find(const uint32_t* nodes, const uint32_t* tris, const float* dataset_points, uint32_t n,
                           float max_dist, xform Tsm, xform Tms, uint8_t* hits, float* dists, float* points,
                           float* normals, uint32_t* face_ids, bool quad, hipStream_t s, const uint32_t* seed_rec, uint32_t* rec_out,
                           uint32_t n_tris, float bound_d2, const NearGrid* grid, const NearGrid* cells, float skip_d2) {
  if (n == 0) return hipSuccess;
  CpcParams p;
  p.nodes = nodes; p.tris = tris; p.dataset_points = dataset_points; p.n = n; p.max_dist = max_dist;
  p.Tsm = Tsm; p.Tms = Tms; p.hits = hits; p.dists = dists; p.points = points; p.normals = normals; p.face_ids = face_ids;
  p.seed_rec = seed_rec; p.rec_out = rec_out; p.n_tris = n_tris; p.bound_d2 = bound_d2;
  p.near_grid = nullptr; p.from_cells = (cells != nullptr) ? 1u : 0u; p.skip_d2 = skip_d2;
  for (int k = 0; k < 3; ++k) { p.gn[k] = 1u; p.gorg[k] = 0.f; p.ginv[k] = 1.f; p.cn[k] = 1u; p.corg[k] = 0.f; p.cinv[k] = 1.f; }
  if (grid != nullptr) {
    p.near_grid = grid->cells;
    for (int k = 0; k < 3; ++k) { p.gn[k] = grid->n[k]; p.gorg[k] = grid->org[k]; p.ginv[k] = grid->inv[k]; }
  }
  if (cells != nullptr)
    for (int k = 0; k < 3; ++k) { p.cn[k] = cells->n[k]; p.corg[k] = cells->org[k]; p.cinv[k] = cells->inv[k]; }
  if (quad) hipLaunchKernelGGL((k_cpc_find<true>), dim3((n + 63u) / 64u), dim3(256), kQuadStackEntries * 64u * sizeof(uint32_t), s, p);
  else hipLaunchKernelGGL((k_cpc_find<false>), dim3((n + 255u) / 256u), dim3(256), 16u * 256u * sizeof(uint32_t), s, p);
  return hipGetLastError();
}

hipError_t launch_compose_poses(const xform* Tbm_dev, xform Tsb, xform* Tsm_out, xform* Tms_out, uint32_t n,
                                hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_compose_poses, dim3((n + 255u) / 256u), dim3(256), 0, s, Tbm_dev, Tsb, Tsm_out, Tms_out, n);
  return hipGetLastError();
}

uint32_t reduce_num_blocks(uint32_t n, uint32_t nposes) {
  // single reduction: two elements per thread keeps >= 256 workgroups in flight for a 128x1024 scan (the streaming
  // side needs the whole chip; measured 9.5 vs 10.0 us with half as many).  Pose batches already fill the chip with
  // nposes x blocks, and every pose's partials are consumed by ONE wave that fetches them 32 at a time per lane, so
  // fewer, larger blocks win there (64-pose correction 0.82 -> 0.69 ms at 4096 elements per block).
  const uint32_t per_block = (nposes >= 4u) ? 4096u : 512u;
  uint32_t nb = (n + per_block - 1u) / per_block;
  if (nb < 1u) nb = 1u;
  if (nb > 1024u) nb = 1024u;
  return nb;
}

hipError_t launch_reduce_partials(const ReduceParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_partials, dim3(p.nblocks, p.nposes), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_reduce_finalize(const double* partials, uint32_t nblocks, uint32_t nposes, cstats* out,
                                  unsigned long long* done, uint32_t seq, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_finalize, dim3(nposes), dim3(64), 0, s, partials, nblocks, out, (nposes == 1u) ? done : nullptr, seq);
  return hipGetLastError();
}

namespace {
// completion tag of a launch chain that returns nothing to the host but its own end: {seq, sum 0} to pinned memory, behind the chain
// on its stream (the kernel boundary before this launch is what makes the chain's results visible)
__global__ void k_host_tag(unsigned long long* done, uint32_t seq) {
  if (threadIdx.x == 0u && blockIdx.x == 0u) publish_tag(done, seq, 0u);
}
}  // namespace
hipError_t launch_host_tag(unsigned long long* done, uint32_t seq, hipStream_t s) {
  hipLaunchKernelGGL(k_host_tag, dim3(1), dim3(64), 0, s, done, seq);
  return hipGetLastError();
}

hipError_t launch_batch_solve(const double* partials, uint32_t nblocks, uint32_t nposes, xform Tsb,
                              xform* Tdelta_out, cstats* stats_out, hipStream_t s) {
  hipLaunchKernelGGL(k_batch_solve, dim3(nposes), dim3(64), 0, s, partials, nblocks, Tsb, Tdelta_out, stats_out);
  return hipGetLastError();
}

hipError_t launch_dataset_from_ranges(const float* ranges, const float* model_tab, uint32_t kind, uint32_t W,
                                      uint32_t H, f3 orig, const float* pin_fc, float rmin, float rmax, float* points,
                                      uint8_t* mask, uint32_t* n_valid, hipStream_t s) {
  const uint32_t n = W * H;
  hipLaunchKernelGGL(k_dataset_from_ranges, dim3((n + 255u) / 256u), dim3(256), 0, s, ranges, model_tab, kind, W, H,
                     orig, pin_fc[0], pin_fc[1], pin_fc[2], pin_fc[3], rmin, rmax, points, mask, n_valid);
  return hipGetLastError();
}

hipError_t launch_pf_update(const PfParams& p, int variant, hipStream_t s) {
  const uint32_t nblocks = (p.n_particles + p.particles_per_block - 1u) / p.particles_per_block;
  const size_t tail_fixed = sizeof(xform) * p.particles_per_block;
  const size_t tail = tail_fixed + sizeof(float) * static_cast<size_t>(p.particles_per_block) * p.n_beams;
  const int trav = variant & 3;          // traversal of the round kernels (lab)
  const bool cpc = (variant & 8) != 0;   // correspondence_type 1
  const int refill = (variant >> 4) & 7;  // 0 = rounds of one ray per lane (lab); 1..4 = persistent lanes
  const bool legacy = ((variant >> 8) & 1) != 0;   // bit 8: the round-2 kernel (k_pf_update_persist, lab), A/B
  const bool leaf2 = ((variant >> 10) & 1) == 0;   // bit 10 set: p.qnodes is the MAP's tree (leaves <= 4) -> loop over the leaf
  if (cpc) {
    // closest-point correspondences (evaluate_cpc): rounds of one beam per lane on the full nodes
    const size_t lds = 16u * 256u * sizeof(uint32_t) + tail;
    if (lds > 160u * 1024u - 64u) return hipErrorInvalidValue;
    if (lds > 65536u) {
      const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pf_update<64, 3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                160 * 1024 - 64);
      if (ae != hipSuccess) return ae;
    }
    hipLaunchKernelGGL((k_pf_update<64, 3>), dim3(nblocks), dim3(256), lds, s, p);
    return hipGetLastError();
  }
  if (trav == 0 && refill != 0 && !legacy && ((variant >> 7) & 1) == 0 && p.qnodes != nullptr) {
    // bit 11: the children of a node in the ray's SLOT order (round 5) instead of sorted by entry distance; bit 12: order-independent
    // likelihood accumulation (round 5: no per-beam storage; 19 stack rows so that the accumulators fit beside them at 7 workgroups per CU)
    const bool slot_order = ((variant >> 11) & 1) != 0, accum = ((variant >> 12) & 1) != 0 && p.gpow != nullptr;
    constexpr int kAccRows = kPfRows - 1;
    const uint32_t PB = p.particles_per_block;
    const size_t acc_off = (static_cast<size_t>(kAccRows) * 256u + 8u * PB + PB + 1u) * sizeof(uint32_t);   // + 1: the kernel's alignment skip
    const size_t lds = accum ? acc_off + static_cast<size_t>(PB) * (sizeof(double) + 2u * sizeof(uint32_t) + static_cast<size_t>(kAccWords) * 8u)
                             : static_cast<size_t>(kPfRows) * 256u * sizeof(uint32_t) + (p.evals != nullptr ? tail_fixed : tail) + sizeof(uint32_t) * PB;
    if (lds > 160u * 1024u - 64u) return hipErrorInvalidValue;   // more beams per particle than one workgroup's LDS holds
#define RMCL_PF_V3(ROWS, L2, SO, AC)                                                                                           \
    {                                                                                                                          \
      if (lds > 65536u) {   /* per launch: the attribute belongs to the function ON THE CURRENT DEVICE (sharded filters) */   \
        const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pf_update_v3<ROWS, L2, SO, AC>),            \
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);                \
        if (ae != hipSuccess) return ae;                                                                                       \
      }                                                                                                                        \
      hipLaunchKernelGGL((k_pf_update_v3<ROWS, L2, SO, AC>), dim3(nblocks), dim3(256), lds, s, p);                              \
      return hipGetLastError();                                                                                                \
    }
    if (accum) {
      if (leaf2 && slot_order) RMCL_PF_V3(kAccRows, true, true, true)
      if (leaf2) RMCL_PF_V3(kAccRows, true, false, true)
      if (slot_order) RMCL_PF_V3(kAccRows, false, true, true)
      RMCL_PF_V3(kAccRows, false, false, true)
    }
    if (leaf2 && slot_order) RMCL_PF_V3(kPfRows, true, true, false)
    if (leaf2) RMCL_PF_V3(kPfRows, true, false, false)
    if (slot_order) RMCL_PF_V3(kPfRows, false, true, false)
    RMCL_PF_V3(kPfRows, false, false, false)
#undef RMCL_PF_V3
  }
  if (g_lab && g_lab->pf_update) return g_lab->pf_update(p, variant, s);
  return kLabMissing;
}

hipError_t launch_pf_motion(const uint32_t* nodes, const uint32_t* tris, xform* poses, void* attrs, uint32_t n,
                            xform T_bnew_bold, double forget_rate, uint32_t max_n_meas, bool collision, hipStream_t s,
                            const SurfaceKernelParams* surface, uint32_t* surface_stats, uint32_t* surface_faces,
                            const MotionNoiseKernelParams* noise) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + 255u) / 256u), block(256);
  SurfaceArgs sx = {};
  MotionNoiseKernelParams nz = {};
  if (noise) nz = *noise;
  if (surface) {
    if (!surface_stats) return hipErrorInvalidValue;
    sx.sp = *surface;
    sx.stats = surface_stats;
    sx.faces = surface_faces;
  }
  // (the collision ray and the surface ray keep their stacks in LDS: 16 words per lane)
#define RMCL_PF_MOTION(C, S, N)                                                                                               \
  hipLaunchKernelGGL((k_pf_motion<C, S, N>), grid, block, ((C) || (S)) ? 16u * 256u * sizeof(uint32_t) : 0u, s, nodes, tris, poses, \
                     reinterpret_cast<pattrs*>(attrs), n, T_bnew_bold, forget_rate, max_n_meas, sx, nz)
  if (noise) {
    if (surface) { if (collision) RMCL_PF_MOTION(true, true, true); else RMCL_PF_MOTION(false, true, true); }
    else if (collision) RMCL_PF_MOTION(true, false, true);
    else RMCL_PF_MOTION(false, false, true);
  } else if (surface) { if (collision) RMCL_PF_MOTION(true, true, false); else RMCL_PF_MOTION(false, true, false); }
  else if (collision) RMCL_PF_MOTION(true, false, false);
  else RMCL_PF_MOTION(false, false, false);
#undef RMCL_PF_MOTION
  return hipGetLastError();
}

hipError_t launch_build_cnodes16(const uint32_t* cnodes, uint32_t n_nodes, uint32_t* cnodes16, hipStream_t s) {
  if (n_nodes == 0u) return hipSuccess;
  const uint32_t nb = (n_nodes * 16u + 255u) / 256u;
  hipLaunchKernelGGL(k_build_cnodes16, dim3(nb), dim3(256), 0, s, reinterpret_cast<const uint4*>(cnodes), n_nodes, reinterpret_cast<uint4*>(cnodes16));
  return hipGetLastError();
}

hipError_t launch_pointcloud2_unpack(const uint8_t* data, uint32_t point_step, uint32_t row_step, uint32_t off_x,
                                     uint32_t off_y, uint32_t off_z, bool is_f64, uint32_t h_skip, uint32_t h_inc,
                                     uint32_t w_skip, uint32_t w_inc, uint32_t out_w, uint32_t out_h, float range_min,
                                     float range_max, float* dirs, float* points, uint8_t* mask, uint32_t* n_valid,
                                     hipStream_t s) {
  const uint32_t n = out_w * out_h;
  if (n == 0) return hipSuccess;
  Pc2Params p{data, point_step, row_step, off_x, off_y, off_z, is_f64 ? 1u : 0u, h_skip, h_inc, w_skip, w_inc,
              out_w, out_h, range_min, range_max, dirs, points, mask, n_valid};
  hipLaunchKernelGGL(k_pointcloud2_unpack, dim3((n + 255u) / 256u), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_pose_moments(const xform* poses, const void* attrs, uint32_t n, int pass, double L_sum, xform Tbm,
                               double* partials, double* out32, hipStream_t s, const uint32_t* labels, uint32_t want) {
  const uint32_t nblocks = partial_blocks(n);
  hipLaunchKernelGGL(k_pose_moments, dim3(nblocks), dim3(256), 0, s, poses, reinterpret_cast<const pattrs*>(attrs), n, pass, L_sum, Tbm,
                     partials, labels, want);
  hipLaunchKernelGGL(k_pose_moments_final, dim3(1), dim3(256), 0, s, partials, nblocks, out32);
  return hipGetLastError();
}

// in-process stand-in for ncclAllReduce on doubles (the loopback communicator of the tests, capi_multi.cpp): every "rank" runs this on its own
// stream over the send buffers of all of them, in rank order (deterministic)
struct LoopbackPtrs { const double* p[64]; };
__global__ void k_loopback_allreduce(LoopbackPtrs send, uint32_t world, double* __restrict__ recv, uint32_t count, uint32_t is_max) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double a = send.p[0][i];
  for (uint32_t r = 1; r < world; ++r) { const double b = send.p[r][i]; a = is_max ? fmax(a, b) : a + b; }
  recv[i] = a;
}
hipError_t launch_loopback_allreduce(const double* const* send, uint32_t world, double* recv, uint32_t count, bool is_max, hipStream_t s) {
  if (count == 0 || world == 0 || world > 64) return world > 64 ? hipErrorInvalidValue : hipSuccess;
  LoopbackPtrs lp;
  for (uint32_t r = 0; r < 64; ++r) lp.p[r] = send[r < world ? r : 0];
  hipLaunchKernelGGL(k_loopback_allreduce, dim3((count + 63u) / 64u), dim3(64), 0, s, lp, world, recv, count, is_max ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_compact_shards(const float* padded, float* dense, uint32_t n_total, uint32_t world, uint32_t cap, hipStream_t s) {
  if (n_total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_compact_shards, dim3((n_total + 255u) / 256u), dim3(256), 0, s, padded, dense, n_total, world, cap);
  return hipGetLastError();
}

hipError_t launch_compact_records(const void* padded, void* dense, uint32_t n_total, uint32_t world, uint32_t cap, uint32_t record_bytes,
                                  hipStream_t s) {
  if (n_total == 0) return hipSuccess;
  if (record_bytes % 4u != 0u) return hipErrorInvalidValue;
  const uint32_t wpr = record_bytes / 4u;
  const size_t threads = static_cast<size_t>(n_total) * wpr;
  hipLaunchKernelGGL(k_compact_records, dim3(static_cast<uint32_t>((threads + 255u) / 256u)), dim3(256), 0, s, static_cast<const uint32_t*>(padded),
                     static_cast<uint32_t*>(dense), n_total, world, cap, wpr);
  return hipGetLastError();
}

}  // namespace rmclhip

extern "C" void rmclhip_internal_register_lab(const rmclhip::LabHooks* hooks) { rmclhip::g_lab = hooks; }
