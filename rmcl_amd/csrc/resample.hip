// resample.hip -- the three resamplers of the particle filter and the likelihood statistics they start from.
//
//   k_likelihood_stats_*   {sum, max} of likelihood.mean (simple_stats_kernel, resampling.cu:41-81)
//   k_pf_extract_weights   likelihood.mean as a dense vector (what a sharded filter all-gathers)
//   k_gladiator_resample   the tournament (resampling.cu:41-219): a champion that loses becomes a perturbed copy of its enemy
//   k_residual_*           residual resampling (ResidualResamplerCPU.cpp:55-203): the reference's sequential loop as data-parallel passes
//   k_sys_fill             systematic (low-variance) resampling to ANY size from ANY weights (include/rmclhip.h states the rules;
//                          tests/adaptive_ref.py restates them in numpy): slot j reads position pos_j of [0, T), T = C[n-1]; its source
//                          is the first i with C[i] > pos_j.  The first slot of a run of equal sources is a copy, every further one is
//                          perturbed as the gladiator perturbs a winning enemy.
//   k_scan_*               inclusive 64-bit prefix sums, ONE text for the residual resampler's copy counts, the systematic
//                          resampler's integer weights w_i = rint(L_i / max * 2^24) and the surface sampler's face weights
//                          w_f = rint(a_f / a_max * 2^32).  Integers: exact, independent of the launch shape.
//
// A "perturbed copy" is ONE text too (six_gaussians .. remember_rate_*): the kernels differ in which Philox words feed the Gaussians,
// where the six noise scales come from and the rule that turns the two distances into a rate.  Random stream = Philox4x32-10 keyed by
// the seed with counter (champion or slot index, step, draw, 0): reproducible, independent of the launch shape and of how the
// particle range is sharded across GPUs.  Transcendentals are evaluated in double and rounded to float (see oracle).
#include "kernels.h"
#include "kld_bins.hip.h"
#include "pf_random.hip.h"

namespace rmclhip {
namespace {

constexpr uint32_t kBlock = 256;

// ---------------------------------------------------------------------------------------------
// the perturbed copy
// ---------------------------------------------------------------------------------------------
struct ResampleConfig {
  float min_noise[6];   // tx ty tz roll pitch yaw
  float likelihood_forget_per_meter, likelihood_forget_per_radian;
  uint32_t trans_dist_metric;
};

ResampleConfig resample_config(const float* cfg8, uint32_t trans_dist_metric) {
  return ResampleConfig{{cfg8[0], cfg8[1], cfg8[2], cfg8[3], cfg8[4], cfg8[5]}, cfg8[6], cfg8[7], trans_dist_metric};
}

// six Gaussians from words kFirst .. kFirst + 5 of the eight words (ra, rb), in pairs: the gladiator and the systematic resampler start
// at word 1 (word 0 chose the enemy / is unused), the residual resampler at word 0
template <int kFirst>
__device__ __forceinline__ void six_gaussians(const uint32_t (&ra)[4], const uint32_t (&rb)[4], float (&Nd)[6]) {
  const uint32_t w[8] = {ra[0], ra[1], ra[2], ra[3], rb[0], rb[1], rb[2], rb[3]};
  box_muller(w[kFirst], w[kFirst + 1], Nd[0], Nd[1]);
  box_muller(w[kFirst + 2], w[kFirst + 3], Nd[2], Nd[3]);
  box_muller(w[kFirst + 4], w[kFirst + 5], Nd[4], Nd[5]);
}

// translation noise, then rotation noise on the Euler angles (EulerAngles e = pose_new.R; e += noise; pose_new.R = e)
__device__ __forceinline__ xform perturbed_pose(const xform& pose, const float (&Nd)[6], const float (&noise)[6]) {
  xform pn = pose;
  pn.t.x = pn.t.x + Nd[0] * noise[0];
  pn.t.y = pn.t.y + Nd[1] * noise[1];
  pn.t.z = pn.t.z + Nd[2] * noise[2];
  float roll, pitch, yaw;
  quat_to_euler(pn.R, roll, pitch, yaw);
  roll = roll + Nd[3] * noise[3];
  pitch = pitch + Nd[4] * noise[4];
  yaw = yaw + Nd[5] * noise[5];
  pn.R = euler_to_quat(roll, pitch, yaw);
  return pn;
}

// how far the copy moved: t2 = |dt|^2 (l2normSquared) and the reference's rotation distance, the norm of the difference quaternion
__device__ __forceinline__ void pose_distances(const xform& pose, const xform& pn, float& t2, float& rot_dist) {
  const xform diff = xmul(xinv(pose), pn);
  t2 = (diff.t.x * diff.t.x + diff.t.y * diff.t.y) + diff.t.z * diff.t.z;
  rot_dist = sqrtf(((diff.R.w * diff.R.w + diff.R.x * diff.R.x) + diff.R.y * diff.R.y) + diff.R.z * diff.R.z);
}

// the tournament's rule (resampling.cu:170-188): the larger of the two forget rates; trans_dist_metric 1 measures |dt|^2
__device__ __forceinline__ float remember_rate_max(const ResampleConfig& cfg, float t2, float rot_dist) {
  const float trans_dist = (cfg.trans_dist_metric == 1u) ? t2 : sqrtf(t2);
  const float frs = static_cast<float>(1.0 - pow(1.0 - static_cast<double>(cfg.likelihood_forget_per_meter), static_cast<double>(trans_dist)));
  const float frr = static_cast<float>(1.0 - pow(1.0 - static_cast<double>(cfg.likelihood_forget_per_radian), static_cast<double>(rot_dist)));
  const float forget_rate = (frs > frr) ? frs : frr;
  return static_cast<float>(1.0 - static_cast<double>(forget_rate));
}

// the residual resampler's rule (ResidualResamplerCPU.cpp:164-170): the product of the two, over |dt|^2
__device__ __forceinline__ float remember_rate_product(const ResampleConfig& cfg, float t2, float rot_dist) {
  return static_cast<float>(pow(static_cast<double>(cfg.likelihood_forget_per_meter), static_cast<double>(t2))) *
         static_cast<float>(pow(static_cast<double>(cfg.likelihood_forget_per_radian), static_cast<double>(rot_dist)));
}

// ---------------------------------------------------------------------------------------------
// likelihood statistics
// ---------------------------------------------------------------------------------------------
// simple_stats_kernel (resampling.cu:41-81): {sum, max} of likelihood.mean; max seeded with 0 like the reference's
// shared-memory init, sum accumulated in double.  Stage 1: <=256 blocks of grid-stride partials; stage 2: one wave.
// likelihoods: `first` + i * stride floats -- the likelihood.mean members of an attribute array (stride 9) or a dense weight vector
// (stride 1: what the sharded filter's all-gather leaves on every rank); the summation order depends on n alone, so both forms of the
// same n values give the same bits
__global__ void __launch_bounds__(kBlock) k_likelihood_stats_partial(const float* __restrict__ first, uint32_t stride, uint32_t n,
                                                                     double* __restrict__ psum, float* __restrict__ pmax) {
  __shared__ double s_sum[4];
  __shared__ float s_max[4];
  double sum = 0.0;
  float mx = 0.0f;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float L = first[static_cast<size_t>(i) * stride];
    sum += static_cast<double>(L);
    mx = (L > mx) ? L : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off);
    const float o = __shfl_down(mx, off);
    mx = (o > mx) ? o : mx;
  }
  if ((threadIdx.x & 63u) == 0u) { s_sum[threadIdx.x >> 6] = sum; s_max[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    pmax[blockIdx.x] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  }
}

__global__ void __launch_bounds__(64) k_likelihood_stats_final(const double* __restrict__ psum, const float* __restrict__ pmax,
                                                               uint32_t nblocks, float* __restrict__ out) {
  double sum = 0.0;
  float mx = 0.0f;
  for (uint32_t i = threadIdx.x; i < nblocks; i += 64u) {
    sum += psum[i];
    mx = fmaxf(mx, pmax[i]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off);
    mx = fmaxf(mx, __shfl_down(mx, off));
  }
  if (threadIdx.x == 0) { out[0] = static_cast<float>(sum); out[1] = mx; }
}

__global__ void k_pf_extract_weights(const pattr36* __restrict__ attrs, uint32_t n, float* __restrict__ w) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = attrs[i].mean;
}

// ---------------------------------------------------------------------------------------------
// gladiator resampling (resampling.cu:41-219)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_gladiator_resample(const xform* __restrict__ poses, const pattr36* __restrict__ attrs,
                                                               uint32_t n, xform* __restrict__ poses_new,
                                                               pattr36* __restrict__ attrs_new, uint32_t first, uint32_t count,
                                                               ResampleConfig cfg, uint32_t key0, uint32_t key1,
                                                               uint32_t step) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t champion = first + k;
  uint32_t ra[4], rb[4];
  philox4x32_10(champion, step, 0u, 0u, key0, key1, ra);
  philox4x32_10(champion, step, 1u, 0u, key0, key1, rb);
  const uint32_t enemy = ra[0] % n;
  const float Lc = attrs[champion].mean, Le = attrs[enemy].mean;
  if (Le > Lc) {
    float Nd[6], t2, rot_dist;
    six_gaussians<1>(ra, rb, Nd);
    const xform pose = poses[enemy];
    pattr36 an = attrs[enemy];
    const xform pn = perturbed_pose(pose, Nd, cfg.min_noise);
    pose_distances(pose, pn, t2, rot_dist);
    an.n_meas = n_meas_scaled(an.n_meas, remember_rate_max(cfg, t2, rot_dist));
    poses_new[k] = pn;
    attrs_new[k] = an;
  } else {
    poses_new[k] = poses[champion];
    attrs_new[k] = attrs[champion];
  }
}

// ---------------------------------------------------------------------------------------------
// residual resampling (ResidualResamplerCPU.cpp:55-203) -- the reference's SEQUENTIAL loop "draw a particle, insert
// size_t(L / sum * N_new) perturbed copies, until the new cloud is full" as four data-parallel passes over a block of draws:
//   counts   c_k = copies draw k inserts (the draw's particle and its share; independent of every other draw),
//   scan     inclusive prefix sums of c_k (64-bit): draw k fills slots [incl_k - c_k, incl_k),
//   fill     slot j finds its draw by binary search, perturbs the copy with ITS Gaussians (Philox counter = slot index).
// Same stream, same arithmetic as oracle/rmcl_oracle.c: orc_residual_resample (which restates the loop statement by statement):
// particles, likelihoods and n_meas bit-exact, poses to float rounding of the double-evaluated transcendentals.
// ---------------------------------------------------------------------------------------------
struct ResidualStats {
  double sum, max;
  unsigned long long expect;   // sum over the particles of their share's integer part = n * E[c_k]
  unsigned long long n_draws;  // written by k_residual_fill: draws the sequential loop would have used
};

__global__ void __launch_bounds__(64) k_residual_stats_final(const double* __restrict__ psum, const float* __restrict__ pmax,
                                                            uint32_t nblocks, ResidualStats* __restrict__ out) {
  // fixed order: lane l sums blocks l, l + 64, ...; then a fixed butterfly
  double s = 0.0;
  float m = 0.0f;
  for (uint32_t b = threadIdx.x; b < nblocks; b += 64u) { s += psum[b]; m = fmaxf(m, pmax[b]); }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off);
    m = fmaxf(m, __shfl_down(m, off));
  }
  if (threadIdx.x == 0) { out->sum = s; out->max = static_cast<double>(m); out->expect = 0ull; out->n_draws = 0ull; }
}

// copies a draw of particle likelihood L inserts when `left` slots are free: the reference's size_t(L / sum * N_new), clamped
__device__ __forceinline__ uint32_t residual_share(float Lf, double weight_sum, uint32_t n_new) {
  const double share = (static_cast<double>(Lf) / weight_sum) * static_cast<double>(n_new);
  if (!(share > 0.0)) return 0u;
  return (share >= static_cast<double>(n_new)) ? n_new : static_cast<uint32_t>(share);
}

__global__ void __launch_bounds__(kBlock) k_residual_expect(const pattr36* __restrict__ attrs, uint32_t n, uint32_t n_new,
                                                            ResidualStats* __restrict__ st) {
  __shared__ unsigned long long s_part[4];
  const double sum = st->sum;
  unsigned long long acc = 0ull;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    acc += residual_share(attrs[i].mean, sum, n_new);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&st->expect, (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));   // integers: order independent
}

__global__ void __launch_bounds__(kBlock) k_residual_counts(const pattr36* __restrict__ attrs, uint32_t n, uint32_t n_new,
                                                            const ResidualStats* __restrict__ st, uint32_t n_draws, uint32_t key0,
                                                            uint32_t key1, uint32_t step, uint32_t* __restrict__ idx_out,
                                                            uint32_t* __restrict__ cnt_out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_draws) return;
  uint32_t r[4];
  philox4x32_10(k, step, 2u, 0u, key0, key1, r);
  const uint32_t random_index = r[0] % n;
  idx_out[k] = random_index;
  cnt_out[k] = residual_share(attrs[random_index].mean, st->sum, n_new);
}

__global__ void __launch_bounds__(kBlock) k_residual_fill(const xform* __restrict__ poses, const pattr36* __restrict__ attrs,
                                                          const uint32_t* __restrict__ draw_idx, const unsigned long long* __restrict__ incl,
                                                          uint32_t n_draws, xform* __restrict__ poses_new, pattr36* __restrict__ attrs_new,
                                                          uint32_t n_new, uint32_t first, uint32_t count, ResampleConfig cfg,
                                                          ResidualStats* __restrict__ st, uint32_t key0, uint32_t key1, uint32_t step) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint32_t j = first + t;                 // global output slot
  // the draw that fills slot j: the first k with incl[k] > j (the host launches this only when incl[n_draws - 1] >= n_new)
  uint32_t lo = 0u, hi = n_draws - 1u;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (incl[mid] > static_cast<unsigned long long>(j)) hi = mid; else lo = mid + 1u;
  }
  const uint32_t k = lo;
  if (j + 1u == n_new) st->n_draws = static_cast<unsigned long long>(k) + 1ull;   // the sequential loop stops after this draw
  const uint32_t src = draw_idx[k];
  const xform pose = poses[src];
  pattr36 an = attrs[src];
  const double L_max_normed = static_cast<double>(an.mean) / st->max;
  uint32_t ra[4], rb[4];
  philox4x32_10(j, step, 3u, 0u, key0, key1, ra);
  philox4x32_10(j, step, 4u, 0u, key0, key1, rb);
  float Nd[6], noise[6], t2, rot_dist;
  six_gaussians<0>(ra, rb, Nd);
#pragma unroll
  for (int d = 0; d < 6; ++d) noise[d] = static_cast<float>(static_cast<double>(cfg.min_noise[d]) / L_max_normed);
  const xform pn = perturbed_pose(pose, Nd, noise);
  pose_distances(pose, pn, t2, rot_dist);
  an.n_meas = n_meas_scaled(an.n_meas, remember_rate_product(cfg, t2, rot_dist));
  poses_new[t] = pn;
  attrs_new[t] = an;
}

// ---------------------------------------------------------------------------------------------
// the scan: inclusive 64-bit prefix sums in three passes, 1024 elements per block -> block totals -> totals scanned by ONE block ->
// added back.  (The residual resampler's counts are <= N_new each, so 32 bits would overflow for peaked weights.)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long block_scan_256(unsigned long long v, unsigned long long* s_wave, unsigned long long& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off, 64);
    if (lane >= static_cast<uint32_t>(off)) incl += o;
  }
  if (lane == 63u) s_wave[wave] = incl;
  __syncthreads();
  unsigned long long base = 0ull;
  for (uint32_t w = 0; w < wave; ++w) base += s_wave[w];
  total = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
  __syncthreads();
  return base + incl;
}

// what the first pass scans: element i of ...
struct ScanCounts {    // ... the residual resampler's copy counts
  const uint32_t* __restrict__ cnt;
  __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return cnt[i]; }
};
struct ScanWeights {   // ... the systematic resampler's integer weights (sys_weight: kld_bins.hip.h, shared with hypotheses.hip)
  const pattr36* __restrict__ attrs;
  double max_l;
  __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return sys_weight(attrs[i].mean, max_l); }
};
struct ScanFaceAreas {   // ... the surface sampler's integer weights w_f = uint64(rint(a_f / a_max * 2^32)); a_f <= a_max: w_f <= 2^32
  const double* __restrict__ area;               // a_f of an eligible face, -1 of any other (surface_sample.hip)
  const unsigned long long* __restrict__ amax_bits;
  __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const {
    const double a = area[i], a_max = __longlong_as_double(static_cast<long long>(*amax_bits));
    if (!(a > 0.0) || !(a <= a_max)) return 0ull;   // not eligible, zero, NaN or +inf (a_max is the largest FINITE area)
    return static_cast<unsigned long long>(rint(a / a_max * 4294967296.0));
  }
};

template <typename Load>
__global__ void __launch_bounds__(kBlock) k_scan_blocks(Load load, uint32_t n, unsigned long long* __restrict__ incl,
                                                        unsigned long long* __restrict__ block_total) {
  __shared__ unsigned long long s_wave[4];
  const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * 1024ull + threadIdx.x * 4u;
  unsigned long long c[4];
#pragma unroll
  for (uint32_t u = 0; u < 4u; ++u) c[u] = (base + u < n) ? load(base + u) : 0ull;
  const unsigned long long mine = (c[0] + c[1]) + (c[2] + c[3]);
  unsigned long long total;
  const unsigned long long end = block_scan_256(mine, s_wave, total);   // inclusive over the threads
  unsigned long long run = end - mine;
#pragma unroll
  for (uint32_t u = 0; u < 4u; ++u) {
    run += c[u];
    if (base + u < n) incl[base + u] = run;
  }
  if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock) k_scan_totals(unsigned long long* __restrict__ block_total, uint32_t nblocks) {
  __shared__ unsigned long long s_wave[4];
  unsigned long long carry = 0ull;
  for (uint32_t b0 = 0; b0 < nblocks; b0 += kBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const unsigned long long v = (b < nblocks) ? block_total[b] : 0ull;
    unsigned long long total;
    const unsigned long long inc = block_scan_256(v, s_wave, total);
    if (b < nblocks) block_total[b] = carry + inc - v;   // exclusive: what precedes block b
    carry += total;
  }
}

__global__ void __launch_bounds__(kBlock) k_scan_add(unsigned long long* __restrict__ incl, uint32_t n, const unsigned long long* __restrict__ block_excl) {
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) incl[i] += block_excl[i >> 10];
}

inline uint32_t blocks_of(uint32_t n, uint32_t per_block) { return static_cast<uint32_t>((static_cast<uint64_t>(n) + per_block - 1u) / per_block); }

// the first pass always; the other two unless `single_block_is_done` and one block held everything
template <typename Load>
void launch_scan(Load load, uint32_t n, unsigned long long* incl, unsigned long long* block_tot, bool single_block_is_done, hipStream_t s) {
  const uint32_t nb = blocks_of(n, 1024u);
  hipLaunchKernelGGL(k_scan_blocks<Load>, dim3(nb), dim3(kBlock), 0, s, load, n, incl, block_tot);
  if (single_block_is_done && nb == 1u) return;
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(kBlock), 0, s, block_tot, nb);
  hipLaunchKernelGGL(k_scan_add, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, s, incl, n, block_tot);
}

// ---------------------------------------------------------------------------------------------
// systematic resampling
// ---------------------------------------------------------------------------------------------
// source of slot j: the first i with incl[i] > pos_j, pos_j = min(T - 1, floor((j + u0) * (T / n_new)))   (T >= 2^24: the caller
// refuses a cloud without a positive finite maximum, and the particle that holds it weighs 2^24)
__device__ __forceinline__ uint32_t sys_source(const unsigned long long* __restrict__ incl, uint32_t n, unsigned long long T, double scale,
                                               double u0, uint32_t j) {
  unsigned long long pos = static_cast<unsigned long long>(floor((static_cast<double>(j) + u0) * scale));
  if (pos > T - 1ull) pos = T - 1ull;
  uint32_t lo = 0u, hi = n - 1u;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (incl[mid] > pos) hi = mid; else lo = mid + 1u;
  }
  return lo;
}

__global__ void __launch_bounds__(kBlock) k_sys_fill(const xform* __restrict__ poses, const pattr36* __restrict__ attrs,
                                                     const unsigned long long* __restrict__ incl, uint32_t n, xform* __restrict__ poses_new,
                                                     pattr36* __restrict__ attrs_new, uint32_t n_new, uint32_t first, uint32_t count, ResampleConfig cfg,
                                                     uint32_t key0, uint32_t key1, uint32_t step) {
  __shared__ uint32_t s_src[kBlock];
  const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = t < count;
  const uint32_t j = first + static_cast<uint32_t>(live ? t : 0ull);   // global slot (first + count <= n_new: no wrap)
  uint32_t r0[4];
  philox4x32_10(0u, step, 5u, 0u, key0, key1, r0);
  const double u0 = (static_cast<double>(r0[0]) + 0.5) * (1.0 / 4294967296.0);
  const unsigned long long T = incl[n - 1u];
  const double scale = static_cast<double>(T) / static_cast<double>(n_new);
  const uint32_t src = sys_source(incl, n, T, scale, u0, j);
  s_src[threadIdx.x] = src;
  __syncthreads();
  if (!live) return;
  // the slot before this one: a neighbour's search, or -- for the block's first lane -- its own (a call that starts at first > 0
  // finds the source of slot first - 1 the same way)
  bool first_of_run = (j == 0u);
  if (!first_of_run) {
    const uint32_t prev = (threadIdx.x > 0u) ? s_src[threadIdx.x - 1u] : sys_source(incl, n, T, scale, u0, j - 1u);
    first_of_run = prev != src;
  }
  const xform pose = poses[src];
  pattr36 an = attrs[src];
  if (first_of_run) {
    poses_new[t] = pose;
    attrs_new[t] = an;
    return;
  }
  // every further copy: the gladiator's winning enemy, Gaussians of slot j from draws 6 and 7
  uint32_t ra[4], rb[4];
  philox4x32_10(j, step, 6u, 0u, key0, key1, ra);
  philox4x32_10(j, step, 7u, 0u, key0, key1, rb);
  float Nd[6], t2, rot_dist;
  six_gaussians<1>(ra, rb, Nd);
  const xform pn = perturbed_pose(pose, Nd, cfg.min_noise);
  pose_distances(pose, pn, t2, rot_dist);
  an.n_meas = n_meas_scaled(an.n_meas, remember_rate_max(cfg, t2, rot_dist));
  poses_new[t] = pn;
  attrs_new[t] = an;
}

// first: likelihood.mean of particle 0, the first float of a 9-float record, or a dense vector (stride 1)
hipError_t likelihood_stats(const float* first, uint32_t stride, uint32_t n, double* psum, float* pmax, float* out2, hipStream_t s) {
  const uint32_t nblocks = partial_blocks(n);
  hipLaunchKernelGGL(k_likelihood_stats_partial, dim3(nblocks), dim3(kBlock), 0, s, first, stride, n, psum, pmax);
  hipLaunchKernelGGL(k_likelihood_stats_final, dim3(1), dim3(64), 0, s, psum, pmax, nblocks, out2);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pf_extract_weights(const void* attrs, uint32_t n, float* weights, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pf_extract_weights, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, s, static_cast<const pattr36*>(attrs), n, weights);
  return hipGetLastError();
}

hipError_t launch_likelihood_stats(const void* attrs, uint32_t n, double* psum, float* pmax, float* out2, hipStream_t s) {
  static_assert(sizeof(pattr36) == 36 && offsetof(pattr36, mean) == 0, "likelihood.mean is the first float of a 9-float record");
  return likelihood_stats(static_cast<const float*>(attrs), 9u, n, psum, pmax, out2, s);
}

// the same blocks, the same order, the same bits
hipError_t launch_likelihood_stats_dense(const float* weights, uint32_t n, double* psum, float* pmax, float* out2, hipStream_t s) {
  return likelihood_stats(weights, 1u, n, psum, pmax, out2, s);
}

hipError_t launch_gladiator_resample(const xform* poses, const void* attrs, uint32_t n, xform* poses_new, void* attrs_new,
                                     uint32_t first, uint32_t count, const float* cfg8, uint32_t trans_dist_metric,
                                     uint64_t seed, uint32_t step, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_gladiator_resample, dim3(blocks_of(count, kBlock)), dim3(kBlock), 0, s, poses, static_cast<const pattr36*>(attrs), n,
                     poses_new, static_cast<pattr36*>(attrs_new), first, count, resample_config(cfg8, trans_dist_metric),
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), step);
  return hipGetLastError();
}

// residual resampling, step 1: {sum, max} in double + the expected number of copies per draw (x n) -> *stats (device)
hipError_t launch_residual_prepare(const void* attrs, uint32_t n, uint32_t n_new, double* psum, float* pmax, void* stats, hipStream_t s) {
  const uint32_t nblocks = partial_blocks(n);
  hipLaunchKernelGGL(k_likelihood_stats_partial, dim3(nblocks), dim3(kBlock), 0, s, static_cast<const float*>(attrs), 9u, n, psum, pmax);
  hipLaunchKernelGGL(k_residual_stats_final, dim3(1), dim3(64), 0, s, psum, pmax, nblocks, static_cast<ResidualStats*>(stats));
  hipLaunchKernelGGL(k_residual_expect, dim3(nblocks), dim3(kBlock), 0, s, static_cast<const pattr36*>(attrs), n, n_new,
                     static_cast<ResidualStats*>(stats));
  return hipGetLastError();
}

// step 2: the particle and the copy count of draws 0 .. n_draws-1 and the inclusive prefix sums of the counts
hipError_t launch_residual_draws(const void* attrs, uint32_t n, uint32_t n_new, const void* stats, uint32_t n_draws, uint64_t seed,
                                 uint32_t step, uint32_t* draw_idx, uint32_t* draw_cnt, unsigned long long* incl,
                                 unsigned long long* block_tot, hipStream_t s) {
  if (n_draws == 0) return hipSuccess;
  hipLaunchKernelGGL(k_residual_counts, dim3(blocks_of(n_draws, kBlock)), dim3(kBlock), 0, s, static_cast<const pattr36*>(attrs), n, n_new,
                     static_cast<const ResidualStats*>(stats), n_draws, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                     step, draw_idx, draw_cnt);
  // all three passes whatever n_draws is: the launches this call has always made
  launch_scan(ScanCounts{draw_cnt}, n_draws, incl, block_tot, false, s);
  return hipGetLastError();
}

// step 3: slots first .. first+count-1 of the new cloud -> poses_new / attrs_new [0 .. count)
hipError_t launch_residual_fill(const xform* poses, const void* attrs, const uint32_t* draw_idx, const unsigned long long* incl,
                                uint32_t n_draws, xform* poses_new, void* attrs_new, uint32_t n_new, uint32_t first, uint32_t count,
                                const float* cfg8, void* stats, uint64_t seed, uint32_t step, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_residual_fill, dim3(blocks_of(count, kBlock)), dim3(kBlock), 0, s, poses, static_cast<const pattr36*>(attrs), draw_idx,
                     incl, n_draws, poses_new, static_cast<pattr36*>(attrs_new), n_new, first, count, resample_config(cfg8, 1u),
                     static_cast<ResidualStats*>(stats), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), step);
  return hipGetLastError();
}

hipError_t launch_sys_scan(const void* attrs, uint32_t n, double max_l, unsigned long long* incl, unsigned long long* block_tot, hipStream_t s) {
  if (n == 0) return hipSuccess;
  // a cloud of at most 1024 particles is scanned by the first pass alone: this call has always skipped the other two then
  launch_scan(ScanWeights{static_cast<const pattr36*>(attrs), max_l}, n, incl, block_tot, true, s);
  return hipGetLastError();
}

// the same three kernels over plain counts (stein.hip: the listed particles of every word of the cell list's table)
hipError_t launch_scan_counts(const uint32_t* counts, uint32_t n, unsigned long long* incl, unsigned long long* block_tot, hipStream_t s) {
  if (n == 0) return hipSuccess;
  launch_scan(ScanCounts{counts}, n, incl, block_tot, true, s);
  return hipGetLastError();
}

// ... and over the surface sampler's face weights: all three passes whatever n_faces is
hipError_t launch_surface_sample_scan(const double* area, const unsigned long long* amax_bits, uint32_t n_faces, unsigned long long* incl,
                                      unsigned long long* block_tot, hipStream_t s) {
  if (n_faces == 0) return hipSuccess;
  launch_scan(ScanFaceAreas{area, amax_bits}, n_faces, incl, block_tot, false, s);
  return hipGetLastError();
}

hipError_t launch_sys_fill(const xform* poses, const void* attrs, const unsigned long long* incl, uint32_t n, xform* poses_new, void* attrs_new,
                           uint32_t n_new, uint32_t first, uint32_t count, const float* cfg8, uint32_t trans_dist_metric, uint64_t seed,
                           uint32_t step, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (n == 0 || n_new == 0 || static_cast<uint64_t>(first) + count > n_new) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sys_fill, dim3(blocks_of(count, kBlock)), dim3(kBlock), 0, s, poses, static_cast<const pattr36*>(attrs), incl, n,
                     poses_new, static_cast<pattr36*>(attrs_new), n_new, first, count, resample_config(cfg8, trans_dist_metric),
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), step);
  return hipGetLastError();
}

}  // namespace rmclhip
