// adaptive.hip -- a particle count that follows the posterior: the KLD-sampling bound's input (occupied bins of pose space) and a
// resampler that produces ANY requested size from ANY weights (systematic, low-variance resampling).  The reference lists this as an
// open item (docs/RMCL.md, Resampling TODOs); its node already adopts the count a resampler returns (rmcl_localization.cpp:633-639).
// include/rmclhip.h states the rules; tests/adaptive_ref.py restates them in numpy.
//
//   k_kld_count_bins   one lane per particle: the 63-bit key of its bin, inserted into an open-addressing table of 64-bit words
//                      (atomicCAS, linear probing); first inserts and counted particles are summed per wave (ballot + popcount) and
//                      added with ONE vector atomicAdd per wave and counter.  The result is a number of distinct keys: the same
//                      for every schedule.
//   k_sys_weights_scan / k_sys_scan_totals / k_sys_scan_add
//                      integer weights w_i = rint(L_i / max * 2^24) and their inclusive 64-bit prefix sums C (1024 per block ->
//                      block totals -> totals scanned by one block -> added back; the shape of the residual resampler's scan).
//                      Integers: C is exact and independent of the launch shape.
//   k_sys_fill         slot j reads position pos_j of [0, T), T = C[n-1]; its source is the first i with C[i] > pos_j (binary
//                      search).  The first slot of a run of equal sources is a copy, every further one is perturbed as the gladiator
//                      perturbs a winning enemy.
#include "kernels.h"
#include "kld_bins.hip.h"
#include "pf_random.hip.h"

namespace rmclhip {
namespace {

constexpr uint32_t kBlock = 256;

// ---------------------------------------------------------------------------------------------
// occupied bins (the key rule and the table's hash: kld_bins.hip.h, shared with hypotheses.hip)
// ---------------------------------------------------------------------------------------------
// counts[0] = distinct keys, counts[1] = counted particles.  table: mask + 1 words (a power of two >= 2 n), all kEmptySlot on entry.
// No lane leaves before the ballots: every wave of the launch reaches them whole.
__global__ void __launch_bounds__(kBlock) k_kld_count_bins(const xform* __restrict__ poses, const pattr36* __restrict__ attrs, uint32_t n,
                                                           KldBins b, unsigned long long* __restrict__ table, unsigned long long mask,
                                                           uint32_t* __restrict__ counts) {
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  bool counted = false, inserted = false;
  if (i < n) {
    const xform T = poses[i];
    const float L = attrs[i].mean;
    unsigned long long key = 0ull;
    counted = kld_particle_key(T, L, b, key);   // kld_bins.hip.h
    if (counted) {
      // at most n keys are ever stored and the table has >= 2 n words: a probe sequence meets its key or an empty word before it
      // has gone round, whatever the other lanes do -- the loop ends by construction
      // A word changes once, from empty to its key: a load that finds a key has found the final one and needs no atomic (a converged
      // cloud puts thousands of particles into each of a few bins -- with the compare-and-swap alone they queue on those words:
      // 11.4 ms for a million particles in one bin against 0.43 ms for a million bins, profiles/adaptive_resample_time.txt).
      unsigned long long slot = mix64(key) & mask;
      for (;;) {
        unsigned long long cur = __atomic_load_n(&table[slot], __ATOMIC_RELAXED);
        if (cur == kEmptySlot) {
          cur = atomicCAS(&table[slot], kEmptySlot, key);
          if (cur == kEmptySlot) { inserted = true; break; }
        }
        if (cur == key) break;
        slot = (slot + 1ull) & mask;
      }
    }
  }
  const unsigned long long m_ins = __ballot(inserted), m_cnt = __ballot(counted);
  if ((threadIdx.x & 63u) == 0u) {
    if (m_ins) atomicAdd(&counts[0], static_cast<uint32_t>(__popcll(m_ins)));
    if (m_cnt) atomicAdd(&counts[1], static_cast<uint32_t>(__popcll(m_cnt)));
  }
}

// ---------------------------------------------------------------------------------------------
// systematic resampling
// ---------------------------------------------------------------------------------------------
// inclusive scan over the 256 threads of a block (the residual resampler's block_scan_256)
__device__ __forceinline__ unsigned long long sys_block_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long& total) {
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

__global__ void __launch_bounds__(kBlock) k_sys_weights_scan(const pattr36* __restrict__ attrs, uint32_t n, double max_l,
                                                             unsigned long long* __restrict__ incl, unsigned long long* __restrict__ block_total) {
  __shared__ unsigned long long s_wave[4];
  const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * 1024ull + threadIdx.x * 4u;
  unsigned long long c[4];
#pragma unroll
  for (uint32_t u = 0; u < 4u; ++u) c[u] = (base + u < n) ? sys_weight(attrs[base + u].mean, max_l) : 0ull;
  const unsigned long long mine = (c[0] + c[1]) + (c[2] + c[3]);
  unsigned long long total;
  const unsigned long long end = sys_block_scan(mine, s_wave, total);
  unsigned long long run = end - mine;
#pragma unroll
  for (uint32_t u = 0; u < 4u; ++u) {
    run += c[u];
    if (base + u < n) incl[base + u] = run;
  }
  if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock) k_sys_scan_totals(unsigned long long* __restrict__ block_total, uint32_t nblocks) {
  __shared__ unsigned long long s_wave[4];
  unsigned long long carry = 0ull;
  for (uint32_t b0 = 0; b0 < nblocks; b0 += kBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const unsigned long long v = (b < nblocks) ? block_total[b] : 0ull;
    unsigned long long total;
    const unsigned long long inc = sys_block_scan(v, s_wave, total);
    if (b < nblocks) block_total[b] = carry + inc - v;   // exclusive: what precedes block b
    carry += total;
  }
}

__global__ void __launch_bounds__(kBlock) k_sys_scan_add(unsigned long long* __restrict__ incl, uint32_t n, const unsigned long long* __restrict__ block_excl) {
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) incl[i] += block_excl[i >> 10];
}

struct SysConfig {
  float min_noise_tx, min_noise_ty, min_noise_tz, min_noise_roll, min_noise_pitch, min_noise_yaw;
  float likelihood_forget_per_meter, likelihood_forget_per_radian;
  uint32_t trans_dist_metric;
};

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
                                                     pattr36* __restrict__ attrs_new, uint32_t n_new, uint32_t first, uint32_t count, SysConfig cfg,
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
  // every further copy: the gladiator's winning enemy (kernels.hip, k_gladiator_resample), Gaussians of slot j from draws 6 and 7
  uint32_t ra[4], rb[4];
  philox4x32_10(j, step, 6u, 0u, key0, key1, ra);
  philox4x32_10(j, step, 7u, 0u, key0, key1, rb);
  float Nd_tx, Nd_ty, Nd_tz, Nd_rx, Nd_ry, Nd_rz;
  box_muller(ra[1], ra[2], Nd_tx, Nd_ty);
  box_muller(ra[3], rb[0], Nd_tz, Nd_rx);
  box_muller(rb[1], rb[2], Nd_ry, Nd_rz);
  xform pn = pose;
  pn.t.x = pn.t.x + Nd_tx * cfg.min_noise_tx;
  pn.t.y = pn.t.y + Nd_ty * cfg.min_noise_ty;
  pn.t.z = pn.t.z + Nd_tz * cfg.min_noise_tz;
  float roll, pitch, yaw;
  quat_to_euler(pn.R, roll, pitch, yaw);
  roll = roll + Nd_rx * cfg.min_noise_roll;
  pitch = pitch + Nd_ry * cfg.min_noise_pitch;
  yaw = yaw + Nd_rz * cfg.min_noise_yaw;
  pn.R = euler_to_quat(roll, pitch, yaw);
  const xform diff = xmul(xinv(pose), pn);
  const float t2 = (diff.t.x * diff.t.x + diff.t.y * diff.t.y) + diff.t.z * diff.t.z;
  const float trans_dist = (cfg.trans_dist_metric == 1u) ? t2 : sqrtf(t2);
  const float rot_dist = sqrtf(((diff.R.w * diff.R.w + diff.R.x * diff.R.x) + diff.R.y * diff.R.y) + diff.R.z * diff.R.z);
  const float frs = static_cast<float>(1.0 - pow(1.0 - static_cast<double>(cfg.likelihood_forget_per_meter), static_cast<double>(trans_dist)));
  const float frr = static_cast<float>(1.0 - pow(1.0 - static_cast<double>(cfg.likelihood_forget_per_radian), static_cast<double>(rot_dist)));
  const float forget_rate = (frs > frr) ? frs : frr;
  const float remember_rate = static_cast<float>(1.0 - static_cast<double>(forget_rate));
  an.n_meas = n_meas_scaled(an.n_meas, remember_rate);
  poses_new[t] = pn;
  attrs_new[t] = an;
}

}  // namespace

hipError_t launch_kld_count_bins(const xform* poses, const void* attrs, uint32_t n, const float* bin_xyz, const float* bin_rpy, float floor_l,
                                 unsigned long long* table, uint64_t table_words, uint32_t* counts2, hipStream_t s) {
  if (n == 0) return hipSuccess;
  // a power of two >= 2 n: the probe loop's guarantee of an empty word
  if (table_words < 2ull * n || (table_words & (table_words - 1ull)) != 0ull) return hipErrorInvalidValue;
  KldBins b;
  for (int d = 0; d < 3; ++d) { b.bin_xyz[d] = bin_xyz[d]; b.bin_rpy[d] = bin_rpy[d]; }
  b.floor_l = floor_l;
  hipLaunchKernelGGL(k_kld_count_bins, dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock)), dim3(kBlock), 0, s, poses,
                     static_cast<const pattr36*>(attrs), n, b, table, static_cast<unsigned long long>(table_words - 1ull), counts2);
  return hipGetLastError();
}

hipError_t launch_sys_scan(const void* attrs, uint32_t n, double max_l, unsigned long long* incl, unsigned long long* block_tot, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t nb = static_cast<uint32_t>((static_cast<uint64_t>(n) + 1023u) / 1024u);
  hipLaunchKernelGGL(k_sys_weights_scan, dim3(nb), dim3(kBlock), 0, s, static_cast<const pattr36*>(attrs), n, max_l, incl, block_tot);
  if (nb > 1u) {
    hipLaunchKernelGGL(k_sys_scan_totals, dim3(1), dim3(kBlock), 0, s, block_tot, nb);
    hipLaunchKernelGGL(k_sys_scan_add, dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock)), dim3(kBlock), 0, s, incl, n, block_tot);
  }
  return hipGetLastError();
}

hipError_t launch_sys_fill(const xform* poses, const void* attrs, const unsigned long long* incl, uint32_t n, xform* poses_new, void* attrs_new,
                           uint32_t n_new, uint32_t first, uint32_t count, const float* cfg8, uint32_t trans_dist_metric, uint64_t seed,
                           uint32_t step, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (n == 0 || n_new == 0 || static_cast<uint64_t>(first) + count > n_new) return hipErrorInvalidValue;
  SysConfig cfg{cfg8[0], cfg8[1], cfg8[2], cfg8[3], cfg8[4], cfg8[5], cfg8[6], cfg8[7], trans_dist_metric};
  hipLaunchKernelGGL(k_sys_fill, dim3(static_cast<uint32_t>((static_cast<uint64_t>(count) + kBlock - 1u) / kBlock)), dim3(kBlock), 0, s, poses,
                     static_cast<const pattr36*>(attrs), incl, n, poses_new, static_cast<pattr36*>(attrs_new), n_new, first, count, cfg,
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), step);
  return hipGetLastError();
}

}  // namespace rmclhip
