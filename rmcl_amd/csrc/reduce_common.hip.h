// reduce_common.hip.h -- what the point-to-plane reduction (kernels.hip: k_reduce_partials, k_reduce_finalize, k_batch_solve) and
// the MICP iterations (micp.hip) both need: the 16 raw sums of rm::statistics_p2l (CorrespondencesCPU.cpp:26-30; gate
// MICPSensorCPU.cpp:70-84) and how one correspondence enters them, the wave that turns partial rows into CrossStatistics, the
// completion tag of a launch chain the host polls, and the length of a moment row.
#pragma once
#include "kernels.h"

namespace rmclhip {
namespace {

constexpr int kAcc = 16;  // sd[3] sm[3] smd[9] cnt
constexpr int kMom = 96;  // a moment row (micp.hip, find_kernel.hip.h): n | D[3] | DD[6] | sN[3] | sND[9] | NN[6] | NND[18] | NNDD[36]
constexpr uint32_t kMomUsed = 82;   // columns of a moment row that carry a moment

// One correspondence of statistics_p2l: dataset point D under the pre-transform, model point I and normal N, into the 16 sums.
// The f32 expressions and the order of the f64 additions are the reduction's contract (micp_host.h restates them for the host).
__device__ __forceinline__ void p2l_accumulate(const xform& Tpre, f3 D, f3 Ii, f3 Ni, float max_dist, double* acc) {
  const f3 Di = xapply(Tpre, D);
  const float spd = dot_plain(sub3(Ii, Di), Ni);
  if (fabsf(spd) < max_dist) {
    const f3 Mi = add3(Di, scale3(Ni, spd));
    const double d[3] = {Di.x, Di.y, Di.z}, m[3] = {Mi.x, Mi.y, Mi.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc[k] += d[k]; acc[3 + k] += m[k]; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[6 + 3 * r + c] += m[r] * d[c];
    acc[15] += 1.0;
  }
}
// ... from the three arrays, element i
__device__ __forceinline__ void p2l_accumulate(const xform& Tpre, const float* dataset_points, const float* model_points,
                                               const float* model_normals, size_t i, float max_dist, double* acc) {
  const float* dp = dataset_points + 3 * i;
  const float* mp = model_points + 3 * i;
  const float* mn = model_normals + 3 * i;
  p2l_accumulate(Tpre, mk3(dp[0], dp[1], dp[2]), mk3(mp[0], mp[1], mp[2]), mk3(mn[0], mn[1], mn[2]), max_dist, acc);
}

// sum the per-block partials of one pose (one wave) and turn the raw moments into CrossStatistics
__device__ __forceinline__ cstats finalize_pose(const double* partials, uint32_t nblocks) {
  // transposed reduction: lane = 16*g + k sums moment k over the blocks b = g, g+4, ... (16 lanes read one
  // 128-B partial: coalesced), then only TWO cross-lane steps (xor 16, 32) for one double per lane and 16
  // v_readlane broadcasts -- instead of 16 moments x 6 butterfly steps = 192 dependent ds_bpermute (measured
  // ~4.5 us of a 14 us solve step)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k0 = lane & 15u, g = lane >> 4;
  // 32 loads in flight per lane: every batch is one L2 round trip (~0.8 us) for this lone wave, so 256 partials
  // cost two round trips (8 in flight: 8 round trips, measured 6 us of the 11 us solve step; one load per
  // iteration serialised 64 round trips)
  double a = 0.0;
  uint32_t b = g;
  for (; b + 124u < nblocks; b += 128u) {
    double v[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) v[u] = partials[static_cast<size_t>(b + 4u * u) * kAcc + k0];
#pragma unroll
    for (int u = 0; u < 32; u += 8) a += ((v[u] + v[u + 1]) + (v[u + 2] + v[u + 3])) + ((v[u + 4] + v[u + 5]) + (v[u + 6] + v[u + 7]));
  }
  for (; b + 28u < nblocks; b += 32u) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partials[static_cast<size_t>(b + 4u * u) * kAcc + k0];
    a += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  }
  for (; b < nblocks; b += 4u) a += partials[static_cast<size_t>(b) * kAcc + k0];
  a += __shfl_xor(a, 16, 64);
  a += __shfl_xor(a, 32, 64);
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = __shfl(a, k, 64);
  cstats s = cs_identity();
  const double n = acc[15];
  if (n > 0.0) {
    const double md[3] = {acc[0] / n, acc[1] / n, acc[2] / n};
    const double mm[3] = {acc[3] / n, acc[4] / n, acc[5] / n};
    s.dataset_mean = mk3(static_cast<float>(md[0]), static_cast<float>(md[1]), static_cast<float>(md[2]));
    s.model_mean = mk3(static_cast<float>(mm[0]), static_cast<float>(mm[1]), static_cast<float>(mm[2]));
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) s.covariance[3 * r + c] = static_cast<float>(acc[6 + 3 * r + c] / n - mm[r] * md[c]);
    // ONE correspondence has no covariance.  The streaming sums give exactly that; sums evaluated from the moments leave their own
    // rounding (~1e-15) instead, a matrix of noise the solve would turn into an arbitrary rotation
    if (n == 1.0)
      for (int k = 0; k < 9; ++k) s.covariance[k] = 0.0f;
    s.n_meas = static_cast<uint32_t>(n);
  }
  return s;
}

// Completion tag of a launch chain whose results go to host-mapped memory and whose caller polls instead of waiting for the
// stream: ONE 8-byte store {seq, xor of every result word}, issued after the results and a system-scope fence.  The SEQUENCE NUMBER
// is what makes the hand-off sound: round 2's form polled a flag the host itself had cleared before the launch -- the same value
// every call -- and about 1 call in 10^4 took the previous call's results (tools/determinism2.py).  Round 5 isolated the mechanism
// (tools/ubench/tag_handoff.hip, tools/tag_retries.py, profiles/r05_tag_handoff.txt): with a per-call value the device's
// "results, __threadfence_system(), tag" order has never been seen violated (6 x 10^6 isolated hand-offs across allocations and
// pinning flags, 9 x 10^5 product calls, not one checksum rejection) -- the failure belonged to the reused flag, not to the store
// order.  The xor stays as a belt: the host accepts a result only when the tag carries this call's sequence number AND the words it
// reads add up to the tag's sum (capi_rcc.cpp wait_done), and keeps polling otherwise.
template <typename Tp>
__device__ __forceinline__ uint32_t xor_words(const Tp& v) {
  static_assert(sizeof(Tp) % 4 == 0, "word-sized results only");
  uint32_t w[sizeof(Tp) / 4];
  __builtin_memcpy(w, &v, sizeof(Tp));
  uint32_t x = 0;
#pragma unroll
  for (uint32_t i = 0; i < sizeof(Tp) / 4; ++i) x ^= w[i];
  return x;
}
__device__ __forceinline__ void publish_tag(unsigned long long* tag, uint32_t seq, uint32_t sum) {
  __threadfence_system();
  __hip_atomic_store(tag, (static_cast<unsigned long long>(sum) << 32) | static_cast<unsigned long long>(seq), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace
}  // namespace rmclhip
