// adaptive.hip -- a particle count that follows the posterior: the KLD-sampling bound's input, the occupied bins of pose space.  (The
// resampler that then produces ANY requested size from ANY weights -- systematic, low-variance resampling -- is in resample.hip with
// the other two.)  The reference lists this as an open item (docs/RMCL.md, Resampling TODOs); its node already adopts the count a
// resampler returns (rmcl_localization.cpp:633-639).  include/rmclhip.h states the rules; tests/adaptive_ref.py restates them in numpy.
//
//   k_kld_count_bins   one lane per particle: the 63-bit key of its bin, inserted into an open-addressing table of 64-bit words
//                      (atomicCAS, linear probing); first inserts and counted particles are summed per wave (ballot + popcount) and
//                      added with ONE vector atomicAdd per wave and counter.  The result is a number of distinct keys: the same
//                      for every schedule.
#include "kernels.h"
#include "kld_bins.hip.h"

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

}  // namespace rmclhip
