// kld_bins.hip.h -- the bin of a particle (include/rmclhip.h, BINS) as device code: ONE statement of the key rule for the kernel that
// fills the table of occupied bins (adaptive.hip) and the kernels that read it back (hypotheses.hip); pattr36, the particle
// attributes as these files and the resamplers (resample.hip) read them.
//   key   63 bits: x | y << 14 | z << 28 (14 bits each, index + 8192) | roll << 42 | pitch << 49 | yaw << 56 (7 bits each)
//   table open addressing over 64-bit words, linear probing from mix64(key) & mask, kEmptySlot where nothing was stored
#pragma once
#include "kernels.h"
#include "pf_random.hip.h"

namespace rmclhip {
namespace {

constexpr unsigned long long kEmptySlot = ~0ull;   // a key has bit 63 clear

struct pattr36 { float mean, sigma; uint32_t n_meas; float state_sigma[6]; };
static_assert(sizeof(pattr36) == 36, "ParticleAttributes must be 36 B");

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN and +-inf

struct KldBins { float bin_xyz[3], bin_rpy[3]; float floor_l; };

__device__ __forceinline__ unsigned long long bin_lin(float t, float width) {
  if (width == 0.0f) return 8192ull;                                   // dimension ignored: index 0
  const float f = fminf(fmaxf(floorf(t / width), -8192.0f), 8191.0f);   // (t finite, width > 0: never NaN)
  return static_cast<unsigned long long>(static_cast<int32_t>(f) + 8192);
}
__device__ __forceinline__ unsigned long long bin_ang(float a, float width) {
  if (width == 0.0f) return 0ull;
  const float f = fminf(fmaxf(floorf((a + 3.14159265358979323846f) / width), 0.0f), 126.0f);
  return static_cast<unsigned long long>(static_cast<int32_t>(f));
}

// splitmix64's finaliser: neighbouring bins differ in a few low bits of one field
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// is the particle counted, and if so the key of its bin
__device__ __forceinline__ bool kld_particle_key(const xform& T, float L, const KldBins& b, unsigned long long& key) {
  const bool counted = finite_f(T.R.x) && finite_f(T.R.y) && finite_f(T.R.z) && finite_f(T.R.w) && finite_f(T.t.x) && finite_f(T.t.y) &&
                       finite_f(T.t.z) && finite_f(L) && L > 0.0f && L >= b.floor_l;
  if (counted) {
    float roll, pitch, yaw;
    quat_to_euler(T.R, roll, pitch, yaw);
    key = bin_lin(T.t.x, b.bin_xyz[0]) | (bin_lin(T.t.y, b.bin_xyz[1]) << 14) | (bin_lin(T.t.z, b.bin_xyz[2]) << 28) |
          (bin_ang(roll, b.bin_rpy[0]) << 42) | (bin_ang(pitch, b.bin_rpy[1]) << 49) | (bin_ang(yaw, b.bin_rpy[2]) << 56);
  }
  return counted;
}

// the systematic resampler's integer weight (resample.hip); a hypothesis weighs the sum of its particles' (hypotheses.hip)
__device__ __forceinline__ unsigned long long sys_weight(float L, double max_l) {
  if (!finite_f(L) || !(L > 0.0f)) return 0ull;
  return static_cast<unsigned long long>(rint((static_cast<double>(L) / max_l) * 16777216.0));
}

}  // namespace
}  // namespace rmclhip
