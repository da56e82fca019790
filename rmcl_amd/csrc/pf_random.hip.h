// pf_random.hip.h -- the counter-based random stream of the particle filter and the Euler -> quaternion step its draws end in, shared
// by the resamplers (resample.hip), the cloud initialisation (particles.hip) and the motion update's noise (kernels.hip): ONE text, so
// that a particle drawn by any of them is the same function of (seed, counter) down to the bit.  Device code only.
//
// Random stream = Philox4x32-10 keyed by the 64-bit seed with a 128-bit counter (index, step / epoch, draw, stream):
//   stream 0: the resamplers   (champion or slot index, step, draw 0..7: gladiator 0 1, residual 2 3 4, systematic 5 6 7;
//                               particle index, step + iteration, draw 8: the Stein step's thinning of full bins, stein.hip;
//                               slot index, step, draw 9 10 11: the recovery injection -- 9 decides whether the slot is replaced,
//                               10 and 11 are the surface sampler's two blocks, particles.hip)
//   stream 1: the initialisers (global particle index, epoch, draw 0..1: uniform and pose + covariance; draw 2 3: the surface
//                               sampler's two blocks of the initialisation on the surface)
//   stream 2: the motion noise (global particle index, step, draw 0..1: the six Gaussians of the sampled odometry model,
//                               motion_noise_compose below)
// reproducible, independent of the launch shape and of how the particle range is sharded across GPUs.  Transcendentals are evaluated in
// double and rounded to float (see oracle).
#pragma once
#include "devmath.h"

namespace rmclhip {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const double u1 = (static_cast<double>(a) + 0.5) * (1.0 / 4294967296.0);
  const double u2 = (static_cast<double>(b) + 0.5) * (1.0 / 4294967296.0);
  const double r = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925 * u2;
  z0 = static_cast<float>(r * cos(ang));
  z1 = static_cast<float>(r * sin(ang));
}

// a uniform draw in [lo, hi] from one word: the initialisations' box (particles.hip) and the surface sampler's yaw (surface_sample.hip.h)
__device__ __forceinline__ float uniform_in(float lo, float hi, uint32_t w) {
  const double u = (static_cast<double>(w) + 0.5) * (1.0 / 4294967296.0);
  return static_cast<float>(static_cast<double>(lo) + (static_cast<double>(hi) - static_cast<double>(lo)) * u);   // lo == hi: lo exactly
}

// rmagine Quaternion <- EulerAngles (ZYX): cos / sin of the float half angles in double, rounded to float, then float products
__device__ __forceinline__ quat euler_to_quat(float roll, float pitch, float yaw) {
  const float cr = static_cast<float>(cos(static_cast<double>(roll / 2.0f))), sr = static_cast<float>(sin(static_cast<double>(roll / 2.0f)));
  const float cp = static_cast<float>(cos(static_cast<double>(pitch / 2.0f))), sp = static_cast<float>(sin(static_cast<double>(pitch / 2.0f)));
  const float cy = static_cast<float>(cos(static_cast<double>(yaw / 2.0f))), sy = static_cast<float>(sin(static_cast<double>(yaw / 2.0f)));
  quat q;
  q.w = cr * cp * cy + sr * sp * sy;
  q.x = sr * cp * cy - cr * sp * sy;
  q.y = cr * sp * cy + sr * cp * sy;
  q.z = cr * cp * sy - sr * sp * cy;
  return q;
}

// The sampled odometry model's draw (include/rmclhip.h, MOTION NOISE): moved * N, with N a zero-mean Gaussian in the body frame of the
// moved pose -- N.t = (z0 s0, z1 s1, z2 s2), N.R = EulerAngles(z3 s3, z4 s4, z5 s5) -- and z the three Box-Muller pairs of
// A = philox((g, step, 0, 2), seed), B = philox((g, step, 1, 2), seed): (A0, A1), (A2, A3), (B0, B1).  g is the GLOBAL particle index.
// No normalisation afterwards, as in xmul everywhere else; the stamp is `moved`'s.  tests/motion_noise_ref.py restates it.
__device__ __forceinline__ xform motion_noise_compose(const xform& moved, uint32_t g, uint32_t step, uint32_t key0, uint32_t key1,
                                                      const float (&sigma)[6]) {
  uint32_t A[4], B[4];
  philox4x32_10(g, step, 0u, 2u, key0, key1, A);
  philox4x32_10(g, step, 1u, 2u, key0, key1, B);
  float z[6];
  box_muller(A[0], A[1], z[0], z[1]);
  box_muller(A[2], A[3], z[2], z[3]);
  box_muller(B[0], B[1], z[4], z[5]);
  xform N;
  N.t = mk3(z[0] * sigma[0], z[1] * sigma[1], z[2] * sigma[2]);
  N.R = euler_to_quat(z[3] * sigma[3], z[4] * sigma[4], z[5] * sigma[5]);
  N.stamp = 0u;
  return xmul(moved, N);
}

// rmagine EulerAngles <- Quaternion (textbook ZYX extraction): the float products ...
struct euler_terms { float sinr_cosp, cosr_cosp, sinp, siny_cosp, cosy_cosp; };
__device__ __forceinline__ euler_terms quat_euler_terms(quat q) {
  euler_terms e;
  e.sinr_cosp = 2.0f * (q.w * q.x + q.y * q.z);
  e.cosr_cosp = 1.0f - 2.0f * (q.x * q.x + q.y * q.y);
  e.sinp = 2.0f * (q.w * q.y - q.z * q.x);
  e.siny_cosp = 2.0f * (q.w * q.z + q.x * q.y);
  e.cosy_cosp = 1.0f - 2.0f * (q.y * q.y + q.z * q.z);
  return e;
}

// ... and atan2 / asin of them in double, rounded to float
__device__ __forceinline__ void quat_to_euler(quat q, float& roll, float& pitch, float& yaw) {
  const euler_terms e = quat_euler_terms(q);
  roll = static_cast<float>(atan2(static_cast<double>(e.sinr_cosp), static_cast<double>(e.cosr_cosp)));
  pitch = (fabsf(e.sinp) >= 1.0f) ? copysignf(static_cast<float>(3.14159265358979323846 / 2.0), e.sinp)
                                  : static_cast<float>(asin(static_cast<double>(e.sinp)));
  yaw = static_cast<float>(atan2(static_cast<double>(e.siny_cosp), static_cast<double>(e.cosy_cosp)));
}

// the same angles NOT rounded to float: what the pose moments sum (kernels.hip: k_pose_moments)
__device__ __forceinline__ void quat_to_euler_f64(quat q, double& roll, double& pitch, double& yaw) {
  const euler_terms e = quat_euler_terms(q);
  roll = atan2(static_cast<double>(e.sinr_cosp), static_cast<double>(e.cosr_cosp));
  pitch = (fabsf(e.sinp) >= 1.0f) ? copysign(3.14159265358979323846 / 2.0, static_cast<double>(e.sinp)) : asin(static_cast<double>(e.sinp));
  yaw = atan2(static_cast<double>(e.siny_cosp), static_cast<double>(e.cosy_cosp));
}

// n_meas after a resampler forgets: uint32(float(n_meas) * rate), the reference's statement (resampling.cu:188), with the
// conversion written out -- C++ leaves a float -> uint32 conversion of NaN, of a negative value or of one >= 2^32 undefined, and
// float(n_meas) IS 2^32 for every n_meas >= 2^32 - 128.  The rule (what the CUDA reference's conversion instruction does; its x86
// CPU resamplers are undefined here): NaN or <= 0 -> 0; >= 2^32 -> 0xFFFFFFFF; otherwise truncate.  Used by k_gladiator_resample,
// k_residual_fill and k_sys_fill (resample.hip); oracle/rmcl_oracle.c: orc_n_meas_scaled pins the same text.
__host__ __device__ __forceinline__ uint32_t n_meas_scaled(uint32_t n_meas, float rate) {
  const float v = static_cast<float>(n_meas) * rate;
  if (!(v > 0.0f)) return 0u;
  if (v >= 4294967296.0f) return 0xFFFFFFFFu;
  return static_cast<uint32_t>(v);
}

}  // namespace rmclhip
