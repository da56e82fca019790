// surface_sample.hip -- the build of the surface sampler (include/rmclhip.h, SURFACE SAMPLER): which record stands for a face, and
// every face's area or "not eligible".  The weights' prefix sums are the resamplers' scan (resample.hip: launch_surface_sample_scan);
// the draw is surface_sample.hip.h.
//
//   k_ss_records   rec_of_face[face id of record r] = min(., r): a face the builder's spatial splits reference from several leaves has
//                  several identical records; the lowest index is kept (integer atomicMin: independent of the order, as pc2scan.hip's
//                  winner resolution)
//   k_ss_areas     one lane per face id: the eligibility rule and a_f in double from the record's float Ng; the largest a_f by an
//                  integer atomicMax on its bits (a positive finite double orders as its bits), one atomic per wave
#include "kernels.h"

namespace rmclhip {
namespace {

constexpr uint32_t kSsBlock = 256;

__global__ void __launch_bounds__(kSsBlock) k_ss_records(const uint32_t* __restrict__ tris, uint32_t n_records, uint32_t n_faces,
                                                         uint32_t* __restrict__ rec_of_face) {
  const uint32_t r = blockIdx.x * kSsBlock + threadIdx.x;
  if (r >= n_records) return;
  const uint32_t face = tris[static_cast<size_t>(r) * kTriDwords + 15u];
  if (face < n_faces) atomicMin(rec_of_face + face, r);
}

__global__ void __launch_bounds__(kSsBlock) k_ss_areas(const uint32_t* __restrict__ tris, const uint32_t* __restrict__ rec_of_face,
                                                       uint32_t n_faces, SurfaceSampleRule rule, double* __restrict__ area,
                                                       unsigned long long* __restrict__ amax_bits) {
  const uint32_t f = blockIdx.x * kSsBlock + threadIdx.x;
  double a = -1.0;
  const uint32_t rec = (f < n_faces) ? rec_of_face[f] : 0xFFFFFFFFu;
  if (rec != 0xFFFFFFFFu) {
    const uint4* q = reinterpret_cast<const uint4*>(tris) + static_cast<size_t>(rec) * 4u;
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];   // v0.xyz e1.x | e1.yz e2.xy | e2.z Ng.xyz | n.xyz face
    const float v0[3] = {__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z)};
    const float e1[3] = {__uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)};
    const float e2[3] = {__uint_as_float(q1.z), __uint_as_float(q1.w), __uint_as_float(q2.x)};
    bool eligible = fabsf(__uint_as_float(q3.z)) >= rule.min_up_cos;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double c = static_cast<double>(v0[d]) + (static_cast<double>(e2[d]) - static_cast<double>(e1[d])) / 3.0;
      eligible = eligible && c >= static_cast<double>(rule.region_min[d]) && c <= static_cast<double>(rule.region_max[d]);
    }
    if (eligible) {
      const double gx = static_cast<double>(__uint_as_float(q2.y)), gy = static_cast<double>(__uint_as_float(q2.z)),
                   gz = static_cast<double>(__uint_as_float(q2.w));
      a = 0.5 * sqrt((gx * gx + gy * gy) + gz * gz);
    }
  }
  if (f < n_faces) area[f] = a;
  static_assert(kSsBlock % 64u == 0u, "whole waves of 64 lanes (gfx950): the butterfly below starts at 32 and lane 0 of every 64 holds the result");
  // the wave's largest finite positive area (NaN and +inf compare false or are excluded; -1 and 0 leave the bits at 0)
  unsigned long long bits = (a > 0.0 && a < __longlong_as_double(0x7FF0000000000000ll)) ? static_cast<unsigned long long>(__double_as_longlong(a)) : 0ull;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(bits, off);
    bits = (o > bits) ? o : bits;
  }
  if ((threadIdx.x & 63u) == 0u && bits != 0ull) atomicMax(amax_bits, bits);
}

}  // namespace

hipError_t launch_surface_sample_records(const uint32_t* tris, uint32_t n_records, uint32_t n_faces, uint32_t* rec_of_face, hipStream_t s) {
  if (n_records == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ss_records, dim3((n_records + kSsBlock - 1u) / kSsBlock), dim3(kSsBlock), 0, s, tris, n_records, n_faces, rec_of_face);
  return hipGetLastError();
}

hipError_t launch_surface_sample_areas(const uint32_t* tris, const uint32_t* rec_of_face, uint32_t n_faces, const SurfaceSampleRule& rule,
                                       double* area, unsigned long long* amax_bits, hipStream_t s) {
  if (n_faces == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ss_areas, dim3((n_faces + kSsBlock - 1u) / kSsBlock), dim3(kSsBlock), 0, s, tris, rec_of_face, n_faces, rule, area,
                     amax_bits);
  return hipGetLastError();
}

}  // namespace rmclhip
