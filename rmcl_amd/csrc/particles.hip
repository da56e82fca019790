// particles.hip -- the particle cloud's first and last step on the device: the two initialisations of the filter node and the channels
// its visualisation publishes (rmcl_ros/src/nodes/rmcl_localization.cpp).
//
//   k_particles_init_uniform        RmclNode::initSamplesUniform (:277-342): every particle uniform in a 6-D box (x y z roll pitch yaw)
//   k_particles_init_pose           RmclNode::initSamples (:165-275): x = L z around a pose guess, L L^T = the guess's covariance
//   k_particles_init_surface        every particle on a drivable face of the map, uniform by area (include/rmclhip.h, SURFACE SAMPLER)
//   k_particles_inject_surface      the recovery injection: a random fraction of a cloud replaced in place by such draws
//   k_particles_pack_visualization  RmclNode::visualize (:797-879): x y z, likelihood {mean, sigma, n_meas}, badness as seven dense arrays
//
// One lane per particle.  The random words of particle i -- the GLOBAL index, `first` + the element of the buffer the launch was
// given -- are a = philox((i, epoch, 0, 1), seed), b = philox((i, epoch, 1, 1), seed): w0..w3 = a, w4..w5 = b[0..1] (pf_random.hip.h;
// the resamplers' counters end in 0, so both may share a seed).  A cloud is therefore the same bits whatever the launch shape and
// however its range is cut into calls or shards.  Arithmetic: every step is the IEEE operation the host restatement
// (tests/particle_init_ref.py) performs, in its order (-ffp-contract=off); transcendentals in double, rounded to float.
//
// Stores.  A pose is 32 B, 16-B aligned: two 16-B stores per lane.  The attributes both initialisations write are the SAME 36 B for
// every particle ({mean 1, sigma 0, n_meas 0}, state_sigma 0), so the attribute array is a stream of dwords with period 9 and no lane
// needs "its" record: a workgroup writes the 2304 dwords of its 256 records as 16-B stores from the first 16-B boundary on (a slice
// of a cloud starts at first * 36 B: 4-B aligned only) and the up to three dwords on either side singly.
#include "kernels.h"
#include "pf_random.hip.h"
#include "surface_sample.hip.h"

namespace rmclhip {
namespace {

constexpr uint32_t kPartBlock = 256;
constexpr uint32_t kAttrDwords = 9;                          // sizeof(ParticleAttributes) / 4
constexpr uint32_t kBlockAttrDwords = kPartBlock * kAttrDwords;   // 2304: a multiple of 4, every workgroup sees the same phase

__device__ __forceinline__ uint32_t init_attr_dword(uint32_t j) { return (j % kAttrDwords == 0u) ? 0x3F800000u : 0u; }   // likelihood.mean = 1.0f

// the attribute records of this workgroup's particles [blockIdx.x * 256, ...) of `count`; lead = dwords from attrs to its first 16-B boundary
__device__ __forceinline__ void store_init_attrs(uint32_t* __restrict__ attrs, uint32_t count, uint32_t lead) {
  const uint32_t s = blockIdx.x * kBlockAttrDwords;
  const uint32_t total = count * kAttrDwords;   // count <= 2^32 / 9 (checked by the launcher)
  const uint32_t e = (total - s < kBlockAttrDwords) ? total : s + kBlockAttrDwords;
  // first index >= s that lies on a 16-B boundary: j = lead (mod 4); s = 0 (mod 4)
  uint32_t v0 = s + lead;
  if (v0 > e) v0 = e;
  const uint32_t nvec = (e - v0) / 4u, v1 = v0 + 4u * nvec;
  for (uint32_t k = threadIdx.x; k < nvec; k += kPartBlock) {
    const uint32_t j = v0 + 4u * k;
    uint4 q;
    q.x = init_attr_dword(j); q.y = init_attr_dword(j + 1u); q.z = init_attr_dword(j + 2u); q.w = init_attr_dword(j + 3u);
    *reinterpret_cast<uint4*>(attrs + j) = q;
  }
  // at most 3 dwords before the first boundary and 3 after the last whole vector
  if (threadIdx.x < 3u && s + threadIdx.x < v0) attrs[s + threadIdx.x] = init_attr_dword(s + threadIdx.x);
  if (threadIdx.x >= 64u && threadIdx.x < 67u && v1 + (threadIdx.x - 64u) < e) attrs[v1 + (threadIdx.x - 64u)] = init_attr_dword(v1 + (threadIdx.x - 64u));
}

__device__ __forceinline__ void store_pose(xform* __restrict__ poses, uint32_t k, const xform& T) {
  float4* dst = reinterpret_cast<float4*>(poses + k);
  dst[0] = make_float4(T.R.x, T.R.y, T.R.z, T.R.w);
  dst[1] = make_float4(T.t.x, T.t.y, T.t.z, __uint_as_float(T.stamp));
}

__device__ __forceinline__ void init_words(uint32_t i, uint32_t epoch, uint32_t key0, uint32_t key1, uint32_t (&w)[6]) {
  uint32_t a[4], b[4];
  philox4x32_10(i, epoch, 0u, 1u, key0, key1, a);
  philox4x32_10(i, epoch, 1u, 1u, key0, key1, b);
  w[0] = a[0]; w[1] = a[1]; w[2] = a[2]; w[3] = a[3]; w[4] = b[0]; w[5] = b[1];
}

struct UniformBox { float lo[6], hi[6]; };

__global__ void __launch_bounds__(kPartBlock) k_particles_init_uniform(xform* __restrict__ poses, uint32_t* __restrict__ attrs, uint32_t first,
                                                                       uint32_t count, UniformBox box, uint32_t key0, uint32_t key1,
                                                                       uint32_t epoch, uint32_t attr_lead) {
  store_init_attrs(attrs, count, attr_lead);
  const uint32_t k = blockIdx.x * kPartBlock + threadIdx.x;
  if (k >= count) return;
  uint32_t w[6];
  init_words(first + k, epoch, key0, key1, w);
  xform T;
  T.t = mk3(uniform_in(box.lo[0], box.hi[0], w[0]), uniform_in(box.lo[1], box.hi[1], w[1]), uniform_in(box.lo[2], box.hi[2], w[2]));
  T.R = euler_to_quat(uniform_in(box.lo[3], box.hi[3], w[3]), uniform_in(box.lo[4], box.hi[4], w[4]), uniform_in(box.lo[5], box.hi[5], w[5]));
  T.stamp = 0u;
  store_pose(poses, k, T);
}

struct PoseInit { xform Tlm; float L[36]; };   // L: row-major lower-triangular factor (rmclhip_chol6_host)

__global__ void __launch_bounds__(kPartBlock) k_particles_init_pose(xform* __restrict__ poses, uint32_t* __restrict__ attrs, uint32_t first,
                                                                    uint32_t count, PoseInit in, uint32_t key0, uint32_t key1, uint32_t epoch,
                                                                    uint32_t attr_lead) {
  store_init_attrs(attrs, count, attr_lead);
  const uint32_t k = blockIdx.x * kPartBlock + threadIdx.x;
  if (k >= count) return;
  uint32_t w[6];
  init_words(first + k, epoch, key0, key1, w);
  float z[6], x[6];
  box_muller(w[0], w[1], z[0], z[1]);
  box_muller(w[2], w[3], z[2], z[3]);
  box_muller(w[4], w[5], z[4], z[5]);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c <= r; ++c) acc = acc + static_cast<double>(in.L[6 * r + c]) * static_cast<double>(z[c]);
    x[r] = static_cast<float>(acc);
  }
  xform Pl;
  Pl.R = euler_to_quat(x[3], x[4], x[5]);
  Pl.t = mk3(x[0], x[1], x[2]);
  Pl.stamp = 0u;
  store_pose(poses, k, xmul(in.Tlm, Pl));   // (stamp: Tlm's, as xmul hands it on)
}

// the surface sampler's draw (surface_sample.hip.h) of global particle first + k from draws 2 and 3 of the initialisers' stream
__global__ void __launch_bounds__(kPartBlock) k_particles_init_surface(xform* __restrict__ poses, uint32_t* __restrict__ attrs, uint32_t first,
                                                                       uint32_t count, SurfaceSampleView sv, uint32_t key0, uint32_t key1,
                                                                       uint32_t epoch, uint32_t attr_lead) {
  store_init_attrs(attrs, count, attr_lead);
  const uint32_t k = blockIdx.x * kPartBlock + threadIdx.x;
  if (k >= count) return;
  uint32_t A[4], B[4];
  philox4x32_10(first + k, epoch, 2u, 1u, key0, key1, A);
  philox4x32_10(first + k, epoch, 3u, 1u, key0, key1, B);
  store_pose(poses, k, surface_sample_pose(sv, A, B));
}

// the recovery injection, in place: slot j = first + k is replaced iff the first word of draw 9 of the resamplers' stream lies below
// the threshold; its pose is the sampler's draw from draws 10 and 11, its attributes the initialisations'.  A slot that stays is not
// read and not written.  The replaced records are scattered: a lane stores the nine dwords of its own (4-B aligned) record.
__global__ void __launch_bounds__(kPartBlock) k_particles_inject_surface(xform* __restrict__ poses, uint32_t* __restrict__ attrs, uint32_t first,
                                                                         uint32_t count, SurfaceSampleView sv, unsigned long long threshold,
                                                                         uint32_t key0, uint32_t key1, uint32_t step,
                                                                         uint32_t* __restrict__ n_injected) {
  const uint32_t k = blockIdx.x * kPartBlock + threadIdx.x;
  bool replace = false;
  if (k < count) {
    uint32_t r[4];
    philox4x32_10(first + k, step, 9u, 0u, key0, key1, r);
    replace = static_cast<unsigned long long>(r[0]) < threshold;
  }
  // the count: one atomic per workgroup (one per wave to a single address is what a launch over a million slots then waits for)
  static_assert(kPartBlock == 256u, "four waves of 64 lanes: the sum below names them");
  __shared__ uint32_t s_count[4];
  const uint64_t m = __ballot(replace);
  if ((threadIdx.x & 63u) == 0u) s_count[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0u) {
    const uint32_t c = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
    if (c) atomicAdd(n_injected, c);
  }
  if (!replace) return;
  uint32_t A[4], B[4];
  philox4x32_10(first + k, step, 10u, 0u, key0, key1, A);
  philox4x32_10(first + k, step, 11u, 0u, key0, key1, B);
  store_pose(poses, k, surface_sample_pose(sv, A, B));
  uint32_t* a = attrs + static_cast<size_t>(k) * kAttrDwords;
#pragma unroll
  for (uint32_t j = 0; j < kAttrDwords; ++j) a[j] = init_attr_dword(j);
}

// out: seven arrays of n floats: x | y | z | likelihood | likelihood_sigma | likelihood_n_meas | badness
__global__ void __launch_bounds__(kPartBlock) k_particles_pack_visualization(const xform* __restrict__ poses, const uint32_t* __restrict__ attrs,
                                                                             uint32_t n, uint32_t max_n_meas, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * kPartBlock + threadIdx.x;
  if (i >= n) return;
  const float4 t = reinterpret_cast<const float4*>(poses + i)[1];   // {t.x, t.y, t.z, stamp}
  const uint32_t* a = attrs + static_cast<size_t>(i) * kAttrDwords;
  const float mean = __uint_as_float(a[0]), sigma = __uint_as_float(a[1]);
  const uint32_t n_meas = a[2];
  const float unc = static_cast<float>(1.0 - static_cast<double>(n_meas) / static_cast<double>(max_n_meas));
  const float badness = mean * (sigma * unc + unc);
  const size_t N = n;
  out[i] = t.x;
  out[N + i] = t.y;
  out[2 * N + i] = t.z;
  out[3 * N + i] = mean;
  out[4 * N + i] = sigma;
  out[5 * N + i] = static_cast<float>(n_meas);
  out[6 * N + i] = badness;
}

// dwords from p (4-B aligned) to the next 16-B boundary
inline uint32_t lead_dwords(const void* p) { return static_cast<uint32_t>((0u - (reinterpret_cast<uintptr_t>(p) >> 2)) & 3u); }

}  // namespace

hipError_t launch_particles_init_uniform(xform* poses, void* attrs, uint32_t first, uint32_t count, const float* bb_min, const float* bb_max,
                                         uint64_t seed, uint32_t epoch, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (count > kMaxInitCount || (reinterpret_cast<uintptr_t>(poses) & 15u) || (reinterpret_cast<uintptr_t>(attrs) & 3u)) return hipErrorInvalidValue;
  UniformBox box;
  for (int d = 0; d < 6; ++d) { box.lo[d] = bb_min[d]; box.hi[d] = bb_max[d]; }
  hipLaunchKernelGGL(k_particles_init_uniform, dim3((count + kPartBlock - 1u) / kPartBlock), dim3(kPartBlock), 0, s, poses,
                     static_cast<uint32_t*>(attrs), first, count, box, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), epoch,
                     lead_dwords(attrs));
  return hipGetLastError();
}

hipError_t launch_particles_init_pose(xform* poses, void* attrs, uint32_t first, uint32_t count, const xform& Tlm, const float* L36, uint64_t seed,
                                      uint32_t epoch, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (count > kMaxInitCount || (reinterpret_cast<uintptr_t>(poses) & 15u) || (reinterpret_cast<uintptr_t>(attrs) & 3u)) return hipErrorInvalidValue;
  PoseInit in;
  in.Tlm = Tlm;
  for (int k = 0; k < 36; ++k) in.L[k] = L36[k];
  hipLaunchKernelGGL(k_particles_init_pose, dim3((count + kPartBlock - 1u) / kPartBlock), dim3(kPartBlock), 0, s, poses,
                     static_cast<uint32_t*>(attrs), first, count, in, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), epoch,
                     lead_dwords(attrs));
  return hipGetLastError();
}

hipError_t launch_particles_init_surface(xform* poses, void* attrs, uint32_t first, uint32_t count, const SurfaceSampleView& sv, uint64_t seed,
                                         uint32_t epoch, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (count > kMaxInitCount || (reinterpret_cast<uintptr_t>(poses) & 15u) || (reinterpret_cast<uintptr_t>(attrs) & 3u) || sv.n_faces == 0 || sv.T == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_particles_init_surface, dim3((count + kPartBlock - 1u) / kPartBlock), dim3(kPartBlock), 0, s, poses,
                     static_cast<uint32_t*>(attrs), first, count, sv, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), epoch,
                     lead_dwords(attrs));
  return hipGetLastError();
}

hipError_t launch_particles_inject_surface(xform* poses, void* attrs, uint32_t first, uint32_t count, const SurfaceSampleView& sv,
                                           unsigned long long threshold, uint64_t seed, uint32_t step, uint32_t* n_injected, hipStream_t s) {
  if (count == 0 || threshold == 0) return hipSuccess;
  if (count > kMaxInitCount || (reinterpret_cast<uintptr_t>(poses) & 15u) || (reinterpret_cast<uintptr_t>(attrs) & 3u) || sv.n_faces == 0 || sv.T == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_particles_inject_surface, dim3((count + kPartBlock - 1u) / kPartBlock), dim3(kPartBlock), 0, s, poses,
                     static_cast<uint32_t*>(attrs), first, count, sv, threshold, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                     step, n_injected);
  return hipGetLastError();
}

hipError_t launch_particles_pack_visualization(const xform* poses, const void* attrs, uint32_t n, uint32_t max_n_meas, float* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(poses) & 15u) || (reinterpret_cast<uintptr_t>(attrs) & 3u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_particles_pack_visualization, dim3((n + kPartBlock - 1u) / kPartBlock), dim3(kPartBlock), 0, s, poses,
                     static_cast<const uint32_t*>(attrs), n, max_n_meas, out);
  return hipGetLastError();
}

}  // namespace rmclhip
