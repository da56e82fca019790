// pc2scan.hip -- sensor_msgs/PointCloud2 bytes -> the range image of a spherical model, on the device: the per-cloud body of the
// reference's Pc2ToScanNode::convert (rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213; empty cells scan_operations.cpp:25-39),
// and for an operator the dataset MICPSphericalSensorCPU::unpackMessage (:181-233) makes of that image.
//
//   k_pc2scan_bin       one lane per point in buffer order: load x / y / z (FLOAT32 or FLOAT64, any alignment), skip non-finite ones,
//                       T * p, range and the two angles, the cell -- and ONE 64-bit integer atomic into the cell's key
//   k_pc2scan_resolve   one lane per cell: the key's range (or range.max + 1), the dataset point and mask, the number of filled cells
//
// The reference's loop is sequential: a later point overwrites an earlier one.  Here the winner of a cell is the extremum of a key that
// holds the point's place in the buffer, so it does not depend on which wave arrives first:
//   default             atomicMax of (i + 1) << 32 | range bits     the LARGEST i wins; 0 = nobody
//   PC2SCAN_NEAREST     atomicMin of range bits << 32 | i           the smallest (range, i) wins (ranges are >= +0: their bit patterns
//                                                                   order like the values); all ones = nobody (a NaN range is no candidate)
// Integer atomics only, and only on the keys: the counts are summed per workgroup (ballot + a four-entry LDS table), written per
// workgroup and added up by the publish launch -- thousands of adds to ONE word serialise at ~10 ns each (measured: 6 144 of them made
// the binning pass 73 us, profiles/pc2scan_time.txt).  The same bits on every run.  Arithmetic: every step is
// the IEEE operation the host restatement (tests/pc2scan_ref.py) performs, in its order; the library is built with -ffp-contract=off
// and correctly rounded float divide / sqrt; atan2 is evaluated in double and rounded to float.
#include "kernels.h"

namespace rmclhip {
namespace {

__device__ __forceinline__ float p2s_load(const uint8_t* p, bool f64) {
  if (f64) { double d; __builtin_memcpy(&d, p, 8); return static_cast<float>(d); }
  float f; __builtin_memcpy(&f, p, 4); return f;
}

// std::isfinite: neither NaN nor +-inf
__device__ __forceinline__ bool p2s_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// ((est - min) / inc) + 0.5 -> id, kept in double: nothing out of an int's range is ever converted, NaN fails the caller's comparison.
// inc == 0 (accepted for size == 1 only, capi_pc2scan.cpp): id 0.
__device__ __forceinline__ double p2s_id(float est, float mn, float inc, bool floor_it) {
  if (inc == 0.0f) return 0.0;
  const float q = (est - mn) / inc;
  const double c = static_cast<double>(q) + 0.5;
  return floor_it ? floor(c) : trunc(c);
}

__device__ __forceinline__ uint32_t p2s_wave_count(bool b) { return static_cast<uint32_t>(__popcll(__ballot(b))); }

constexpr uint32_t kP2sWaves = kPc2ScanBlock / 64u;

__global__ void __launch_bounds__(kPc2ScanBlock) k_pc2scan_bin(const Pc2ScanParams p) {
  const uint32_t i = blockIdx.x * kPc2ScanBlock + threadIdx.x;
  bool fin = false, in_image = false, cand = false;
  if (i < p.n_points) {
    const uint32_t row = i / p.width, col = i - row * p.width;
    const uint8_t* ptr = p.data + static_cast<size_t>(row) * p.row_step + static_cast<size_t>(col) * p.point_step;
    const bool f64 = p.is_f64 != 0u;
    const float x = p2s_load(ptr + p.off_x, f64), y = p2s_load(ptr + p.off_y, f64), z = p2s_load(ptr + p.off_z, f64);
    fin = p2s_finite(x) && p2s_finite(y) && p2s_finite(z);
    if (fin) {
      f3 ps = mk3(x, y, z);
      if (p.has_T) ps = xapply(p.T, ps);
      const float range_est = sqrtf((ps.x * ps.x + ps.y * ps.y) + ps.z * ps.z);   // Vector3::l2norm
      const float theta_est = static_cast<float>(atan2(static_cast<double>(ps.y), static_cast<double>(ps.x)));
      const float den = (p.flags & kPc2ScanTrueElevation) ? sqrtf(ps.x * ps.x + ps.y * ps.y) : range_est;   // the reference: atan2(z, range)
      const float phi_est = static_cast<float>(atan2(static_cast<double>(ps.z), static_cast<double>(den)));
      const bool floor_it = (p.flags & kPc2ScanFloor) != 0u;
      const double phi_id = p2s_id(phi_est, p.phi_min, p.phi_inc, floor_it);
      double theta_id = p2s_id(theta_est, p.theta_min, p.theta_inc, floor_it);
      if (p.theta_period != 0.0) {   // PC2SCAN_WRAP_THETA and 2 pi / theta.inc integral
        if (theta_id >= static_cast<double>(p.W)) theta_id -= p.theta_period;
        else if (theta_id < 0.0) theta_id += p.theta_period;
      }
      in_image = phi_id >= 0.0 && phi_id < static_cast<double>(p.H) && theta_id >= 0.0 && theta_id < static_cast<double>(p.W);
      cand = in_image && p.rmin <= range_est && range_est <= p.rmax;   // Interval::inside
      if (cand) {
        // both ids are whole numbers in [0, size): the conversions are exact, the cell is inside the W * H keys
        const uint32_t cell = static_cast<uint32_t>(phi_id) * p.W + static_cast<uint32_t>(theta_id);
        const unsigned long long rb = __float_as_uint(range_est);
        if (p.flags & kPc2ScanNearest) atomicMin(p.keys + cell, (rb << 32) | static_cast<unsigned long long>(i));
        else atomicMax(p.keys + cell, (static_cast<unsigned long long>(i + 1u) << 32) | rb);
      }
    }
  }
  // every lane of the workgroup reaches this point: the workgroup's three counts, one row per workgroup
  __shared__ uint32_t wave_cnt[kP2sWaves][3];
  const uint32_t n_fin = p2s_wave_count(fin), n_img = p2s_wave_count(in_image), n_cand = p2s_wave_count(cand);
  if ((threadIdx.x & 63u) == 0u) {
    wave_cnt[threadIdx.x >> 6][0] = n_fin; wave_cnt[threadIdx.x >> 6][1] = n_img; wave_cnt[threadIdx.x >> 6][2] = n_cand;
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    uint32_t sum = 0u;
    for (uint32_t w = 0; w < kP2sWaves; ++w) sum += wave_cnt[w][threadIdx.x];
    p.bin_counts[3u * blockIdx.x + threadIdx.x] = sum;
  }
}

__global__ void __launch_bounds__(kPc2ScanBlock) k_pc2scan_resolve(const Pc2ScanParams p) {
  const uint32_t n = p.W * p.H, i = blockIdx.x * kPc2ScanBlock + threadIdx.x;
  bool filled = false;
  if (i < n) {
    const unsigned long long key = p.keys[i];
    const bool nearest = (p.flags & kPc2ScanNearest) != 0u;
    filled = nearest ? (key != ~0ull) : (key != 0ull);
    const float r = filled ? __uint_as_float(static_cast<uint32_t>(nearest ? (key >> 32) : key)) : p.range_empty;
    p.ranges[i] = r;
    if (p.ds_points != nullptr) {
      // k_dataset_from_ranges for kModelSpherical: dir(vid, hid) * range, no origin; the mask is the range test of the image
      const uint32_t vid = i / p.W, hid = i - vid * p.W;
      const float* tab = p.model_tab;
      const float cp = tab[vid], sp = tab[p.H + vid], ct = tab[2u * p.H + hid], st = tab[2u * p.H + p.W + hid];
      const f3 pt = scale3(mk3(cp * ct, cp * st, sp), r);
      p.ds_points[3u * i] = pt.x; p.ds_points[3u * i + 1u] = pt.y; p.ds_points[3u * i + 2u] = pt.z;
      const bool out_of_range = (r < p.rmin) || (r > p.rmax);
      p.ds_mask[i] = out_of_range ? 0 : 1;
    }
  }
  __shared__ uint32_t wave_cnt[kP2sWaves];
  const uint32_t n_filled = p2s_wave_count(filled);
  if ((threadIdx.x & 63u) == 0u) wave_cnt[threadIdx.x >> 6] = n_filled;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t sum = 0u;
    for (uint32_t w = 0; w < kP2sWaves; ++w) sum += wave_cnt[w];
    p.cell_counts[blockIdx.x] = sum;
  }
}

// behind the two passes, one workgroup: the per-workgroup rows added up (integers: any order gives the same sums), the four totals to
// host-mapped memory (the caller waits for the stream)
__global__ void __launch_bounds__(kPc2ScanBlock) k_pc2scan_publish(const uint32_t* __restrict__ bin_counts, uint32_t n_bin_blocks,
                                                                   const uint32_t* __restrict__ cell_counts, uint32_t n_cell_blocks,
                                                                   uint32_t* __restrict__ host) {
  __shared__ uint32_t wave_sum[kP2sWaves][4];
  uint32_t s[4] = {0u, 0u, 0u, 0u};
  for (uint32_t b = threadIdx.x; b < n_bin_blocks; b += kPc2ScanBlock) {
    s[0] += bin_counts[3u * b]; s[1] += bin_counts[3u * b + 1u]; s[2] += bin_counts[3u * b + 2u];
  }
  for (uint32_t b = threadIdx.x; b < n_cell_blocks; b += kPc2ScanBlock) s[3] += cell_counts[b];
  for (uint32_t k = 0; k < 4u; ++k) {
    for (uint32_t off = 32u; off != 0u; off >>= 1) s[k] += __shfl_xor(s[k], off);
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 4u) {
    uint32_t sum = 0u;
    for (uint32_t w = 0; w < kP2sWaves; ++w) sum += wave_sum[w][threadIdx.x];
    host[threadIdx.x] = sum;
  }
}

}  // namespace

hipError_t launch_pc2scan(const Pc2ScanParams& p, uint32_t* counters_host, hipStream_t s) {
  const size_t n_cells = static_cast<size_t>(p.W) * p.H;
  const uint32_t n_bin_blocks = pc2scan_blocks(p.n_points), n_cell_blocks = pc2scan_blocks(n_cells);
  if (n_cells != 0u)
    if (const hipError_t e = hipMemsetAsync(p.keys, (p.flags & kPc2ScanNearest) ? 0xFF : 0x00, n_cells * sizeof(unsigned long long), s)) return e;
  if (n_bin_blocks != 0u) {   // (an empty image still counts the finite points: no point is inside it, no key is touched)
    hipLaunchKernelGGL(k_pc2scan_bin, dim3(n_bin_blocks), dim3(kPc2ScanBlock), 0, s, p);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  if (n_cell_blocks != 0u) {
    hipLaunchKernelGGL(k_pc2scan_resolve, dim3(n_cell_blocks), dim3(kPc2ScanBlock), 0, s, p);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_pc2scan_publish, dim3(1), dim3(kPc2ScanBlock), 0, s, p.bin_counts, n_bin_blocks, p.cell_counts, n_cell_blocks, counters_host);
  return hipGetLastError();
}

}  // namespace rmclhip
