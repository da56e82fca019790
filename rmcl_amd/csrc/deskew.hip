// deskew.hip -- motion-compensated PointCloud2 input: cloud bytes + a per-point time field + the sensor's motion during the scan ->
// every point cast from the pose the sensor had when it was measured (include/rmclhip.h, MOTION-COMPENSATED INPUT, states the rules).
//
//   k_deskew<false>   the operator form: per point the origin and direction of an OnDn model (set_model_ondn's table: origins
//                     [0, 3n), directions [3n, 6n)) and the dataset point and mask k_dataset_from_ranges makes of them
//   k_deskew<true>    the cloud form: per point one 12-byte xyz record in the frame of the reference time, NaN where the mask is 0
//
// One lane per OUTPUT point, rows and columns picked as k_pointcloud2_unpack picks them; fields are read bytewise (pc2_load.hip.h).
// The knots -- at most 64 x (8 + 28) bytes, part of the launch parameters -- are staged in LDS once per workgroup; a lane finds its
// segment with six halvings, forms s in double (times are seconds since some epoch: a float holds them to 128 s / 2^24 at best) and
// interpolates in float (deskew_pose.h: nlerp, no transcendental).  The four counts are summed across the wave by ballot, across the workgroup
// through LDS, and leave as one atomic add per workgroup and counter: integer adds, the same totals in any order.
#include "deskew_pose.h"
#include "kernels.h"
#include "pc2_load.hip.h"
#include "wave_sum.hip.h"

namespace rmclhip {
namespace {

// the time field as a double: UINT32 (Ouster t, ns), FLOAT32 (Velodyne time, s) or FLOAT64
__device__ __forceinline__ double deskew_load_time(const uint8_t* p, uint32_t type) {
  if (type == kTimeF64) { double d; __builtin_memcpy(&d, p, 8); return d; }
  if (type == kTimeF32) { float f; __builtin_memcpy(&f, p, 4); return static_cast<double>(f); }
  uint32_t u; __builtin_memcpy(&u, p, 4); return static_cast<double>(u);
}

template <bool kCloud>
__global__ void __launch_bounds__(kDeskewBlock) k_deskew(const DeskewParams p) {
  __shared__ double s_times[kDeskewMaxKnots];
  __shared__ quat s_q[kDeskewMaxKnots];
  __shared__ f3 s_t[kDeskewMaxKnots];
  if (threadIdx.x < p.n_knots) {   // n_knots <= 64 < kDeskewBlock
    s_times[threadIdx.x] = p.knots.times[threadIdx.x];
    s_q[threadIdx.x] = p.knots.q[threadIdx.x];
    s_t[threadIdx.x] = p.knots.t[threadIdx.x];
  }
  __syncthreads();
  const size_t n = static_cast<size_t>(p.out_w) * p.out_h;
  const size_t id = static_cast<size_t>(blockIdx.x) * kDeskewBlock + threadIdx.x;
  bool valid = false, fin = false, clamped = false, t_bad = false;
  if (id < n) {
    const uint32_t ti = static_cast<uint32_t>(id / p.out_w), tj = static_cast<uint32_t>(id - static_cast<size_t>(ti) * p.out_w);
    const size_t si = static_cast<size_t>(ti) * p.h_inc + p.h_skip, sj = static_cast<size_t>(tj) * p.w_inc + p.w_skip;
    const uint8_t* ptr = p.data + si * p.row_step + sj * p.point_step;
    const bool f64 = p.is_f64 != 0u;
    const float x = pc2_load(ptr + p.off_x, f64), y = pc2_load(ptr + p.off_y, f64), z = pc2_load(ptr + p.off_z, f64);
    const double t = p.t_offset + p.t_scale * deskew_load_time(ptr + p.off_t, p.t_type);
    fin = (fabsf(x) <= 3.402823466e38f) && (fabsf(y) <= 3.402823466e38f) && (fabsf(z) <= 3.402823466e38f);
    float range = 0.0f;
    f3 d = mk3(0.f, 0.f, 0.f);
    if (fin) {
      range = sqrtf((x * x + y * y) + z * z);
      d = mk3(x / range, y / range, z / range);
    }
    // the pose: a non-finite time takes the first knot (and masks the point out)
    t_bad = !deskew_finite(t);
    uint32_t k = 0u;
    float s = 0.0f;
    if (!t_bad) {
      k = deskew_segment(s_times, p.n_knots, t);
      s = deskew_fraction(t, s_times[k], s_times[k + 1u], &clamped);
    }
    quat q;
    f3 tr;
    deskew_interp(s_q[k], s_t[k], s_q[k + 1u], s_t[k + 1u], s, &q, &tr);
    const f3 dir = qrot(q, d);
    const f3 pt = add3(scale3(dir, range), tr);   // k_dataset_from_ranges, kModelOnDn
    const bool out_of_range = (range < p.range_min) || (range > p.range_max);
    valid = !out_of_range && !t_bad;
    if constexpr (kCloud) {
      const float nan = __uint_as_float(0x7FC00000u);
      p.points[3u * id] = valid ? pt.x : nan; p.points[3u * id + 1u] = valid ? pt.y : nan; p.points[3u * id + 2u] = valid ? pt.z : nan;
    } else {
      p.origs[3u * id] = tr.x; p.origs[3u * id + 1u] = tr.y; p.origs[3u * id + 2u] = tr.z;
      p.dirs[3u * id] = dir.x; p.dirs[3u * id + 1u] = dir.y; p.dirs[3u * id + 2u] = dir.z;
      p.points[3u * id] = pt.x; p.points[3u * id + 1u] = pt.y; p.points[3u * id + 2u] = pt.z;
      p.mask[id] = valid ? 1 : 0;
    }
  }
  // every lane of the workgroup reaches this point: the four counts across the wave by ballot, across the workgroup's waves through
  // LDS, then one atomic add per workgroup and counter, each counter in a cache line of its own -- adds to one word serialise at
  // ~10 ns each, and one add per WAVE and counter was most of this launch
  __shared__ uint32_t s_cnt[kDeskewBlock / 64u][kDeskewCounters];
  const uint32_t n_valid = wave_count(valid), n_fin = wave_count(fin), n_clamped = wave_count(clamped), n_bad = wave_count(t_bad);
  if ((threadIdx.x & 63u) == 0u) {
    uint32_t* row = s_cnt[threadIdx.x >> 6];
    row[kDeskewValid] = n_valid; row[kDeskewFinite] = n_fin; row[kDeskewClamped] = n_clamped; row[kDeskewTimeNonFinite] = n_bad;
  }
  __syncthreads();
  if (threadIdx.x < kDeskewCounters) {
    uint32_t sum = 0u;
    for (uint32_t w = 0; w < kDeskewBlock / 64u; ++w) sum += s_cnt[w][threadIdx.x];
    if (sum != 0u) atomicAdd(p.counters + threadIdx.x * kDeskewCounterStride, sum);
  }
}

}  // namespace

hipError_t launch_deskew(const DeskewParams& p, bool cloud_form, hipStream_t s) {
  const size_t n = static_cast<size_t>(p.out_w) * p.out_h;
  if (n == 0u) return hipSuccess;
  const dim3 grid(static_cast<uint32_t>((n + kDeskewBlock - 1u) / kDeskewBlock)), block(kDeskewBlock);
  if (cloud_form) hipLaunchKernelGGL(k_deskew<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_deskew<false>, grid, block, 0, s, p);
  return hipGetLastError();
}

}  // namespace rmclhip
