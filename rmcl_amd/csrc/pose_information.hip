// pose_information.hip -- the 6 x 6 normal matrix of the point-to-plane problem over a find's correspondences (gfx950).
//
//  k_pose_information_partials   one streaming pass over nposes x n correspondences: gate exactly as k_reduce_partials
//                                (rm::statistics_p2l), then the 28 distinct entries of sum u u^T, u = [N ; D x N ; r], and the count
//  k_pose_information_finalize   one wave per pose folds the workgroups' rows in a fixed order
//
// What the sums mean and how the host turns them into a covariance: include/rmclhip.h (POSE COVARIANCE), DESIGN.md 4.12.
#include "kernels.h"
#include "robust_host.h"
#include "wave_sum.hip.h"

namespace rmclhip {

namespace {

constexpr int kSums = 28;   // upper triangle of the 7 x 7 matrix sum u u^T, row by row
constexpr int kVals = 32;   // kSums, the count, padding: two groups of 16 for wave_sum16_lds
constexpr int kWsum = 29, kRssPlain = 30;   // the weighted form alone: sum w, sum r^2 (the plain form leaves them 0)
static_assert(kVals == static_cast<int>(kPoseInfoRow), "row layout");

// Per-lane f64 accumulators -- the plain form: the 28 products of a correspondence are multiply + add on values its lane already holds
// (no fused multiply-add: every term is the rounded product, which is what the tests' error bound counts), no MFMA --, summed over the
// wave through LDS and over the workgroup's four waves in wave order.  Nothing is added across workgroups here: a workgroup's row is a
// function of its correspondences alone.
template <bool kWeighted>
__device__ __forceinline__ void pose_information_partials(const ReduceParams& p, int kernel, float c) {
  __shared__ double red[4][kVals];
  __shared__ double s_wsum[4][64 * 17];
  const uint32_t pose = blockIdx.y;
  const xform Tpre = (p.Tpre_dev != nullptr) ? p.Tpre_dev[pose] : p.Tpre;
  const float max_dist = p.max_dist;
  double acc[kVals];
#pragma unroll
  for (int k = 0; k < kVals; ++k) acc[k] = 0.0;
  const size_t mbase = static_cast<size_t>(pose) * p.n;
  const size_t stride = static_cast<size_t>(gridDim.x) * 256u;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < p.n; i += stride) {
    const bool dok = (p.dataset_mask == nullptr) || (p.dataset_mask[i] > 0);
    if (dok && (p.model_mask == nullptr || p.model_mask[mbase + i] > 0)) {
      const float* dp = p.dataset_points + 3 * i;
      const float* mp = p.model_points + 3 * (mbase + i);
      const float* mn = p.model_normals + 3 * (mbase + i);
      // the gate of k_reduce_partials, operation for operation: the two kernels keep the same correspondences
      const f3 Di = xapply(Tpre, mk3(dp[0], dp[1], dp[2]));
      const f3 Ii = mk3(mp[0], mp[1], mp[2]);
      const f3 Ni = mk3(mn[0], mn[1], mn[2]);
      const float spd = dot_plain(sub3(Ii, Di), Ni);
      if (fabsf(spd) < max_dist) {   // false for NaN: a miss's NaN point / normal never reaches the sums
        const double dx = Di.x, dy = Di.y, dz = Di.z, nx = Ni.x, ny = Ni.y, nz = Ni.z;
        const double u[7] = {nx, ny, nz, dy * nz - dz * ny, dz * nx - dx * nz, dx * ny - dy * nx, static_cast<double>(spd)};
        int k = 0;
        if constexpr (kWeighted) {
          // the weight of robust.hip's reduction (robust_host.h) at the same residual: w == 1 adds the very values of the plain form
          const double wd = static_cast<double>(robust_weight(kernel, c, spd));
#pragma unroll
          for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b) acc[k++] += wd * (u[a] * u[b]);
          acc[kWsum] += wd;
          acc[kRssPlain] += u[6] * u[6];
        } else {
#pragma unroll
          for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b) acc[k++] += u[a] * u[b];
        }
        acc[kSums] += 1.0;
      }
    }
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = acc[16 * h + k];
    // (the wave's scratch is reused by the second half: LDS operations of one wave complete in order)
    const double wsum = wave_sum16_lds(v, &s_wsum[wave][0], lane);
    if (lane < 16u) red[wave][16 * h + lane] = wsum;
  }
  __syncthreads();
  if (threadIdx.x < static_cast<uint32_t>(kVals)) {
    const double v = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    // write-through store, read by the finalize launch after the kernel boundary (as k_reduce_partials)
    __hip_atomic_store(p.partials + (static_cast<size_t>(pose) * p.nblocks + blockIdx.x) * kVals + threadIdx.x, v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(256) k_pose_information_partials(const ReduceParams p) { pose_information_partials<false>(p, 0, 0.0f); }

// the same pass with M-estimator weights (include/rmclhip.h, ROBUST MICP): same grid, same mapping, same fold
__global__ void __launch_bounds__(256) k_pose_information_partials_robust(const ReduceParams p, int kernel, const RobustScale* __restrict__ scale) {
  pose_information_partials<true>(p, kernel, scale->c);
}

// lane = 32 g + k adds value k of the rows g, g + 2, g + 4, ... in ascending order (eight loads in flight), one xor step joins the
// two halves: a fixed order for a given number of rows
__global__ void __launch_bounds__(64) k_pose_information_finalize(const double* __restrict__ partials, uint32_t nblocks,
                                                                 double* __restrict__ rows_out) {
  const uint32_t pose = blockIdx.x, lane = threadIdx.x & 63u, k0 = lane & 31u, g = lane >> 5;
  const double* rows = partials + static_cast<size_t>(pose) * nblocks * kVals;
  double a = 0.0;
  uint32_t b = g;
  for (; b + 14u < nblocks; b += 16u) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = rows[static_cast<size_t>(b + 2u * u) * kVals + k0];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; b < nblocks; b += 2u) a += rows[static_cast<size_t>(b) * kVals + k0];
  a += __shfl_xor(a, 32, 64);
  if (lane < static_cast<uint32_t>(kVals)) rows_out[static_cast<size_t>(pose) * kVals + lane] = a;
}

}  // namespace

hipError_t launch_pose_information(const ReduceParams& p, double* rows_out, hipStream_t s) {
  hipLaunchKernelGGL(k_pose_information_partials, dim3(p.nblocks, p.nposes), dim3(256), 0, s, p);
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_pose_information_finalize, dim3(p.nposes), dim3(64), 0, s, p.partials, p.nblocks, rows_out);
  return hipGetLastError();
}

hipError_t launch_pose_information_robust(const ReduceParams& p, int32_t kernel, const RobustScale* scale_dev, double* rows_out, hipStream_t s) {
  hipLaunchKernelGGL(k_pose_information_partials_robust, dim3(p.nblocks, p.nposes), dim3(256), 0, s, p, kernel, scale_dev);
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_pose_information_finalize, dim3(p.nposes), dim3(64), 0, s, p.partials, p.nblocks, rows_out);
  return hipGetLastError();
}

}  // namespace rmclhip
