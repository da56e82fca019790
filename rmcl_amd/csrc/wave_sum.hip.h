// wave_sum.hip.h -- wave64 sums of per-lane double accumulators through LDS, shared by the streaming reductions
// (kernels.hip k_reduce_partials, micp.hip k_micp_iter, pose_information.hip), and the wave64 count of a per-lane flag (deskew.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rmclhip {

// wave64 sum of 16 doubles per lane through LDS instead of cross-lane shuffles: every lane stores its 16 values (row = lane),
// lane L adds column L & 15 over the 16 rows of slice L >> 4, two xor steps join the four slices.  The 17 shuffles of the
// halving butterfly are a chain of dependent ds_bpermute round trips (~3.4k clocks measured for a lone wave); here all stores
// and all loads are independent (~0.6k).  scratch: 64 x 17 doubles owned by this wave; LDS operations of one wave complete in
// order, so no barrier is needed.  Afterwards lanes 0..15 hold the totals of values 0..15.
__device__ __forceinline__ double wave_sum16_lds(const double (&v)[16], double* scratch, uint32_t lane) {
#pragma unroll
  for (int k = 0; k < 16; ++k) scratch[lane * 17u + static_cast<uint32_t>(k)] = v[k];
  const uint32_t col = lane & 15u, row0 = (lane >> 4) * 16u;
  double a[16];
#pragma unroll
  for (uint32_t r = 0; r < 16u; ++r) a[r] = scratch[(row0 + r) * 17u + col];
  double t = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  t += ((a[8] + a[9]) + (a[10] + a[11])) + ((a[12] + a[13]) + (a[14] + a[15]));
  t += __shfl_xor(t, 16, 64);
  t += __shfl_xor(t, 32, 64);
  return t;
}

// wave64 sum of a per-lane flag: one ballot.  Every lane of the wave calls it (exited lanes count as 0); all lanes get the total.
__device__ __forceinline__ uint32_t wave_count(bool b) { return static_cast<uint32_t>(__popcll(__ballot(b))); }

}  // namespace rmclhip
