// pc2_load.hip.h -- one field of a sensor_msgs/PointCloud2 record, read bytewise: records of any point_step (22 bytes, say) leave
// their fields unaligned, and an aligned load instruction on such an address faults.  Shared by kernels.hip (k_pointcloud2_unpack)
// and deskew.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rmclhip {

// x / y / z: FLOAT32, or FLOAT64 cast to float
__device__ __forceinline__ float pc2_load(const uint8_t* p, bool f64) {
  if (f64) { double d; __builtin_memcpy(&d, p, 8); return static_cast<float>(d); }
  float f; __builtin_memcpy(&f, p, 4); return f;
}

}  // namespace rmclhip
