// pc2scan_host_loop.cpp -- what a caller of the spherical operator had to do before rmclhip_rcc_set_input_pointcloud2_scan existed: bin
// an unorganised PointCloud2 into the (phi, theta) grid on ONE host thread, the shape of Pc2ToScanNode::convert
// (rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213), then hand the image to rmclhip_rcc_set_dataset_from_ranges.  Written for
// tools/pc2scan_time.py (which builds it: g++ -O2 -shared -fPIC) to put a number on that loop; the arithmetic is the one pinned in
// include/rmclhip.h (atan2 in double, rounded to float; flags 0), so the image equals the device's -- the tool checks that.
#include <cmath>
#include <cstdint>
#include <cstring>

extern "C" uint32_t pc2scan_host_loop(const uint8_t* data, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                                      uint32_t off_z, float phi_min, float phi_inc, uint32_t H, float theta_min, float theta_inc, uint32_t W,
                                      float range_min, float range_max, float* ranges) {
  const float empty = static_cast<float>(static_cast<double>(range_max) + 1.0);
  for (size_t c = 0; c < static_cast<size_t>(W) * H; ++c) ranges[c] = empty;
  uint32_t stored = 0;
  for (uint32_t i = 0; i < n_points; ++i) {
    const uint8_t* p = data + static_cast<size_t>(i) * point_step;
    float x, y, z;
    std::memcpy(&x, p + off_x, 4);
    std::memcpy(&y, p + off_y, 4);
    std::memcpy(&z, p + off_z, 4);
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
    const float range = std::sqrt((x * x + y * y) + z * z);
    const float theta = static_cast<float>(std::atan2(static_cast<double>(y), static_cast<double>(x)));
    const float phi = static_cast<float>(std::atan2(static_cast<double>(z), static_cast<double>(range)));
    const double pc = std::trunc(static_cast<double>((phi - phi_min) / phi_inc) + 0.5);
    const double tc = std::trunc(static_cast<double>((theta - theta_min) / theta_inc) + 0.5);
    if (!(pc >= 0.0 && pc < static_cast<double>(H) && tc >= 0.0 && tc < static_cast<double>(W))) continue;
    if (!(range_min <= range && range <= range_max)) continue;
    ranges[static_cast<size_t>(pc) * W + static_cast<size_t>(tc)] = range;
    ++stored;
  }
  return stored;
}
