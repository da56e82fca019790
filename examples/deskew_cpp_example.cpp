// deskew_cpp_example.cpp -- a sensor_msgs/PointCloud2 taken WHILE THE SENSOR MOVED, through include/rmcl_hip/rmcl_hip.hpp:
//   two odometry poses (the tf lookups at the scan's first and last stamp) -> ScanMotion::fromBasePoses
//   cloud bytes + per-point time + motion -> RCCHipOnDn::setInputPointCloud2Deskewed -> correctOnce
// Every ray is cast from the pose the sensor had when it measured it (an OnDn model), and the dataset points are moved into the frame
// of the reference stamp -- one device pass, no host loop over the points.  The same bytes through an operator that takes the scan as
// taken from one pose end decimetres off (tests/test_gpu_deskew.py shows both).
//
//   g++ -std=c++17 -Iinclude examples/deskew_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o deskew_example
//   ./deskew_example mesh.bin cloud.bin width
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32; cloud.bin: the message's `data`, `width` points per row, 16-byte points
//       {x, y, z, time: f32}, each in the sensor's own frame at its own time; time in [0, 1]: the scan's first to its last stamp
//
// Prints one "key value..." line per result; tests/test_gpu_deskew_example.py compares them with the Python path on the same input.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

static rm::Transform yaw_pose(float x, float y, float z, double yaw) {
  rm::Transform T = rm::identity();
  T.R.z = static_cast<float>(std::sin(yaw / 2));
  T.R.w = static_cast<float>(std::cos(yaw / 2));
  T.t = {x, y, z};
  return T;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s mesh.bin cloud.bin width\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size()) return 2;
  if (std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);

  fh = std::fopen(argv[2], "rb");
  if (!fh) { std::perror("cloud"); return 2; }
  std::vector<uint8_t> cloud;
  uint8_t chunk[4096];
  for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), fh)) != 0;) cloud.insert(cloud.end(), chunk, chunk + got);
  std::fclose(fh);
  const uint32_t point_step = 16u;
  const uint32_t width = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0));
  if (width == 0u) return 2;
  const uint32_t height = static_cast<uint32_t>(cloud.size() / point_step / width);
  // the fields of the message: x, y, z FLOAT32 at 0 / 4 / 8, time FLOAT32 at 12 (seconds since the scan's first stamp)
  const rmclhip_pointcloud2_layout layout{width, height, point_step, width * point_step, 0u, 4u, 8u, 7u};
  const rmclhip_pointcloud2_time time_field{12u, 7u, 1.0, 0.0};

  // odometry at the scan's first and last stamp: 0.4 m forward and 0.15 rad of yaw in between.  The node localises at the LAST stamp.
  const rm::Transform T_o_b_last = yaw_pose(0.5f, -0.3f, 0.2f, 0.4);
  const rm::Transform T_o_b_first = T_o_b_last * ~yaw_pose(0.4f, 0.0f, 0.0f, 0.15);
  const rm::Transform Tsb = rm::identity();
  const rm::Transform Tom = rm::identity();                                          // odom is the map here: the truth is T_o_b_last
  const rm::Transform Tbo_est = T_o_b_last * yaw_pose(0.1f, 0.1f, 0.0f, 0.05);      // the estimate the correction starts from

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);

    // 16 slerp knots per segment: the device's nlerp between them is below float resolution for this turn
    const rm::ScanMotion motion = rm::ScanMotion::fromBasePoses(Tsb, {T_o_b_first, T_o_b_last}, {0.0, 1.0}, 1.0, 16u);
    std::printf("knots %zu\n", motion.knots.size());
    std::printf("first_knot_t %.9g %.9g %.9g\n", motion.knots.front().t.x, motion.knots.front().t.y, motion.knots.front().t.z);

    rm::RCCHipOnDn rcc(map);
    rcc.setTsb(Tsb);
    rcc.params.max_dist = 1.0f;
    rcc.adaptive_max_dist_min = 1.0f;
    uint32_t model_w = 0, model_h = 0;
    const rmclhip_deskew_stats st = rcc.setInputPointCloud2Deskewed(cloud.data(), cloud.size(), layout, time_field, motion, rm::Interval{0.1f, 100.0f},
                                                                    nullptr, nullptr, false, &model_w, &model_h);
    std::printf("stats %u %u %u %u %u\n", st.n_points, st.n_finite, st.n_valid, st.n_time_clamped, st.n_time_nonfinite);
    std::printf("model %u %u\n", model_w, model_h);
    rm::CrossStatistics so;
    const rm::Transform T_onew_oold = rcc.correctOnce(Tom, Tbo_est, 40, 0.0, true, &so);
    const rm::Transform Tbm = Tom * T_onew_oold * Tbo_est;
    std::printf("pose_t %.9g %.9g %.9g\n", Tbm.t.x, Tbm.t.y, Tbm.t.z);
    std::printf("pose_q %.9g %.9g %.9g %.9g\n", Tbm.R.x, Tbm.R.y, Tbm.R.z, Tbm.R.w);
    std::printf("truth_t %.9g %.9g %.9g\n", T_o_b_last.t.x, T_o_b_last.t.y, T_o_b_last.t.z);
    std::printf("n_meas %u\n", so.n_meas);

    // the cloud form: the compensated points alone, for a consumer that needs no rays (closest-point correspondences, a viewer)
    rm::Pc2DeskewHip conv(ctx);
    conv.time_ = time_field;
    conv.range_ = rm::Interval{0.1f, 100.0f};
    const rm::DeviceView<const float> pts = conv.convert(cloud.data(), cloud.size(), layout, motion);
    std::printf("cloud_form %zu %u\n", pts.size() / 3, conv.stats().n_valid);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
