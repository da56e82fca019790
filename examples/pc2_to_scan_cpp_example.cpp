// pc2_to_scan_cpp_example.cpp -- an unorganised sensor_msgs/PointCloud2 feeding the SPHERICAL operators through
// include/rmcl_hip/rmcl_hip.hpp: what the reference's Pc2ToScanNode (rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213) does on one
// host thread -- transform, two atan2, bin into the (phi, theta) grid, later points overwrite earlier ones -- on the device, and
// without the scan ever coming back to the host:
//   cloud bytes -> RCCHipSpherical::setInputPointCloud2 -> correctOnce          (the MICP-L sensor; the model is set once)
//   cloud bytes -> Pc2ToScanHip::convert -> ScanMapSegmentationHipNode::scanCB   (the conversion node feeding the segmentation node)
//
//   g++ -std=c++17 -Iinclude examples/pc2_to_scan_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o pc2_to_scan_example
//   ./pc2_to_scan_example mesh.bin cloud.bin flags
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32; cloud.bin: the message's `data`, height 1, 22-byte points
//       {x, y, z, intensity: f32; ring: u16; time: f32} in the sensor frame; flags: an OR of RMCLHIP_PC2SCAN_* (0: the reference's rule)
//
// Prints one "key value..." line per result; tests/test_gpu_pc2scan.py compares them with the Python path on the same input.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

static rm::Transform from_rpy(float x, float y, float z, double roll, double pitch, double yaw) {
  const double cr = std::cos(roll / 2), sr = std::sin(roll / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2);
  const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2);
  rm::Transform T = rm::identity();
  T.R.x = static_cast<float>(sr * cp * cy - cr * sp * sy);
  T.R.y = static_cast<float>(cr * sp * cy + sr * cp * sy);
  T.R.z = static_cast<float>(cr * cp * sy - sr * sp * cy);
  T.R.w = static_cast<float>(cr * cp * cy + sr * sp * sy);
  T.t = {x, y, z};
  return T;
}

// FNV-1a, 64 bit, over the image's bytes: what a subscriber of the scan would compare
static unsigned long long digest(const rm::Context& ctx, const rm::DeviceView<const float>& ranges) {
  rm::Memory<float, rm::RAM> host;
  rm::download(ctx, ranges, host);
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(host.raw());
  for (size_t i = 0; i < host.size() * sizeof(float); i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s mesh.bin cloud.bin flags\n", argv[0]); return 2; }
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
  const uint32_t point_step = 22u;
  const uint32_t n_points = static_cast<uint32_t>(cloud.size() / point_step);
  // the fields of the message: x, y, z FLOAT32 at 0 / 4 / 8; height 1 = unorganised
  const rmclhip_pointcloud2_layout layout{n_points, 1u, point_step, n_points * point_step, 0u, 4u, 8u, 7u};
  const uint32_t flags = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0));

  const float pi = 3.14159265358979323846f;
  rm::SphericalModel model;
  model.phi = {-pi / 4, (pi / 2) / 31, 32};
  model.theta = {-pi, 2 * pi / 32, 32};
  model.range = {0.1f, 100.0f};
  const rm::Transform Tbm_truth = from_rpy(0.5f, -0.3f, 0.2f, 0.02, -0.03, 0.4);
  const rm::Transform Tbm_est = Tbm_truth * from_rpy(0.2f, 0.1f, 0.05f, 0.0, 0.0, 2.0 * 3.14159265358979323846 / 180.0);

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);

    // ---- the MICP-L sensor: model once, then per message cloud -> dataset -> correction ------------------------------------------
    {
      rm::RCCHipSpherical rcc(map);
      rcc.setTsb(rm::identity());
      rcc.setModel(model);
      rcc.params.max_dist = 1.0f;
      rcc.adaptive_max_dist_min = 0.15f;
      rmclhip_pc2scan_stats st{};
      const rm::DeviceView<const float> ranges = rcc.setInputPointCloud2(cloud.data(), cloud.size(), layout, nullptr, flags, false, &st);
      std::printf("stats %u %u %u %u %u\n", st.n_points, st.n_finite, st.n_in_image, st.n_in_range, st.n_cells_filled);
      std::printf("image_digest %llu\n", digest(*ctx, ranges));
      rm::CrossStatistics so;
      const rm::Transform T = rcc.correctOnce(rm::identity(), Tbm_est, 5, 0.0, false, &so);
      std::printf("correct_once_t %.9g %.9g %.9g\n", T.t.x, T.t.y, T.t.z);
      std::printf("correct_once_q %.9g %.9g %.9g %.9g\n", T.R.x, T.R.y, T.R.z, T.R.w);
      std::printf("correct_once_n_meas %u\n", so.n_meas);
      // the next message: the same call, nothing of the model is rebuilt
      const rm::DeviceView<const float> again = rcc.setInputPointCloud2(cloud.data(), cloud.size(), layout, nullptr, flags);
      std::printf("image_digest_again %llu\n", digest(*ctx, again));
    }

    // ---- Pc2ToScanNode -> ScanMapSegmentationEmbreeNode: the scan goes from one node to the next in device memory -----------------
    {
      rm::Pc2ToScanHip conv(ctx);
      conv.setModel(model);
      conv.flags_ = flags;
      const rm::DeviceView<const float> ranges = conv.convert(cloud.data(), cloud.size(), layout);
      std::printf("node_image_digest %llu\n", digest(*ctx, ranges));
      std::printf("node_stats %u %u %u %u %u\n", conv.stats().n_points, conv.stats().n_finite, conv.stats().n_in_image, conv.stats().n_in_range,
                  conv.stats().n_cells_filled);
      rm::ScanMapSegmentationHipNode node(map);
      const rm::SegmentationCounts n = node.scanCB(model, ranges, Tbm_est);
      std::printf("segment_counts %u %u\n", n.outlier_scan, n.outlier_map);
      // a cloud in another frame: the node's tf lookup becomes setSensorTransform
      conv.setSensorTransform(from_rpy(0.1f, 0.0f, 0.3f, 0.0, 0.0, 10.0 * 3.14159265358979323846 / 180.0));
      const rm::DeviceView<const float> moved = conv.convert(cloud.data(), cloud.size(), layout);
      std::printf("node_transformed %llu %u\n", digest(*ctx, moved), conv.stats().n_cells_filled);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
