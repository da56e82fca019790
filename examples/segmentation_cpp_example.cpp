// segmentation_cpp_example.cpp -- map segmentation on the device through include/rmcl_hip/rmcl_hip.hpp: what the reference's
// ScanMapSegmentationEmbreeNode / O1DnMapSegmentationEmbreeNode do per scan (rmcl_ros/src/nodes/filter/scan_map_segmentation_embree.cpp:
// 76-185, o1dn_map_segmentation_embree.cpp) as ONE call.  examples/simulator_cpp_example.cpp carries the same node with its body written
// out on the host (simulate, download 16 B per ray, classify in a loop); here the trace, the classification and the compaction of the
// two clouds stay on the device and two counts come back.
//
//   g++ -std=c++17 -Iinclude examples/segmentation_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o segmentation_example
//   ./segmentation_example mesh.bin scan.bin [qx qy qz qw tx ty tz]
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32; scan.bin: 32*32 f32 measured ranges; the sensor's pose in the map
//
// Prints one "key value..." line per result; tests/test_gpu_segmentation.py compares them with the decision rule restated in numpy.
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

// a cloud as a subscriber of `outlier_scan` / `outlier_map` would see it: width + the points (summed here)
static void print_cloud(const char* key, const rm::Memory<rm::Vector, rm::VRAM_HIP>& cloud) {
  rm::Memory<rm::Vector, rm::RAM> host;
  cloud.download(host);
  double sx = 0, sy = 0, sz = 0;
  for (size_t i = 0; i < host.size(); i++) { sx += host[i].x; sy += host[i].y; sz += host[i].z; }
  std::printf("%s %zu %.9g %.9g %.9g\n", key, host.size(), sx, sy, sz);
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 10) { std::fprintf(stderr, "usage: %s mesh.bin scan.bin [qx qy qz qw tx ty tz]\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size()) return 2;
  if (std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);

  const float pi = 3.14159265358979323846f;
  rm::SphericalModel model;
  model.phi = {-pi / 4, (pi / 2) / 31, 32};
  model.theta = {-pi, 2 * pi / 32, 32};
  model.range = {0.1f, 100.0f};
  rm::Memory<float, rm::RAM> ranges(model.size());
  fh = std::fopen(argv[2], "rb");
  if (!fh) { std::perror("scan"); return 2; }
  if (std::fread(ranges.raw(), 4, ranges.size(), fh) != ranges.size()) return 2;
  std::fclose(fh);

  rm::Transform T_sensor_map = from_rpy(0.5f, -0.3f, 0.2f, 0.02, -0.03, 0.4);
  if (argc == 10) {
    T_sensor_map.R = {std::strtof(argv[3], nullptr), std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)};
    T_sensor_map.t = {std::strtof(argv[7], nullptr), std::strtof(argv[8], nullptr), std::strtof(argv[9], nullptr)};
  }

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);

    // ---- ScanMapSegmentationEmbreeNode: the scan already lives in device memory (a driver that writes there, or the previous stage) ----
    {
      rm::ScanMapSegmentationHipNode node(map);
      rm::Memory<float, rm::VRAM_HIP> ranges_dev(ctx);
      ranges_dev = ranges;
      const rm::SegmentationCounts n = node.scanCB(model, rm::DeviceView<const float>{ranges_dev.raw(), ranges_dev.size()}, T_sensor_map);
      if (n.outlier_scan != node.cloud_outlier_scan_.size() || n.outlier_map != node.cloud_outlier_map_.size()) return 1;
      print_cloud("seg_outlier_scan", node.cloud_outlier_scan_);
      print_cloud("seg_outlier_map", node.cloud_outlier_map_);

      // ... and from a message in host memory, on the same node (the model did not change: nothing is re-sent)
      node.scanCB(model, ranges, T_sensor_map);
      print_cloud("seg_host_ranges_outlier_scan", node.cloud_outlier_scan_);
      print_cloud("seg_host_ranges_outlier_map", node.cloud_outlier_map_);
    }

    // ---- the simulator's own segment(): labels as well (the inlier set is the dataset mask of a following correction) ---------------
    {
      rm::SphereSimulatorHip sim(map);
      sim.setTsb(rm::identity());
      sim.setModel(model);
      rm::Memory<rm::Vector, rm::VRAM_HIP> outlier_scan, outlier_map;
      rm::Memory<uint8_t, rm::VRAM_HIP> labels;
      sim.segment(T_sensor_map, ranges, rm::SegmentationParams{}, outlier_scan, outlier_map, &labels);
      rm::Memory<uint8_t, rm::RAM> labels_host;
      labels.download(labels_host);
      size_t hist[4] = {0, 0, 0, 0};
      for (size_t i = 0; i < labels_host.size(); i++) hist[labels_host[i] & 3u]++;
      std::printf("seg_labels %zu %zu %zu %zu\n", hist[0], hist[1], hist[2], hist[3]);
    }

    // ---- O1DnMapSegmentationEmbreeNode: the same directions from an origin off the sensor frame's; the reference's pint_s (no origin
    //      when both ranges are valid) and the reading that adds it ---------------------------------------------------------------------
    {
      rm::O1DnModel o1;
      o1.width = model.getWidth(); o1.height = model.getHeight(); o1.range = model.range; o1.orig = rm::Vector{0.05f, -0.02f, 0.4f};
      for (uint32_t vid = 0; vid < model.getHeight(); vid++)
        for (uint32_t hid = 0; hid < model.getWidth(); hid++) o1.dirs.push_back(model.getDirection(vid, hid));
      rm::O1DnMapSegmentationHipNode node(map);
      node.scanCB(o1, ranges, T_sensor_map);
      print_cloud("o1dn_outlier_scan", node.cloud_outlier_scan_);
      print_cloud("o1dn_outlier_map", node.cloud_outlier_map_);
      node.pint_with_origin_ = true;
      node.scanCB(o1, ranges, T_sensor_map);
      print_cloud("o1dn_with_origin_outlier_scan", node.cloud_outlier_scan_);
      print_cloud("o1dn_with_origin_outlier_map", node.cloud_outlier_map_);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
