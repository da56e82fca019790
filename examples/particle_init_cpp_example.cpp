// particle_init_cpp_example.cpp -- the particle cloud's first and last step through include/rmcl_hip/rmcl_hip.hpp: what the reference's
// RmclNode::initSamplesUniform, initSamples(PoseWithCovarianceStamped) and visualize do in host loops
// (rmcl_ros/src/nodes/rmcl_localization.cpp:277-342, 165-275, 797-879), here on the device: the cloud is created where the filter
// uses it, and 28 B per particle come back for the visualisation.
//
//   g++ -std=c++17 -Iinclude examples/particle_init_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o particle_init_example
//   ./particle_init_example mesh.bin [n_particles [seed]]
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32
//
// Prints one "key value..." line per result; tests/test_gpu_particle_init.py compares them with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

int main(int argc, char** argv) {
  if (argc < 2 || argc > 4) { std::fprintf(stderr, "usage: %s mesh.bin [n_particles [seed]]\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size()) return 2;
  if (std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);
  const size_t n = argc > 2 ? std::strtoul(argv[2], nullptr, 10) : 1000;
  const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 42;

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);

    // ---- global localisation: the cloud uniform in a box, one sensor update, the statistics the resampler starts from ----------------
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.resize(n);
    const float bb_min[6] = {-4.0f, -4.0f, -1.5f, 0.0f, 0.0f, -3.14f}, bb_max[6] = {4.0f, 4.0f, 1.5f, 0.0f, 0.0f, 3.14f};
    rm::initSamplesUniform(cloud, bb_min, bb_max, seed, 0);

    std::vector<rm::RangeMeasurement> beams(3);
    const rm::Vector dirs[3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.6f, 0.0f, 0.8f}};
    for (size_t b = 0; b < beams.size(); b++) {
      beams[b] = rm::RangeMeasurement{};
      beams[b].dir = dirs[b];
      beams[b].range = 3.0f + static_cast<float>(b);
    }
    rm::PCDSensorUpdaterHip updater(map);
    updater.setInput(beams, rm::identity());
    updater.update(cloud.posesView(), cloud.attrsView());
    rm::GladiatorResamplerHip resampler(ctx);
    const rmclhip_likelihood_stats st = resampler.computeStats(cloud.attrsView());
    std::printf("uniform_stats %.9g %.9g\n", st.sum, st.max);

    // ---- what RViz would show of it: seven float arrays instead of the 68-B records and a host loop --------------------------------------
    rm::Memory<float, rm::RAM> viz;
    rm::packVisualization(*ctx, rm::DeviceView<const rm::Transform>{cloud.poses.raw(), n},
                          rm::DeviceView<const rm::ParticleAttributes>{cloud.attrs.raw(), n}, viz);
    double sums[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t c = 0; c < 7; c++)
      for (size_t i = 0; i < n; i++) sums[c] += viz[c * n + i];
    std::printf("viz_sums %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", sums[0], sums[1], sums[2], sums[3], sums[4], sums[5], sums[6]);

    // ---- /initialpose: a pose guess with RViz's covariance (x, y and yaw only), the same update -----------------------------------------
    double cov[36] = {0};
    cov[0] = 0.25; cov[7] = 0.25; cov[35] = 0.0685;
    rm::Transform guess = rm::identity();
    guess.R = {0.0f, 0.0f, 0.19866933f, 0.98006658f};   // yaw 0.4
    guess.t = {0.5f, -0.3f, 0.2f};
    const double chol_err = rm::initSamples(cloud, guess, cov, seed, 1);
    updater.update(cloud.posesView(), cloud.attrsView());
    const rmclhip_likelihood_stats sp = resampler.computeStats(cloud.attrsView());
    std::printf("pose_stats %.9g %.9g\n", sp.sum, sp.max);
    std::printf("pose_chol_err %.17g\n", chol_err);
    rm::Memory<rm::Transform, rm::RAM> poses;
    cloud.poses.download(poses);
    size_t off_plane = 0;
    for (size_t i = 0; i < n; i++) off_plane += (poses[i].t.z != guess.t.z || poses[i].R.x != 0.0f || poses[i].R.y != 0.0f) ? 1 : 0;
    std::printf("pose_off_plane %zu\n", off_plane);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
