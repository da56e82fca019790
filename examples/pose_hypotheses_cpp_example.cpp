// pose_hypotheses_cpp_example.cpp -- a particle cloud whose posterior still has two modes, through include/rmcl_hip/rmcl_hip.hpp.
// The node's estimateStats (rmcl_ros/src/nodes/rmcl_localization.cpp:642-731) reports ONE Markley mean and covariance; while two rooms
// explain the scan equally well that mean lies between them.  PoseEstimatorHip::estimateHypotheses groups the occupied bins of pose
// space (the bins of the adaptive resampler), weighs the groups and reports a mean and covariance per group, heaviest first.
//
//   g++ -std=c++17 -Iinclude examples/pose_hypotheses_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o pose_hypotheses_example
//   ./pose_hypotheses_example [n_particles [seed]]
//
// Prints one "key value..." line per result; tests/test_gpu_hypotheses.py compares them with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

static void print_estimate(const char* what, const rmclhip_pose_estimate& e) {
  std::printf("%s %u %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", what, e.n_particles, e.pose.t.x, e.pose.t.y, e.pose.t.z, e.pose.R.x, e.pose.R.y,
              e.pose.R.z, e.pose.R.w);
}

int main(int argc, char** argv) {
  if (argc > 3 || (argc > 1 && argv[1][0] == '-')) { std::fprintf(stderr, "usage: %s [n_particles [seed]]\n", argv[0]); return 2; }
  const size_t n = argc > 1 ? std::strtoul(argv[1], nullptr, 10) : 30000;
  const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 42;
  if (n < 3) { std::fprintf(stderr, "at least 3 particles\n"); return 2; }

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.resize(n);
    // two rooms that look alike: two thirds of the particles around one pose, the last third six metres further, turned round
    double cov[36] = {0};
    cov[0] = 0.04; cov[7] = 0.04; cov[35] = 0.01;
    rm::Transform a = rm::identity(), b = rm::identity();
    a.R = {0.0f, 0.0f, 0.19866933f, 0.98006658f};    // yaw 0.4
    a.t = {1.5f, -2.0f, 0.0f};
    b.R = {0.0f, 0.0f, -0.97572336f, 0.21900669f};   // yaw -2.7
    b.t = {7.5f, -2.0f, 0.0f};
    const size_t n_a = n - n / 3;
    rm::initSamples(*ctx, rm::DeviceView<rm::Transform>{cloud.poses.raw(), n_a}, rm::DeviceView<rm::ParticleAttributes>{cloud.attrs.raw(), n_a}, a,
                    cov, seed, 0, 0);
    rm::initSamples(*ctx, rm::DeviceView<rm::Transform>{cloud.poses.raw() + n_a, n - n_a},
                    rm::DeviceView<rm::ParticleAttributes>{cloud.attrs.raw() + n_a, n - n_a}, b, cov, seed, 0, static_cast<uint32_t>(n_a));

    rm::PoseEstimatorHip estimator(ctx);
    print_estimate("global", estimator.estimateStats(cloud));          // between the rooms
    const std::vector<rmclhip_pose_hypothesis> hyps = estimator.estimateHypotheses(cloud, 2);
    std::printf("clusters %u\n", estimator.last_clusters);
    for (size_t r = 0; r < hyps.size(); ++r) {
      char name[32];
      std::snprintf(name, sizeof(name), "hypothesis%zu", r);
      print_estimate(name, hyps[r].estimate);
      std::printf("share%zu %.9g %u\n", r, hyps[r].weight_share, hyps[r].n_bins);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
