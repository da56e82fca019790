// adaptive_resample_cpp_example.cpp -- the filter node's resample step with the particle count adopted, through
// include/rmcl_hip/rmcl_hip.hpp.  The reference's node takes the count a resampler returns (res.n_particles,
// rmcl_ros/src/nodes/rmcl_localization.cpp:633-639) and runs every stage on poses(0, n_particles_); its resamplers never change it
// ("Improve strategies to reduce the number of particles more intelligently", docs/RMCL.md).  AdaptiveResamplerHip does: the
// KLD-sampling bound on the occupied bins of pose space, then systematic resampling to that size.
//
//   g++ -std=c++17 -Iinclude examples/adaptive_resample_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o adaptive_resample_example
//   ./adaptive_resample_example cloud_out.bin [n_particles [seed]]
//       cloud_out.bin: u32 n, n poses (32 B each), n attributes (36 B each) -- the cloud after the last resample step
//
// Prints one "key value..." line per result; tests/test_gpu_adaptive.py compares them, and the dumped cloud, with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <utility>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

int main(int argc, char** argv) {
  if (argc < 2 || argc > 4) { std::fprintf(stderr, "usage: %s cloud_out.bin [n_particles [seed]]\n", argv[0]); return 2; }
  const size_t capacity = argc > 2 ? std::strtoul(argv[2], nullptr, 10) : 20000;
  const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 42;

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    // the node's particle double buffer: room for `capacity` particles each, n_particles of them in use
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx), cloud_next(ctx);
    cloud.resize(capacity);
    cloud_next.resize(capacity);
    size_t n_particles = capacity;

    rm::AdaptiveResamplerHip resampler(ctx);
    resampler.seed = seed;
    resampler.init();

    // one resample step of the node: poses(0, n_particles) -> the other buffer, whole; the count it returns is adopted
    auto resample = [&](const char* what) {
      const rm::ParticleUpdateDynamicResults res =
          resampler.update(rm::DeviceView<rm::Transform>{cloud.poses.raw(), n_particles},
                           rm::DeviceView<rm::ParticleAttributes>{cloud.attrs.raw(), n_particles}, cloud_next.posesView(), cloud_next.attrsView());
      std::swap(cloud, cloud_next);
      n_particles = res.n_particles;
      std::printf("%s %zu %u\n", what, n_particles, resampler.last_bins);
    };

    // ---- global localisation: uniform in a box -- nearly every particle has a bin of its own, the bound asks for all the room there is ----
    const float bb_min[6] = {-50.0f, -50.0f, 0.0f, 0.0f, 0.0f, -3.14f}, bb_max[6] = {50.0f, 50.0f, 0.0f, 0.0f, 0.0f, 3.14f};
    rm::initSamplesUniform(cloud, bb_min, bb_max, seed, 0);
    resample("global");

    // ---- converged: the cloud around one pose -- a few bins carry the posterior, the count follows ----------------------------------
    double cov[36] = {0};
    cov[0] = 0.04; cov[7] = 0.04; cov[35] = 0.01;
    rm::Transform guess = rm::identity();
    guess.R = {0.0f, 0.0f, 0.19866933f, 0.98006658f};   // yaw 0.4
    guess.t = {0.5f, -0.3f, 0.2f};
    n_particles = capacity;
    rm::initSamples(cloud, guess, cov, seed, 1);
    resample("converged");
    resample("again");   // ... and stays there: every later stage of the cycle pays for n_particles, not for the capacity

    rm::Memory<rm::Transform, rm::RAM> poses;
    rm::Memory<rm::ParticleAttributes, rm::RAM> attrs;
    cloud.poses.download(poses);
    cloud.attrs.download(attrs);
    std::FILE* out = std::fopen(argv[1], "wb");
    if (!out) { std::perror("cloud_out"); return 2; }
    const uint32_t n32 = static_cast<uint32_t>(n_particles);
    std::fwrite(&n32, 4, 1, out);
    std::fwrite(&poses[0], sizeof(rm::Transform), n_particles, out);
    std::fwrite(&attrs[0], sizeof(rm::ParticleAttributes), n_particles, out);
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
