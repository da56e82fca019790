// motion_noise_cpp_example.cpp -- the sampled odometry model through include/rmcl_hip/rmcl_hip.hpp: a cloud around a pose guess is moved
// by odometry steps, and every particle's step is composed with its own Gaussian draw whose spread follows the step
// (TFMotionUpdaterHip::setNoise).  A robot that stands does not diffuse; one that turns spreads in yaw.  The reference has no such
// model: its resamplers' constant noise stands in for it (ResidualResamplerCPU.cpp:92-94).
//
//   g++ -std=c++17 -Iinclude examples/motion_noise_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o motion_noise_example
//   ./motion_noise_example mesh.bin cloud_out.bin [n_particles [seed]]
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       cloud_out.bin: u32 n, n poses (32 B each), n attributes (36 B each) -- the cloud after the last step
//
// Prints one "key value..." line per result; tests/test_gpu_motion_noise.py compares them, and the dumped cloud, with the Python binding's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

static double spread_x(const rm::Memory<rm::Transform, rm::RAM>& poses, size_t n) {
  double s = 0.0, s2 = 0.0;
  for (size_t i = 0; i < n; i++) { s += poses[i].t.x; s2 += static_cast<double>(poses[i].t.x) * poses[i].t.x; }
  return std::sqrt(s2 / n - (s / n) * (s / n));
}

int main(int argc, char** argv) {
  if (argc < 3 || argc > 5) { std::fprintf(stderr, "usage: %s mesh.bin cloud_out.bin [n_particles [seed]]\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size()) return 2;
  if (std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);
  const size_t n = argc > 3 ? std::strtoul(argv[3], nullptr, 10) : 1000;
  const uint64_t seed = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 42;

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);

    // ---- a cloud in a small box 1 m in front of a wall, heading towards it ---------------------------------------------------------
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.resize(n);
    const float bb_min[6] = {3.4f, -2.0f, -0.5f, 0.0f, 0.0f, -0.3f}, bb_max[6] = {4.0f, 2.0f, 0.5f, 0.0f, 0.0f, 0.3f};
    rm::initSamplesUniform(cloud, bb_min, bb_max, seed, 0);
    rm::Memory<rm::Transform, rm::RAM> poses;
    rm::Memory<rm::ParticleAttributes, rm::RAM> attrs;
    cloud.poses.download(poses);
    std::vector<rm::Transform> poses0(n);
    std::vector<rm::ParticleAttributes> attrs0(n);
    cloud.attrs.download(attrs);
    std::memcpy(poses0.data(), &poses[0], n * sizeof(rm::Transform));
    std::memcpy(attrs0.data(), &attrs[0], n * sizeof(rm::ParticleAttributes));
    std::printf("spread_x_0 %.9g\n", spread_x(poses, n));

    // ---- the model: AMCL's alphas, but little lateral and no vertical slip ---------------------------------------------------------
    rm::MotionNoiseParams noise;
    noise.alpha_trans_trans[1] = 0.05f;
    noise.alpha_trans_trans[2] = 0.0f;
    noise.alpha_trans_rot[2] = 0.0f;
    rm::Transform stand = rm::identity(), drive = rm::identity();
    drive.R = {0.0f, 0.0f, 0.024997396f, 0.99968752f};   // yaw 0.05
    drive.t = {0.3f, 0.0f, 0.0f};
    const std::array<float, 6> s_stand = noise.sigma(stand), s_drive = noise.sigma(drive);
    std::printf("sigma_stand %.9g %.9g %.9g %.9g %.9g %.9g\n", s_stand[0], s_stand[1], s_stand[2], s_stand[3], s_stand[4], s_stand[5]);
    std::printf("sigma_drive %.9g %.9g %.9g %.9g %.9g %.9g\n", s_drive[0], s_drive[1], s_drive[2], s_drive[3], s_drive[4], s_drive[5]);

    rm::TFMotionUpdaterHip motion(map);
    motion.check_collision = true;
    motion.setNoise(noise, seed);
    motion.update(cloud.posesView(), cloud.attrsView(), stand, 0.0);      // step 0: standing still changes nothing
    cloud.poses.download(poses);
    std::printf("stand_unchanged %d\n", std::memcmp(&poses[0], poses0.data(), n * sizeof(rm::Transform)) == 0 ? 1 : 0);
    for (int k = 0; k < 3; k++) motion.update(cloud.posesView(), cloud.attrsView(), drive, 0.01);   // steps 1, 2, 3
    std::printf("steps %u\n", motion.step());
    cloud.poses.download(poses);
    cloud.attrs.download(attrs);
    size_t killed = 0;
    for (size_t i = 0; i < n; i++) killed += (attrs[i].likelihood.mean == 0.0f) ? 1 : 0;
    std::printf("spread_x_3 %.9g\n", spread_x(poses, n));
    std::printf("killed %zu\n", killed);

    // ---- the sharded filter draws the same noise: global particle indices, its own step count ---------------------------------------
    rm::PCDSensorUpdaterHipSharded sharded(std::vector<int>{0}, verts.data(), nv, faces.data(), nf);
    sharded.setParticles(poses0, attrs0);
    sharded.setNoise(noise, seed);
    sharded.motionUpdate(stand, 0.0, true);
    for (int k = 0; k < 3; k++) sharded.motionUpdate(drive, 0.01, true);
    std::vector<rm::Transform> ps;
    std::vector<rm::ParticleAttributes> as;
    sharded.download(ps, as);
    const bool same = std::memcmp(ps.data(), &poses[0], n * sizeof(rm::Transform)) == 0 &&
                      std::memcmp(as.data(), &attrs[0], n * sizeof(rm::ParticleAttributes)) == 0;
    std::printf("sharded_equal %d\n", same ? 1 : 0);
    motion.reset();
    sharded.reset();
    std::printf("steps_after_reset %u %u\n", motion.step(), sharded.motionStep());

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror("cloud_out"); return 2; }
    const uint32_t n32 = static_cast<uint32_t>(n);
    std::fwrite(&n32, 4, 1, out);
    std::fwrite(&poses[0], sizeof(rm::Transform), n, out);
    std::fwrite(&attrs[0], sizeof(rm::ParticleAttributes), n, out);
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
