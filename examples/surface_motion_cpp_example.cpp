// surface_motion_cpp_example.cpp -- a ground robot's particles kept on the mesh it drives on, through include/rmcl_hip/rmcl_hip.hpp:
// the cloud is created on the device, put on the surface below it (constrainToSurface), and then moved by three odometry steps with
// the constraint in the motion update's own launch (TFMotionUpdaterHip::surface).  The reference lists a MotionUpdater constrained to
// the mesh surface as an open item (docs/RMCL.md:69-72).
//
//   g++ -std=c++17 -Iinclude examples/surface_motion_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o surface_motion_example
//   ./surface_motion_example mesh.bin cloud_out.bin [n_particles [seed]]
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       cloud_out.bin: u32 n, n poses (32 B each), n attributes (36 B each) -- the cloud after the last step
//
// Prints one "key value..." line per result; tests/test_gpu_surface.py compares them, and the dumped cloud, with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

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

    // ---- global localisation of a ground robot: uniform in a box around the floor, then onto the floor -------------------------------
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.resize(n);
    const float bb_min[6] = {-9.0f, -9.0f, -0.3f, -0.1f, -0.1f, -3.14f}, bb_max[6] = {9.0f, 9.0f, 0.8f, 0.1f, 0.1f, 3.14f};
    rm::initSamplesUniform(cloud, bb_min, bb_max, seed, 0);
    rm::SurfaceParams sp;
    sp.height = 0.1f;
    sp.probe_up = 0.5f;
    sp.probe_down = 1.0f;
    sp.align = 1u;
    const rm::SurfaceStats s0 = rm::constrainToSurface(map, cloud, sp);
    std::printf("constrain %u %u %u %u\n", s0.n_particles, s0.n_snapped, s0.n_missed, s0.n_steep);

    // ---- three odometry steps of 0.25 m with a slight turn; what leaves the floor or meets a wall taller than the step is killed --------
    rm::TFMotionUpdaterHip motion(map);
    motion.check_collision = true;
    motion.surface = sp;
    motion.surface->on_miss = 1u;
    rm::Transform step = rm::identity();
    step.R = {0.0f, 0.0f, 0.024997396f, 0.99968752f};   // yaw 0.05
    step.t = {0.25f, 0.0f, 0.0f};
    for (int k = 0; k < 3; k++) {
      motion.update(cloud.posesView(), cloud.attrsView(), step, 0.01);
      const rm::SurfaceStats sk = motion.surfaceStats();
      std::printf("step_%d %u %u %u %u\n", k, sk.n_particles, sk.n_snapped, sk.n_missed, sk.n_steep);
    }

    rm::Memory<rm::Transform, rm::RAM> poses;
    rm::Memory<rm::ParticleAttributes, rm::RAM> attrs;
    cloud.poses.download(poses);
    cloud.attrs.download(attrs);
    size_t killed = 0;
    for (size_t i = 0; i < n; i++) killed += (attrs[i].likelihood.mean == 0.0f) ? 1 : 0;
    std::printf("killed %zu\n", killed);
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
