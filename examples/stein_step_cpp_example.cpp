// stein_step_cpp_example.cpp -- a cloud moved towards the map WITHOUT collapsing onto it, through include/rmcl_hip/rmcl_hip.hpp:
//   a map -> DistanceFieldHip -> PCDSensorUpdaterHip::setField -> a cloud drawn around a pose guess (initSamples)
//   -> PCDSensorUpdaterHip::steinStep -> one sensor update
// A Stein variational step moves every particle by the kernel-weighted average of its neighbours' Gauss-Newton steps on the field and
// pushes it away from its neighbours; it moves poses and leaves the likelihood attributes alone, so the sensor update comes after it.
//
//   hipcc -std=c++17 -Iinclude examples/stein_step_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o stein_step_example
//   ./stein_step_example mesh.bin guess.bin beams.bin [cell [margin [n_particles [iterations]]]]
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       guess.bin: u32 1, one pose (32 B): the centre of the cloud
//       beams.bin: u32 n, n range measurements (64 B each), sensor frame; the sensor sits at the base (Tsb = identity)
//
// Prints one "key value..." line per result; tests/test_gpu_stein.py compares them with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

template <typename T>
static bool read_records(const char* path, std::vector<T>& a) {
  std::FILE* fh = std::fopen(path, "rb");
  if (!fh) { std::perror(path); return false; }
  uint32_t n = 0;
  bool ok = std::fread(&n, 4, 1, fh) == 1;
  a.resize(n);
  ok = ok && std::fread(a.data(), sizeof(T), n, fh) == n;
  std::fclose(fh);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 4 || argc > 8) {
    std::fprintf(stderr, "usage: %s mesh.bin guess.bin beams.bin [cell [margin [n_particles [iterations]]]]\n", argv[0]);
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size()) return 2;
  if (std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);
  std::vector<rm::Transform> guess;
  std::vector<rm::RangeMeasurement> beams;
  if (!read_records(argv[2], guess) || !read_records(argv[3], beams)) return 2;
  if (guess.size() != 1 || beams.empty()) return 2;
  const float cell = argc > 4 ? static_cast<float>(std::atof(argv[4])) : 0.0f;
  const float margin = argc > 5 ? static_cast<float>(std::atof(argv[5])) : 0.5f;
  const size_t n = argc > 6 ? static_cast<size_t>(std::atol(argv[6])) : 64u;
  const uint32_t iterations = argc > 7 ? static_cast<uint32_t>(std::atol(argv[7])) : 4u;

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);
    auto field = std::make_shared<rm::DistanceFieldHip>(map, rm::FieldParams(cell, margin));
    rm::PCDSensorUpdaterHip updater(map);
    updater.config_.correspondence_type = 1u;
    updater.setField(field);
    updater.setInput(beams, rm::identity());

    // a cloud around the guess: sigma 0.15 m in x, y, z and 0.08 rad in yaw
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.resize(n);
    double covariance[36] = {0.0};
    covariance[0] = covariance[7] = covariance[14] = 0.15 * 0.15;
    covariance[35] = 0.08 * 0.08;
    rm::initSamples(cloud, guess[0], covariance, 7u);

    rm::SteinParams params;   // bandwidths 0.25 m and 0.2 rad, repulsion 0.25
    params.iterations = iterations;
    rm::Memory<rm::SteinResult, rm::VRAM_HIP> rows(ctx);
    rows.resize(n);
    const rm::SteinStats st = updater.steinStep(cloud.posesView(), params, rm::DeviceView<rm::SteinResult>{rows.raw(), rows.size()});
    std::printf("particles %u not_finite %u no_beams %u bins %u thinned_bins %u\n", st.n_particles, st.n_not_finite, st.n_no_beams, st.n_bins,
                st.n_thinned_bins);
    std::printf("cost_sum %.17g\n", st.cost_sum);
    rm::Memory<rm::SteinResult, rm::RAM> h_rows;
    rows.download(h_rows);
    std::printf("rows");
    for (size_t i = 0; i < h_rows.size() && i < 3; ++i)
      std::printf(" %.9g %u %u %.9g", h_rows[i].cost, h_rows[i].n_used, h_rows[i].n_neighbours, h_rows[i].kernel_weight);
    std::printf("\n");

    // the moved poses have not been scored: one closest-point sensor update from the same field
    updater.update(cloud.posesView(), cloud.attrsView());
    rm::Memory<rm::ParticleAttributes, rm::RAM> h_attrs;
    cloud.attrs.download(h_attrs);
    std::printf("means");
    for (size_t i = 0; i < h_attrs.size() && i < 3; ++i) std::printf(" %.9g", h_attrs[i].likelihood.mean);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
