// band_field_cpp_example.cpp -- a fine distance field on a map whose dense lattice is refused, through include/rmcl_hip/rmcl_hip.hpp:
//   the outline of a 100 m x 100 m x 3 m building (four walls) at a cell of 0.05 m is 2.4e8 lattice nodes: DistanceFieldHip refuses it
//   DistanceFieldHip::banded stores the fine nodes only in the bricks within `band` of a wall and answers the rest from a coarse lattice
//   the handle is a DistanceFieldHip: the lookup, PCDSensorUpdaterHip::setField + update and refine work on it unchanged
//
//   g++ -std=c++17 -Iinclude examples/band_field_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o band_field_example
//   ./band_field_example [cell [band]]
//
// Prints what it did, and "OK" when every check held; tests/test_gpu_band_field.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

int main(int argc, char** argv) {
  const float cell = argc > 1 ? static_cast<float>(std::atof(argv[1])) : 0.05f;
  const float band = argc > 2 ? static_cast<float>(std::atof(argv[2])) : 0.5f;
  const float L = 100.0f, H = 3.0f;
  const std::vector<float> verts = {0, 0, 0, L, 0, 0, L, L, 0, 0, L, 0, 0, 0, H, L, 0, H, L, L, H, 0, L, H};
  const std::vector<uint32_t> faces = {0, 1, 5, 0, 5, 4, 1, 2, 6, 1, 6, 5, 2, 3, 7, 2, 7, 6, 3, 0, 4, 3, 4, 7};
  bool ok = true;
  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), 8u, faces.data(), 8u);

    try {
      rm::DistanceFieldHip dense(map, rm::FieldParams(cell, 0.0f));
      std::printf("dense field built: %llu nodes\n", static_cast<unsigned long long>(dense.info().n_nodes));
    } catch (const std::exception& e) {
      std::printf("dense field refused: %s\n", e.what());
    }

    auto field = rm::DistanceFieldHip::banded(map, rm::BandFieldParams(cell, 0.0f, band));
    const rm::FieldInfo fi = field->info();
    const rm::BandFieldInfo bi = field->bandInfo();
    std::printf("banded field built: %u x %u x %u logical nodes (%.0f MB dense), %llu of %llu bricks stored, %.1f MB\n", fi.n[0], fi.n[1], fi.n[2],
                4e-6 * static_cast<double>(fi.n_nodes), static_cast<unsigned long long>(bi.n_stored),
                static_cast<unsigned long long>(bi.n_bricks), 1e-6 * static_cast<double>(bi.bytes));

    // the lookup: 0.2 m in front of a wall (a stored brick: within (sqrt(3) / 2) cell of the truth), and the middle of the hall (a far
    // brick: some distance beyond the band)
    const std::vector<rm::Vector> where = {{30.0f, 0.2f, 1.5f}, {99.8f, 40.0f, 1.0f}, {50.0f, 50.0f, 1.5f}};
    const std::vector<float> dist = field->query(where);
    std::printf("query %.6f %.6f %.6f\n", dist[0], dist[1], dist[2]);
    const float tol = 0.8660254f * fi.cell;
    ok = ok && std::fabs(dist[0] - 0.2f) <= tol && std::fabs(dist[1] - 0.2f) <= tol && dist[2] > band;

    // one sensor update of two particles with one beam that ends 0.1 m in front of the wall y = 0 for the first of them
    std::vector<rm::RangeMeasurement> beams(1);
    beams[0] = rm::RangeMeasurement{};
    beams[0].orig = {0.0f, 0.0f, 0.0f};
    beams[0].dir = {0.0f, -1.0f, 0.0f};
    beams[0].range = 4.9f;
    rm::Memory<rm::Transform, rm::RAM> h_poses(2);
    rm::Memory<rm::ParticleAttributes, rm::RAM> h_attrs(2);
    for (size_t i = 0; i < 2; ++i) {
      h_poses[i] = rm::identity();
      h_attrs[i] = rm::ParticleAttributes{};
    }
    h_poses[0].t = {30.0f, 5.0f, 1.5f};
    h_poses[1].t = {30.0f, 50.0f, 1.5f};
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.poses = h_poses;
    cloud.attrs = h_attrs;
    rm::Memory<float, rm::VRAM_HIP> errors(ctx);
    errors.resize(2);
    rm::PCDSensorUpdaterHip updater(map);
    updater.config_.correspondence_type = 1u;
    updater.setField(field);
    updater.setErrorOutput(errors.raw());
    updater.setInput(beams, rm::identity());
    updater.update(cloud.posesView(), cloud.attrsView());
    rm::Memory<float, rm::RAM> h_err;
    errors.download(h_err);
    std::printf("errors %.6f %.6f\n", h_err[0], h_err[1]);
    ok = ok && std::fabs(h_err[0] - 0.1f) <= tol && h_err[1] > band;

    // refine within the band: the first particle is pulled onto the wall its beam saw, the second has no beam within max_dist
    rm::RefineParams rp;
    rp.max_dist = band;
    const rm::RefineStats st = updater.refine(cloud.posesView(), rp);
    std::printf("refine moved %u of %u, %u without beams\n", st.n_moved, st.n_particles, st.n_no_beams);
    ok = ok && st.n_moved == 1u && st.n_no_beams == 1u;
    // beyond the band the field holds no fine values: refused
    rp.max_dist = 2.0f * band;
    try {
      updater.refine(cloud.posesView(), rp);
      ok = false;
    } catch (const std::exception& e) {
      std::printf("refine with max_dist > band refused: %s\n", e.what());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
