// distance_field_cpp_example.cpp -- the closest-point sensor update answered by lookup, through include/rmcl_hip/rmcl_hip.hpp:
//   a map -> DistanceFieldHip (a lattice of distances to the closest triangle, built on the device once)
//   PCDSensorUpdaterHip with correspondence_type 1 + setField -> one update of a particle cloud
// The beam error is the distance of the beam's end point to the surface -- the likelihood-field model -- read from the lattice with
// eight loads and a trilinear blend instead of one tree query per (particle, beam).
//
//   g++ -std=c++17 -Iinclude examples/distance_field_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o distance_field_example
//   ./distance_field_example mesh.bin particles.bin beams.bin [cell [margin]]
//       mesh.bin: u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       particles.bin: u32 n, n poses (32 B each), n attributes (36 B each)
//       beams.bin: u32 n, n range measurements (64 B each), sensor frame; the sensor sits at the base (Tsb = identity)
//
// Prints one "key value..." line per result; tests/test_gpu_field.py compares them with the Python binding's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

template <typename T>
static bool read_records(const char* path, std::vector<T>& a, std::vector<rm::ParticleAttributes>* b = nullptr) {
  std::FILE* fh = std::fopen(path, "rb");
  if (!fh) { std::perror(path); return false; }
  uint32_t n = 0;
  bool ok = std::fread(&n, 4, 1, fh) == 1;
  a.resize(n);
  ok = ok && std::fread(a.data(), sizeof(T), n, fh) == n;
  if (b) {
    b->resize(n);
    ok = ok && std::fread(b->data(), sizeof(rm::ParticleAttributes), n, fh) == n;
  }
  std::fclose(fh);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 4 || argc > 6) { std::fprintf(stderr, "usage: %s mesh.bin particles.bin beams.bin [cell [margin]]\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size()) return 2;
  if (std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);
  std::vector<rm::Transform> poses;
  std::vector<rm::ParticleAttributes> attrs;
  std::vector<rm::RangeMeasurement> beams;
  if (!read_records(argv[2], poses, &attrs) || !read_records(argv[3], beams)) return 2;
  if (poses.empty() || beams.empty()) return 2;
  const float cell = argc > 4 ? static_cast<float>(std::atof(argv[4])) : 0.0f;
  const float margin = argc > 5 ? static_cast<float>(std::atof(argv[5])) : 0.0f;

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);

    auto field = std::make_shared<rm::DistanceFieldHip>(map, rm::FieldParams(cell, margin));
    const rm::FieldInfo fi = field->info();
    std::printf("nodes %u %u %u\n", fi.n[0], fi.n[1], fi.n[2]);
    std::printf("origin %.9g %.9g %.9g\n", fi.origin[0], fi.origin[1], fi.origin[2]);
    std::printf("cell %.9g %.9g\n", fi.cell, fi.inv_cell);
    std::printf("size %llu %llu\n", static_cast<unsigned long long>(fi.n_nodes), static_cast<unsigned long long>(fi.bytes));

    // the lookup alone: the distance of the first three particles' positions to the surface
    std::vector<rm::Vector> where;
    for (size_t i = 0; i < poses.size() && i < 3; ++i) where.push_back(poses[i].t);
    const std::vector<float> dist = field->query(where);
    std::printf("query");
    for (float d : dist) std::printf(" %.9g", d);
    std::printf("\n");

    // one sensor update: closest-point errors (correspondence_type 1) from the field
    rm::Memory<rm::Transform, rm::RAM> h_poses(poses.size());
    rm::Memory<rm::ParticleAttributes, rm::RAM> h_attrs(attrs.size());
    for (size_t i = 0; i < poses.size(); ++i) { h_poses[i] = poses[i]; h_attrs[i] = attrs[i]; }
    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx);
    cloud.poses = h_poses;
    cloud.attrs = h_attrs;
    rm::Memory<float, rm::VRAM_HIP> errors(ctx);
    errors.resize(poses.size() * beams.size());

    rm::PCDSensorUpdaterHip updater(map);
    updater.config_.correspondence_type = 1u;
    updater.setField(field);
    updater.setErrorOutput(errors.raw());
    updater.setInput(beams, rm::identity());
    updater.update(cloud.posesView(), cloud.attrsView());

    rm::Memory<float, rm::RAM> h_err;
    errors.download(h_err);
    cloud.attrs.download(h_attrs);
    std::printf("errors");
    for (size_t i = 0; i < h_err.size() && i < 3; ++i) std::printf(" %.9g", h_err[i]);
    std::printf("\n");
    std::printf("means");
    for (size_t i = 0; i < h_attrs.size() && i < 3; ++i) std::printf(" %.9g", h_attrs[i].likelihood.mean);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
