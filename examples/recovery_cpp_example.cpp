// recovery_cpp_example.cpp -- global localisation on the surface and recovery from a kidnapping, through include/rmcl_hip/rmcl_hip.hpp.
//
// A two-storey building: a 10 m x 10 m ground floor at z = 0 with walls, an upper floor at z = 3 whose room is cut to 4.5 m x 7 m by
// two more walls.  The cloud is initialised ON the two floors (SurfaceSamplerHip: uniform by area, no particle in the air or outside), the
// filter runs cycles of {sensor update from the distance field, likelihood statistics -> Recovery, adaptive resampler, injection} while
// the robot stands on the ground floor, then the robot is put on the upper floor without the filter being told.  The likelihood drops,
// the fast average falls below the slow one, and the injection brings particles back to both floors -- among them the right one.
//
//   g++ -std=c++17 -Iinclude examples/recovery_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o recovery_example
//   ./recovery_example run [n_particles [cycles_before [cycles_after [seed]]]]
//
// Prints one line per cycle: "cycle k floor F n N sum S p_inject P injected J share0 A share1 B" -- the floor the robot stands on, the
// particle count, the likelihood sum, what the recovery rule asked for and got, and the share of the cloud on each floor afterwards.
// The recovery alphas are 0.1 / 0.5, not AMCL's 0.001 / 0.1: those need hundreds of cycles, this example runs thirty.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;

namespace {

struct Rect { int axis; float at, lo[2], hi[2]; };   // the plane x_axis = at, bounded in the other two coordinates (in x y z order)

// ground floor, upper floor, four outer walls over both storeys, the upper floor's inner walls at x = 4.5 and y = 7
const Rect kRects[] = {{2, 0.f, {0.f, 0.f}, {10.f, 10.f}}, {2, 3.f, {0.f, 0.f}, {10.f, 10.f}}, {0, 0.f, {0.f, 0.f}, {10.f, 6.f}},
                       {0, 10.f, {0.f, 0.f}, {10.f, 6.f}}, {1, 0.f, {0.f, 0.f}, {10.f, 6.f}}, {1, 10.f, {0.f, 0.f}, {10.f, 6.f}},
                       {0, 4.5f, {0.f, 3.f}, {10.f, 6.f}}, {1, 7.f, {0.f, 3.f}, {10.f, 6.f}}};

void add_rect(const Rect& r, std::vector<float>& v, std::vector<uint32_t>& f) {
  const int a = (r.axis + 1) % 3, b = (r.axis + 2) % 3;   // the two free coordinates ...
  const int lo_a = a < b ? 0 : 1, lo_b = 1 - lo_a;        // ... and where the rectangle keeps their bounds (x y z order)
  const uint32_t k = static_cast<uint32_t>(v.size() / 3);
  const float ca[4] = {r.lo[lo_a], r.hi[lo_a], r.hi[lo_a], r.lo[lo_a]}, cb[4] = {r.lo[lo_b], r.lo[lo_b], r.hi[lo_b], r.hi[lo_b]};
  for (int c = 0; c < 4; ++c) {
    float p[3];
    p[r.axis] = r.at; p[a] = ca[c]; p[b] = cb[c];
    v.insert(v.end(), p, p + 3);
  }
  const uint32_t idx[6] = {k, k + 1, k + 2, k, k + 2, k + 3};
  f.insert(f.end(), idx, idx + 6);
}

// the range a beam from o along d (unit) measures in the building, or a negative value if it leaves it
float cast(const float o[3], const float d[3]) {
  float best = -1.f;
  for (const Rect& r : kRects) {
    if (std::fabs(d[r.axis]) < 1e-6f) continue;
    const float t = (r.at - o[r.axis]) / d[r.axis];
    if (t < 1e-3f || (best > 0.f && t >= best)) continue;
    const int a = (r.axis + 1) % 3, b = (r.axis + 2) % 3;
    const int lo_a = a < b ? 0 : 1, lo_b = 1 - lo_a;
    const float pa = o[a] + t * d[a], pb = o[b] + t * d[b];
    if (pa >= r.lo[lo_a] && pa <= r.hi[lo_a] && pb >= r.lo[lo_b] && pb <= r.hi[lo_b]) best = t;
  }
  return best;
}

// what the robot's sensor (at the base, `height` above the floor, yaw 0) measures at (x, y) on `floor`: 24 horizontal beams, 8 tilted up
std::vector<rm::RangeMeasurement> measure(float x, float y, int floor, float height) {
  std::vector<rm::RangeMeasurement> beams;
  const float o[3] = {x, y, 3.f * static_cast<float>(floor) + height};
  for (int k = 0; k < 32; ++k) {
    const float az = 6.2831853f * static_cast<float>(k % 24) / 24.f + (k >= 24 ? 0.4f : 0.f), el = k >= 24 ? 0.6f : 0.f;
    const float d[3] = {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)};
    const float range = cast(o, d);
    if (range < 0.f) continue;
    rm::RangeMeasurement m;
    std::memset(&m, 0, sizeof(m));
    m.dir = {d[0], d[1], d[2]};
    m.range = range;
    m.cov[0] = m.cov[4] = m.cov[8] = 0.1f;
    beams.push_back(m);
  }
  return beams;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || argc > 6 || std::strcmp(argv[1], "run") != 0) {
    std::fprintf(stderr, "usage: %s run [n_particles [cycles_before [cycles_after [seed]]]]\n", argv[0]);
    return 2;
  }
  const size_t capacity = argc > 2 ? std::strtoul(argv[2], nullptr, 10) : 20000;
  const int cycles_before = argc > 3 ? std::atoi(argv[3]) : 20, cycles_after = argc > 4 ? std::atoi(argv[4]) : 10;
  const uint64_t seed = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 42;
  const float height = 1.2f;   // of the sensor above the floor the robot stands on

  try {
    std::vector<float> verts;
    std::vector<uint32_t> faces;
    for (const Rect& r : kRects) add_rect(r, verts, faces);
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), static_cast<uint32_t>(verts.size() / 3), faces.data(),
                                            static_cast<uint32_t>(faces.size() / 3));

    // where the robot can stand: the two floors (the walls are too steep), the sensor `height` above them
    rm::SurfaceSampleParams sp;
    sp.height = height;
    rm::SurfaceSamplerHip sampler(map, sp);
    const rm::SurfaceSampleInfo si = sampler.info();
    std::printf("sampler faces %u eligible %u area %.9g\n", si.n_faces, si.n_eligible, si.area_eligible);

    rm::ParticleCloud<rm::VRAM_HIP> cloud(ctx), cloud_next(ctx);
    cloud.resize(capacity);
    cloud_next.resize(capacity);
    size_t n_particles = capacity;
    rm::initSamplesSurface(cloud, sampler, seed, 0);

    rm::PCDSensorUpdaterHip updater(map);
    updater.config_.correspondence_type = 1u;
    updater.config_.dist_sigma = 0.1f;
    updater.config_.max_n_meas = 64u;    // a short memory: the accumulated likelihood follows the last two scans
    updater.setField(std::make_shared<rm::DistanceFieldHip>(map, rm::FieldParams(0.1f, 1.0f)));

    rm::AdaptiveResamplerHip resampler(ctx);
    resampler.seed = seed;
    resampler.init();
    rm::Recovery recovery(0.1, 0.5);

    for (int cycle = 0; cycle < cycles_before + cycles_after; ++cycle) {
      const int floor = cycle < cycles_before ? 0 : 1;   // the kidnapping: nobody tells the filter
      updater.setInput(measure(3.0f, 4.0f, floor, height), rm::identity());
      rm::DeviceView<rm::Transform> poses{cloud.poses.raw(), n_particles};
      rm::DeviceView<rm::ParticleAttributes> attrs{cloud.attrs.raw(), n_particles};
      updater.update(poses, attrs);
      const rmclhip_likelihood_stats stats = resampler.computeStats(attrs);
      // statistics -> recovery averages -> resampler -> injection -> reset when anything was injected
      const size_t n_new = resampler.update(poses, attrs, cloud_next.posesView(), cloud_next.attrsView(), recovery, sampler).n_particles;
      const double p_inject = resampler.last_p_inject;
      const uint32_t injected = resampler.last_injected;
      std::swap(cloud, cloud_next);
      n_particles = n_new;

      rm::Memory<rm::Transform, rm::RAM> h_poses;
      cloud.poses.download(h_poses);
      size_t on[2] = {0, 0};
      for (size_t i = 0; i < n_particles; ++i) ++on[h_poses[i].t.z < 1.5f + height ? 0 : 1];
      std::printf("cycle %d floor %d n %zu sum %.9g p_inject %.9g injected %u share0 %.6f share1 %.6f\n", cycle, floor, n_particles,
                  static_cast<double>(stats.sum), p_inject, injected, static_cast<double>(on[0]) / static_cast<double>(n_particles),
                  static_cast<double>(on[1]) / static_cast<double>(n_particles));
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
