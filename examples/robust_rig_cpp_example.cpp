// robust_rig_cpp_example.cpp -- MICP-L's correction of a two-sensor rig with M-estimator weights (include/rmclhip.h, ROBUST MICP FOR
// SENSOR RIGS), through include/rmcl_hip/rmcl_hip.hpp: a lidar in whose scan something stands in front of the mapped wall and a small
// clean depth sensor on another mount, corrected together by the plain rig loop and by the robust one, and the pose covariance each
// would publish.
//
//   g++ -std=c++17 -Iinclude examples/robust_rig_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o robust_rig_example
//   ./robust_rig_example mesh.bin lidar.bin depth.bin
//       mesh.bin:            u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       lidar.bin, depth.bin: u32 n, n*3 f32 points (sensor frame), n u8 mask -- one scan of the 32 x 32 / 16 x 16 model below
//
// Prints one "key value..." line per result; tests/test_gpu_robust_rig_example.py reads them.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

static rm::Transform from_rpy(float x, float y, float z, double roll, double pitch, double yaw) {
  const double cr = std::cos(roll / 2), sr = std::sin(roll / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2);
  const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2);
  rm::Transform T = rm::identity();
  T.R = {static_cast<float>(sr * cp * cy - cr * sp * sy), static_cast<float>(cr * sp * cy + sr * cp * sy),
         static_cast<float>(cr * cp * sy - sr * sp * cy), static_cast<float>(cr * cp * cy + sr * sp * sy)};
  T.t = {x, y, z};
  return T;
}

static bool read_scan(const char* path, uint32_t expect, rm::PointCloud_<rm::RAM>* out) {
  std::FILE* fh = std::fopen(path, "rb");
  if (!fh) { std::perror(path); return false; }
  uint32_t n = 0;
  bool ok = std::fread(&n, 4, 1, fh) == 1 && n == expect;
  if (ok) {
    out->points.resize(n);
    out->mask.resize(n);
    ok = std::fread(out->points.raw(), sizeof(rm::Vector), n, fh) == n && std::fread(out->mask.raw(), 1, n, fh) == n;
  }
  std::fclose(fh);
  if (!ok) std::fprintf(stderr, "%s: expected one scan of %u points\n", path, expect);
  return ok;
}

static double trace6(const rm::PoseCovariance& c) {
  double t = 0.0;
  for (int k = 0; k < 6; ++k) t += c.covariance[6 * k + k];
  return t;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s mesh.bin lidar.bin depth.bin\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size() || std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);
  rm::PointCloud_<rm::RAM> scan[2];
  if (!read_scan(argv[2], 32u * 32u, &scan[0]) || !read_scan(argv[3], 16u * 16u, &scan[1])) return 2;

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);
    const float pi = 3.14159265358979323846f;
    rm::SphericalModel lidar_model{}, depth_model{};
    lidar_model.phi = {-pi / 4, (pi / 2) / 31, 32};
    lidar_model.theta = {-pi, 2 * pi / 32, 32};
    lidar_model.range = {0.1f, 100.0f};
    depth_model.phi = {-pi / 8, (pi / 4) / 15, 16};
    depth_model.theta = {-pi / 4, (pi / 2) / 15, 16};
    depth_model.range = {0.1f, 100.0f};
    const rm::Transform Tsb[2] = {from_rpy(0.1f, 0.0f, 0.3f, 0, 0, 10.0 * pi / 180), from_rpy(-0.2f, 0.1f, 0.5f, 0, 0.1, -1.0)};
    const rm::Transform Tom = rm::identity();
    const rm::Transform truth = from_rpy(0.5f, -0.3f, 0.2f, 0.02, -0.03, 0.4);
    const rm::Transform estimate = truth * from_rpy(0.2f, 0.0f, 0.0f, 0, 0, 2.0 * pi / 180);   // 0.2 m / 2 degrees off
    const std::vector<rm::Transform> Tbo = {estimate, estimate};
    const std::vector<double> weights = {1.0, 0.37};   // merge_weight_multiplier: the rig trusts the small sensor less per measurement

    rm::RCCHipSpherical lidar(map), depth(map);
    rm::RCCHipSpherical* rcc[2] = {&lidar, &depth};
    for (int s = 0; s < 2; ++s) {
      rcc[s]->setTsb(Tsb[s]);
      rcc[s]->setModel(s == 0 ? lidar_model : depth_model);
      rcc[s]->params.max_dist = 1.0f;
      rcc[s]->adaptive_max_dist_min = 1.0f;
      rcc[s]->dataset.points = scan[s].points;   // upload
      rcc[s]->dataset.mask = scan[s].mask;
    }
    const std::vector<rm::CorrespondencesHIP*> sensors = {&lidar, &depth};

    // the plain rig loop (every gated-in correspondence at full weight) and the robust one, ten iterations each.  Every sensor has its own
    // parameters: its scale follows ITS residuals
    const rm::Transform T_plain = rm::correctOnce(sensors, Tom, Tbo, weights, 10, 0.0);
    const std::vector<rm::RobustParams> tukey = {rm::RobustParams(RMCLHIP_ROBUST_TUKEY), rm::RobustParams(RMCLHIP_ROBUST_TUKEY)};
    std::vector<rm::RobustStatistics> stats_s;
    rm::CrossStatistics merged;
    const rm::Transform T_robust = rm::correctOnceRobust(sensors, Tom, Tbo, weights, 10, 0.0, tukey, &merged, &stats_s);

    // the error each leaves: the corrected estimate against the truth
    const rm::Transform T_all[2] = {T_plain, T_robust};
    double err[2];
    for (int k = 0; k < 2; ++k) {
      const rm::Transform d = ~truth * (T_all[k] * estimate);
      err[k] = std::sqrt(static_cast<double>(d.t.x) * d.t.x + static_cast<double>(d.t.y) * d.t.y + static_cast<double>(d.t.z) * d.t.z);
    }
    std::printf("plain_error %.9g\nrobust_error %.9g\n", err[0], err[1]);
    std::printf("robust %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", T_robust.t.x, T_robust.t.y, T_robust.t.z, T_robust.R.x, T_robust.R.y,
                T_robust.R.z, T_robust.R.w);
    for (int s = 0; s < 2; ++s)
      std::printf("sensor%d %u %.17g %.9g\n", s, stats_s[s].stats.n_meas, stats_s[s].weight_sum, stats_s[s].scale);
    std::printf("merged_n_meas %u\n", merged.n_meas);

    // the covariance each loop would publish: the sensors' information at their last pre-transforms, carried sensor -> base -> odometry
    // frame and merged with the multipliers.  The weighted form discounts what the robust loop discounted
    rm::PoseInformation info_plain{};
    rm::PoseInformationRobust info_robust{};
    for (int s = 0; s < 2; ++s) {
      const rm::Transform Tso = Tbo[s] * Tsb[s];
      info_plain = rm::merge(info_plain, Tbo[s] * (Tsb[s] * rcc[s]->computePoseInformation(~Tso * T_plain * Tso, 0.0)), weights[s]);
      const rm::PoseInformationRobust r = rcc[s]->computePoseInformationRobust(~Tso * T_robust * Tso, 0.0, tukey[s]);
      info_robust.info = rm::merge(info_robust.info, Tbo[s] * (Tsb[s] * r.info), weights[s]);
      info_robust.weight_sum += weights[s] * r.weight_sum;
      info_robust.rss_unweighted += weights[s] * r.rss_unweighted;
    }
    const rm::PoseCovariance cov_plain = rm::poseCovariance(info_plain), cov_robust = rm::poseCovariance(info_robust);
    std::printf("plain_cov_trace %.9g\nrobust_cov_trace %.9g\n", trace6(cov_plain), trace6(cov_robust));
    std::printf("plain_s2 %.9g\nrobust_s2 %.9g\n", cov_plain.s2, cov_robust.s2);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
