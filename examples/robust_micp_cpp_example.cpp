// robust_micp_cpp_example.cpp -- MICP-L's correction of one sensor with M-estimator weights (include/rmclhip.h, ROBUST MICP), through
// include/rmcl_hip/rmcl_hip.hpp: a scan in which something stands in front of the mapped wall, corrected by the plain loop and by the
// robust one, and the outlier map the weights give.
//
//   g++ -std=c++17 -Iinclude examples/robust_micp_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o robust_micp_example
//   ./robust_micp_example mesh.bin dataset.bin
//       mesh.bin:    u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       dataset.bin: u32 n, n*3 f32 points (sensor frame), n u8 mask -- one scan of the 32 x 32 model below
//
// Prints one "key value..." line per result; tests/test_gpu_robust_example.py compares them with the Python binding's.
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s mesh.bin dataset.bin\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror("mesh"); return 2; }
  uint32_t nv = 0, nf = 0;
  if (std::fread(&nv, 4, 1, fh) != 1 || std::fread(&nf, 4, 1, fh) != 1) return 2;
  std::vector<float> verts(3 * static_cast<size_t>(nv));
  std::vector<uint32_t> faces(3 * static_cast<size_t>(nf));
  if (std::fread(verts.data(), 4, verts.size(), fh) != verts.size() || std::fread(faces.data(), 4, faces.size(), fh) != faces.size()) return 2;
  std::fclose(fh);
  fh = std::fopen(argv[2], "rb");
  if (!fh) { std::perror("dataset"); return 2; }
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, fh) != 1 || n != 32u * 32u) { std::fprintf(stderr, "dataset: expected %u points\n", 32u * 32u); return 2; }
  rm::PointCloud_<rm::RAM> dataset_cpu;
  dataset_cpu.points.resize(n);
  dataset_cpu.mask.resize(n);
  if (std::fread(dataset_cpu.points.raw(), sizeof(rm::Vector), n, fh) != n || std::fread(dataset_cpu.mask.raw(), 1, n, fh) != n) return 2;
  std::fclose(fh);

  try {
    auto ctx = std::make_shared<rm::Context>(0);
    auto map = std::make_shared<rm::HipMap>(ctx, verts.data(), nv, faces.data(), nf);
    const float pi = 3.14159265358979323846f;
    rm::SphericalModel model{};
    model.phi = {-pi / 4, (pi / 2) / 31, 32};
    model.theta = {-pi, 2 * pi / 32, 32};
    model.range = {0.1f, 100.0f};
    const rm::Transform Tsb = from_rpy(0.1f, 0.0f, 0.3f, 0, 0, 10.0 * pi / 180);
    const rm::Transform Tom = rm::identity();
    const rm::Transform truth = from_rpy(0.5f, -0.3f, 0.2f, 0.02, -0.03, 0.4);
    const rm::Transform Tbo = truth * from_rpy(0.2f, 0.0f, 0.0f, 0, 0, 2.0 * pi / 180);   // the estimate, 0.2 m / 2 degrees off

    rm::RCCHipSpherical rcc(map);
    rcc.setTsb(Tsb);
    rcc.setModel(model);
    rcc.params.max_dist = 1.0f;
    rcc.adaptive_max_dist_min = 1.0f;
    rcc.dataset.points = dataset_cpu.points;   // upload
    rcc.dataset.mask = dataset_cpu.mask;

    // the plain correction (every gated-in correspondence at full weight) and the robust one, ten iterations each
    const rm::Transform T_plain = rcc.correctOnce(Tom, Tbo, 10, 0.0, false);
    const rm::RobustParams tukey(RMCLHIP_ROBUST_TUKEY);
    rm::RobustStatistics stats_s;
    const rm::Transform T_robust = rcc.correctOnceRobust(Tom, Tbo, 10, 0.0, tukey, &stats_s);
    std::printf("plain %.9g %.9g %.9g\n", T_plain.t.x, T_plain.t.y, T_plain.t.z);
    std::printf("robust %.9g %.9g %.9g\n", T_robust.t.x, T_robust.t.y, T_robust.t.z);
    std::printf("scale %.9g %.9g\nn_meas %u\nweight_sum %.17g\n", stats_s.scale, stats_s.median_abs_residual, stats_s.stats.n_meas, stats_s.weight_sum);

    // the outlier map at the result: the weight of every ray, 0 where masked or gated out
    const rm::Transform Tso = Tbo * Tsb;
    const rm::Transform T_snew_sold = ~Tso * T_robust * Tso;
    const std::vector<float> w = rcc.robustWeights(T_snew_sold, 0.0, tukey);
    size_t low = 0;
    for (float x : w) low += (x < 0.5f) ? 1u : 0u;
    std::printf("weights %zu %zu\n", w.size(), low);

    // the operator form and the free function on the operator's own views give the same bytes
    const rm::RobustStatistics op_s = rcc.computeRobustStatistics(T_snew_sold, 0.0, tukey);
    const rm::RobustStatistics free_s = rm::statistics_p2l_robust(T_snew_sold, rm::watch(rcc.dataset), rcc.modelView(), rcc.params, tukey);
    std::printf("free_equals_operator %d\n", std::memcmp(&free_s, &op_s, sizeof(free_s)) == 0 ? 1 : 0);
    std::printf("weight_sum_at_result %.17g\n", op_s.weight_sum);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
