// pose_covariance_cpp_example.cpp -- what MICPLocalizationNode::publishPose (rmcl_ros/src/nodes/micp_localization.cpp:1062-1076) can
// publish instead of its guessed diagonal: the covariance of the corrected pose from the point-to-plane information matrix of the
// correction's own correspondences, through include/rmcl_hip/rmcl_hip.hpp.
//
//   g++ -std=c++17 -Iinclude examples/pose_covariance_cpp_example.cpp -Lrmcl_amd -lrmclhip -Wl,-rpath,$PWD/rmcl_amd -o pose_covariance_example
//   ./pose_covariance_example mesh.bin dataset.bin
//       mesh.bin:    u32 nv, u32 nf, nv*3 f32, nf*3 u32
//       dataset.bin: u32 n, n*3 f32 points (sensor frame), n u8 mask -- one scan of the 32 x 32 model below
//
// Prints one "key value..." line per result; tests/test_gpu_pose_covariance_example.py compares them with the Python binding's.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rmcl_hip/rmcl_hip.hpp"

namespace rm = rmcl_hip;   // the reference's callers write rm:: for rmagine

// geometry_msgs::msg::PoseWithCovarianceStamped, as far as publishPose fills it
struct PoseWithCovarianceStamped {
  rm::Transform pose;
  std::array<double, 36> covariance;   // row-major, x y z rot-x rot-y rot-z
};

static rm::Transform from_rpy(float x, float y, float z, double roll, double pitch, double yaw) {
  const double cr = std::cos(roll / 2), sr = std::sin(roll / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2);
  const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2);
  rm::Transform T = rm::identity();
  T.R = {static_cast<float>(sr * cp * cy - cr * sp * sy), static_cast<float>(cr * sp * cy + sr * cp * sy),
         static_cast<float>(cr * cp * sy - sr * sp * cy), static_cast<float>(cr * cp * cy + sr * sp * sy)};
  T.t = {x, y, z};
  return T;
}

// the node's state after correctOnce, as far as publishPose reads it
struct NodeState {
  rm::RCCHipSpherical* sensor;
  rm::Transform Tsb, Tbo_latest, Tom, T_onew_oold;   // T_onew_oold: what the last correction's loop ended with
  double convergence_progress;
};

// publishPose with the covariance computed: the sensor's information over the correspondences of the last find at the pre-transform of
// the last iteration, carried sensor -> base -> odom, inverted where the scan constrains the pose and capped where it does not
static PoseWithCovarianceStamped publishPose(const NodeState& s, rm::PoseInformation* info_out, rm::PoseCovariance* report_out) {
  PoseWithCovarianceStamped pose;
  const rm::Transform T_bnew_bold = ~s.Tbo_latest * s.T_onew_oold * s.Tbo_latest;
  const rm::Transform T_snew_sold = ~s.Tsb * T_bnew_bold * s.Tsb;
  const rm::PoseInformation info_s = s.sensor->computePoseInformation(T_snew_sold, s.convergence_progress);
  const rm::PoseInformation info_o = s.Tbo_latest * (s.Tsb * info_s);
  rm::PoseCovarianceParams params = rm::poseCovarianceParams();
  params.degenerate_variance = 100.0;   // (10 m)^2, (10 rad)^2: "the scan says nothing about this direction"
  const rm::PoseCovariance cov = rm::poseCovariance(info_o, params);
  std::memcpy(pose.covariance.data(), cov.covariance, sizeof(cov.covariance));
  pose.pose = s.Tom * s.Tbo_latest;
  *info_out = info_o;
  *report_out = cov;
  return pose;
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
    const rm::Transform Tbo = rm::identity();
    const rm::Transform truth = from_rpy(0.5f, -0.3f, 0.2f, 0.02, -0.03, 0.4);
    const rm::Transform Tom_est = truth * from_rpy(0.2f, 0.1f, 0.05f, 0, 0, 2.0 * pi / 180);

    rm::RCCHipSpherical rcc(map);
    rcc.setTsb(Tsb);
    rcc.setModel(model);
    rcc.params.max_dist = 1.0f;
    rcc.adaptive_max_dist_min = 0.15f;
    rcc.dataset.points = dataset_cpu.points;   // upload
    rcc.dataset.mask = dataset_cpu.mask;

    // correctOnce's inner loop (micp_localization.cpp:915-964), one sensor, five iterations on fixed correspondences
    const double convergence_progress = 0.25;
    rcc.find(Tom_est * Tbo);
    rm::Transform T_onew_oold = rm::identity();
    rm::Transform T_snew_sold_last = rm::identity();
    for (int i = 0; i < 5; ++i) {
      const rm::Transform T_bnew_bold = ~Tbo * T_onew_oold * Tbo;
      T_snew_sold_last = ~Tsb * T_bnew_bold * Tsb;
      rm::CrossStatistics Cmerged = rm::cross_statistics_identity();
      Cmerged += Tbo * (Tsb * rcc.computeCrossStatistics(T_snew_sold_last, convergence_progress));
      T_onew_oold = T_onew_oold * rm::umeyama_transform(Cmerged);
    }
    const rm::Transform T_final = ~Tsb * (~Tbo * T_onew_oold * Tbo) * Tsb;
    const rm::CrossStatistics stats_final = rcc.computeCrossStatistics(T_final, convergence_progress);

    NodeState state{&rcc, Tsb, Tbo, Tom_est * T_onew_oold, T_onew_oold, convergence_progress};
    rm::PoseInformation info;
    rm::PoseCovariance report;
    const PoseWithCovarianceStamped pose = publishPose(state, &info, &report);
    std::printf("n_meas %u %u\n", info.n_meas, stats_final.n_meas);
    std::printf("pose %.9g %.9g %.9g\n", pose.pose.t.x, pose.pose.t.y, pose.pose.t.z);
    std::printf("s2 %.17g\nrss %.17g\n", report.s2, info.rss);
    std::printf("covariance");
    for (double c : pose.covariance) std::printf(" %.17g", c);
    std::printf("\ninformation_diag %.17g %.17g %.17g %.17g %.17g %.17g\n", info.A[0], info.A[7], info.A[14], info.A[21], info.A[28], info.A[35]);
    std::printf("degenerate %u %u\neig_trans %.17g %.17g %.17g\n", report.n_degenerate_trans, report.n_degenerate_rot, report.eig_trans[0],
                report.eig_trans[1], report.eig_trans[2]);
    // after five iterations the remaining Gauss-Newton step is small: the two solvers agree on where the minimum is
    const std::array<double, 6> xi = rm::solve(info);
    std::printf("remaining_step %.9g %.9g %.9g %.9g %.9g %.9g\n", xi[0], xi[1], xi[2], xi[3], xi[4], xi[5]);

    // the free function on the operator's own views == the operator form (sensor frame)
    rm::UmeyamaReductionConstraints params_local = rcc.params;
    params_local.max_dist = static_cast<float>(rcc.params.max_dist * (1.0 - convergence_progress) + rcc.adaptive_max_dist_min * convergence_progress);
    const rm::PoseInformation free_s = rm::pose_information_p2l(T_final, rm::watch(rcc.dataset), rcc.modelView(), params_local);
    const rm::PoseInformation op_s = rcc.computePoseInformation(T_final, convergence_progress);
    std::printf("free_equals_operator %d\n", std::memcmp(&free_s, &op_s, sizeof(free_s)) == 0 ? 1 : 0);

    // a pose batch (the v1 corrector's shape): the information at the estimate and at the truth from the batch's model buffers
    rcc.correctBatch({Tom_est * Tbo, truth * Tbo});
    const std::vector<rm::PoseInformation> batch = rcc.computePoseInformationBatch(2, convergence_progress);
    std::printf("batch_n_meas %u %u\nbatch_rss %.17g %.17g\n", batch[0].n_meas, batch[1].n_meas, batch[0].rss, batch[1].rss);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
