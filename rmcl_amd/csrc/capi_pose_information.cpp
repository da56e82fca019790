// capi_pose_information.cpp -- POSE COVARIANCE of include/rmclhip.h: the point-to-plane information matrix of a correction's
// correspondences (kernels: pose_information.hip) as a free function on caller-owned views and after a find / a pose batch, and the host
// algebra that carries it between frames, merges the sensors' and turns it into a covariance with a degeneracy report.
#include "capi_internal.h"

static_assert(sizeof(rmclhip_pose_information) == 44 * 8, "PoseInformation layout");

// a result row of launch_pose_information (upper triangle of sum u u^T row by row, u = [N ; D x N ; r], then the count)
void pose_information_unpack_row(const double* row, rmclhip_pose_information* out) {
  double S[7][7];
  int k = 0;
  for (int a = 0; a < 7; ++a)
    for (int b = a; b < 7; ++b) { S[a][b] = row[k]; S[b][a] = row[k]; ++k; }
  for (int a = 0; a < 6; ++a) {
    for (int b = 0; b < 6; ++b) out->A[6 * a + b] = S[a][b];
    out->g[a] = S[a][6];
  }
  out->rss = S[6][6];
  out->n_meas = static_cast<uint32_t>(row[k]);
  out->pad = 0;
}

namespace {

// the launches + the rows' way to the host on `stream`, which the call waits for
rmclhip_status run(ReduceParams& p, DevBuf<double>& partials, DevBuf<double>& rows, hipStream_t stream,
                   rmclhip_pose_information* out) {
  p.nblocks = reduce_num_blocks(p.n, p.nposes);
  HIPCHK(partials.reserve(static_cast<size_t>(p.nposes) * p.nblocks * kPoseInfoRow));
  HIPCHK(rows.reserve(static_cast<size_t>(p.nposes) * kPoseInfoRow));
  p.partials = partials.p;
  HIPCHK(launch_pose_information(p, rows.p, stream));
  std::vector<double> h(static_cast<size_t>(p.nposes) * kPoseInfoRow);
  HIPCHK(hipMemcpyAsync(h.data(), rows.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (uint32_t i = 0; i < p.nposes; ++i) pose_information_unpack_row(h.data() + static_cast<size_t>(i) * kPoseInfoRow, out + i);
  return RMCLHIP_OK;
}

// the checks the two operator forms share; *n_out = correspondences per pose
rmclhip_status rcc_check(const char* who, const rmclhip_rcc* r, uint32_t* n_out) {
  if (r->nposes_last == 0 || r->n_model == 0) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": no find has run");
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  const uint32_t n = (r->n_dataset < r->n_model) ? r->n_dataset : r->n_model;
  if (n == 0) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": empty dataset");
  *n_out = n;
  return RMCLHIP_OK;
}

void rcc_params(const rmclhip_rcc* r, uint32_t n, uint32_t nposes, const xform& Tpre, double convergence_progress, ReduceParams* p) {
  std::memset(p, 0, sizeof(*p));
  p->dataset_points = r->ds_pts;
  p->dataset_mask = r->ds_has_mask ? r->ds_msk : nullptr;
  p->model_points = r->d_points.p;
  p->model_normals = r->d_normals.p;
  p->model_mask = r->d_hits.p;
  p->n = n;
  p->nposes = nposes;
  // CorrespondencesCPU.cpp:21-23 (float operands, double arithmetic, float store): the rule of rmclhip_rcc_compute_cross_statistics
  p->max_dist = static_cast<float>(static_cast<double>(r->max_dist) * (1.0 - convergence_progress) +
                                   static_cast<double>(r->adaptive_max_dist_min) * convergence_progress);
  p->Tpre = Tpre;
}

// ---- symmetric eigen-decomposition, cyclic Jacobi in double: A (n x n, row-major, n <= 6) -> eigenvalues ascending, eigenvector k =
// column k of V.  A rotation is skipped where the off-diagonal entry is exactly zero: a direction no correspondence touches (a zero row
// and column) keeps its unit vector exactly.
void jacobi_eig(int n, const double* A_in, double* lam, double* V) {
  double A[36];
  for (int i = 0; i < n * n; ++i) A[i] = A_in[i];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[n * i + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) (i == j ? diag : off) += A[n * i + j] * A[n * i + j];
    if (off == 0.0 || off <= 1e-34 * diag) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[n * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[n * q + q] - A[n * p + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {   // columns p, q
          const double akp = A[n * k + p], akq = A[n * k + q];
          A[n * k + p] = c * akp - s * akq;
          A[n * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {   // rows p, q
          const double apk = A[n * p + k], aqk = A[n * q + k];
          A[n * p + k] = c * apk - s * aqk;
          A[n * q + k] = s * apk + c * aqk;
        }
        A[n * p + q] = 0.0; A[n * q + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double vkp = V[n * k + p], vkq = V[n * k + q];
          V[n * k + p] = c * vkp - s * vkq;
          V[n * k + q] = s * vkp + c * vkq;
        }
      }
  }
  int order[6];
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order, order + n, [&](int a, int b) { return A[n * a + a] < A[n * b + b]; });
  double Vs[36];
  for (int k = 0; k < n; ++k) {
    lam[k] = A[n * order[k] + order[k]];
    for (int i = 0; i < n; ++i) Vs[n * i + k] = V[n * i + order[k]];
  }
  for (int i = 0; i < n * n; ++i) V[i] = Vs[i];
}

bool finite_info(const rmclhip_pose_information* in) {
  for (int i = 0; i < 36; ++i) if (!std::isfinite(in->A[i])) return false;
  for (int i = 0; i < 6; ++i) if (!std::isfinite(in->g[i])) return false;
  return std::isfinite(in->rss);
}

// eigenpairs of the 3 x 3 diagonal block at `first` of A / n_meas; eigenvector k in vec[3 k .. 3 k + 2]
uint32_t block_report(const rmclhip_pose_information* in, int first, double min_eig, double* eig, double* vec) {
  double B[9], V[9];
  const double inv_n = (in->n_meas > 0u) ? 1.0 / static_cast<double>(in->n_meas) : 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[3 * i + j] = in->A[6 * (first + i) + first + j] * inv_n;
  jacobi_eig(3, B, eig, V);
  uint32_t n_deg = 0;
  for (int k = 0; k < 3; ++k) {
    for (int i = 0; i < 3; ++i) vec[3 * k + i] = V[3 * i + k];
    if (eig[k] < min_eig) ++n_deg;
  }
  return n_deg;
}

}  // namespace

extern "C" {

rmclhip_status rmclhip_pose_information_p2l(rmclhip_ctx* ctx, const rmclhip_transform* Tpre, const float* dataset_points,
                                            const uint8_t* dataset_mask, const float* model_points, const float* model_normals,
                                            const uint8_t* model_mask, uint32_t n, float max_dist, rmclhip_pose_information* out) {
  ApiGuard guard_("rmclhip_pose_information_p2l");
  if (!ctx || !Tpre || !out) return fail(RMCLHIP_ERR_INVALID, "pose_information_p2l: null");
  if (n == 0) { std::memset(out, 0, sizeof(*out)); return RMCLHIP_OK; }
  if (!dataset_points || !model_points || !model_normals) return fail(RMCLHIP_ERR_INVALID, "pose_information_p2l: null view");
  std::lock_guard<std::mutex> lock(ctx->p2l_mtx);
  HIPCHK(hipSetDevice(ctx->device));
  if (rmclhip_status st = ctx_p2l_ensure(ctx)) return st;
  ReduceParams p;
  std::memset(&p, 0, sizeof(p));
  p.dataset_points = dataset_points; p.dataset_mask = dataset_mask;
  p.model_points = model_points; p.model_normals = model_normals; p.model_mask = model_mask;
  p.n = n; p.nposes = 1; p.max_dist = max_dist;
  p.Tpre = to_x(Tpre);
  return run(p, ctx->pinfo_partials, ctx->pinfo_rows, ctx->p2l_stream, out);
}

rmclhip_status rmclhip_rcc_pose_information(rmclhip_rcc* r, const rmclhip_transform* T_snew_sold, double convergence_progress,
                                            rmclhip_pose_information* out) {
  ApiGuard guard_("rmclhip_rcc_pose_information");
  if (!r || !T_snew_sold || !out) return fail(RMCLHIP_ERR_INVALID, "rcc_pose_information: null");
  if (r->nposes_last > 1) return fail(RMCLHIP_ERR_INVALID, "rcc_pose_information: last find was a batch");
  uint32_t n = 0;
  if (rmclhip_status st = rcc_check("rcc_pose_information", r, &n)) return st;
  HIPCHK(hipSetDevice(r->ctx->device));
  ReduceParams p;
  rcc_params(r, n, 1, to_x(T_snew_sold), convergence_progress, &p);
  return run(p, r->d_pinfo_partials, r->d_pinfo_rows, r->stream, out);
}

rmclhip_status rmclhip_rcc_pose_information_batch(rmclhip_rcc* r, uint32_t nposes, double convergence_progress,
                                                  rmclhip_pose_information* out) {
  ApiGuard guard_("rmclhip_rcc_pose_information_batch");
  if (!r || !out) return fail(RMCLHIP_ERR_INVALID, "rcc_pose_information_batch: null");
  uint32_t n = 0;
  if (rmclhip_status st = rcc_check("rcc_pose_information_batch", r, &n)) return st;
  if (nposes != r->nposes_last)
    return fail(RMCLHIP_ERR_INVALID, "rcc_pose_information_batch: the last find held " + std::to_string(r->nposes_last) + " poses, not " +
                                         std::to_string(nposes));
  if (r->n_model != n && nposes > 1) return fail(RMCLHIP_ERR_INVALID, "rcc_pose_information_batch: dataset size != model size");
  HIPCHK(hipSetDevice(r->ctx->device));
  ReduceParams p;
  rcc_params(r, n, nposes, xidentity(), convergence_progress, &p);
  return run(p, r->d_pinfo_partials, r->d_pinfo_rows, r->stream, out);
}

rmclhip_status rmclhip_pose_information_transform(const rmclhip_transform* T, const rmclhip_pose_information* in,
                                                  rmclhip_pose_information* out) {
  if (!T || !in || !out) return fail(RMCLHIP_ERR_INVALID, "pose_information_transform: null");
  // R as devmath.h quat_to_mat forms it, in double, from the quaternion normalised in double: a float32 quaternion is a unit one to
  // 1e-7 only, and R (a x b) = (R a) x (R b), which the frame change rests on, holds for rotations alone
  const double qn = std::sqrt((static_cast<double>(T->R.x) * T->R.x + static_cast<double>(T->R.y) * T->R.y) +
                              (static_cast<double>(T->R.z) * T->R.z + static_cast<double>(T->R.w) * T->R.w));
  if (!(qn > 0.0) || !std::isfinite(qn)) return fail(RMCLHIP_ERR_INVALID, "pose_information_transform: not a rotation");
  const double x = T->R.x / qn, y = T->R.y / qn, z = T->R.z / qn, w = T->R.w / qn;
  const double R[3][3] = {{2.0 * (w * w + x * x) - 1.0, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), 2.0 * (w * w + y * y) - 1.0, 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 2.0 * (w * w + z * z) - 1.0}};
  const double t[3] = {T->t.x, T->t.y, T->t.z};
  const double tx[3][3] = {{0.0, -t[2], t[1]}, {t[2], 0.0, -t[0]}, {-t[1], t[0], 0.0}};
  double X[6][6];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      X[i][j] = R[i][j];
      X[i][3 + j] = 0.0;
      X[3 + i][3 + j] = R[i][j];
      X[3 + i][j] = (tx[i][0] * R[0][j] + tx[i][1] * R[1][j]) + tx[i][2] * R[2][j];
    }
  double XA[6][6], A2[36], g2[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double a = 0.0;
      for (int k = 0; k < 6; ++k) a += X[i][k] * in->A[6 * k + j];
      XA[i][j] = a;
    }
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      double a = 0.0;
      for (int k = 0; k < 6; ++k) a += XA[i][k] * X[j][k];
      A2[6 * i + j] = a;
    }
    double b = 0.0;
    for (int k = 0; k < 6; ++k) b += X[i][k] * in->g[k];
    g2[i] = b;
  }
  for (int i = 0; i < 6; ++i)   // symmetric by construction up to rounding: make it exactly so
    for (int j = i + 1; j < 6; ++j) A2[6 * i + j] = A2[6 * j + i] = 0.5 * (A2[6 * i + j] + A2[6 * j + i]);
  const double rss = in->rss;
  const uint32_t n_meas = in->n_meas;
  std::memcpy(out->A, A2, sizeof(A2));
  std::memcpy(out->g, g2, sizeof(g2));
  out->rss = rss; out->n_meas = n_meas; out->pad = 0;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pose_information_merge(const rmclhip_pose_information* a, const rmclhip_pose_information* b, double weight_b,
                                              rmclhip_pose_information* out) {
  if (!a || !b || !out) return fail(RMCLHIP_ERR_INVALID, "pose_information_merge: null");
  if (!(weight_b >= 0.0) || !std::isfinite(weight_b)) return fail(RMCLHIP_ERR_INVALID, "pose_information_merge: weight_b must be finite and >= 0");
  rmclhip_pose_information r;
  for (int i = 0; i < 36; ++i) r.A[i] = a->A[i] + weight_b * b->A[i];
  for (int i = 0; i < 6; ++i) r.g[i] = a->g[i] + weight_b * b->g[i];
  r.rss = a->rss + weight_b * b->rss;
  r.n_meas = a->n_meas + b->n_meas;
  r.pad = 0;
  *out = r;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pose_information_solve_host(const rmclhip_pose_information* in, double rcond, double xi_out[6]) {
  if (!in || !xi_out) return fail(RMCLHIP_ERR_INVALID, "pose_information_solve_host: null");
  if (!(rcond >= 0.0) || !std::isfinite(rcond) || !finite_info(in))
    return fail(RMCLHIP_ERR_INVALID, "pose_information_solve_host: rcond must be finite and >= 0, the information finite");
  double lam[6], V[36];
  jacobi_eig(6, in->A, lam, V);
  const double cut = rcond * lam[5];
  double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < 6; ++k) {
    if (!(lam[k] > cut) || !(lam[k] > 0.0)) continue;
    double vg = 0.0;
    for (int i = 0; i < 6; ++i) vg += V[6 * i + k] * in->g[i];
    for (int i = 0; i < 6; ++i) xi[i] += V[6 * i + k] * (vg / lam[k]);
  }
  for (int i = 0; i < 6; ++i) xi_out[i] = xi[i];
  return RMCLHIP_OK;
}

void rmclhip_pose_covariance_params_default(rmclhip_pose_covariance_params* out) {
  if (!out) return;
  out->sigma = 0.0;
  out->rcond = 1e-9;
  out->degenerate_variance = 1e6;
  out->min_eig_trans = 1e-3;
  out->min_eig_rot = 1e-3;
}

// the covariance of both forms: dof = the measurements beyond the six unknowns when the noise is estimated (sigma <= 0) -- n_meas - 6
// of the plain form, weight_sum - 6 of the robust one; `count` names it in the refusal
static rmclhip_status pose_covariance(const std::string& who, const rmclhip_pose_information* in, const rmclhip_pose_covariance_params* p,
                                      double dof, const char* count, rmclhip_pose_covariance* out) {
  if (!(p->rcond >= 0.0) || !std::isfinite(p->rcond) || !(p->degenerate_variance >= 0.0) || !std::isfinite(p->degenerate_variance) ||
      p->sigma != p->sigma || p->min_eig_trans != p->min_eig_trans || p->min_eig_rot != p->min_eig_rot)
    return fail(RMCLHIP_ERR_INVALID, who + ": rcond and degenerate_variance must be finite and >= 0, no parameter NaN");
  if (!finite_info(in)) return fail(RMCLHIP_ERR_INVALID, who + ": the information holds non-finite values");
  double s2;
  if (p->sigma > 0.0) {
    s2 = p->sigma * p->sigma;
  } else {
    if (!(dof > 0.0))
      return fail(RMCLHIP_ERR_INVALID, who + ": sigma <= 0 estimates the noise from the residuals, which needs " + count + " > 6");
    s2 = in->rss / dof;
  }
  rmclhip_pose_covariance r;
  std::memset(&r, 0, sizeof(r));
  double lam[6], V[36];
  jacobi_eig(6, in->A, lam, V);
  const double cut = p->rcond * lam[5];
  double c[6];
  for (int k = 0; k < 6; ++k) c[k] = (lam[k] > cut && lam[k] > 0.0) ? s2 / lam[k] : p->degenerate_variance;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      double a = 0.0;
      for (int k = 0; k < 6; ++k) a += (V[6 * i + k] * c[k]) * V[6 * j + k];
      r.covariance[6 * i + j] = a;
      r.covariance[6 * j + i] = a;
    }
  r.n_degenerate_trans = block_report(in, 0, p->min_eig_trans, r.eig_trans, r.eigvec_trans);
  r.n_degenerate_rot = block_report(in, 3, p->min_eig_rot, r.eig_rot, r.eigvec_rot);
  r.s2 = s2;
  *out = r;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pose_covariance_host(const rmclhip_pose_information* in, const rmclhip_pose_covariance_params* p,
                                            rmclhip_pose_covariance* out) {
  if (!in || !p || !out) return fail(RMCLHIP_ERR_INVALID, "pose_covariance_host: null");
  const double dof = (in->n_meas > 6u) ? static_cast<double>(in->n_meas - 6u) : 0.0;
  return pose_covariance("pose_covariance_host", in, p, dof, "n_meas", out);
}

rmclhip_status rmclhip_pose_covariance_robust_host(const rmclhip_pose_information_robust* in, const rmclhip_pose_covariance_params* p,
                                                   rmclhip_pose_covariance* out) {
  if (!in || !p || !out) return fail(RMCLHIP_ERR_INVALID, "pose_covariance_robust_host: null");
  if (!(in->weight_sum >= 0.0) || !std::isfinite(in->weight_sum))
    return fail(RMCLHIP_ERR_INVALID, "pose_covariance_robust_host: weight_sum must be finite and >= 0");
  return pose_covariance("pose_covariance_robust_host", &in->info, p, in->weight_sum - 6.0, "weight_sum", out);
}

}  // extern "C"
