// pose_estimate_host.h -- the host side of RmclNode::estimateStats (rmcl_localization.cpp:642-731), shared by every entry point that
// fills a rmclhip_pose_estimate: the sharded filter's (capi_pf_sharded.cpp), the single-device one and the per-hypothesis one
// (capi_hypotheses.cpp).  The three moment passes (kernels.hip: k_pose_moments) are the caller's: a callable
//   moments(int pass, double L_sum, const xform& Tbm, double* out32) -> rmclhip_status
// that leaves the 24 sums + 8 maxima of one pass over ITS particles in out32.  Everything else -- the likelihood statistics, the
// refusals, the Markley mean's eigenvector, the order of the passes -- is stated once, here.
#pragma once
#include "capi_internal.h"

// largest eigenvector of a symmetric 4x4 matrix (cyclic Jacobi, double)
inline void sym4_largest_eigenvector(const double* M10, double* q) {
  double A[4][4], V[4][4];
  int k = 0;
  for (int a = 0; a < 4; ++a) for (int b = a; b < 4; ++b) { A[a][b] = A[b][a] = M10[k++]; }
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) V[a][b] = (a == b) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int a = 0; a < 4; ++a) for (int b = a + 1; b < 4; ++b) off += A[a][b] * A[a][b];
    if (off < 1e-300) break;
    for (int p = 0; p < 3; ++p)
      for (int qq = p + 1; qq < 4; ++qq) {
        if (A[p][qq] == 0.0) continue;
        const double theta = (A[qq][qq] - A[p][p]) / (2.0 * A[p][qq]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int i = 0; i < 4; ++i) { const double ip = A[i][p], iq = A[i][qq]; A[i][p] = c * ip - sn * iq; A[i][qq] = sn * ip + c * iq; }
        for (int i = 0; i < 4; ++i) { const double pi_ = A[p][i], qi = A[qq][i]; A[p][i] = c * pi_ - sn * qi; A[qq][i] = sn * pi_ + c * qi; }
        for (int i = 0; i < 4; ++i) { const double ip = V[i][p], iq = V[i][qq]; V[i][p] = c * ip - sn * iq; V[i][qq] = sn * ip + c * iq; }
      }
  }
  int best = 0;
  for (int a = 1; a < 4; ++a) if (A[a][a] > A[best][best]) best = a;
  double n = 0.0;
  for (int a = 0; a < 4; ++a) n += V[a][best] * V[a][best];
  n = std::sqrt(n);
  const double sgn = (V[3][best] < 0.0) ? -1.0 : 1.0;   // canonical sign: w >= 0
  for (int a = 0; a < 4; ++a) q[a] = sgn * V[a][best] / n;
}

// *out is zeroed first; n_use: the particles the passes run over (0: refused, "no particles"); who: the caller's name in the messages
template <class Moments>
inline rmclhip_status pose_estimate_passes(const char* who_, uint32_t n_use, Moments&& moments, rmclhip_pose_estimate* out) {
  const std::string who(who_);
  std::memset(out, 0, sizeof(*out));
  if (n_use == 0) return fail(RMCLHIP_ERR_INVALID, who + ": no particles");
  double m[32];
  if (rmclhip_status st = moments(0, 1.0, xidentity(), m)) return st;
  const double L_sum = m[0], L_n = m[2];
  // every particle killed by the collision test: w = L / 0, a NaN matrix into the Jacobi sweeps, a NaN pose out
  if (!(L_sum > 0.0)) return fail(RMCLHIP_ERR_INVALID, who + ": the likelihoods sum to zero (or NaN): no weighted mean");
  const double L_mean = L_sum / L_n;
  out->n_particles = n_use;
  out->likelihood_mean = L_mean;
  out->likelihood_sigma = std::sqrt(std::max(m[1] / L_n - L_mean * L_mean, 0.0));
  out->likelihood_max = std::max(m[24], 0.0);   // L_max starts at 0.0 in the reference (:665)
  out->likelihood_min = -m[25];
  for (int k = 0; k < 3; ++k) { out->trans_bb_max[k] = static_cast<float>(m[26 + k]); out->trans_bb_min[k] = static_cast<float>(-m[29 + k]); }
  // first pass: mean (rm::markley_mean with weights L_i / L_sum)
  if (rmclhip_status st = moments(1, L_sum, xidentity(), m)) return st;
  double q[4];
  sym4_largest_eigenvector(m, q);
  xform Tbm = xidentity();
  Tbm.R.x = static_cast<float>(q[0]); Tbm.R.y = static_cast<float>(q[1]); Tbm.R.z = static_cast<float>(q[2]); Tbm.R.w = static_cast<float>(q[3]);
  Tbm.t = mk3(static_cast<float>(m[10]), static_cast<float>(m[11]), static_cast<float>(m[12]));
  from_x(Tbm, &out->pose);
  // second pass: covariance around the mean
  if (rmclhip_status st = moments(2, L_sum, Tbm, m)) return st;
  int k = 0;
  for (int a = 0; a < 6; ++a) for (int b = a; b < 6; ++b) { out->covariance[6 * a + b] = out->covariance[6 * b + a] = m[k++]; }
  return RMCLHIP_OK;
}
