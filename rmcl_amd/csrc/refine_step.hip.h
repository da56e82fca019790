// refine_step.hip.h -- one Gauss-Newton step of a particle on the distance field (include/rmclhip.h, REFINE ON THE FIELD), shared by
// refine.hip (k_field_refine: the whole Levenberg-Marquardt loop) and stein.hip (k_stein_drive: the first candidate step alone;
// k_stein_pair: the length limit and the candidate rule applied to the neighbour-averaged move).  The pass, the solve, the limit and
// the candidate live here once; every operation is in the header's order (the library is built without contraction).
#pragma once
#include "field_lookup.hip.h"
#include "surface.hip.h"

namespace rmclhip {
namespace {

// what one pass leaves in every lane: the cost, the upper triangle of A row by row, b, and the number of used beams
struct RefineSums {
  double C;
  double A[21];
  double b[6];
  uint32_t n_used;
};

__device__ __forceinline__ double refine_wave_sum(double x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
  return x;
}

// kBanded: the field's layout (field_lookup.hip.h); a beam whose cell a banded field answers from its coarse lattice is not valid
template <bool kBanded>
__device__ __forceinline__ void refine_pass(const RefineKernelParams& p, const xform& pose, uint32_t lane, RefineSums& S) {
  const xform Tsm = xmul(pose, p.Tsb);
  S.C = 0.0;
  S.n_used = 0u;
#pragma unroll
  for (int k = 0; k < 21; ++k) S.A[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) S.b[k] = 0.0;
  for (uint32_t b = lane; b < p.n_beams; b += 64u) {
    const float* bm = p.beams + 16u * static_cast<size_t>(b);
    // the end point of k_pf_update_field
    const f3 dir = qrot(Tsm.R, mk3(bm[3], bm[4], bm[5]));
    const f3 org = xapply(Tsm, mk3(bm[0], bm[1], bm[2]));
    const f3 M = add3(org, scale3(dir, bm[6]));
    const float pk[3] = {M.x, M.y, M.z};
    float d = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    bool valid = field_point_finite(pk);
    if (valid) {
      uint32_t i[3];
      float f[3], o[3];
      valid = !field_locate(p.fv, pk, i, f, o);
      if (valid) {
        float v[2][2][2];
        const bool fine = field_cell<kBanded>(p.fv, i, f, v);
        d = field_blend(v, f);
        g[0] = field_lerp(field_lerp(v[0][0][1] - v[0][0][0], v[0][1][1] - v[0][1][0], f[1]),
                          field_lerp(v[1][0][1] - v[1][0][0], v[1][1][1] - v[1][1][0], f[1]), f[2]) * p.fv.inv_cell;
        g[1] = field_lerp(field_lerp(v[0][1][0] - v[0][0][0], v[0][1][1] - v[0][0][1], f[0]),
                          field_lerp(v[1][1][0] - v[1][0][0], v[1][1][1] - v[1][0][1], f[0]), f[2]) * p.fv.inv_cell;
        g[2] = field_lerp(field_lerp(v[1][0][0] - v[0][0][0], v[1][0][1] - v[0][0][1], f[0]),
                          field_lerp(v[1][1][0] - v[0][1][0], v[1][1][1] - v[0][1][1], f[0]), f[1]) * p.fv.inv_cell;
        valid = fine && (fabsf(d) <= 3.402823466e38f) && field_point_finite(g);
      }
    }
    const bool used = valid && (d < p.max_dist);
    const float m = used ? d : p.max_dist;   // min(d, max_dist) of a valid beam, max_dist of any other
    S.C += static_cast<double>(m) * static_cast<double>(m);
    if (used) {
      const f3 L = sub3(M, pose.t);
      const double J[6] = {g[0], g[1], g[2], L.y * g[2] - L.z * g[1], L.z * g[0] - L.x * g[2], L.x * g[1] - L.y * g[0]};
      const double r = d;
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c = a; c < 6; ++c) S.A[k++] += J[a] * J[c];
        S.b[a] += J[a] * r;
      }
      ++S.n_used;
    }
  }
  S.C = refine_wave_sum(S.C);
#pragma unroll
  for (int k = 0; k < 21; ++k) S.A[k] = refine_wave_sum(S.A[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) S.b[k] = refine_wave_sum(S.b[k]);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) S.n_used += __shfl_xor(S.n_used, s, 64);
}

// the whole step is multiplied by the smallest of 1, max_step_trans / |v| (if |v| > 0) and max_step_rot / |omega| (if |omega| > 0)
__device__ __forceinline__ void refine_limit(double (&delta)[6], float max_step_trans, float max_step_rot) {
  const double nv = sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
  const double nw = sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
  double scale = 1.0;
  if (nv > 0.0) { const double q = static_cast<double>(max_step_trans) / nv; if (q < scale) scale = q; }
  if (nw > 0.0) { const double q = static_cast<double>(max_step_rot) / nw; if (q < scale) scale = q; }
#pragma unroll
  for (int a = 0; a < 6; ++a) delta[a] = delta[a] * scale;
}

// the step: delta = -(A + lambda diag(A) + 1e-9 I)^-1 b over the free degrees of freedom, limited in length.  False: a pivot of the
// Cholesky factor is not positive (the step is rejected).
__device__ __forceinline__ bool refine_solve(const double (&A)[21], const double (&b)[6], uint32_t mask, double lambda, float max_step_trans,
                                             float max_step_rot, double (&delta)[6]) {
  double H[6][6], rhs[6];
  {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = a; c < 6; ++c) { H[a][c] = A[k]; H[c][a] = A[k]; ++k; }
      rhs[a] = b[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    if (((mask >> a) & 1u) == 0u) {
#pragma unroll
      for (int c = 0; c < 6; ++c) { H[a][c] = 0.0; H[c][a] = 0.0; }
      H[a][a] = 1.0;
      rhs[a] = 0.0;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) H[a][a] = (H[a][a] + lambda * H[a][a]) + 1e-9;
  // H = G G^T, column by column, the sums taken in increasing k
  double G[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = H[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= G[j][k] * G[j][k];
    ok = ok && (s > 0.0);
    G[j][j] = sqrt(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = H[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= G[i][k] * G[j][k];
      G[i][j] = t / G[j][j];
    }
  }
  if (!ok) return false;
  double y[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= G[i][k] * y[k];
    y[i] = s / G[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= G[k][i] * x[k];
    x[i] = s / G[i][i];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) delta[a] = ((mask >> a) & 1u) ? -x[a] : 0.0;
  refine_limit(delta, max_step_trans, max_step_rot);
  return true;
}

// t' = t + float(v) on the free axes; q' = normalise((omega / 2, 1) * R)
__device__ __forceinline__ xform refine_candidate(const xform& pose, const double (&delta)[6], uint32_t mask) {
  xform c = pose;
  if (mask & 1u) c.t.x = pose.t.x + static_cast<float>(delta[0]);
  if (mask & 2u) c.t.y = pose.t.y + static_cast<float>(delta[1]);
  if (mask & 4u) c.t.z = pose.t.z + static_cast<float>(delta[2]);
  if (mask & 0x38u) {
    quat dq;
    dq.x = static_cast<float>(0.5 * delta[3]); dq.y = static_cast<float>(0.5 * delta[4]); dq.z = static_cast<float>(0.5 * delta[5]); dq.w = 1.0f;
    c.R = surface_qnormalise(qmul(dq, pose.R));
  }
  return c;
}

}  // namespace
}  // namespace rmclhip
