// refine.hip -- damped Gauss-Newton refinement of particles on the map's distance field (include/rmclhip.h, REFINE ON THE FIELD, states
// the arithmetic; tests/refine_ref.py restates it in numpy).
//
//   k_field_refine    one wave per particle, four particles per 256-thread workgroup, the whole Levenberg-Marquardt loop in one launch.
//                     A pass deals the beams as k_pf_update_field does (lane l takes beams l, l + 64, ...: neighbouring end points
//                     gather from neighbouring cells), forms the same Tsm and the same end point, reads the lookup's eight corners
//                     once for the value and its gradient (field_lookup.hip.h) and sums cost, normal equations and count per lane in
//                     double; a butterfly (xor 32, 16, ..., 1) leaves the totals in every lane.  The 6 x 6 solve is wave-uniform:
//                     every lane holds the same A and b and runs the same Cholesky, so no value is broadcast and no branch diverges.
//
// Pose, lambda and the accept decision are wave-uniform; the waves of a workgroup share nothing (each parks its current A and b in a
// row of LDS of its own; no barrier), so the result of a particle does not depend on the launch shape.  The beams are read from their device records in every pass: 64 B per beam, shared
// by every wave of the device, they stay in the caches; transforming them to the base frame once would change the bits of the end
// point against the sensor update's.  The pass, the solve and the candidate are refine_step.hip.h's, shared with stein.hip.
#include "refine_step.hip.h"

namespace rmclhip {
namespace {

template <bool kBanded>
__global__ void __launch_bounds__(256) k_field_refine(const RefineKernelParams p) {
  // the current pose's A (21) and b (6) of each of the four waves, parked here while a candidate is evaluated: they are needed again
  // only if the candidate is turned down.  One wave writes and reads its own row; LDS operations of one wave complete in order.
  __shared__ double s_ab[4][27];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pi = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (pi >= p.n_particles) return;   // the whole wave leaves
  double* ab = s_ab[threadIdx.x >> 6];
  xform cur = p.poses[pi], cand = cur;
  const bool finite = surface_pose_finite(cur);
  const uint32_t mask = p.dof_mask & 0x3Fu;
  double C0 = 0.0, C = 0.0, lambda = static_cast<double>(p.lambda0);
  uint32_t n_start = 0u, n_cur = 0u, accepted = 0u;
  // pass 0 evaluates the start pose; every later pass solves for a candidate and evaluates it (all conditions are wave-uniform)
  for (uint32_t it = 0; it <= p.iterations; ++it) {
    bool evaluate = true;
    if (it != 0u) {
      double A[21], b[6], delta[6];
#pragma unroll
      for (int k = 0; k < 21; ++k) A[k] = ab[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) b[k] = ab[21 + k];
      evaluate = refine_solve(A, b, mask, lambda, p.max_step_trans, p.max_step_rot, delta);
      if (evaluate) cand = refine_candidate(cur, delta, mask);
    }
    bool accept = false;
    if (evaluate) {
      RefineSums S;
      refine_pass<kBanded>(p, cand, lane, S);
      accept = (it == 0u) || (S.C < C);
      if (accept) {
        cur = cand;
        C = S.C;
        n_cur = S.n_used;
        if (lane == 0u) {
#pragma unroll
          for (int k = 0; k < 21; ++k) ab[k] = S.A[k];
#pragma unroll
          for (int k = 0; k < 6; ++k) ab[21 + k] = S.b[k];
        }
      }
    }
    if (it == 0u) {
      C0 = C;
      n_start = n_cur;
      if (!(finite && mask != 0u && n_start != 0u)) break;
    } else if (accept) {
      const double l3 = lambda / 3.0;
      lambda = (l3 > 1e-6) ? l3 : 1e-6;
      ++accepted;
    } else {
      lambda = lambda * 10.0;
    }
  }
  if (lane != 0u) return;
  if (accepted != 0u) p.poses[pi] = cur;
  if (p.rows != nullptr) {
    uint32_t* row = p.rows + 4u * static_cast<size_t>(pi);
    row[0] = __float_as_uint(static_cast<float>(C0));
    row[1] = __float_as_uint(static_cast<float>(C));
    row[2] = n_cur;
    row[3] = accepted;
  }
  if (p.counters != nullptr) {
    if (accepted != 0u) atomicAdd(p.counters + 0, 1u);
    if (!finite) atomicAdd(p.counters + 2, 1u);
    else if (n_start == 0u) atomicAdd(p.counters + 1, 1u);
  }
}

}  // namespace

hipError_t launch_field_refine(const RefineKernelParams& p, hipStream_t s) {
  if (p.n_particles == 0u) return hipSuccess;
  if (p.n_beams == 0u || p.n_beams > kRefineMaxBeams || p.iterations > kRefineMaxIterations) return hipErrorInvalidValue;
  const uint32_t nblocks = (p.n_particles + 3u) / 4u;
  if (p.fv.lat != nullptr) hipLaunchKernelGGL(k_field_refine<false>, dim3(nblocks), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(k_field_refine<true>, dim3(nblocks), dim3(256), 0, s, p);   // a banded field
  return hipGetLastError();
}

}  // namespace rmclhip
