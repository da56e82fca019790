// field.hip -- reading the map's distance field (include/rmclhip.h, DISTANCE FIELD, states the geometry and the lookup; DESIGN.md
// 4.14).  What builds a field, dense or banded, is field_build.hip.
//
//   k_field_query     the lookup alone, one lane per point
//   k_pf_update_field the sensor update of correspondence_type 1 answered from the lattice: k_pf_update<64, 3> (pf_common.hip.h) with
//                     the tree query replaced by the lookup -- same Tsm, same end point, same evaluation, same in-order merge.  No
//                     traversal, no stack: LDS holds the workgroup's Tsm and its beam evaluations only.
//
// k_field_query and k_pf_update_field are instantiated on the layout: <false> reads the dense lattice, <true> a banded field's table,
// bricks and coarse lattice (field_lookup.hip.h, field_corners_banded).
//
// The lookup (field_lookup.hip.h, shared with refine.hip) is eight dependent gathers and seven lerps in a stated float order.  Rays are
// dealt beam-minor: the lanes of a wave hold consecutive beams of one particle, Tsm is a wave-uniform LDS read, and the end points of
// neighbouring beams fall into neighbouring cells.
#include "field_lookup.hip.h"

namespace rmclhip {
namespace {

template <bool kBanded>
__global__ void __launch_bounds__(256) k_field_query(const FieldView fv, const float* __restrict__ points, size_t n, float* __restrict__ out) {
  const size_t id = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  if (id >= n) return;
  const float* pp = points + 3u * id;
  out[id] = field_lookup<kBanded>(fv, mk3(pp[0], pp[1], pp[2]));
}

template <bool kBanded>
__global__ void __launch_bounds__(256) k_pf_update_field(const PfFieldParams p) {
  // LDS: [ Tsm (PB xforms) | evals (PB * n_beams floats) ]
  extern __shared__ uint32_t lds_dyn[];
  xform* s_Tsm = reinterpret_cast<xform*>(lds_dyn);
  float* s_eval = reinterpret_cast<float*>(s_Tsm + p.particles_per_block);

  const uint32_t PB = p.particles_per_block;
  const uint32_t p0 = blockIdx.x * PB;
  if (p0 >= p.n_particles) return;
  const uint32_t np = min(PB, p.n_particles - p0);
  if (threadIdx.x < np) s_Tsm[threadIdx.x] = xmul(p.poses[p0 + threadIdx.x], p.Tsb);
  __syncthreads();

  const float sq = p.dist_sigma * p.dist_sigma;
  const uint32_t nrays = np * p.n_beams;
  for (uint32_t r = threadIdx.x; r < nrays; r += 256u) {
    const uint32_t pi = r / p.n_beams, b = r - pi * p.n_beams;
    const xform Tsm = s_Tsm[pi];
    const float* bm = p.beams + 16u * b;
    // meas_m = Tsm * meas_s; evaluate_cpc: the distance of meas_m.mean() = orig + dir * range to the surface (k_pf_update<64, 3>)
    const f3 dir = qrot(Tsm.R, mk3(bm[3], bm[4], bm[5]));
    const f3 org = xapply(Tsm, mk3(bm[0], bm[1], bm[2]));
    const f3 mean = add3(org, scale3(dir, bm[6]));
    const float error = field_lookup<kBanded>(p.fv, mean);
    if (p.errors) p.errors[static_cast<size_t>(p0 + pi) * p.n_beams + b] = error;
    const float arg = -(error * error) / sq / 2;
    s_eval[r] = static_cast<float>(exp(static_cast<double>(arg)) / sqrt(static_cast<double>(2 * sq) * 3.14159265358979323846));
  }
  __syncthreads();
  // in-order merge, one lane per particle (sequential semantics of sensorUpdate)
  if (threadIdx.x < np) {
    pattrs* A = reinterpret_cast<pattrs*>(p.attrs) + (p0 + threadIdx.x);
    g1d L = A->likelihood;
    const float* ev = s_eval + threadIdx.x * p.n_beams;
    for (uint32_t b = 0; b < p.n_beams; ++b) {
      g1d m; m.mean = ev[b]; m.sigma = 0.0f; m.n_meas = 1;
      L = g1d_add(L, m);
      L.n_meas = min(L.n_meas, p.max_n_meas);
    }
    A->likelihood = L;
  }
}

}  // namespace

hipError_t launch_field_query(const FieldView& fv, const float* points, size_t n, float* out, hipStream_t s) {
  if (n == 0u) return hipSuccess;
  const size_t blocks = (n + 255u) / 256u;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // lat == nullptr: a banded field
  if (fv.lat != nullptr) hipLaunchKernelGGL(k_field_query<false>, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, fv, points, n, out);
  else hipLaunchKernelGGL(k_field_query<true>, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, fv, points, n, out);
  return hipGetLastError();
}

hipError_t launch_pf_update_field(const PfFieldParams& p, hipStream_t s) {
  const uint32_t nblocks = (p.n_particles + p.particles_per_block - 1u) / p.particles_per_block;
  const size_t lds = sizeof(xform) * p.particles_per_block + sizeof(float) * static_cast<size_t>(p.particles_per_block) * p.n_beams;
  if (lds > 65536u) return hipErrorInvalidValue;   // the caller deals at most 8192 beams to a workgroup
  if (p.fv.lat != nullptr) hipLaunchKernelGGL(k_pf_update_field<false>, dim3(nblocks), dim3(256), lds, s, p);
  else hipLaunchKernelGGL(k_pf_update_field<true>, dim3(nblocks), dim3(256), lds, s, p);
  return hipGetLastError();
}

}  // namespace rmclhip
