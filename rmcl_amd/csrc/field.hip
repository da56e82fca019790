// field.hip -- the map's distance field (include/rmclhip.h, DISTANCE FIELD, states the geometry and the lookup).
//
//   k_field_build     one lane per node of one level of the coarse-to-fine build: the library's closest-point query
//                     (nearest_lane_ww, min d2 then min face id) at the node, started from the record the previous level found for
//                     the node nearest to it -- an actual candidate, so the result is the unseeded query's
//   k_field_query     the lookup alone, one lane per point
//   k_pf_update_field the sensor update of correspondence_type 1 answered from the lattice: k_pf_update<64, 3> (pf_common.hip.h) with
//                     the tree query replaced by the lookup -- same Tsm, same end point, same evaluation, same in-order merge.  No
//                     traversal, no stack: LDS holds the workgroup's Tsm and its beam evaluations only.
//
// k_field_query and k_pf_update_field are instantiated on the layout: <false> reads the dense lattice, <true> a banded field's table,
// bricks and coarse lattice (field_lookup.hip.h, field_corners_banded; the build is band_field.hip).
//
// The lookup (field_lookup.hip.h, shared with refine.hip) is eight dependent gathers and seven lerps in a stated float order.  Rays are
// dealt beam-minor: the lanes of a wave hold consecutive beams of one particle, Tsm is a wave-uniform LDS read, and the end points of
// neighbouring beams fall into neighbouring cells.
#include "field_lookup.hip.h"

namespace rmclhip {
namespace {

__global__ void __launch_bounds__(256) k_field_build(const FieldBuildParams p) {
  extern __shared__ uint32_t lds_dyn[];
  const size_t total = static_cast<size_t>(p.cn[0]) * p.cn[1] * p.cn[2];
  const size_t id = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  const bool live = id < total;
  const size_t ii = live ? id : 0u;
  const uint32_t cx = static_cast<uint32_t>(ii % p.cn[0]);
  const size_t cyz = ii / p.cn[0];
  const uint32_t cy = static_cast<uint32_t>(cyz % p.cn[1]), cz = static_cast<uint32_t>(cyz / p.cn[1]);
  const uint32_t ix = cx * p.stride, iy = cy * p.stride, iz = cz * p.stride;   // < n: cn = (n - 1) / stride + 1
  // node (i, j, k): origin + (float(i) cell, float(j) cell, float(k) cell), product first, then sum
  const f3 P = mk3(p.fv.origin[0] + static_cast<float>(ix) * p.fv.cell, p.fv.origin[1] + static_cast<float>(iy) * p.fv.cell,
                   p.fv.origin[2] + static_cast<float>(iz) * p.fv.cell);
  const bool ok = live && (P.x == P.x) && (P.y == P.y) && (P.z == P.z);
  uint32_t sr = kNone;
  if (p.seed_rec != nullptr && ok) {
    const uint32_t px = min((ix + p.pstride / 2u) / p.pstride, p.pn[0] - 1u), py = min((iy + p.pstride / 2u) / p.pstride, p.pn[1] - 1u),
                   pz = min((iz + p.pstride / 2u) / p.pstride, p.pn[2] - 1u);
    sr = p.seed_rec[(static_cast<size_t>(pz) * p.pn[1] + py) * p.pn[0] + px];
  }
  NearHit seed = near_seed_from_record(p.tris, sr, p.n_tris, P, ok);
  // a record whose distance overflows to NaN is no bound (k_pf_update<64, 3>: its bound check)
  if (!(seed.d2 <= 3.0e38f)) { seed.d2 = 3.0e38f; seed.face = kInvalidFace; seed.rec = 0; seed.p = mk3(0.f, 0.f, 0.f); }
  NearHit nh;
  nearest_lane_ww<16>(p.nodes, p.tris, P, ok, lds_dyn + threadIdx.x, 256u, nh, &seed);
  if (!live) return;
  const bool found = nh.face != kInvalidFace;
  if (p.rec_out != nullptr) p.rec_out[id] = found ? nh.rec : kNone;
  if (p.dist_out != nullptr) p.dist_out[id] = found ? sqrtf(nh.d2) : __uint_as_float(0x7FC00000u);
}

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

hipError_t launch_field_build(const FieldBuildParams& p, hipStream_t s) {
  const size_t total = static_cast<size_t>(p.cn[0]) * p.cn[1] * p.cn[2];
  if (total == 0u) return hipSuccess;
  const size_t blocks = (total + 255u) / 256u;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_field_build, dim3(static_cast<uint32_t>(blocks)), dim3(256), 16u * 256u * sizeof(uint32_t), s, p);
  return hipGetLastError();
}

hipError_t launch_field_query(const FieldView& fv, const float* points, size_t n, float* out, hipStream_t s) {
  if (n == 0u) return hipSuccess;
  const size_t blocks = (n + 255u) / 256u;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // lat == nullptr: a banded field (band_field.hip)
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
