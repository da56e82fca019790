// field_build.hip -- what builds a distance field, dense (include/rmclhip.h, DISTANCE FIELD) or banded (BANDED DISTANCE
// FIELD): the dense field's logical lattice, its fine nodes stored only in bricks of 8 cells per axis near the surface,
// every other brick answered from a coarse lattice of the bricks' corners.  The lookups are field.hip's, refine.hip's and stein.hip's
// kernels instantiated on the layout (field_lookup.hip.h).
//
//   field_node_query  the value of one logical node: the library's closest-point query (nearest_lane_ww, min d2 then min face id) at
//                     the node, started from a record an earlier, coarser query found near it -- an actual candidate, so the result
//                     is the unseeded query's.  Every node value of either layout comes from here: a banded field holds the dense
//                     field's bytes.
//   k_field_level     one lane per node of one level of a coarse-to-fine build: every stride-th logical node per axis, the last node
//                     of an axis at n_k - 1 wherever that falls, seeded from the level before.  Leaves the found records for the next
//                     level (and for the fill); the level that is the dense lattice or the coarse lattice leaves the distances.
//   k_band_classify   one lane per brick: STORED iff the smallest of its eight coarse corners is <= reach, or one is NaN.
//   k_band_table      one lane per brick, after the exact prefix sums of the flags (resample.hip's scan): the brick's stored index
//                     -- its rank among the stored bricks in brick order, never an arrival order -- and the list of stored bricks.
//   k_band_fill       one workgroup per stored brick: its 9 x 9 x 9 node values, three rounds of 256 lanes, every query started from
//                     the record the coarse build found at the brick corner nearest to the node.  Nodes beyond n_k - 1 hold NaN and
//                     are never read.
//
// A value is written by one lane and depends on the map and the geometry alone: every device builds the same bytes.
#include "pf_common.hip.h"

namespace rmclhip {
namespace {

// the closest-point distance at logical node (ix, iy, iz), started from record sr (kNone: unseeded); a lane that is not live runs
// the query's barriers and finds nothing
__device__ __forceinline__ void field_node_query(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ tris, uint32_t n_tris,
                                                 const FieldView& fv, uint32_t ix, uint32_t iy, uint32_t iz, bool live, uint32_t sr,
                                                 uint32_t* lds_stack, float& dist, uint32_t& rec) {
  // node (i, j, k): origin + (float(i) cell, float(j) cell, float(k) cell), product first, then sum
  const f3 P = mk3(fv.origin[0] + static_cast<float>(ix) * fv.cell, fv.origin[1] + static_cast<float>(iy) * fv.cell,
                   fv.origin[2] + static_cast<float>(iz) * fv.cell);
  const bool ok = live && (P.x == P.x) && (P.y == P.y) && (P.z == P.z);
  NearHit seed = near_seed_from_record(tris, ok ? sr : kNone, n_tris, P, ok);
  // a record whose distance overflows to NaN is no bound (k_pf_update<64, 3>: its bound check)
  if (!(seed.d2 <= 3.0e38f)) { seed.d2 = 3.0e38f; seed.face = kInvalidFace; seed.rec = 0; seed.p = mk3(0.f, 0.f, 0.f); }
  NearHit nh;
  nearest_lane_ww<16>(nodes, tris, P, ok, lds_stack, 256u, nh, &seed);
  const bool found = nh.face != kInvalidFace;
  rec = found ? nh.rec : kNone;
  dist = found ? sqrtf(nh.d2) : __uint_as_float(0x7FC00000u);
}

__global__ void __launch_bounds__(256) k_field_level(const FieldBuildParams p) {
  extern __shared__ uint32_t lds_dyn[];
  const size_t total = static_cast<size_t>(p.cn[0]) * p.cn[1] * p.cn[2];
  const size_t id = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  const bool live = id < total;
  const size_t ii = live ? id : 0u;
  const uint32_t cx = static_cast<uint32_t>(ii % p.cn[0]);
  const size_t cyz = ii / p.cn[0];
  const uint32_t cy = static_cast<uint32_t>(cyz % p.cn[1]), cz = static_cast<uint32_t>(cyz / p.cn[1]);
  // the last node of an axis is the lattice's last: a level of ceil((n_k - 1) / stride) + 1 nodes ends on it, one of
  // (n_k - 1) / stride + 1 never passes it (the products fit: c_k * stride < n_k - 1 + stride)
  const uint32_t ix = min(cx * p.stride, p.fv.n[0] - 1u), iy = min(cy * p.stride, p.fv.n[1] - 1u), iz = min(cz * p.stride, p.fv.n[2] - 1u);
  uint32_t sr = kNone;
  if (p.seed_rec != nullptr && live) {
    const uint32_t px = min((ix + p.pstride / 2u) / p.pstride, p.pn[0] - 1u), py = min((iy + p.pstride / 2u) / p.pstride, p.pn[1] - 1u),
                   pz = min((iz + p.pstride / 2u) / p.pstride, p.pn[2] - 1u);
    sr = p.seed_rec[(static_cast<size_t>(pz) * p.pn[1] + py) * p.pn[0] + px];
  }
  float dist;
  uint32_t rec;
  field_node_query(p.nodes, p.tris, p.n_tris, p.fv, ix, iy, iz, live, sr, lds_dyn + threadIdx.x, dist, rec);
  if (!live) return;
  if (p.rec_out != nullptr) p.rec_out[id] = rec;
  if (p.dist_out != nullptr) p.dist_out[id] = dist;
}

__global__ void __launch_bounds__(256) k_band_classify(const FieldView v, const float* __restrict__ coarse, float reach,
                                                       uint32_t* __restrict__ flags) {
  const size_t total = static_cast<size_t>(v.nb[0]) * v.nb[1] * v.nb[2];
  const size_t id = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  if (id >= total) return;
  const size_t bx = id % v.nb[0], byz = id / v.nb[0], by = byz % v.nb[1], bz = byz / v.nb[1];
  const size_t cx = static_cast<size_t>(v.nb[0]) + 1u, cxy = cx * (static_cast<size_t>(v.nb[1]) + 1u);
  const float* c0 = coarse + (bz * cxy + by * cx + bx);
  const float c[8] = {c0[0], c0[1], c0[cx], c0[cx + 1u], c0[cxy], c0[cxy + 1u], c0[cxy + cx], c0[cxy + cx + 1u]};
  bool stored = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) stored = stored || !(c[k] > reach);   // <= reach, or NaN
  flags[id] = stored ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_band_table(size_t total, const uint32_t* __restrict__ flags, const unsigned long long* __restrict__ incl,
                                                    uint32_t* __restrict__ table, uint32_t* __restrict__ stored) {
  const size_t id = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  if (id >= total) return;
  if (flags[id] != 0u) {
    const unsigned long long s = incl[id] - 1ull;   // < total <= 2^32 - 2: fits a word and is never kBandFar
    table[id] = static_cast<uint32_t>(s);
    stored[s] = static_cast<uint32_t>(id);
  } else {
    table[id] = kBandFar;
  }
}

__global__ void __launch_bounds__(256) k_band_fill(const BandFillParams p) {
  __shared__ uint32_t s_stack[16u * 256u];
  const size_t sidx = blockIdx.x;
  if (sidx >= p.n_stored) return;
  const size_t b = p.stored[sidx];
  const uint32_t bx = static_cast<uint32_t>(b % p.fv.nb[0]);
  const size_t byz = b / p.fv.nb[0];
  const uint32_t by = static_cast<uint32_t>(byz % p.fv.nb[1]), bz = static_cast<uint32_t>(byz / p.fv.nb[1]);
  const size_t cx = static_cast<size_t>(p.fv.nb[0]) + 1u, cxy = cx * (static_cast<size_t>(p.fv.nb[1]) + 1u);
  float* out = p.bricks + sidx * kBandBrickNodes;
  // three rounds; every lane runs every round (the query's inactive lanes do nothing), lanes 729 .. 767 of the last store nothing
  for (uint32_t l = threadIdx.x; l < 768u; l += 256u) {
    const bool in_brick = l < kBandBrickNodes;
    const uint32_t ll = in_brick ? l : 0u;
    const uint32_t lx = ll % 9u, ly = (ll / 9u) % 9u, lz = ll / 81u;
    const uint32_t ix = 8u * bx + lx, iy = 8u * by + ly, iz = 8u * bz + lz;
    const bool live = in_brick && ix < p.fv.n[0] && iy < p.fv.n[1] && iz < p.fv.n[2];
    uint32_t sr = kNone;
    if (live) sr = p.coarse_rec[(bz + (lz >= 4u ? 1u : 0u)) * cxy + (by + (ly >= 4u ? 1u : 0u)) * cx + (bx + (lx >= 4u ? 1u : 0u))];
    float dist;
    uint32_t rec;
    field_node_query(p.nodes, p.tris, p.n_tris, p.fv, live ? ix : 0u, live ? iy : 0u, live ? iz : 0u, live, sr, s_stack + threadIdx.x, dist, rec);
    if (in_brick) out[l] = live ? dist : __uint_as_float(0x7FC00000u);
  }
}

// one lane per item, 256 lanes per workgroup
inline bool blocks_of(size_t total, uint32_t& blocks) {
  const size_t b = (total + 255u) / 256u;
  if (b > 0x7FFFFFFFull) return false;
  blocks = static_cast<uint32_t>(b);
  return true;
}

}  // namespace

hipError_t launch_field_level(const FieldBuildParams& p, hipStream_t s) {
  const size_t total = static_cast<size_t>(p.cn[0]) * p.cn[1] * p.cn[2];
  if (total == 0u) return hipSuccess;
  uint32_t blocks;
  if (!blocks_of(total, blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_field_level, dim3(blocks), dim3(256), 16u * 256u * sizeof(uint32_t), s, p);
  return hipGetLastError();
}

hipError_t launch_band_classify(const FieldView& v, const float* coarse, float reach, uint32_t* flags, hipStream_t s) {
  const size_t total = static_cast<size_t>(v.nb[0]) * v.nb[1] * v.nb[2];
  if (total == 0u) return hipSuccess;
  uint32_t blocks;
  if (!blocks_of(total, blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_band_classify, dim3(blocks), dim3(256), 0, s, v, coarse, reach, flags);
  return hipGetLastError();
}

hipError_t launch_band_table(const FieldView& v, const uint32_t* flags, const unsigned long long* incl, uint32_t* table, uint32_t* stored,
                             hipStream_t s) {
  const size_t total = static_cast<size_t>(v.nb[0]) * v.nb[1] * v.nb[2];
  if (total == 0u) return hipSuccess;
  uint32_t blocks;
  if (!blocks_of(total, blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_band_table, dim3(blocks), dim3(256), 0, s, total, flags, incl, table, stored);
  return hipGetLastError();
}

hipError_t launch_band_fill(const BandFillParams& p, hipStream_t s) {
  if (p.n_stored == 0u) return hipSuccess;
  if (p.n_stored > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_band_fill, dim3(p.n_stored), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace rmclhip
