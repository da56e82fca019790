// field_lookup.hip.h -- the distance field's lookup (include/rmclhip.h, "THE LOOKUP at a point P"), shared by field.hip (the value
// alone: k_field_query, k_pf_update_field) and refine.hip (the value and its gradient from the same eight corners).  Index, fraction
// and clamping live here once; every float operation is in the header's order (the library is built without contraction).  The
// arrays it reads, of either layout, are built by field_build.hip.
#pragma once
#include "pf_common.hip.h"

namespace rmclhip {
namespace {

__device__ __forceinline__ float field_lerp(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ bool field_point_finite(const float (&pk)[3]) {
  return (fabsf(pk[0]) <= 3.402823466e38f) && (fabsf(pk[1]) <= 3.402823466e38f) && (fabsf(pk[2]) <= 3.402823466e38f);
}

// the cell of a finite point: its first corner, the fractions f, the offsets o to the clamped point (0 on axes that are not clamped).
// Returns whether any axis is clamped.  i_k <= n_k - 2, so all eight corners lie in the lattice wherever P is.
__device__ __forceinline__ bool field_locate(const FieldView& fv, const float (&pk)[3], uint32_t (&i)[3], float (&f)[3], float (&o)[3]) {
  bool clamped = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float top = static_cast<float>(fv.n[k] - 1u);
    const float u = (pk[k] - fv.origin[k]) * fv.inv_cell;
    const float c = fminf(fmaxf(u, 0.0f), top);
    i[k] = min(static_cast<uint32_t>(static_cast<int>(floorf(c))), fv.n[k] - 2u);
    f[k] = c - static_cast<float>(i[k]);
    const bool out = (u < 0.0f) || (u > top);
    o[k] = out ? pk[k] - (fv.origin[k] + c * fv.cell) : 0.0f;
    clamped = clamped || out;
  }
  return clamped;
}

// the eight corner values v[z][y][x] of the cell at i
__device__ __forceinline__ void field_corners(const FieldView& fv, const uint32_t (&i)[3], float (&v)[2][2][2]) {
  const size_t nx = fv.n[0], nxy = nx * fv.n[1];
  const float* c0 = fv.lat + (static_cast<size_t>(i[2]) * nxy + static_cast<size_t>(i[1]) * nx + i[0]);
  // the two x-neighbours of a corner pair are adjacent in memory
  v[0][0][0] = c0[0]; v[0][0][1] = c0[1]; v[0][1][0] = c0[nx]; v[0][1][1] = c0[nx + 1u];
  v[1][0][0] = c0[nxy]; v[1][0][1] = c0[nxy + 1u]; v[1][1][0] = c0[nxy + nx]; v[1][1][1] = c0[nxy + nx + 1u];
}

// lerp four times along x, twice along y, once along z
__device__ __forceinline__ float field_blend(const float (&v)[2][2][2], const float (&f)[3]) {
  const float x00 = field_lerp(v[0][0][0], v[0][0][1], f[0]), x10 = field_lerp(v[0][1][0], v[0][1][1], f[0]);
  const float x01 = field_lerp(v[1][0][0], v[1][0][1], f[0]), x11 = field_lerp(v[1][1][0], v[1][1][1], f[0]);
  const float y0 = field_lerp(x00, x10, f[1]), y1 = field_lerp(x01, x11, f[1]);
  return field_lerp(y0, y1, f[2]);
}

// the same eight values out of a banded field (include/rmclhip.h, BANDED DISTANCE FIELD).  The cell's brick is b_k = i_k >> 3.
//   STORED  v: the cell's corners out of the brick, at local index i_k & 7 -- the dense lattice's values; f untouched; returns true
//   FAR     the cell is the brick: v its coarse corners, f_k replaced by F_k = (c_k - float(8 b_k)) / float(e_k); returns false.
//           c_k is float(i_k) + f_k: f_k = c_k - float(i_k) was exact, so the sum is c_k to the bit.
__device__ __forceinline__ bool field_corners_banded(const FieldView& fv, const uint32_t (&i)[3], float (&f)[3], float (&v)[2][2][2]) {
  const uint32_t b[3] = {i[0] >> 3, i[1] >> 3, i[2] >> 3};
  const uint32_t s = fv.table[(static_cast<size_t>(b[2]) * fv.nb[1] + b[1]) * fv.nb[0] + b[0]];
  if (s != kBandFar) {
    const float* c0 = fv.bricks + (static_cast<size_t>(s) * kBandBrickNodes + ((i[2] & 7u) * 81u + (i[1] & 7u) * 9u + (i[0] & 7u)));
    v[0][0][0] = c0[0]; v[0][0][1] = c0[1]; v[0][1][0] = c0[9]; v[0][1][1] = c0[10];
    v[1][0][0] = c0[81]; v[1][0][1] = c0[82]; v[1][1][0] = c0[90]; v[1][1][1] = c0[91];
    return true;
  }
  const size_t cx = static_cast<size_t>(fv.nb[0]) + 1u, cxy = cx * (static_cast<size_t>(fv.nb[1]) + 1u);
  const float* c0 = fv.coarse + (static_cast<size_t>(b[2]) * cxy + static_cast<size_t>(b[1]) * cx + b[0]);
  v[0][0][0] = c0[0]; v[0][0][1] = c0[1]; v[0][1][0] = c0[cx]; v[0][1][1] = c0[cx + 1u];
  v[1][0][0] = c0[cxy]; v[1][0][1] = c0[cxy + 1u]; v[1][1][0] = c0[cxy + cx]; v[1][1][1] = c0[cxy + cx + 1u];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t e = min(8u, (fv.n[k] - 1u) - 8u * b[k]);
    const float c = static_cast<float>(i[k]) + f[k];
    f[k] = (c - static_cast<float>(8u * b[k])) / static_cast<float>(e);
  }
  return false;
}

// the corners of either layout: false for a cell answered from the coarse lattice (never of a dense field)
template <bool kBanded>
__device__ __forceinline__ bool field_cell(const FieldView& fv, const uint32_t (&i)[3], float (&f)[3], float (&v)[2][2][2]) {
  if constexpr (kBanded) {
    return field_corners_banded(fv, i, f, v);
  } else {
    field_corners(fv, i, v);
    return true;
  }
}

// include/rmclhip.h, "the lookup at a point P", line by line
template <bool kBanded>
__device__ __forceinline__ float field_lookup(const FieldView& fv, f3 P) {
  const float pk[3] = {P.x, P.y, P.z};
  if (!field_point_finite(pk)) return __uint_as_float(0x7FC00000u);
  uint32_t i[3];
  float f[3], o[3], v[2][2][2];
  const bool clamped = field_locate(fv, pk, i, f, o);
  (void)field_cell<kBanded>(fv, i, f, v);
  const float d = field_blend(v, f);
  return clamped ? d + sqrtf((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) : d;
}

}  // namespace
}  // namespace rmclhip
