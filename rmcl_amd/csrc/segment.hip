// segment.hip -- map segmentation on the device: the per-scan body of the reference's ScanMapSegmentationEmbreeNode /
// O1DnMapSegmentationEmbreeNode (rmcl_ros/src/nodes/filter/scan_map_segmentation_embree.cpp:100-185, o1dn_map_segmentation_embree.cpp).
// The trace is the find kernel writing {ranges, normals} (capi_segment.cpp); what is here labels every ray from its measured and its
// simulated range and compacts the two outlier clouds IN BUFFER ORDER (the order the reference's nested loops push them in):
//
//   k_segment_classify   one lane per ray, consecutive lanes = consecutive buffer ids: the label, and per workgroup the number of scan
//                        outliers and of map outliers among its kSegBlock rays
//   k_segment_scatter    same grid: a workgroup's two base offsets are the sums of the counts BELOW its index, a ray's position is
//                        base + its rank among the workgroup's selected rays; the last workgroup writes the two totals
//
// The order across workgroups comes from the kernel boundary between the two launches: no workgroup waits for another inside a launch, and
// no atomic decides a position, so the clouds are the same bits on every run.  Within a wave a ray's rank is mbcnt of the ballot; across
// the 16 waves of a workgroup a 16-entry table in LDS.
#include "kernels.h"

namespace rmclhip {
namespace {

// traverse.hip.h pinhole_direction, restated (that header brings the traversal kernels with it): same operation order as
// oracle/rmcl_oracle.c:orc_pinhole_direction
__device__ __forceinline__ f3 seg_pinhole_direction(float fx, float fy, float cx, float cy, uint32_t vid, uint32_t hid) {
  const float pX = (static_cast<float>(hid) - cx) / fx;
  const float pY = (static_cast<float>(vid) - cy) / fy;
  const float d = sqrtf((pX * pX + pY * pY) + 1.0f * 1.0f);
  return mk3(1.0f / d, -(pX / d), -(pY / d));
}

// model.getDirection(vid, hid) / model.getOrigin(vid, hid) from the tables the find kernel reads (kernels.h FindParams::model_tab)
__device__ __forceinline__ void seg_ray(const SegmentParams& p, uint32_t i, f3& dir, f3& orig) {
  orig = p.orig;
  if (p.kind == kModelSpherical) {
    const uint32_t vid = i / p.W, hid = i - vid * p.W;
    const float* tab = p.model_tab;
    const float cp = tab[vid], sp = tab[p.H + vid], ct = tab[2u * p.H + hid], st = tab[2u * p.H + p.W + hid];
    dir = mk3(cp * ct, cp * st, sp);
  } else if (p.kind == kModelPinhole) {
    const uint32_t vid = i / p.W, hid = i - vid * p.W;
    dir = seg_pinhole_direction(p.pin_f[0], p.pin_f[1], p.pin_c[0], p.pin_c[1], vid, hid);
  } else if (p.kind == kModelOnDn) {
    const float* og = p.model_tab + 3u * static_cast<size_t>(i);
    const float* dr = p.model_tab + 3u * (static_cast<size_t>(p.W) * p.H + i);
    orig = mk3(og[0], og[1], og[2]);
    dir = mk3(dr[0], dr[1], dr[2]);
  } else {
    const float* dr = p.model_tab + 3u * static_cast<size_t>(i);
    dir = mk3(dr[0], dr[1], dr[2]);
  }
}

// the origin is zero for the spherical and the pinhole model (the find kernel adds it for O1Dn / OnDn only)
__device__ __forceinline__ f3 seg_point(const SegmentParams& p, f3 dir, float r, f3 orig, bool with_origin) {
  const f3 pt = scale3(dir, r);
  return (with_origin && (p.kind == kModelO1Dn || p.kind == kModelOnDn)) ? add3(pt, orig) : pt;
}

// Interval::inside: NaN is outside (do not write it as !(r < min || r > max))
__device__ __forceinline__ bool seg_inside(const SegmentParams& p, float r) { return p.rmin <= r && r <= p.rmax; }

// ranks of the workgroup's selected rays in lane order (= buffer order): rank_* of this lane among the lanes with sel_* set, tot_* the
// workgroup's counts.  Every lane of the workgroup calls it (ballots and a barrier inside).
__device__ __forceinline__ void seg_block_ranks(bool sel_scan, bool sel_map, uint32_t (*wave_cnt)[2], uint32_t& rank_scan, uint32_t& rank_map,
                                                uint32_t& tot_scan, uint32_t& tot_map) {
  const unsigned long long b_scan = __ballot(sel_scan), b_map = __ballot(sel_map);
  const uint32_t wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  rank_scan = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b_scan >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b_scan), 0u));
  rank_map = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b_map >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b_map), 0u));
  if ((threadIdx.x & 63u) == 0u) {
    wave_cnt[wave][0] = static_cast<uint32_t>(__popcll(b_scan));
    wave_cnt[wave][1] = static_cast<uint32_t>(__popcll(b_map));
  }
  __syncthreads();
  tot_scan = 0u; tot_map = 0u;
  for (uint32_t w = 0; w < nwaves; ++w) {
    const uint32_t c0 = wave_cnt[w][0], c1 = wave_cnt[w][1];
    if (w < wave) { rank_scan += c0; rank_map += c1; }
    tot_scan += c0; tot_map += c1;
  }
}

__global__ void __launch_bounds__(kSegBlock) k_segment_classify(const SegmentParams p) {
  __shared__ uint32_t wave_cnt[kSegBlock / 64u][2];
  const uint32_t n = p.W * p.H, i = blockIdx.x * kSegBlock + threadIdx.x;
  uint8_t label = kSegNone;
  if (i < n) {
    const float r_real = p.ranges_real[i], r_sim = p.ranges_sim[i];
    const bool real_valid = seg_inside(p, r_real), sim_valid = seg_inside(p, r_sim);
    if (real_valid && sim_valid) {
      f3 dir, orig;
      seg_ray(p, i, dir, orig);
      const f3 preal_s = seg_point(p, dir, r_real, orig, true);
      const f3 pint_s = seg_point(p, dir, r_sim, orig, p.pint_with_origin != 0u);   // the reference leaves the origin out here
      f3 nint_s = mk3(p.normals_sim[3u * static_cast<size_t>(i)], p.normals_sim[3u * static_cast<size_t>(i) + 1u], p.normals_sim[3u * static_cast<size_t>(i) + 2u]);
      nint_s = scale3(nint_s, 1.0f / sqrtf(dot_plain(nint_s, nint_s)));   // normalizeInplace
      const float plane_distance = fabsf(dot_plain(sub3(preal_s, pint_s), nint_s));
      if (r_real < r_sim) label = (plane_distance > p.min_dist_outlier_scan) ? kSegOutlierScan : kSegInlier;   // something in front of the surface
      else label = (plane_distance > p.min_dist_outlier_map) ? kSegOutlierMap : kSegInlier;                    // the ray cut the surface
    } else if (real_valid) {
      label = kSegOutlierScan;   // measured, not simulated
    } else if (sim_valid) {
      label = kSegOutlierMap;    // the map promises a surface the sensor did not see
    }
    p.labels[i] = label;
  }
  uint32_t rank_scan, rank_map, tot_scan, tot_map;
  seg_block_ranks(label == kSegOutlierScan, label == kSegOutlierMap, wave_cnt, rank_scan, rank_map, tot_scan, tot_map);
  if (threadIdx.x == 0u) {
    p.block_counts[2u * blockIdx.x] = tot_scan;
    p.block_counts[2u * blockIdx.x + 1u] = tot_map;
  }
}

__global__ void __launch_bounds__(kSegBlock) k_segment_scatter(const SegmentParams p) {
  __shared__ uint32_t wave_cnt[kSegBlock / 64u][2];
  __shared__ uint32_t wave_base[kSegBlock / 64u][2];
  const uint32_t n = p.W * p.H, i = blockIdx.x * kSegBlock + threadIdx.x;
  // the two base offsets: sums of the counts of the workgroups below this one (integers: any order gives the same sum)
  uint32_t base_scan = 0u, base_map = 0u;
  for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kSegBlock) {
    base_scan += p.block_counts[2u * b];
    base_map += p.block_counts[2u * b + 1u];
  }
  for (uint32_t off = 32u; off != 0u; off >>= 1) {
    base_scan += __shfl_xor(base_scan, off);
    base_map += __shfl_xor(base_map, off);
  }
  if ((threadIdx.x & 63u) == 0u) {
    wave_base[threadIdx.x >> 6][0] = base_scan;
    wave_base[threadIdx.x >> 6][1] = base_map;
  }
  const uint8_t label = (i < n) ? p.labels[i] : static_cast<uint8_t>(kSegNone);
  uint32_t rank_scan, rank_map, tot_scan, tot_map;
  seg_block_ranks(label == kSegOutlierScan, label == kSegOutlierMap, wave_cnt, rank_scan, rank_map, tot_scan, tot_map);   // (its barrier covers wave_base)
  base_scan = 0u; base_map = 0u;
  for (uint32_t w = 0; w < kSegBlock / 64u; ++w) {
    base_scan += wave_base[w][0];
    base_map += wave_base[w][1];
  }
  // base + rank < n: the workgroups below hold at most blockIdx.x * kSegBlock rays, the rank is below this workgroup's ray count
  if (label == kSegOutlierScan && p.outlier_scan_xyz != nullptr) {
    f3 dir, orig;
    seg_ray(p, i, dir, orig);
    const f3 pt = seg_point(p, dir, p.ranges_real[i], orig, true);   // preal_s
    float* o = p.outlier_scan_xyz + 3u * static_cast<size_t>(base_scan + rank_scan);
    o[0] = pt.x; o[1] = pt.y; o[2] = pt.z;
  } else if (label == kSegOutlierMap && p.outlier_map_xyz != nullptr) {
    f3 dir, orig;
    seg_ray(p, i, dir, orig);
    // both ranges valid: pint_s without the origin (unless the flag adds it); the measured range invalid: with it
    const bool with_origin = !seg_inside(p, p.ranges_real[i]) || p.pint_with_origin != 0u;
    const f3 pt = seg_point(p, dir, p.ranges_sim[i], orig, with_origin);
    float* o = p.outlier_map_xyz + 3u * static_cast<size_t>(base_map + rank_map);
    o[0] = pt.x; o[1] = pt.y; o[2] = pt.z;
  }
  if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u) {
    const uint32_t n_scan = base_scan + tot_scan, n_map = base_map + tot_map;
    if (p.counts_dev) { p.counts_dev[0] = n_scan; p.counts_dev[1] = n_map; }
    if (p.counts_host) { p.counts_host[0] = n_scan; p.counts_host[1] = n_map; }
  }
}

}  // namespace

hipError_t launch_segment(const SegmentParams& p, hipStream_t s) {
  const uint32_t n = p.W * p.H;
  if (n == 0u) return hipSuccess;
  const uint32_t nblocks = (n + kSegBlock - 1u) / kSegBlock;
  hipLaunchKernelGGL(k_segment_classify, dim3(nblocks), dim3(kSegBlock), 0, s, p);
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_segment_scatter, dim3(nblocks), dim3(kSegBlock), 0, s, p);
  return hipGetLastError();
}

}  // namespace rmclhip
