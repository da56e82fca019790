// capi_segment.cpp -- map segmentation of the correspondence operator (see capi_internal.h; kernels in segment.hip)
#include "capi_internal.h"

// what both entry points check before the first HIP call
static rmclhip_status segment_check(const char* who, const rmclhip_rcc* r, const rmclhip_transform* Tbm, const float* ranges_real,
                                    const rmclhip_segmentation_params* sp, bool* nothing_to_do) {
  *nothing_to_do = false;
  if (!r || !Tbm || !ranges_real || !sp) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": null");
  // (NaN fails both comparisons)
  if (!(sp->min_dist_outlier_scan >= 0.0f) || !(sp->min_dist_outlier_map >= 0.0f))
    return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": min_dist_outlier_scan / min_dist_outlier_map must be numbers >= 0");
  if ((sp->flags & ~RMCLHIP_SEG_PINT_WITH_ORIGIN) != 0u) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": unknown flag bits");
  if (r->kind == kModelNone || r->W == 0 || r->H == 0) *nothing_to_do = true;
  return RMCLHIP_OK;
}

// optional H2D of the measured ranges, trace into the operator's scratch, classify, scatter: all on the handle's stream
static rmclhip_status segment_enqueue(rmclhip_rcc* r, const rmclhip_transform* Tbm, const float* ranges_real, int ranges_is_device,
                                      const rmclhip_segmentation_params* sp, const rmclhip_segmentation_views* out) {
  const size_t n = static_cast<size_t>(r->W) * r->H;
  HIPCHK(r->h_seg_counts.reserve(2));
  HIPCHK(r->d_seg_ranges.reserve(n));
  HIPCHK(r->d_seg_normals.reserve(3 * n));
  HIPCHK(r->d_seg_block_counts.reserve(2 * ((n + kSegBlock - 1u) / kSegBlock)));
  const rmclhip_segmentation_views none{nullptr, nullptr, nullptr, nullptr};
  const rmclhip_segmentation_views& v = out ? *out : none;
  if (!v.labels_dev) HIPCHK(r->d_seg_labels.reserve(n));
  const float* real_dev = ranges_real;
  if (!ranges_is_device) {
    HIPCHK(r->d_seg_real.reserve(n));
    HIPCHK(hipMemcpyAsync(r->d_seg_real.p, ranges_real, n * sizeof(float), hipMemcpyHostToDevice, r->stream));
    real_dev = r->d_seg_real.p;
  }
  // Simulator::simulate<Bundle<Ranges, Normals>>(Tbm): the find kernel with the scratch as its bundle
  FindParams fp;
  fill_find_params(r, fp, 1);
  fp.hits = nullptr; fp.points = nullptr; fp.face_ids = nullptr;
  fp.ranges = r->d_seg_ranges.p;
  fp.normals = r->d_seg_normals.p;
  fp.Tsm = xmul(to_x(Tbm), r->Tsb);
  fp.Tms = xinv(fp.Tsm);
  HIPCHK(launch_find(fp, r->kind, find_variant(r, 1), r->stream));
  SegmentParams p;
  std::memset(&p, 0, sizeof(p));
  p.ranges_real = real_dev;
  p.ranges_sim = r->d_seg_ranges.p;
  p.normals_sim = r->d_seg_normals.p;
  p.model_tab = r->d_model_tab.p;
  p.kind = r->kind; p.W = r->W; p.H = r->H;
  p.orig = r->orig;
  p.pin_f[0] = r->pin_fc[0]; p.pin_f[1] = r->pin_fc[1]; p.pin_c[0] = r->pin_fc[2]; p.pin_c[1] = r->pin_fc[3];
  p.rmin = r->range.min; p.rmax = r->range.max;
  p.min_dist_outlier_scan = sp->min_dist_outlier_scan;
  p.min_dist_outlier_map = sp->min_dist_outlier_map;
  p.pint_with_origin = (sp->flags & RMCLHIP_SEG_PINT_WITH_ORIGIN) ? 1u : 0u;
  p.labels = v.labels_dev ? v.labels_dev : r->d_seg_labels.p;
  p.block_counts = r->d_seg_block_counts.p;
  p.outlier_scan_xyz = v.outlier_scan_xyz_dev;
  p.outlier_map_xyz = v.outlier_map_xyz_dev;
  p.counts_dev = v.counts_dev;
  p.counts_host = r->h_seg_counts.d;
  HIPCHK(launch_segment(p, r->stream));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_segment_async(rmclhip_rcc* r, const rmclhip_transform* Tbm, const float* ranges_real, int ranges_is_device,
                                         const rmclhip_segmentation_params* sp, const rmclhip_segmentation_views* out) {
  ApiGuard guard_("rmclhip_rcc_segment_async");
  bool nothing = false;
  if (rmclhip_status st = segment_check("rcc_segment_async", r, Tbm, ranges_real, sp, &nothing)) return st;
  if (nothing) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  return segment_enqueue(r, Tbm, ranges_real, ranges_is_device, sp, out);
}

rmclhip_status rmclhip_rcc_segment(rmclhip_rcc* r, const rmclhip_transform* Tbm, const float* ranges_real, int ranges_is_device,
                                   const rmclhip_segmentation_params* sp, const rmclhip_segmentation_views* out, uint32_t counts_out[2]) {
  ApiGuard guard_("rmclhip_rcc_segment");
  if (counts_out) counts_out[0] = counts_out[1] = 0u;
  bool nothing = false;
  if (rmclhip_status st = segment_check("rcc_segment", r, Tbm, ranges_real, sp, &nothing)) return st;
  if (nothing) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  if (rmclhip_status st = segment_enqueue(r, Tbm, ranges_real, ranges_is_device, sp, out)) return st;
  // the scatter launch has stored the totals in host-mapped memory when the stream is idle
  HIPCHK(hipStreamSynchronize(r->stream));
  if (counts_out) { counts_out[0] = r->h_seg_counts.h[0]; counts_out[1] = r->h_seg_counts.h[1]; }
  return RMCLHIP_OK;
}
