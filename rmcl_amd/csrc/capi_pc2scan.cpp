// capi_pc2scan.cpp -- sensor_msgs/PointCloud2 bytes -> range image of a spherical model (Pc2ToScanNode::convert,
// rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213), as a free function on a context and as the dataset input of a spherical
// operator (see capi_internal.h; kernels in pc2scan.hip)
#include "capi_internal.h"

static_assert(RMCLHIP_PC2SCAN_TRUE_ELEVATION == kPc2ScanTrueElevation && RMCLHIP_PC2SCAN_FLOOR == kPc2ScanFloor &&
              RMCLHIP_PC2SCAN_WRAP_THETA == kPc2ScanWrapTheta && RMCLHIP_PC2SCAN_NEAREST == kPc2ScanNearest, "pc2scan flag values");

static constexpr uint32_t kPc2ScanAllFlags =
    RMCLHIP_PC2SCAN_TRUE_ELEVATION | RMCLHIP_PC2SCAN_FLOOR | RMCLHIP_PC2SCAN_WRAP_THETA | RMCLHIP_PC2SCAN_NEAREST;

// what both entry points check before the first HIP call; fills everything of the launch parameters that is not a pointer
static rmclhip_status pc2scan_check(const char* who, const uint8_t* data, size_t nbytes, const rmclhip_pointcloud2_layout* L,
                                    const rmclhip_transform* T, const rmclhip_spherical_model* m, uint32_t flags, Pc2ScanParams* p) {
  const std::string w(who);
  if (!L || !m) return fail(RMCLHIP_ERR_INVALID, w + ": null");
  if ((flags & ~kPc2ScanAllFlags) != 0u) return fail(RMCLHIP_ERR_INVALID, w + ": unknown flag bits");
  if (L->datatype != 7u && L->datatype != 8u)
    return fail(RMCLHIP_ERR_UNSUPPORTED, w + ": Field X has unknown DataType (FLOAT32 / FLOAT64 only)");
  const uint64_t n_points = static_cast<uint64_t>(L->width) * L->height;
  if (n_points > 0x80000000ull) return fail(RMCLHIP_ERR_INVALID, w + ": more than 2^31 points");
  if (n_points) {
    if (!data) return fail(RMCLHIP_ERR_INVALID, w + ": data is null");
    const uint32_t fsz = (L->datatype == 8u) ? 8u : 4u;
    const uint32_t max_off = std::max(L->offset_x, std::max(L->offset_y, L->offset_z));
    const uint64_t last = static_cast<uint64_t>(L->height - 1u) * L->row_step + static_cast<uint64_t>(L->width - 1u) * L->point_step +
                          max_off + fsz;
    if (last > nbytes) return fail(RMCLHIP_ERR_INVALID, w + ": cloud data shorter than its layout");
  }
  if (T) {
    const float v[7] = {T->R.x, T->R.y, T->R.z, T->R.w, T->t.x, T->t.y, T->t.z};
    for (float f : v)
      if (!std::isfinite(f)) return fail(RMCLHIP_ERR_INVALID, w + ": T_sensor_cloud is not finite");
  }
  // inc == 0 is the one-row / one-column scanner of scan_to_scan.cpp:92-94: every point has id 0 on that axis
  if ((m->phi.inc == 0.0f && m->phi.size != 1u) || (m->theta.inc == 0.0f && m->theta.size != 1u))
    return fail(RMCLHIP_ERR_INVALID, w + ": a zero increment needs size 1");
  if (static_cast<uint64_t>(m->phi.size) * m->theta.size > 0x80000000ull) return fail(RMCLHIP_ERR_INVALID, w + ": more than 2^31 cells");
  std::memset(p, 0, sizeof(*p));
  p->n_points = static_cast<uint32_t>(n_points);
  p->width = L->width; p->point_step = L->point_step; p->row_step = L->row_step;
  p->off_x = L->offset_x; p->off_y = L->offset_y; p->off_z = L->offset_z;
  p->is_f64 = (L->datatype == 8u) ? 1u : 0u;
  p->has_T = T ? 1u : 0u;
  p->T = T ? to_x(T) : xidentity();
  p->phi_min = m->phi.min; p->phi_inc = m->phi.inc; p->H = m->phi.size;
  p->theta_min = m->theta.min; p->theta_inc = m->theta.inc; p->W = m->theta.size;
  p->theta_period = 0.0;
  if ((flags & RMCLHIP_PC2SCAN_WRAP_THETA) && m->theta.inc != 0.0f) {
    const double period = 2.0 * 3.14159265358979323846 / static_cast<double>(m->theta.inc);
    if (std::fabs(period - std::nearbyint(period)) < 1e-3) p->theta_period = std::nearbyint(period);
  }
  p->rmin = m->range.min; p->rmax = m->range.max;
  p->range_empty = static_cast<float>(static_cast<double>(m->range.max) + 1.0);   // fillEmpty, scan_operations.cpp:25-39
  p->flags = flags;
  return RMCLHIP_OK;
}

// grow-only scratch of one owner for this launch; points the launch parameters at it
static hipError_t pc2scan_scratch(Pc2ScanScratch& sc, Pc2ScanParams& p) {
  const size_t n_cells = static_cast<size_t>(p.W) * p.H;
  if (const hipError_t e = sc.h_counters.reserve(4)) return e;
  if (const hipError_t e = sc.keys.reserve(n_cells)) return e;
  const size_t n_bin_blocks = pc2scan_blocks(p.n_points);
  if (const hipError_t e = sc.block_counts.reserve(3 * n_bin_blocks + pc2scan_blocks(n_cells))) return e;
  p.keys = sc.keys.p;
  p.bin_counts = sc.block_counts.p;
  p.cell_counts = sc.block_counts.p + 3 * n_bin_blocks;
  return hipSuccess;
}

static void pc2scan_stats(const Pc2ScanParams& p, const uint32_t* c, rmclhip_pc2scan_stats* stats) {
  if (!stats) return;
  stats->n_points = p.n_points;
  stats->n_finite = c[0]; stats->n_in_image = c[1]; stats->n_in_range = c[2]; stats->n_cells_filled = c[3];
}

rmclhip_status rmclhip_pointcloud2_to_scan(rmclhip_ctx* ctx, const uint8_t* data, size_t nbytes, const rmclhip_pointcloud2_layout* L,
                                           int src_is_device, const rmclhip_transform* T, const rmclhip_spherical_model* m, uint32_t flags,
                                           float* ranges_out, int ranges_is_device, rmclhip_pc2scan_stats* stats) {
  ApiGuard guard_("rmclhip_pointcloud2_to_scan");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!ctx) return fail(RMCLHIP_ERR_INVALID, "pointcloud2_to_scan: null");
  Pc2ScanParams p;
  if (rmclhip_status st = pc2scan_check("pointcloud2_to_scan", data, nbytes, L, T, m, flags, &p)) return st;
  const size_t n_cells = static_cast<size_t>(p.W) * p.H;
  if (n_cells && !ranges_out) return fail(RMCLHIP_ERR_INVALID, "pointcloud2_to_scan: ranges_out is null");
  std::lock_guard<std::mutex> lock(ctx->pc2_mtx);
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->pc2_stream == nullptr) HIPCHK(hipStreamCreateWithFlags(&ctx->pc2_stream, hipStreamNonBlocking));
  HIPCHK(pc2scan_scratch(ctx->pc2, p));
  p.data = data;
  if (!src_is_device && p.n_points) {
    HIPCHK(ctx->pc2_raw.reserve(nbytes));
    HIPCHK(hipMemcpyAsync(ctx->pc2_raw.p, data, nbytes, hipMemcpyHostToDevice, ctx->pc2_stream));
    p.data = ctx->pc2_raw.p;
  }
  if (ranges_is_device) {
    p.ranges = ranges_out;
  } else {
    HIPCHK(ctx->pc2.ranges.reserve(n_cells));
    p.ranges = ctx->pc2.ranges.p;
  }
  HIPCHK(launch_pc2scan(p, ctx->pc2.h_counters.d, ctx->pc2_stream));
  if (!ranges_is_device && n_cells)
    HIPCHK(hipMemcpyAsync(ranges_out, p.ranges, n_cells * sizeof(float), hipMemcpyDeviceToHost, ctx->pc2_stream));
  HIPCHK(hipStreamSynchronize(ctx->pc2_stream));
  pc2scan_stats(p, ctx->pc2.h_counters.h, stats);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_input_pointcloud2_scan(rmclhip_rcc* r, const uint8_t* data, size_t nbytes,
                                                      const rmclhip_pointcloud2_layout* L, int src_is_device, const rmclhip_transform* T,
                                                      uint32_t flags, const float** ranges_dev_out, rmclhip_pc2scan_stats* stats) {
  ApiGuard guard_("rmclhip_rcc_set_input_pointcloud2_scan");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (ranges_dev_out) *ranges_dev_out = nullptr;
  if (r) drop_moment_set(r);
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2_scan: null");
  if (r->kind != kModelSpherical)
    return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2_scan: the operator has no spherical model (rmclhip_rcc_set_model_spherical)");
  Pc2ScanParams p;
  if (rmclhip_status st = pc2scan_check("rcc_set_input_pointcloud2_scan", data, nbytes, L, T, &r->sph_model, flags, &p)) return st;
  const size_t n_cells = static_cast<size_t>(r->W) * r->H;
  HIPCHK(hipSetDevice(r->ctx->device));
  // the handle's state as rmclhip_rcc_set_dataset_from_ranges leaves it; the MODEL (W, H, tables, tile planes, a captured graph) stays.
  // Everything below is enqueued on the handle's stream, behind whatever still reads the old dataset.
  r->n_dataset = static_cast<uint32_t>(n_cells);
  r->cpc_rec_n = 0;
  r->ds_has_mask = true;
  HIPCHK(pc2scan_scratch(r->pc2, p));
  HIPCHK(r->pc2.ranges.reserve(n_cells));
  HIPCHK(r->d_ds_points.reserve(3 * n_cells));
  HIPCHK(r->d_ds_mask.reserve(n_cells));
  r->ds_pts = r->d_ds_points.p;
  r->ds_msk = r->d_ds_mask.p;
  p.data = data;
  if (!src_is_device && p.n_points) {
    HIPCHK(r->d_raw.reserve(nbytes));
    HIPCHK(hipMemcpyAsync(r->d_raw.p, data, nbytes, hipMemcpyHostToDevice, r->stream));
    p.data = r->d_raw.p;
  }
  p.ranges = r->pc2.ranges.p;
  p.model_tab = r->d_model_tab.p;
  p.ds_points = n_cells ? r->d_ds_points.p : nullptr;
  p.ds_mask = r->d_ds_mask.p;
  HIPCHK(launch_pc2scan(p, r->pc2.h_counters.d, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  pc2scan_stats(p, r->pc2.h_counters.h, stats);
  if (ranges_dev_out) *ranges_dev_out = r->pc2.ranges.p;
  return RMCLHIP_OK;
}
