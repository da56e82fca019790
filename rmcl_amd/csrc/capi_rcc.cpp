// capi_rcc.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- rcc -------------------------------------------------------------------------------------
rmclhip_status rmclhip_rcc_create(rmclhip_ctx* ctx, rmclhip_map* map, rmclhip_rcc** out) {
  ApiGuard guard_("rmclhip_rcc_create");
  if (!out) return fail(RMCLHIP_ERR_INVALID, "rcc_create: out is null");
  *out = nullptr;
  if (!ctx || !map) return fail(RMCLHIP_ERR_INVALID, "rcc_create: NO MAP");
  HIPCHK(hipSetDevice(ctx->device));
  rmclhip_rcc* r = new rmclhip_rcc();
  r->ctx = ctx;
  ctx_retain(ctx);
  r->map = map;
  rmclhip_map_retain(map);
  hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&r->ev0);
  if (e == hipSuccess) e = hipEventCreate(&r->ev1);
  if (e == hipSuccess) e = r->h_stats.reserve(2);
  if (e == hipSuccess) e = r->h_state.reserve(1);
  if (e == hipSuccess) e = r->d_state.reserve(2);
  if (e == hipSuccess) e = r->h_fast_status.reserve(1);
  if (e == hipSuccess) e = r->h_done.reserve(2);
  if (e == hipSuccess) r->h_done.h[0] = r->h_done.h[1] = 0ull;
  if (e == hipSuccess) e = r->h_mom.reserve(1);
  if (e == hipSuccess) std::memset(r->h_mom.h, 0, sizeof(MicpHostBlock));
  if (e == hipSuccess) e = r->d_counter.reserve(1);
  if (e == hipSuccess) e = r->h_call.reserve(1);
  if (e == hipSuccess) e = r->d_call.reserve(1);
  if (e != hipSuccess) {
    rmclhip_rcc_destroy(r);
    return fail(RMCLHIP_ERR_HIP, std::string("rcc_create: ") + hipGetErrorString(e));
  }
  *out = r;
  return RMCLHIP_OK;
}

void rmclhip_rcc_destroy(rmclhip_rcc* r) {
  ApiGuard guard_("rmclhip_rcc_destroy");
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
#define DBG_STEP(x)                                                                                       \
  do {                                                                                                  \
    const hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess && std::getenv("RMCLHIP_DEBUG")) std::fprintf(stderr, "[rmclhip debug] %s -> %s\n", #x, hipGetErrorString(e_)); \
  } while (0)
  if (r->stream) DBG_STEP(hipStreamSynchronize(r->stream));
  DBG_STEP(hipPeekAtLastError());
  if (r->micp_exec) DBG_STEP(hipGraphExecDestroy(r->micp_exec));
  if (r->micp_graph) DBG_STEP(hipGraphDestroy(r->micp_graph));
  if (r->ev_join) DBG_STEP(hipEventDestroy(r->ev_join));
  if (r->ev0) DBG_STEP(hipEventDestroy(r->ev0));
  if (r->ev1) DBG_STEP(hipEventDestroy(r->ev1));
  if (r->stream) DBG_STEP(hipStreamDestroy(r->stream));
#undef DBG_STEP
  rmclhip_map_release(r->map);
  ctx_release(r->ctx);
  delete r;
}

rmclhip_status rmclhip_rcc_set_tsb(rmclhip_rcc* r, const rmclhip_transform* Tsb) {
  ApiGuard guard_("rmclhip_rcc_set_tsb");
  if (!r || !Tsb) return fail(RMCLHIP_ERR_INVALID, "rcc_set_tsb: null");
  r->Tsb = to_x(Tsb);
  return RMCLHIP_OK;
}


rmclhip_status rmclhip_rcc_set_model_spherical(rmclhip_rcc* r, const rmclhip_spherical_model* m) {
  ApiGuard guard_("rmclhip_rcc_set_model_spherical");
  if (!r || !m) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_spherical: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  const uint32_t H = m->phi.size, W = m->theta.size;
  r->kind = kModelSpherical;
  r->sph_model = *m;
  r->graph_dirty = true;
  r->W = W; r->H = H;
  r->range = m->range;
  r->orig = mk3(0.f, 0.f, 0.f);
  r->tile_planes_ok = false;
  r->ang_aspect = (H > 1u && W > 1u && m->theta.inc != 0.0f && std::isfinite(m->phi.inc / m->theta.inc)) ? std::fabs(m->phi.inc / m->theta.inc) : 0.0f;
  if (W == 0 || H == 0) return RMCLHIP_OK;
  // trig tables with the host libm, exactly what rmagine's getDirection evaluates per ray:
  // phi = phi.min + float(vid) * phi.inc, theta likewise
  std::vector<float> tab(2 * static_cast<size_t>(H) + 2 * static_cast<size_t>(W));
  for (uint32_t v = 0; v < H; ++v) {
    const float phi = m->phi.min + static_cast<float>(v) * m->phi.inc;
    tab[v] = cosf(phi);
    tab[H + v] = sinf(phi);
  }
  for (uint32_t h = 0; h < W; ++h) {
    const float th = m->theta.min + static_cast<float>(h) * m->theta.inc;
    tab[2 * H + h] = cosf(th);
    tab[2 * H + W + h] = sinf(th);
  }
  HIPCHK(r->d_model_tab.reserve(tab.size()));
  HIPCHK(upload_on(r->stream, r->d_model_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  return rebuild_tile_planes(r);
}

rmclhip_status rmclhip_rcc_set_model_o1dn(rmclhip_rcc* r, uint32_t width, uint32_t height, rmclhip_interval range,
                                          rmclhip_vec3 orig, const float* dirs) {
  ApiGuard guard_("rmclhip_rcc_set_model_o1dn");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_o1dn: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->kind = kModelO1Dn;
  r->ang_aspect = 0.0f;
  r->graph_dirty = true;
  r->W = width; r->H = height;
  r->range = range;
  r->orig = mk3(orig.x, orig.y, orig.z);
  const size_t n = static_cast<size_t>(width) * height;
  r->tile_planes_ok = false;
  if (n == 0) return RMCLHIP_OK;
  if (!dirs) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_o1dn: dirs is null");
  HIPCHK(r->d_model_tab.reserve(3 * n));
  HIPCHK(upload_on(r->stream, r->d_model_tab.p, dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  return rebuild_tile_planes(r);
}

rmclhip_status rmclhip_rcc_set_model_pinhole(rmclhip_rcc* r, uint32_t width, uint32_t height, rmclhip_interval range,
                                             float fx, float fy, float cx, float cy) {
  ApiGuard guard_("rmclhip_rcc_set_model_pinhole");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_pinhole: null");
  if (!(fx != 0.f) || !(fy != 0.f)) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_pinhole: zero focal length");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->kind = kModelPinhole;
  r->ang_aspect = 0.0f;
  r->graph_dirty = true;
  r->W = width; r->H = height;
  r->range = range;
  r->orig = mk3(0.f, 0.f, 0.f);
  r->pin_fc[0] = fx; r->pin_fc[1] = fy; r->pin_fc[2] = cx; r->pin_fc[3] = cy;
  return rebuild_tile_planes(r);
}

rmclhip_status rmclhip_rcc_set_model_ondn(rmclhip_rcc* r, uint32_t width, uint32_t height, rmclhip_interval range,
                                          const float* origs, const float* dirs) {
  ApiGuard guard_("rmclhip_rcc_set_model_ondn");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_ondn: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->kind = kModelOnDn;
  r->ang_aspect = 0.0f;
  r->tile_planes_ok = false;
  r->tuned_kind = r->tuned_batch_kind = 0; r->tuned_frontier = r->tuned_batch_frontier = true; r->tuned_tile = 0; r->tuned_xcd_mapping = 0;
  r->graph_dirty = true;
  r->W = width; r->H = height;
  r->range = range;
  r->orig = mk3(0.f, 0.f, 0.f);
  const size_t n = static_cast<size_t>(width) * height;
  if (n == 0) return RMCLHIP_OK;
  if (!origs || !dirs) return fail(RMCLHIP_ERR_INVALID, "rcc_set_model_ondn: origs / dirs is null");
  HIPCHK(r->d_model_tab.reserve(6 * n));
  HIPCHK(upload_on(r->stream, r->d_model_tab.p, origs, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(upload_on(r->stream, r->d_model_tab.p + 3 * n, dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_params(rmclhip_rcc* r, float max_dist, float adaptive_max_dist_min) {
  ApiGuard guard_("rmclhip_rcc_set_params");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_params: null");
  r->max_dist = max_dist;
  r->adaptive_max_dist_min = adaptive_max_dist_min;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_dataset(rmclhip_rcc* r, const float* pts, const uint8_t* mask, uint32_t n,
                                       int src_is_device) {
  ApiGuard guard_("rmclhip_rcc_set_dataset");
  if (r) drop_moment_set(r);
  if (!r || (!pts && n > 0)) return fail(RMCLHIP_ERR_INVALID, "rcc_set_dataset: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->n_dataset = n;
  r->cpc_rec_n = 0;   // a new dataset: the closest-point records of the old one mean nothing
  r->ds_has_mask = (mask != nullptr);
  if (n == 0) return RMCLHIP_OK;
  const hipMemcpyKind kind = src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(r->d_ds_points.reserve(3 * static_cast<size_t>(n)));
  HIPCHK(upload_on(r->stream, r->d_ds_points.p, pts, 3 * static_cast<size_t>(n) * sizeof(float), kind));
  if (mask) {
    HIPCHK(r->d_ds_mask.reserve(n));
    HIPCHK(upload_on(r->stream, r->d_ds_mask.p, mask, n, kind));
  }
  r->ds_pts = r->d_ds_points.p;
  r->ds_msk = mask ? r->d_ds_mask.p : nullptr;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_dataset_view(rmclhip_rcc* r, const float* pts_dev, const uint8_t* mask_dev, uint32_t n) {
  ApiGuard guard_("rmclhip_rcc_set_dataset_view");
  if (r) drop_moment_set(r);
  if (!r || (!pts_dev && n > 0)) return fail(RMCLHIP_ERR_INVALID, "rcc_set_dataset_view: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->n_dataset = n;
  r->cpc_rec_n = 0;
  r->ds_has_mask = (mask_dev != nullptr);
  r->ds_pts = pts_dev;
  r->ds_msk = mask_dev;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_dataset_from_ranges(rmclhip_rcc* r, const float* ranges, uint32_t n,
                                                   uint32_t* n_valid_out) {
  ApiGuard guard_("rmclhip_rcc_set_dataset_from_ranges");
  if (r) drop_moment_set(r);
  if (!r || !ranges) return fail(RMCLHIP_ERR_INVALID, "rcc_set_dataset_from_ranges: null");
  if (r->kind == kModelNone) return fail(RMCLHIP_ERR_INVALID, "rcc_set_dataset_from_ranges: no sensor model set");
  if (n != r->W * r->H) return fail(RMCLHIP_ERR_INVALID, "rcc_set_dataset_from_ranges: n != model size");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->n_dataset = n;
  r->cpc_rec_n = 0;
  r->ds_has_mask = true;
  if (n_valid_out) *n_valid_out = 0;
  if (n == 0) return RMCLHIP_OK;
  HIPCHK(r->d_ds_points.reserve(3 * static_cast<size_t>(n)));
  HIPCHK(r->d_ds_mask.reserve(n));
  // stage the ranges in the (not yet used) ranges model buffer region of a scratch allocation
  DevBuf<float> d_r;
  HIPCHK(d_r.reserve(n));
  hipError_t e = upload_on(r->stream, d_r.p, ranges, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(r->d_counter.p, 0, sizeof(uint32_t), r->stream);
  if (e == hipSuccess)
    e = launch_dataset_from_ranges(d_r.p, r->d_model_tab.p, r->kind, r->W, r->H, r->orig, r->pin_fc, r->range.min, r->range.max,
                                   r->d_ds_points.p, r->d_ds_mask.p, r->d_counter.p, r->stream);
  uint32_t nv = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&nv, r->d_counter.p, sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  r->ds_pts = r->d_ds_points.p;
  r->ds_msk = r->d_ds_mask.p;
  if (e != hipSuccess) return fail(RMCLHIP_ERR_HIP, std::string("dataset_from_ranges: ") + hipGetErrorString(e));
  if (n_valid_out) *n_valid_out = nv;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_input_pointcloud2(rmclhip_rcc* r, const uint8_t* data, size_t nbytes,
                                                 const rmclhip_pointcloud2_layout* L, const rmclhip_filter1d* fh,
                                                 const rmclhip_filter1d* fw, rmclhip_interval range, int src_is_device,
                                                 uint32_t* out_width, uint32_t* out_height, uint32_t* n_valid_out) {
  ApiGuard guard_("rmclhip_rcc_set_input_pointcloud2");
  if (r) drop_moment_set(r);
  if (!r || !L) return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2: null");
  if (L->datatype != 7u && L->datatype != 8u)
    return fail(RMCLHIP_ERR_UNSUPPORTED, "rcc_set_input_pointcloud2: Field X has unknown DataType (FLOAT32 / FLOAT64 only)");
  const rmclhip_filter1d none{0u, 0u, 1u};
  const rmclhip_filter1d h = fh ? *fh : none, w = fw ? *fw : none;
  if (h.increment == 0u || w.increment == 0u || static_cast<uint64_t>(h.skip_begin) + h.skip_end > L->height ||
      static_cast<uint64_t>(w.skip_begin) + w.skip_end > L->width)
    return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2: bad filter options");
  const uint32_t ow = (L->width - w.skip_begin - w.skip_end) / w.increment;
  const uint32_t oh = (L->height - h.skip_begin - h.skip_end) / h.increment;
  const size_t n = static_cast<size_t>(ow) * oh;
  const uint32_t fsz = (L->datatype == 8u) ? 8u : 4u;
  if (n) {
    if (!data) return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2: data is null");
    const uint32_t max_off = std::max(L->offset_x, std::max(L->offset_y, L->offset_z));
    const uint64_t last = static_cast<uint64_t>((oh - 1u) * h.increment + h.skip_begin) * L->row_step +
                          static_cast<uint64_t>((ow - 1u) * w.increment + w.skip_begin) * L->point_step + max_off + fsz;
    if (last > nbytes) return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2: cloud data shorter than its layout");
  }
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  r->kind = kModelO1Dn;
  r->ang_aspect = 0.0f;
  r->graph_dirty = true;
  r->W = ow; r->H = oh;
  r->range = range;
  r->orig = mk3(0.f, 0.f, 0.f);
  r->n_dataset = static_cast<uint32_t>(n);
  r->cpc_rec_n = 0;
  r->ds_has_mask = true;
  if (out_width) *out_width = ow;
  if (out_height) *out_height = oh;
  if (n_valid_out) *n_valid_out = 0;
  r->tile_planes_ok = false;
  if (n == 0) return RMCLHIP_OK;
  HIPCHK(r->d_model_tab.reserve(3 * n));
  HIPCHK(r->d_ds_points.reserve(3 * n));
  HIPCHK(r->d_ds_mask.reserve(n));
  r->ds_pts = r->d_ds_points.p;
  r->ds_msk = r->d_ds_mask.p;
  const uint8_t* d_data = data;
  if (!src_is_device) {
    HIPCHK(r->d_raw.reserve(nbytes));
    HIPCHK(hipMemcpyAsync(r->d_raw.p, data, nbytes, hipMemcpyHostToDevice, r->stream));
    d_data = r->d_raw.p;
  }
  HIPCHK(hipMemsetAsync(r->d_counter.p, 0, sizeof(uint32_t), r->stream));
  HIPCHK(launch_pointcloud2_unpack(d_data, L->point_step, L->row_step, L->offset_x, L->offset_y, L->offset_z, L->datatype == 8u,
                                   h.skip_begin, h.increment, w.skip_begin, w.increment, ow, oh, range.min, range.max,
                                   r->d_model_tab.p, r->d_ds_points.p, r->d_ds_mask.p, r->d_counter.p, r->stream));
  if (rmclhip_status st = rebuild_tile_planes(r)) return st;   // the directions just written are the O1Dn model
  uint32_t nv = 0;
  HIPCHK(hipMemcpyAsync(&nv, r->d_counter.p, sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  if (n_valid_out) *n_valid_out = nv;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_input_views(rmclhip_rcc* r, const float** model_table_dev, uint32_t* width, uint32_t* height,
                                       const float** dataset_points_dev, const uint8_t** dataset_mask_dev, uint32_t* n_dataset) {
  ApiGuard guard_("rmclhip_rcc_input_views");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_input_views: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  const bool has_table = (r->kind == kModelSpherical || r->kind == kModelO1Dn || r->kind == kModelOnDn) && r->W != 0u && r->H != 0u;
  if (model_table_dev) *model_table_dev = has_table ? r->d_model_tab.p : nullptr;
  if (width) *width = r->W;
  if (height) *height = r->H;
  if (dataset_points_dev) *dataset_points_dev = r->n_dataset ? r->ds_pts : nullptr;
  if (dataset_mask_dev) *dataset_mask_dev = (r->n_dataset && r->ds_has_mask) ? r->ds_msk : nullptr;
  if (n_dataset) *n_dataset = r->n_dataset;
  return RMCLHIP_OK;
}

static uint32_t pick_tile_w_log2(uint32_t H, bool packet, float ang_aspect = 0.0f) {
  // Spherical models whose COLUMNS are much sparser than their rows (row spacing / column spacing < 0.5: a 32 x 32 or 16 x 16 model
  // over the full circle) get tall tiles, as square in angle as 64 rays allow: 16 wide x 4 tall tiles of such a model span half the
  // horizon, and the rays of a wave share nothing (round 4, 2000 poses x 32x32: 0.47 -> 0.27 ms; profiles/r04_v1_batch_breakdown.txt).
  if (!packet && ang_aspect > 0.0f && ang_aspect < 0.5f) {
    uint32_t hp = 1;
    while (hp < H && hp < 64u) hp <<= 1;                         // tile height <= the model's (rounded up to a power of two)
    uint32_t min_twl = 0;
    while ((64u >> min_twl) > hp) ++min_twl;
    const float want = 0.5f * std::log2(64.0f * ang_aspect);     // log2 of the width that makes the tile square in angle
    int twl = static_cast<int>(std::lround(want));
    twl = std::max(twl, static_cast<int>(min_twl));
    twl = std::min(std::max(twl, 0), 4);                         // (never wider than the general rule below)
    return static_cast<uint32_t>(twl);
  }
  // The 64 rays of a wave (kind 2: of a block) are a tile of the scan image.  The wave-packet traversal (kind 0), whose rays walk
  // together, keeps round 1's square 8x8 tiles (images at least 8 rows tall; flatter tiles for 2-D scanners).  For the per-ray
  // traversals round 3 re-measured the shapes with the frontier start in place (profiles/r03_find_tile_shapes.txt): 16 wide x 4 tall
  // is faster or equal in 10 of 12 (size, map) cells of kinds 23 / 2 -- C2 16.9 -> 16.5 us (sphere), 25.3 -> 24.5 us (room) -- and
  // neutral for pose batches (kind 24).
  const uint32_t max_th = packet ? 8u : 4u;
  uint32_t th = 1;
  while (th < H && th < max_th) th <<= 1;
  uint32_t twl = 0;
  while ((64u >> twl) > th) ++twl;
  return twl;  // tile = 2^twl wide, 64 >> twl tall
}

RMCL_INTERNAL rmclhip_status ensure_model_buffers(rmclhip_rcc* r, size_t n_total) {
  drop_moment_set(r);   // every find form comes through here first
  // only what the selected bundle carries (rmclhip_rcc_set_outputs); a deselected buffer keeps what it has
  if (r->out_mask & RMCLHIP_OUT_HITS) HIPCHK(r->d_hits.reserve(n_total));
  if (r->out_mask & RMCLHIP_OUT_RANGES) HIPCHK(r->d_ranges.reserve(n_total));
  if (r->out_mask & RMCLHIP_OUT_POINTS) HIPCHK(r->d_points.reserve(3 * n_total));
  if (r->out_mask & RMCLHIP_OUT_NORMALS) HIPCHK(r->d_normals.reserve(3 * n_total));
  if (r->out_mask & RMCLHIP_OUT_FACE_IDS) HIPCHK(r->d_face_ids.reserve(n_total));
  return RMCLHIP_OK;
}

// traversal kind of a launch of `nposes` scans (tools/latency_explore.py, tools/perf_explore.py)
RMCL_INTERNAL int find_variant(const rmclhip_rcc* r, uint32_t nposes) {
  if (r->variant != 15) return r->variant;
  if (nposes == 1u && r->tuned_kind != 0) return r->tuned_kind;   // measured on this operator's own map and model (rmclhip_rcc_autotune)
  if (nposes > 1u && r->tuned_batch_kind != 0) return r->tuned_batch_kind;
  const uint64_t rays = static_cast<uint64_t>(r->W) * r->H * nposes;
  if (rays <= 57344u) return 2;   // bound by the slowest ray's fetch chain: four lanes per ray (crossover measured between
                                  // 49152 rays -- quads 13.6 / 20.8 us vs 16.4 / 23.4 -- and 65536 -- 15.9 / 26.3 vs 16.3 / 23.7)
  // one lane per ray, starting at the map's FRONTIER instead of the root (traverse.hip.h frontier_start): from 65 536 to 262 144
  // rays kind 23 is the fastest or within 3 % of it on both benchmark maps (profiles/r03_find_variants_ab.txt), which replaces
  // round 2's three brackets (19 / 21 / 22) by one; larger launches and pose batches are bound by cache-line accesses and issue
  // slots: the 64-B quantised nodes of the FILTER's tree (leaves <= 2: the per-lane triangle loop is short).  At 262 144 rays the
  // sphere prefers 24 (24.9 vs 28.1 us) and the room 23 (38.9 vs 41.1); at 524 288 both prefer 24 (40.5 / 57.8 vs 43.6 / 59.3)
  if (rays <= 262144u) return 23;  // full-precision nodes, branch-free step, one-round-trip leaves, quad-finished tails, leaf trigger
  return 24;                       // quantised nodes of the filter's tree, 16 LDS rows, leaf trigger
}

// `kind`: the traversal the caller is about to launch when it is not the automatic rule's (enqueue_find_with_moments replaces 24 by
// 23); tree, frontier table, tile shape and pre-load bound all follow THAT kind (the tables of the filter's tree under a
// walk of the map's tree start rays at wrong nodes)
RMCL_INTERNAL void fill_find_params(rmclhip_rcc* r, FindParams& p, uint32_t nposes, int kind) {
  const int v = kind >= 0 ? kind : find_variant(r, nposes);
  std::memset(&p, 0, sizeof(p));
  p.nodes = r->map->d_nodes.p;
  p.qnodes = r->map->d_qnodes.p;
  p.cnodes = r->map->d_cnodes.p;
  p.cnodes16 = r->descent_wide ? r->map->d_cnodes16.p : nullptr;
  p.tris = r->map->d_tris.p;
  p.n_nodes = r->map->info.n_nodes;
  p.frontier = r->map->d_frontier.p;
  p.n_frontier = r->map->n_frontier;
  p.frontier_groups = r->map->d_frontier_groups;
  {
    const BvhInfo& bi = r->map->info;
    p.scene_center = mk3(0.5f * (bi.bbox_min[0] + bi.bbox_max[0]), 0.5f * (bi.bbox_min[1] + bi.bbox_max[1]), 0.5f * (bi.bbox_min[2] + bi.bbox_max[2]));
    const float dx = bi.bbox_max[0] - bi.bbox_min[0], dy = bi.bbox_max[1] - bi.bbox_min[1], dz = bi.bbox_max[2] - bi.bbox_min[2];
    p.scene_half_diag = 0.5f * std::sqrt(dx * dx + dy * dy + dz * dz) + bi.pad;
  }
  p.model_tab = r->d_model_tab.p;
  p.W = r->W; p.H = r->H;
  p.tile_w_log2 = (r->tile_override > 0) ? static_cast<uint32_t>(r->tile_override - 1)
                  : ((r->tuned_tile > 0 && !find_kind(v).packet()) ? static_cast<uint32_t>(r->tuned_tile - 1) : pick_tile_w_log2(r->H, find_kind(v).packet(), r->ang_aspect));
  const uint32_t tw = 1u << p.tile_w_log2, th = 64u >> p.tile_w_log2;
  p.tiles_x = (r->W + tw - 1) / tw;
  p.tiles_y = (r->H + th - 1) / th;
  p.tfar = r->range.max;
  p.orig_s = r->orig;
  p.pin_f[0] = r->pin_fc[0]; p.pin_f[1] = r->pin_fc[1]; p.pin_c[0] = r->pin_fc[2]; p.pin_c[1] = r->pin_fc[3];
  p.nposes = nposes;
  // bundle attribute selection (rmclhip_rcc_set_outputs): the kernel skips the stores of a null output
  p.hits = (r->out_mask & RMCLHIP_OUT_HITS) ? r->d_hits.p : nullptr;
  p.ranges = (r->out_mask & RMCLHIP_OUT_RANGES) ? r->d_ranges.p : nullptr;
  p.points = (r->out_mask & RMCLHIP_OUT_POINTS) ? r->d_points.p : nullptr;
  p.normals = (r->out_mask & RMCLHIP_OUT_NORMALS) ? r->d_normals.p : nullptr;
  p.face_ids = (r->out_mask & RMCLHIP_OUT_FACE_IDS) ? r->d_face_ids.p : nullptr;
  p.tile_planes = (r->tile_planes_ok && (nposes == 1u ? r->tuned_frontier : r->tuned_batch_frontier)) ? r->d_tile_planes.p : nullptr;
  {
    // kind 24 (and its frontier-less twin 22: rays on the quantised nodes, triangles in a per-lane loop) walks the FILTER's tree --
    // the same BVH2 cut at leaves of <= 2 instead of <= 4 triangles, the same record array (layout.h): pose batches 6-10 % faster
    // (profiles/r03_find_variants_ab.txt).  That tree has its own node numbering, hence its own frontier table.
    uint32_t need = r->map->info.stack_need;
    if (find_kind(v).filter_tree && r->map->d_qnodes_pf.p != nullptr) {
      p.qnodes = r->map->d_qnodes_pf.p;
      p.frontier = r->map->d_frontier_pf.p;
      p.n_frontier = r->map->n_frontier_pf;
      p.frontier_groups = r->map->d_frontier_groups_pf;
      need = r->map->info.stack_need_pf;
    }
    // The frontier start pre-loads a lane's stack (up to 19 entries for kind 23, 12 for kind 24, more for the quad kind); map_upload's
    // stack_need <= 64 bounds a descent from the ROOT only.  From the frontier the descent may still push what the tree's deepest path
    // pushes, so the start may leave at most 64 - stack_need entries (traverse.hip.h frontier_start returns the root beyond that); a
    // tree that leaves no room for even two starts every ray at the root.
    p.descent_final_cap = r->descent_final_cap;
    p.xcd_mapping = (r->xcd_mapping_override >= 0) ? static_cast<uint32_t>(r->xcd_mapping_override) : r->tuned_xcd_mapping;
    p.descent_levels = (r->descent_levels & 0xFFu) | (r->descent_leaf_cap << 8) | (r->descent_carry ? 1u << 16 : 0u);   // (traverse.hip.h frontier_descent_start: levels | most leaves per ray << 8 | pending candidates << 16)
    p.frontier_max_preload = (need < 64u) ? 64u - need : 0u;
    if (p.frontier_max_preload < 2u) p.tile_planes = nullptr;
  }
}

// The frontier start's plane table belongs to (model, tiling): rebuilt -- one small launch on the handle's stream -- by whatever
// changes either (the model setters, set_variant's tile shape), never inside a find (finds are captured into graphs).
RMCL_INTERNAL rmclhip_status rebuild_tile_planes(rmclhip_rcc* r, bool keep_tuning) {
  r->tile_planes_ok = false;
  if (!keep_tuning) {
    r->tuned_kind = r->tuned_batch_kind = 0;   // a measurement belongs to the model it was taken with
    r->tuned_frontier = r->tuned_batch_frontier = true;
    r->tuned_tile = 0;
    r->tuned_xcd_mapping = 0;
  }
  if (r->kind == kModelOnDn || r->kind == kModelNone || r->W == 0 || r->H == 0) return RMCLHIP_OK;
  FindParams p;
  fill_find_params(r, p, 1);
  HIPCHK(r->d_tile_planes.reserve(static_cast<size_t>(p.tiles_x) * p.tiles_y * 16u));
  HIPCHK(launch_tile_planes(p, r->kind, r->d_tile_planes.p, r->stream));
  r->tile_planes_ok = true;
  r->graph_dirty = true;
  return RMCLHIP_OK;
}

// ---- completion tags, the gate, the moments' hand-over to the host: shared with the corrections (capi_micp.cpp) --------------------
// Wait for the completion tag the LAST kernel of a chain stores in host-mapped memory after its results
// (reduce_common.hip.h publish_tag), instead of hipStreamSynchronize: the tag arrives ~9 us before the stream's completion signal has made its way
// through the runtime (measured on the MICP loop: 84 -> 75 us per correction).
// The tag carries {sequence number of the call, xor of every result word}: the result is accepted only when the sequence number is
// this call's AND the words the host reads add up to the tag's sum; otherwise polling continues.  (Round 2 polled a flag of constant
// value that the host cleared before each launch and read a stale result 1 call in ~10^4; the per-call sequence number is what cured
// it -- the checksum has not rejected a block since, profiles/r05_tag_handoff.txt -- and the xor remains as a belt.)  20 ms without an
// acceptable tag, or wait mode "block" (rmclhip_ctx_set_wait_mode), falls back to the stream.
static inline uint32_t xor_host(const void* p, size_t bytes) {
  const volatile uint32_t* w = static_cast<const volatile uint32_t*>(p);
  uint32_t x = 0;
  for (size_t i = 0; i < bytes / 4; ++i) x ^= w[i];
  return x;
}
// how often a poller saw ITS sequence number in the tag while the result words did not (yet) add up to the tag's sum: the event the
// checksum exists for (rmclhip_debug_tag_retries; profiles/r05_tag_handoff.txt)
static std::atomic<unsigned long long> g_tag_sum_retries{0};

rmclhip_status rmclhip_debug_tag_retries(unsigned long long* retries_out) {
  if (!retries_out) return fail(RMCLHIP_ERR_INVALID, "debug_tag_retries: null");
  *retries_out = g_tag_sum_retries.load();
  return RMCLHIP_OK;
}

RMCL_INTERNAL uint32_t next_seq(rmclhip_rcc* r) {
  if (++r->done_seq == 0u) r->done_seq = 1u;
  return r->done_seq;
}
static inline uint32_t done_sum(const DoneCheck& c) {
  uint32_t x = xor_host(c.base, c.base_bytes);
  if (c.code == nullptr || *c.code == 0u)
    for (int k = 0; k < 3; ++k) if (c.extra[k]) x ^= xor_host(c.extra[k], c.extra_bytes[k]);
  return x;
}
RMCL_INTERNAL hipError_t wait_done(const rmclhip_ctx* ctx, volatile const unsigned long long* tag, uint32_t seq, const DoneCheck& chk,
                                   hipStream_t stream) {
  if (ctx->wait_block.load(std::memory_order_relaxed)) return hipStreamSynchronize(stream);
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
  for (uint32_t spins = 0;; ++spins) {
    const unsigned long long t = *tag;
    if (static_cast<uint32_t>(t) == seq) {
      std::atomic_thread_fence(std::memory_order_acquire);
      if (done_sum(chk) == static_cast<uint32_t>(t >> 32)) return hipSuccess;
      g_tag_sum_retries.fetch_add(1, std::memory_order_relaxed);   // this call's tag, but the words read do not add up to it (yet)
    }
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
    if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() > t_end) return hipStreamSynchronize(stream);
  }
}

// Wait for the end of what the handle's stream holds.  SPIN mode: a one-thread launch behind the chain stores a completion tag in pinned
// memory, which the host sees ~7 us before the stream's own completion signal (a synchronous 128x1024 find: 31.6 -> 24.5 us, round 4);
// the chain has ended -- kernel boundary -- when that launch runs, so its results are complete.  BLOCK mode: hipStreamSynchronize.
RMCL_INTERNAL hipError_t wait_chain_end(rmclhip_rcc* r) {
  if (r->ctx->wait_block.load(std::memory_order_relaxed)) return hipStreamSynchronize(r->stream);
  const uint32_t seq = next_seq(r);
  if (const hipError_t e = launch_host_tag(r->h_done.d, seq, r->stream)) return e;
  DoneCheck none;
  return wait_done(r->ctx, r->h_done.h, seq, none, r->stream);
}

RMCL_INTERNAL float adaptive_max_dist(const rmclhip_rcc* r, double p) {
  // CorrespondencesCPU.cpp:21-23 (float operands, double arithmetic, float store)
  return static_cast<float>(static_cast<double>(r->max_dist) * (1.0 - p) +
                            static_cast<double>(r->adaptive_max_dist_min) * p);
}

// ---- the gate-stable moments on the host (micp_host.h; micp.hip k_micp_publish) -----------------------------------------------
// The band of max_dist' values a speculating find classifies for: max_dist' = max_dist (1 - p) + adaptive_max_dist_min p moves with
// the node's convergence_progress_ from one correction to the next (micp_localization.cpp:988-1007), the find does not know the
// next value, so it takes +-8 % around the last one, clipped to what the two parameters allow.  A max_dist' outside the band
// costs the first computeCrossStatistics of that correction one moment pass of its own (what every call cost before round 4).
RMCL_INTERNAL void gate_band(const rmclhip_rcc* r, float centre, float* lo, float* hi) {
  const float a = std::min(r->max_dist, r->adaptive_max_dist_min), b = std::max(r->max_dist, r->adaptive_max_dist_min);
  *lo = std::max(a, 0.92f * centre);
  *hi = std::min(b, 1.08f * centre);
  if (!(*lo <= centre)) *lo = centre;   // (centre outside [a, b]: parameters changed since; also NaN-safe)
  if (!(*hi >= centre)) *hi = centre;
}

// wait for the tag of a publish launch and take a verified copy of the block (see wait_done for why the sum is checked)
RMCL_INTERNAL hipError_t wait_moments(rmclhip_rcc* r, uint32_t seq, float lo, float hi, float rho_cap, float tau_cap) {
  const MicpHostBlock* hb = r->h_mom.h;
  auto block_sum = [hb]() -> uint32_t {
    uint32_t x = xor_host(hb->mom, sizeof(hb->mom));
    const uint32_t code = *reinterpret_cast<const volatile uint32_t*>(&hb->code);
    const uint32_t n = *reinterpret_cast<const volatile uint32_t*>(&hb->n_uncertain);
    x ^= code ^ n;
    if (n <= kMicpHostMaxUnc) x ^= xor_host(hb->unc, static_cast<size_t>(n) * 9u * sizeof(float));   // (written whenever they fit)
    return x;
  };
  hipError_t e = hipSuccess;
  bool unverified = false;
  if (r->ctx->wait_block.load(std::memory_order_relaxed)) e = hipStreamSynchronize(r->stream);
  else {
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
    volatile const unsigned long long* tag = r->h_done.h;
    for (uint32_t spins = 0;; ++spins) {
      const unsigned long long t = *tag;
      if (static_cast<uint32_t>(t) == seq) {
        std::atomic_thread_fence(std::memory_order_acquire);
        if (block_sum() == static_cast<uint32_t>(t >> 32)) break;
        g_tag_sum_retries.fetch_add(1, std::memory_order_relaxed);
      }
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();
#endif
      if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() > t_end) {
        // 20 ms without this sequence number: either the device is that slow, or a later launch of this handle has already
        // replaced the tag (h_done is shared by every tagged launch).  Drain the stream, then accept the block only if the tag
        // still is this publish's and its sum matches; otherwise the caller takes the streaming reduction
        e = hipStreamSynchronize(r->stream);
        const unsigned long long t2 = *tag;
        std::atomic_thread_fence(std::memory_order_acquire);
        unverified = !(static_cast<uint32_t>(t2) == seq && block_sum() == static_cast<uint32_t>(t2 >> 32));
        break;
      }
    }
  }
  r->mset_pending = false;
  if (e != hipSuccess || unverified) { r->mset.valid = false; return e; }
  MicpMomentSet& ms = r->mset;
  std::memcpy(ms.mom, hb->mom, sizeof(ms.mom));
  ms.gate_lo = lo; ms.gate_hi = hi; ms.rho_cap = rho_cap; ms.tau_cap = tau_cap;
  ms.n_unc = hb->n_uncertain;
  ms.valid = (hb->code == 0u && ms.n_unc <= kMicpHostMaxUnc);
  if (ms.valid) ms.set_undecided(hb->unc, ms.n_unc);   // (component-major copy, padded for the eight-lane sums)
  return hipSuccess;
}

// caps of the next moment set from the pre-transforms the last loop met (as rmclhip_rcc_correct_once learns them)
RMCL_INTERNAL void learn_caps(rmclhip_rcc* r, float max_rho, float max_tau) {
  r->fast_rho_cap = std::max(0.002f, std::max(2.0f * max_rho, 0.9f * r->fast_rho_cap));
  r->fast_tau_cap = std::max(0.005f, std::max(2.0f * max_tau, 0.9f * r->fast_tau_cap));
  r->fast_info.rho_cap = r->fast_rho_cap;
  r->fast_info.tau_cap = r->fast_tau_cap;
}

// Arms the moment epilogue of the find `fp` of kind `fv` (one that has it): one partial row per workgroup (*nb of them) and *wpb mask words
// per workgroup, the gate band and the caps the rows are good for, and -- allocated and zeroed once per handle -- the area through
// which the workgroups of the fold hand their sums over (micp.hip fold_hand_over_row)
RMCL_INTERNAL rmclhip_status arm_moment_epilogue(rmclhip_rcc* r, FindParams& fp, int fv, uint32_t nred, float lo, float hi, float rho_cap,
                                                 float tau_cap, uint32_t* nb_out, uint32_t* wpb_out) {
  const uint32_t nb = find_launch_shape(fp, fv, true).grid_x, wpb = find_kind(fv).tiles_per_block();
  HIPCHK(r->d_fast_partials.reserve(static_cast<size_t>(nb) * kMicpFastMoments));
  HIPCHK(r->d_fast_mask.reserve(static_cast<size_t>(nb) * wpb));
  fp.mom_dataset_points = r->ds_pts;
  fp.mom_dataset_mask = r->ds_has_mask ? r->ds_msk : nullptr;
  fp.mom_n = nred;
  fp.mom_gate_lo = lo; fp.mom_gate_hi = hi; fp.mom_rho_cap = rho_cap; fp.mom_tau_cap = tau_cap;
  fp.mom_partials = r->d_fast_partials.p;
  fp.mom_unc_mask = r->d_fast_mask.p;
  if (!r->d_fold_rows.p) {
    const size_t bytes = kMicpFoldBlocks * kMicpFastMoments * sizeof(double) + kMicpFoldBlocks * sizeof(uint32_t);
    HIPCHK(r->d_fold_rows.reserve((bytes + sizeof(double) - 1u) / sizeof(double)));
    HIPCHK(hipMemset(r->d_fold_rows.p, 0, bytes));
    HIPCHK(hipDeviceSynchronize());
    r->d_fold_flags = reinterpret_cast<uint32_t*>(r->d_fold_rows.p + kMicpFoldBlocks * kMicpFastMoments);
  }
  r->last_fast_rows = nb; r->last_fast_words = wpb * nb;
  *nb_out = nb; *wpb_out = wpb;
  return RMCLHIP_OK;
}

// find + moment epilogue + publish on the handle's stream (the kinds that have it), or find + moment pass + publish (any other kind);
// the caller waits with wait_moments(seq, ...)
RMCL_INTERNAL rmclhip_status enqueue_find_with_moments(rmclhip_rcc* r, const xform& Tsm, float lo, float hi, float rho_cap, float tau_cap,
                                                       uint32_t seq, bool epilogue_allowed) {
  const uint32_t nred = nred_of(r);
  int fv = find_variant(r, 1);
  // scans above 262 144 rays would take kind 24, which has no moment epilogue: the separate moment pass over half a million
  // correspondences costs more (~40 us) than kind 23 loses against kind 24 there (~3 us) -- a correction of a 256 x 2048 scan 93 -> 6x us
  if (epilogue_allowed && fv == 24 && r->variant == 15) fv = 23;
  FindParams fp;
  fill_find_params(r, fp, 1, fv);   // the tree and tables of the kind that RUNS
  fp.Tsm = Tsm;
  fp.Tms = xinv(Tsm);
  r->last_moment_find_kind = fv;
  r->last_moment_find_tiled = epilogue_allowed && find_kind(fv).moments;
  if (r->last_moment_find_tiled) {
    uint32_t nb, wpb;
    if (rmclhip_status st = arm_moment_epilogue(r, fp, fv, nred, lo, hi, rho_cap, tau_cap, &nb, &wpb)) return st;
    HIPCHK(launch_find_moments(fp, r->kind, fv, r->stream));
    HIPCHK(launch_micp_publish_tiled(r->ds_pts, r->d_points.p, r->d_normals.p, nred, nb, r->d_fast_partials.p, r->d_fast_mask.p, r->W,
                                     fp.tiles_x, fp.tile_w_log2, wpb, r->h_mom.d, r->h_done.d, seq, r->d_fold_rows.p, r->d_fold_flags,
                                     r->stream));
  } else {
    HIPCHK(r->d_fast_partials.reserve(static_cast<size_t>(micp_fast_blocks(nred)) * kMicpFastMoments));
    HIPCHK(r->d_fast_mask.reserve((static_cast<size_t>(nred) + 63u) / 64u));
    r->last_fast_rows = micp_fast_blocks(nred); r->last_fast_words = (nred + 63u) / 64u;
    MicpCallLite cl{};
    cl.gate_lo = lo; cl.gate_hi = hi; cl.max_dist = hi; cl.rho_cap = rho_cap; cl.tau_cap = tau_cap; cl.seq = seq;
    HIPCHK(launch_find(fp, r->kind, fv, r->stream));
    HIPCHK(launch_micp_moments_publish(r->ds_pts, r->ds_has_mask ? r->ds_msk : nullptr, r->d_points.p, r->d_normals.p, r->d_hits.p, nred,
                                       r->d_fast_partials.p, r->d_fast_mask.p, cl, r->h_mom.d, r->h_done.d, r->stream));
  }
  return RMCLHIP_OK;
}

// `speculate` (out, nullable): set when the find was enqueued WITH the moment epilogue + publish for the computeCrossStatistics calls
// that will follow it (r->mset_pending, r->mset_seq, r->pend_*): the reference's caller loop (micp_localization.cpp:900-964)
// alternates find() and n x computeCrossStatistics(), so a find that was followed by such calls expects them again.
RMCL_INTERNAL rmclhip_status find_enqueue(rmclhip_rcc* r, const xform& Tbm, bool* speculate) {
  const size_t n = static_cast<size_t>(r->W) * r->H;
  r->n_model = static_cast<uint32_t>(n);
  r->nposes_last = 1;
  if (rmclhip_status st = ensure_model_buffers(r, n)) return st;
  if (speculate) {
    *speculate = false;
    // what the last loop met bounds what this one may meet
    if (r->ccs_since_find != 0u) learn_caps(r, r->ccs_max_rho, r->ccs_max_tau);
    r->ccs_loop = r->ccs_since_find != 0u;
    r->ccs_since_find = 0u; r->ccs_max_rho = 0.f; r->ccs_max_tau = 0.f;
    const int fv = find_variant(r, 1);
    if (r->ccs_loop && r->fast_mode == 1 && r->n_dataset != 0u && find_kind(fv).moments && r->ccs_last_maxd == r->ccs_last_maxd &&
        micp_outputs_selected(r)) {
      gate_band(r, r->ccs_last_maxd, &r->pend_lo, &r->pend_hi);
      r->pend_rho = r->fast_rho_cap; r->pend_tau = r->fast_tau_cap;
      r->mset_seq = next_seq(r);
      if (rmclhip_status st = enqueue_find_with_moments(r, xmul(Tbm, r->Tsb), r->pend_lo, r->pend_hi, r->pend_rho, r->pend_tau, r->mset_seq, true))
        return st;
      r->mset_pending = true;
      ++r->ccs_info.speculative_finds;
      *speculate = true;
      return RMCLHIP_OK;
    }
  }
  FindParams p;
  fill_find_params(r, p, 1);
  p.Tsm = xmul(Tbm, r->Tsb);
  p.Tms = xinv(p.Tsm);
  const int variant = find_variant(r, p.nposes);
  HIPCHK(launch_find(p, r->kind, variant, r->stream));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_find_async(rmclhip_rcc* r, const rmclhip_transform* Tbm_est) {
  ApiGuard guard_("rmclhip_rcc_find_async");
  if (!r || !Tbm_est) return fail(RMCLHIP_ERR_INVALID, "rcc_find: null");
  // RCCOptix.cpp:30-34: nothing to do for an empty model
  if (r->kind == kModelNone || r->W == 0 || r->H == 0) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  bool spec = false;
  return find_enqueue(r, to_x(Tbm_est), &spec);   // (a speculating find's publish is awaited by the first computeCrossStatistics)
}

// Wait for a handle's stream the way the context's wait mode says (rmclhip_ctx_set_wait_mode): SPIN polls hipStreamQuery, then one
// hipStreamSynchronize (immediate) keeps the runtime's own view in order; BLOCK goes to hipStreamSynchronize at once.  20 ms of polling
// at most.  Measured late in round 3 (a synchronous 128x1024 find at the C ABI, median of 200): 32.0 us either way -- on this runtime
// hipStreamSynchronize spins for short waits itself, so for a find the mode only says whose loop burns the core; it is the polled
// completion TAG of the calls that return results (wait_done: computeCrossStatistics 21.5 vs 27.3 us) that the mode really moves.
// For the particle filter's short kernels the polling loop was SLOWER than hipStreamSynchronize (likelihood statistics 19 -> 31 us):
// those entry points call hipStreamSynchronize directly.
static hipError_t stream_wait(const rmclhip_ctx* ctx, hipStream_t stream) {
  if (!ctx->wait_block.load(std::memory_order_relaxed)) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; ++spins) {
      const hipError_t q = hipStreamQuery(stream);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) return q;
      if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
  }
  return hipStreamSynchronize(stream);
}

rmclhip_status rmclhip_rcc_find(rmclhip_rcc* r, const rmclhip_transform* Tbm_est) {
  ApiGuard guard_("rmclhip_rcc_find");
  if (!r || !Tbm_est) return fail(RMCLHIP_ERR_INVALID, "rcc_find: null");
  if (r->kind == kModelNone || r->W == 0 || r->H == 0) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  const bool timed = r->kernel_timing;
  r->reduce_timing_pending = false;   // the events are reused below
  r->find_timing_pending = false;
  if (timed) HIPCHK(hipEventRecord(r->ev0, r->stream));
  bool spec = false;
  if (rmclhip_status st = find_enqueue(r, to_x(Tbm_est), &spec)) return st;
  if (timed) HIPCHK(hipEventRecord(r->ev1, r->stream));
  if (spec) {
    // the publish launch's tag says the find before it on this stream is complete as well -- and reaches the host sooner than the
    // stream's own completion does (see wait_done); the events are read when rmclhip_rcc_last_kernel_ms asks for them
    HIPCHK(wait_moments(r, r->mset_seq, r->pend_lo, r->pend_hi, r->pend_rho, r->pend_tau));
    r->find_timing_pending = timed;
    return RMCLHIP_OK;
  }
  if (timed) {
    HIPCHK(stream_wait(r->ctx, r->stream));
    HIPCHK(hipEventElapsedTime(&r->last_find_ms, r->ev0, r->ev1));
    return RMCLHIP_OK;
  }
  // (round 5, built, measured and removed: the find storing its own completion tag from its last wave instead of the one-thread kernel
  // behind it -- 39 to 70 us per call against 24: profiles/r05_sync_find_tag.txt)
  HIPCHK(wait_chain_end(r));
  return RMCLHIP_OK;
}

// squared search radius of a bounded closest-point query: everything with sqrtf(d2) <= max_dist must stay inside it (sqrtf rounds
// to nearest: d2 <= max_dist^2 (1 + 2^-22) covers every such d2), so hits -- and every output of a point that hits -- are those of
// the unbounded search
static float cpc_bound_d2(const rmclhip_rcc* r) {
  if (!r->cpc_bounded || !(r->max_dist >= 0.0f)) return 3.0e38f;
  const double m = static_cast<double>(r->max_dist);
  const double b = m * m * (1.0 + 1.0 / 1048576.0) + 1e-30;
  return b < 3.0e38 ? static_cast<float>(b) : 3.0e38f;
}

// The map's near grid: ~2 M cubic cells over the map's box (at most 256 per axis), each holding the record closest to its centre --
// one cold closest-point launch over the cell centres, once per map (a few ms; 8 MB), under the map's mutex: operators of one map may
// be used from different threads.
// `full`: every cell gets a record (the particle filter's closest-point mode queries beam END points, metres from any surface);
// otherwise cells farther than two coarse cell diagonals from the surface get none (scan points lie near it) -- the cheap build.
RMCL_INTERNAL rmclhip_status ensure_near_grid(rmclhip_map* m, hipStream_t stream, bool full, const NearGrid** out) {
  *out = nullptr;
  std::lock_guard<std::mutex> lock(m->grid_mtx);
  if (m->grid_slot[1].ready) { *out = &m->grid_slot[1].g; return RMCLHIP_OK; }   // the full grid serves every caller
  rmclhip_map::GridSlot& slot = m->grid_slot[full ? 1 : 0];
  if (slot.ready) { *out = &slot.g; return RMCLHIP_OK; }
  if (slot.failed) return RMCLHIP_OK;
  float ext[3];
  double vol = 1.0;
  for (int k = 0; k < 3; ++k) {
    ext[k] = std::max(m->info.bbox_max[k] - m->info.bbox_min[k], 1e-3f);
    ext[k] *= 1.02f;   // a thin margin: points of a scan lie ON the surface, i.e. on the box's faces
    vol *= ext[k];
  }
  if (!(vol > 0.0) || !std::isfinite(vol)) { slot.failed = true; return RMCLHIP_OK; }
  const float cell = static_cast<float>(std::cbrt(vol / 2.0e6));
  NearGrid g = {};
  size_t total = 1;
  for (int k = 0; k < 3; ++k) {
    g.n[k] = std::max(1u, std::min(256u, static_cast<uint32_t>(std::ceil(ext[k] / cell))));
    g.org[k] = 0.5f * (m->info.bbox_min[k] + m->info.bbox_max[k]) - 0.5f * ext[k];
    g.inv[k] = static_cast<float>(g.n[k]) / ext[k];
    total *= g.n[k];
  }
  DevBuf<uint32_t> cells, coarse;
  hipError_t e = cells.reserve(total);
  if (e != hipSuccess) { slot.failed = true; (void)hipGetLastError(); return RMCLHIP_OK; }   // (a map too large for the table simply runs without it)
  // coarse to fine: a grid of a quarter of the resolution first (its cells far from any surface are the expensive, unbounded queries:
  // 64 x fewer of them), then the full grid with every cell seeded from its coarse parent
  // (slot 0: cells farther than two coarse cell diagonals from the surface get no record: a query point there runs unseeded, as before)
  const float cdiag = 4.0f * cell * 1.7320508f;
  const float skip_d2 = full ? 3.0e38f : (2.0f * cdiag) * (2.0f * cdiag);
  NearGrid c = g;
  size_t ctotal = 1;
  for (int k = 0; k < 3; ++k) { c.n[k] = (g.n[k] + 3u) / 4u; c.inv[k] = g.inv[k] * static_cast<float>(c.n[k]) / static_cast<float>(g.n[k]); ctotal *= c.n[k]; }
  e = coarse.reserve(ctotal);
  if (e == hipSuccess)
    e = launch_cpc_find(m->d_nodes.p, m->d_tris.p, nullptr, static_cast<uint32_t>(ctotal), 0.f, xidentity(), xidentity(), nullptr, nullptr, nullptr, nullptr,
                        nullptr, false, stream, nullptr, coarse.p, m->info.n_records, 3.0e38f, nullptr, &c);
  c.cells = coarse.p;
  if (e == hipSuccess)
    e = launch_cpc_find(m->d_nodes.p, m->d_tris.p, nullptr, static_cast<uint32_t>(total), 0.f, xidentity(), xidentity(), nullptr, nullptr, nullptr, nullptr,
                        nullptr, false, stream, nullptr, cells.p, m->info.n_records, 3.0e38f, &c, &g, skip_d2);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    slot.failed = true;
    return fail(RMCLHIP_ERR_HIP, std::string("near grid: ") + hipGetErrorString(e));
  }
  slot.cells = std::move(cells);
  g.cells = slot.cells.p;
  slot.g = g;
  slot.ready = true;
  m->bytes += total * sizeof(uint32_t);
  *out = &slot.g;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_find_cpc(rmclhip_rcc* r, const rmclhip_transform* Tbm_est) {
  ApiGuard guard_("rmclhip_rcc_find_cpc");
  if (!r || !Tbm_est) return fail(RMCLHIP_ERR_INVALID, "rcc_find_cpc: null");
  if (r->n_dataset == 0) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  // CPCEmbree.cpp:20-25: model buffers are sized like the DATASET (grow-only)
  const size_t n = r->n_dataset;
  if (rmclhip_status st = ensure_model_buffers(r, n)) return st;
  r->n_model = r->n_dataset;
  r->nposes_last = 1;
  const xform Tsm = xmul(to_x(Tbm_est), r->Tsb);
  const bool quad = (r->variant == 15) ? true : (r->variant == 2);  // four lanes per point read the child-major nodes
  // tracking: the record every point was closest to in the previous call of this operator bounds this call's search (same
  // results; rmclhip_rcc_set_cpc_tracking).  The records belong to one dataset of one size: anything else starts cold.
  const uint32_t* seed = nullptr;
  if (r->cpc_tracking) {
    HIPCHK(r->d_cpc_rec.reserve(n));
    if (r->d_cpc_rec.p != r->cpc_rec_ptr) { r->cpc_rec_ptr = r->d_cpc_rec.p; r->cpc_rec_n = 0; }   // (re)allocated
    if (r->cpc_rec_n == r->n_dataset && r->cpc_rec_pts == r->ds_pts) seed = r->d_cpc_rec.p;
  }
  const NearGrid* grid = nullptr;
  if (r->cpc_grid) { if (rmclhip_status gst = ensure_near_grid(r->map, r->stream, false, &grid)) return gst; }
  HIPCHK(launch_cpc_find(quad ? r->map->d_cnodes.p : r->map->d_nodes.p, r->map->d_tris.p, r->ds_pts, r->n_dataset,
                         r->max_dist, Tsm, xinv(Tsm), (r->out_mask & RMCLHIP_OUT_HITS) ? r->d_hits.p : nullptr,
                         (r->out_mask & RMCLHIP_OUT_RANGES) ? r->d_ranges.p : nullptr, (r->out_mask & RMCLHIP_OUT_POINTS) ? r->d_points.p : nullptr,
                         (r->out_mask & RMCLHIP_OUT_NORMALS) ? r->d_normals.p : nullptr,
                         (r->out_mask & RMCLHIP_OUT_FACE_IDS) ? r->d_face_ids.p : nullptr, quad, r->stream, seed, r->cpc_tracking ? r->d_cpc_rec.p : nullptr, r->map->info.n_records,
                         cpc_bound_d2(r), grid));
  if (r->cpc_tracking) { r->cpc_rec_n = r->n_dataset; r->cpc_rec_pts = r->ds_pts; }
  HIPCHK(wait_chain_end(r));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_cpc_tracking(rmclhip_rcc* r, int on) {
  ApiGuard guard_("rmclhip_rcc_set_cpc_tracking");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_cpc_tracking: null");
  r->cpc_tracking = on != 0;
  r->cpc_rec_n = 0;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_cpc_grid(rmclhip_rcc* r, int on) {
  ApiGuard guard_("rmclhip_rcc_set_cpc_grid");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_cpc_grid: null");
  r->cpc_grid = on != 0;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_set_cpc_bounded(rmclhip_rcc* r, int on) {
  ApiGuard guard_("rmclhip_rcc_set_cpc_bounded");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_cpc_bounded: null");
  r->cpc_bounded = on != 0;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_sync(rmclhip_rcc* r) {
  ApiGuard guard_("rmclhip_rcc_sync");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_sync: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  // SPIN mode: a one-thread launch behind whatever the stream holds stores a completion tag that the host sees several microseconds
  // before the stream's own completion signal (what the synchronous find does since round 4); BLOCK mode: hipStreamSynchronize
  if (hipStreamQuery(r->stream) == hipSuccess) return RMCLHIP_OK;
  HIPCHK(wait_chain_end(r));
  return RMCLHIP_OK;
}


RMCL_INTERNAL rmclhip_status reduce_enqueue(rmclhip_rcc* r, const xform& Tpre, const xform* Tpre_dev, float max_dist,
                                     uint32_t nposes, const ReduceTail& tail) {
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  const uint32_t n = nred_of(r);
  if (n == 0) return fail(RMCLHIP_ERR_INVALID, "computeCrossStatistics: empty dataset or model (call find first)");
  if (r->n_model != n && nposes > 1) return fail(RMCLHIP_ERR_INVALID, "batch reduction needs dataset size == model size");
  const uint32_t nb = reduce_num_blocks(n, nposes);
  HIPCHK(r->d_partials.reserve(static_cast<size_t>(nposes) * nb * 16));
  ReduceParams p = reduce_params(r, n, max_dist, nb);
  p.nposes = nposes;
  p.Tpre = Tpre;
  p.Tpre_dev = Tpre_dev;
  HIPCHK(launch_reduce_partials(p, r->stream));
  if (tail.mode == kTailStats) HIPCHK(launch_reduce_finalize(r->d_partials.p, nb, nposes, tail.stats_out, tail.done, tail.seq, r->stream));
  else if (tail.mode == kTailBatchSolve) HIPCHK(launch_batch_solve(r->d_partials.p, nb, nposes, r->Tsb, tail.Tdelta_out, tail.stats_out, r->stream));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_compute_cross_statistics(rmclhip_rcc* r, const rmclhip_transform* T_snew_sold,
                                                    double convergence_progress, rmclhip_cross_statistics* out) {
  ApiGuard guard_("rmclhip_rcc_compute_cross_statistics");
  if (!r || !T_snew_sold || !out) return fail(RMCLHIP_ERR_INVALID, "computeCrossStatistics: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  if (r->nposes_last != 1) return fail(RMCLHIP_ERR_INVALID, "computeCrossStatistics: last find was a batch");
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  // ---- from the moments of this find's correspondences, when a set covers (pre-transform, max_dist'): no launch, no wait.
  // The reference's caller (micp_localization.cpp:915-964) calls this once per sensor and iteration on FIXED correspondences.
  {
    const xform Tpre = to_x(T_snew_sold);
    const float maxd = adaptive_max_dist(r, convergence_progress);
    const float rho = micp_rho(Tpre), tau = micp_tau(Tpre);
    ++r->ccs_since_find;
    r->ccs_last_maxd = maxd;
    r->ccs_max_rho = std::max(r->ccs_max_rho, rho);
    r->ccs_max_tau = std::max(r->ccs_max_tau, tau);
    const uint32_t nred = nred_of(r);
    if (r->fast_mode != 0 && nred != 0 && maxd == maxd) {
      ++r->ccs_info.calls;
      if (r->mset_pending) HIPCHK(wait_moments(r, r->mset_seq, r->pend_lo, r->pend_hi, r->pend_rho, r->pend_tau));
      if (!micp_set_covers(r->mset, Tpre, maxd) && r->mset_passes < 2u && rho == rho && tau == tau) {
        // no covering set (the find did not speculate, or max_dist' / the pre-transform left what it speculated for): ONE moment
        // pass over the find's outputs now -- costs what the streaming reduction below costs -- serves the rest of the loop
        ++r->mset_passes;
        ++r->ccs_info.passes;
        float lo, hi;
        gate_band(r, maxd, &lo, &hi);
        const float rho_cap = std::max(r->fast_rho_cap, 2.0f * rho), tau_cap = std::max(r->fast_tau_cap, 2.0f * tau);
        HIPCHK(r->d_fast_partials.reserve(static_cast<size_t>(micp_fast_blocks(nred)) * kMicpFastMoments));
        HIPCHK(r->d_fast_mask.reserve((static_cast<size_t>(nred) + 63u) / 64u));
        r->last_fast_rows = micp_fast_blocks(nred); r->last_fast_words = (nred + 63u) / 64u;
        MicpCallLite cl{};
        cl.gate_lo = lo; cl.gate_hi = hi; cl.max_dist = maxd; cl.rho_cap = rho_cap; cl.tau_cap = tau_cap; cl.seq = next_seq(r);
        HIPCHK(launch_micp_moments_publish(r->ds_pts, r->ds_has_mask ? r->ds_msk : nullptr, r->d_points.p, r->d_normals.p, r->d_hits.p, nred,
                                           r->d_fast_partials.p, r->d_fast_mask.p, cl, r->h_mom.d, r->h_done.d, r->stream));
        HIPCHK(wait_moments(r, cl.seq, lo, hi, rho_cap, tau_cap));
        if (!r->mset.valid) r->mset_passes = 2u;   // too many undecided correspondences: a second pass would find as many
      }
      if (micp_set_covers(r->mset, Tpre, maxd)) {
        ++r->ccs_info.from_moments;
        from_cs(micp_statistics_from_set(r->mset, Tpre, maxd), out);
        return RMCLHIP_OK;
      }
    }
  }
  ReduceTail tail;
  tail.mode = kTailStats;
  tail.stats_out = r->h_stats.d;  // host-mapped: the finalize launch writes the 64-B result straight to the host
  tail.done = r->h_done.d;
  tail.seq = next_seq(r);
  const bool timed = r->kernel_timing;
  r->find_timing_pending = false;   // the events are reused
  r->reduce_timing_pending = false;
  if (timed) HIPCHK(hipEventRecord(r->ev0, r->stream));
  if (rmclhip_status st = reduce_enqueue(r, to_x(T_snew_sold), nullptr, adaptive_max_dist(r, convergence_progress), 1, tail))
    return st;
  if (timed) HIPCHK(hipEventRecord(r->ev1, r->stream));
  DoneCheck chk; chk.base = &r->h_stats.h[0]; chk.base_bytes = sizeof(cstats);
  HIPCHK(wait_done(r->ctx, r->h_done.h, tail.seq, chk, r->stream));
  r->reduce_timing_pending = timed;   // the events are read when rmclhip_rcc_last_kernel_ms asks for them
  from_cs(r->h_stats.h[0], out);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_download(rmclhip_rcc* r, uint8_t* hits, float* ranges, float* points, float* normals,
                                    uint32_t* face_ids) {
  ApiGuard guard_("rmclhip_rcc_download");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_download: null");
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  const size_t n = static_cast<size_t>(r->n_model) * (r->nposes_last ? r->nposes_last : 1);
  if (n == 0) return RMCLHIP_OK;
  // an attribute that no find of this size has written yet (deselected all along: rmclhip_rcc_set_outputs) has nothing to hand out
  if ((hits && r->d_hits.cap < n) || (ranges && r->d_ranges.cap < n) || (points && r->d_points.cap < 3 * n) ||
      (normals && r->d_normals.cap < 3 * n) || (face_ids && r->d_face_ids.cap < n))
    return fail(RMCLHIP_ERR_INVALID, "rcc_download: a requested attribute was never selected for a find of this size (rmclhip_rcc_set_outputs)");
  if (hits) HIPCHK(hipMemcpy(hits, r->d_hits.p, n, hipMemcpyDeviceToHost));
  if (ranges) HIPCHK(hipMemcpy(ranges, r->d_ranges.p, n * sizeof(float), hipMemcpyDeviceToHost));
  if (points) HIPCHK(hipMemcpy(points, r->d_points.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (normals) HIPCHK(hipMemcpy(normals, r->d_normals.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (face_ids) HIPCHK(hipMemcpy(face_ids, r->d_face_ids.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_device_views(rmclhip_rcc* r, const uint8_t** hits, const float** ranges,
                                        const float** points, const float** normals, const uint32_t** face_ids,
                                        uint32_t* n) {
  ApiGuard guard_("rmclhip_rcc_device_views");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_device_views: null");
  // (a buffer too small for the last find belongs to an attribute no find of that size selected: no view of it)
  const size_t nt = static_cast<size_t>(r->n_model) * (r->nposes_last ? r->nposes_last : 1);
  if (hits) *hits = (r->d_hits.cap >= nt) ? r->d_hits.p : nullptr;
  if (ranges) *ranges = (r->d_ranges.cap >= nt) ? r->d_ranges.p : nullptr;
  if (points) *points = (r->d_points.cap >= 3 * nt) ? r->d_points.p : nullptr;
  if (normals) *normals = (r->d_normals.cap >= 3 * nt) ? r->d_normals.p : nullptr;
  if (face_ids) *face_ids = (r->d_face_ids.cap >= nt) ? r->d_face_ids.p : nullptr;
  if (n) *n = static_cast<uint32_t>(nt);
  return RMCLHIP_OK;
}

// ---- the rmagine-level Simulator interface (rmclhip.h) ----------------------------------------------------------------------
rmclhip_status rmclhip_rcc_set_outputs(rmclhip_rcc* r, uint32_t mask) {
  ApiGuard guard_("rmclhip_rcc_set_outputs");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_outputs: null");
  if (mask == 0u || (mask & ~RMCLHIP_OUT_ALL) != 0u) return fail(RMCLHIP_ERR_INVALID, "rcc_set_outputs: mask must name at least one of the five attributes and nothing else");
  if (mask != r->out_mask) {
    r->out_mask = mask;
    drop_moment_set(r);   // (the set summarises buffers the next find may no longer write)
    r->graph_dirty = true;   // the captured chain holds the find's output pointers by value
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_get_outputs(const rmclhip_rcc* r, uint32_t* mask) {
  if (!r || !mask) return fail(RMCLHIP_ERR_INVALID, "rcc_get_outputs: null");
  *mask = r->out_mask;
  return RMCLHIP_OK;
}

// Simulator::simulate into the caller's bundle: the find kernel with the caller's pointers as its outputs.  One pose from the host goes by
// value (no copy, no compose launch: what rmclhip_rcc_find does); batches and device-resident poses are composed with Tsb on the device.
static rmclhip_status simulate_enqueue(rmclhip_rcc* r, const rmclhip_transform* Tbm, uint32_t nposes, int Tbm_is_device,
                                       const rmclhip_bundle_views* out) {
  if (nposes > 32768) return fail(RMCLHIP_ERR_UNSUPPORTED, "simulate: at most 32768 poses per call");
  FindParams p;
  fill_find_params(r, p, nposes);
  p.hits = out->hits_dev; p.ranges = out->ranges_dev; p.points = out->points_xyz_dev; p.normals = out->normals_xyz_dev;
  p.face_ids = out->face_ids_dev;
  if (nposes == 1u && !Tbm_is_device) {
    p.Tsm = xmul(to_x(Tbm), r->Tsb);
    p.Tms = xinv(p.Tsm);
  } else {
    HIPCHK(r->d_Tsm.reserve(nposes)); HIPCHK(r->d_Tms.reserve(nposes));
    const xform* src = reinterpret_cast<const xform*>(Tbm);
    if (!Tbm_is_device) {
      HIPCHK(r->d_Tbm.reserve(nposes));
      // (pageable source: the copy has staged the caller's poses when it returns; the stream orders the launches behind the DMA)
      HIPCHK(hipMemcpyAsync(r->d_Tbm.p, Tbm, sizeof(xform) * nposes, hipMemcpyHostToDevice, r->stream));
      src = r->d_Tbm.p;
    }
    HIPCHK(launch_compose_poses(src, r->Tsb, r->d_Tsm.p, r->d_Tms.p, nposes, r->stream));
    p.Tsm_arr = r->d_Tsm.p;
    p.Tms_arr = r->d_Tms.p;
  }
  if (rmclhip_status st = batch_order_enqueue(r, p, find_variant(r, nposes))) return st;   // (batches: world order)
  HIPCHK(launch_find(p, r->kind, find_variant(r, nposes), r->stream));
  return RMCLHIP_OK;
}

static rmclhip_status simulate_check(const char* who, rmclhip_rcc* r, const rmclhip_transform* Tbm, uint32_t nposes,
                                     const rmclhip_bundle_views* out, bool* nothing_to_do) {
  *nothing_to_do = false;
  if (!r || !out || (!Tbm && nposes)) return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": null");
  if (nposes == 0 || r->kind == kModelNone || r->W == 0 || r->H == 0) { *nothing_to_do = true; return RMCLHIP_OK; }
  if (!out->hits_dev && !out->ranges_dev && !out->points_xyz_dev && !out->normals_xyz_dev && !out->face_ids_dev)
    return fail(RMCLHIP_ERR_INVALID, std::string(who) + ": the bundle carries no attribute");
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_simulate_async(rmclhip_rcc* r, const rmclhip_transform* Tbm, uint32_t nposes, int Tbm_is_device,
                                          const rmclhip_bundle_views* out) {
  ApiGuard guard_("rmclhip_rcc_simulate_async");
  bool nothing = false;
  if (rmclhip_status st = simulate_check("simulate_async", r, Tbm, nposes, out, &nothing)) return st;
  if (nothing) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  return simulate_enqueue(r, Tbm, nposes, Tbm_is_device, out);
}

rmclhip_status rmclhip_rcc_simulate(rmclhip_rcc* r, const rmclhip_transform* Tbm, uint32_t nposes, int Tbm_is_device,
                                    const rmclhip_bundle_views* out) {
  ApiGuard guard_("rmclhip_rcc_simulate");
  bool nothing = false;
  if (rmclhip_status st = simulate_check("simulate", r, Tbm, nposes, out, &nothing)) return st;
  if (nothing) return RMCLHIP_OK;
  HIPCHK(hipSetDevice(r->ctx->device));
  if (rmclhip_status st = simulate_enqueue(r, Tbm, nposes, Tbm_is_device, out)) return st;
  HIPCHK(wait_chain_end(r));
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status ctx_p2l_ensure(rmclhip_ctx* ctx) {
  if (ctx->p2l_stream != nullptr) return RMCLHIP_OK;
  hipStream_t s = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = ctx->p2l_h_stats.reserve(1);
  if (e == hipSuccess) e = ctx->p2l_h_done.reserve(1);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    ctx->p2l_h_stats.release(); ctx->p2l_h_done.release();
    (void)hipStreamDestroy(s);
    return fail(RMCLHIP_ERR_HIP, std::string("statistics_p2l: ") + hipGetErrorString(e));
  }
  *ctx->p2l_h_done.h = 0ull;
  ctx->p2l_stream = s;
  return RMCLHIP_OK;
}

// rm::statistics_p2l on caller-owned device views: the operator's streaming reduction with the context's own scratch
rmclhip_status rmclhip_statistics_p2l(rmclhip_ctx* ctx, const rmclhip_transform* Tpre, const float* dataset_points,
                                      const uint8_t* dataset_mask, const float* model_points, const float* model_normals,
                                      const uint8_t* model_mask, uint32_t n, float max_dist, rmclhip_cross_statistics* out) {
  ApiGuard guard_("rmclhip_statistics_p2l");
  if (!ctx || !Tpre || !out) return fail(RMCLHIP_ERR_INVALID, "statistics_p2l: null");
  if (n == 0) { from_cs(cs_identity(), out); return RMCLHIP_OK; }   // CrossStatistics::Identity(): nothing measured
  if (!dataset_points || !model_points || !model_normals) return fail(RMCLHIP_ERR_INVALID, "statistics_p2l: null view");
  std::lock_guard<std::mutex> lock(ctx->p2l_mtx);
  HIPCHK(hipSetDevice(ctx->device));
  if (rmclhip_status st = ctx_p2l_ensure(ctx)) return st;
  const uint32_t nb = reduce_num_blocks(n, 1);
  HIPCHK(ctx->p2l_partials.reserve(static_cast<size_t>(nb) * 16u));
  ReduceParams p;
  std::memset(&p, 0, sizeof(p));
  p.dataset_points = dataset_points; p.dataset_mask = dataset_mask;
  p.model_points = model_points; p.model_normals = model_normals; p.model_mask = model_mask;
  p.n = n; p.nposes = 1; p.max_dist = max_dist;
  p.Tpre = to_x(Tpre);
  p.partials = ctx->p2l_partials.p; p.nblocks = nb;
  if (++ctx->p2l_seq == 0u) ctx->p2l_seq = 1u;
  HIPCHK(launch_reduce_partials(p, ctx->p2l_stream));
  HIPCHK(launch_reduce_finalize(ctx->p2l_partials.p, nb, 1, ctx->p2l_h_stats.d, ctx->p2l_h_done.d, ctx->p2l_seq, ctx->p2l_stream));
  DoneCheck chk; chk.base = ctx->p2l_h_stats.h; chk.base_bytes = sizeof(cstats);
  HIPCHK(wait_done(ctx, ctx->p2l_h_done.h, ctx->p2l_seq, chk, ctx->p2l_stream));
  from_cs(*ctx->p2l_h_stats.h, out);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_rcc_correct_batch(rmclhip_rcc* r, const rmclhip_transform* Tbm, uint32_t nposes,
                                         rmclhip_transform* Tdelta_out, rmclhip_cross_statistics* stats_out) {
  ApiGuard guard_("rmclhip_rcc_correct_batch");
  if (!r || !Tbm || !Tdelta_out) return fail(RMCLHIP_ERR_INVALID, "correct_batch: null");
  if (nposes == 0) return RMCLHIP_OK;
  if (r->kind == kModelNone || r->W == 0 || r->H == 0) return fail(RMCLHIP_ERR_INVALID, "correct_batch: no sensor model");
  if (nposes > 32768) return fail(RMCLHIP_ERR_UNSUPPORTED, "correct_batch: at most 32768 poses per call");
  if (!micp_outputs_selected(r)) return fail(RMCLHIP_ERR_INVALID, kNeedMicpOutputs);
  HIPCHK(hipSetDevice(r->ctx->device));
  const size_t n = static_cast<size_t>(r->W) * r->H;
  if (r->n_dataset != n) return fail(RMCLHIP_ERR_INVALID, "correct_batch: dataset size != model size");
  if (nposes > r->h_bT.cap || nposes > r->h_bS.cap) {
    HIPCHK(hipStreamSynchronize(r->stream));
    const uint32_t cap = std::max(nposes, 64u);
    HIPCHK(r->h_bT.reserve(cap));
    HIPCHK(r->h_bS.reserve(cap));
  }
  if (rmclhip_status st = find_batch_enqueue(r, Tbm, nposes)) return st;
  ReduceTail tail;
  tail.mode = kTailBatchSolve;
  tail.Tdelta_out = r->h_bT.d;
  tail.stats_out = r->h_bS.d;
  if (rmclhip_status st = reduce_enqueue(r, xidentity(), nullptr, r->max_dist, nposes, tail)) return st;
  HIPCHK(wait_chain_end(r));
  std::memcpy(Tdelta_out, r->h_bT.h, sizeof(xform) * nposes);
  if (stats_out) std::memcpy(stats_out, r->h_bS.h, sizeof(cstats) * nposes);
  return RMCLHIP_OK;
}

