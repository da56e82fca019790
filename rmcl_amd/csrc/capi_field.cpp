// capi_field.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- the map's distance field (include/rmclhip.h, DISTANCE FIELD, states the geometry and the lookup; kernels: field_build.hip, field.hip) ----
void rmclhip_field_params_default(rmclhip_field_params* out) {
  if (!out) return;
  out->cell = 0.0f;
  out->margin = 0.0f;
  out->max_nodes = 1ull << 26;
}

// the geometry of a field over [bmin, bmax], in the header's operation order.  banded: the logical lattice of a banded field
// (capi_band_field.cpp) -- no cap on the nodes, at most 2^20 cells per axis; bytes is left 0
RMCL_INTERNAL rmclhip_status field_layout(const std::string& who, const float* bmin, const float* bmax, const rmclhip_field_params* params,
                                          rmclhip_field_info* out, bool banded) {
  rmclhip_field_params p;
  rmclhip_field_params_default(&p);
  if (params) p = *params;
  if (!std::isfinite(p.cell) || p.cell < 0.0f) return fail(RMCLHIP_ERR_INVALID, who + ": cell must be finite and >= 0 (0: automatic)");
  if (!std::isfinite(p.margin) || p.margin < 0.0f) return fail(RMCLHIP_ERR_INVALID, who + ": margin must be finite and >= 0");
  float ext[3];
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(bmin[k]) || !std::isfinite(bmax[k]) || bmin[k] > bmax[k]) return fail(RMCLHIP_ERR_INVALID, who + ": the box is not finite or has min > max");
    ext[k] = (bmax[k] - bmin[k]) + 2.0f * p.margin;
    out->origin[k] = bmin[k] - p.margin;
    if (!std::isfinite(ext[k]) || !std::isfinite(out->origin[k])) return fail(RMCLHIP_ERR_INVALID, who + ": the box plus its margin overflows float32");
  }
  float cell = p.cell;
  if (cell == 0.0f) {
    const double vol = std::max(static_cast<double>(ext[0]), 1e-3) * std::max(static_cast<double>(ext[1]), 1e-3) * std::max(static_cast<double>(ext[2]), 1e-3);
    cell = static_cast<float>(std::cbrt(vol / 2.0e6));
  }
  if (!(cell > 0.0f) || !std::isfinite(cell) || !std::isfinite(1.0f / cell)) return fail(RMCLHIP_ERR_INVALID, who + ": the cell size is not a positive float32");
  const std::string too_many = who + ": the lattice has more than max_nodes nodes (a larger cell, a smaller margin, or a larger max_nodes)";
  uint64_t total = 1;
  for (int k = 0; k < 3; ++k) {
    const float steps = std::ceil(ext[k] / cell);
    if (!(steps < 2147483648.0f)) return fail(RMCLHIP_ERR_INVALID, too_many);
    out->n[k] = std::max(2u, static_cast<uint32_t>(steps) + 1u);
    if (banded) {
      if (out->n[k] - 1u > (1u << 20)) return fail(RMCLHIP_ERR_INVALID, who + ": more than 2^20 cells on an axis (a larger cell or a smaller margin)");
    } else if (out->n[k] > p.max_nodes / total) return fail(RMCLHIP_ERR_INVALID, too_many);   // total * n_k > max_nodes, without the overflow
    total *= out->n[k];
  }
  out->cell = cell;
  out->inv_cell = 1.0f / cell;
  out->n_nodes = total;
  out->bytes = banded ? 0u : total * sizeof(float);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_layout_host(const float* bbox_min, const float* bbox_max, const rmclhip_field_params* params, rmclhip_field_info* info_out) {
  ApiGuard guard_("rmclhip_field_layout_host");
  if (!bbox_min || !bbox_max || !info_out) return fail(RMCLHIP_ERR_INVALID, "field_layout_host: null");
  std::memset(info_out, 0, sizeof(*info_out));
  rmclhip_field_info info{};
  if (rmclhip_status st = field_layout("field_layout_host", bbox_min, bbox_max, params, &info, false)) return st;
  *info_out = info;
  return RMCLHIP_OK;
}

RMCL_INTERNAL FieldView field_view(const rmclhip_field* fd) {
  FieldView v;
  v.lat = fd->d_lat.p;
  for (int k = 0; k < 3; ++k) { v.n[k] = fd->info.n[k]; v.origin[k] = fd->info.origin[k]; }
  v.cell = fd->info.cell;
  v.inv_cell = fd->info.inv_cell;
  // a banded field (capi_band_field.cpp): lat is null
  v.table = fd->d_table.p;
  v.coarse = fd->d_coarse.p;
  v.bricks = fd->d_bricks.p;
  for (int k = 0; k < 3; ++k) v.nb[k] = fd->band.nb[k];
  return v;
}

RMCL_INTERNAL void field_release(rmclhip_field* fd) {
  if (!fd || fd->refs.fetch_sub(1) != 1) return;
  (void)hipSetDevice(fd->ctx->device);
  if (fd->stream) (void)hipStreamSynchronize(fd->stream);
  if (fd->accounted) {
    std::lock_guard<std::mutex> lock(fd->map->grid_mtx);
    fd->map->bytes -= fd->accounted;
  }
  if (fd->stream) (void)hipStreamDestroy(fd->stream);
  rmclhip_map_release(fd->map);
  ctx_release(fd->ctx);
  delete fd;
}

RMCL_INTERNAL rmclhip_status hip_status(const std::string& who, hipError_t e) {
  if (e == hipSuccess) return RMCLHIP_OK;
  (void)hipGetLastError();
  return fail(e == hipErrorOutOfMemory ? RMCLHIP_ERR_NOMEM : RMCLHIP_ERR_HIP, who + ": " + hipGetErrorString(e));
}

RMCL_INTERNAL rmclhip_status field_create_check(const std::string& who, const rmclhip_ctx* ctx, const rmclhip_map* map, rmclhip_field** out) {
  if (!out) return fail(RMCLHIP_ERR_INVALID, who + ": out is null");
  *out = nullptr;
  if (!ctx || !map) return fail(RMCLHIP_ERR_INVALID, who + ": NO MAP");
  if (map->ctx != ctx) return fail(RMCLHIP_ERR_INVALID, who + ": the map belongs to another context");
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status field_new(const std::string& who, rmclhip_ctx* ctx, rmclhip_map* map, const rmclhip_field_info& info, rmclhip_field** out) {
  if (map->info.n_faces == 0u || map->info.n_records == 0u) return fail(RMCLHIP_ERR_INVALID, who + ": the map has no faces");
  HIPCHK(hipSetDevice(ctx->device));
  rmclhip_field* fd = new rmclhip_field();
  fd->ctx = ctx;
  ctx_retain(ctx);
  fd->map = map;
  rmclhip_map_retain(map);
  fd->info = info;
  if (rmclhip_status st = hip_status(who, hipStreamCreateWithFlags(&fd->stream, hipStreamNonBlocking))) {
    field_release(fd);
    return st;
  }
  *out = fd;
  return RMCLHIP_OK;
}

RMCL_INTERNAL FieldBuildParams field_build_params(const rmclhip_field* fd) {
  FieldBuildParams p;
  std::memset(&p, 0, sizeof(p));
  p.nodes = fd->map->d_nodes.p;
  p.tris = fd->map->d_tris.p;
  p.n_tris = fd->map->info.n_records;
  p.fv = field_view(fd);
  return p;
}

RMCL_INTERNAL hipError_t field_level_step(FieldBuildParams& p, uint32_t stride, const uint32_t* cn, uint32_t* rec_out, float* dist_out, hipStream_t s) {
  p.stride = stride;
  for (int k = 0; k < 3; ++k) p.cn[k] = cn[k];
  p.rec_out = rec_out;
  p.dist_out = dist_out;
  const hipError_t e = launch_field_level(p, s);
  p.seed_rec = rec_out;
  p.pstride = stride;
  for (int k = 0; k < 3; ++k) p.pn[k] = cn[k];
  return e;
}

// Coarse to fine, as ensure_near_grid builds the near grid: the nodes far from any surface are the expensive, unbounded queries, and
// there are 4096 x fewer of them at every 16th node per axis than in the lattice.  Each level leaves the record it found per node;
// the next starts every query from the record of the previous level's nearest node.  The stream orders the levels.
static rmclhip_status field_build(rmclhip_field* fd) {
  const std::string who = "field_create";
  HIPCHK_AS(who, fd->d_lat.reserve(fd->info.n_nodes));
  {
    std::lock_guard<std::mutex> lock(fd->map->grid_mtx);
    fd->map->bytes += fd->info.bytes;
    fd->accounted = fd->info.bytes;
  }
  FieldBuildParams p = field_build_params(fd);
  BuildScratch sc;
  const uint32_t n_max = std::max(fd->info.n[0], std::max(fd->info.n[1], fd->info.n[2]));
  for (uint32_t stride = 16u; stride >= 1u; stride >>= 2) {
    if (stride > 1u && n_max <= 2u * stride) continue;   // a level of two nodes per axis prunes nothing
    uint32_t cn[3];
    size_t total = 1;
    for (int k = 0; k < 3; ++k) { cn[k] = (fd->info.n[k] - 1u) / stride + 1u; total *= cn[k]; }
    uint32_t* d_rec = nullptr;
    if (stride > 1u) HIPCHK_AS(who, sc.alloc(&d_rec, total));
    HIPCHK_AS(who, field_level_step(p, stride, cn, d_rec, stride == 1u ? fd->d_lat.p : nullptr, fd->stream));
  }
  return hip_status(who, hipStreamSynchronize(fd->stream));
}

rmclhip_status rmclhip_field_create(rmclhip_ctx* ctx, rmclhip_map* map, const rmclhip_field_params* params, rmclhip_field** out) {
  ApiGuard guard_("rmclhip_field_create");
  if (rmclhip_status st = field_create_check("field_create", ctx, map, out)) return st;
  rmclhip_field_info info{};
  if (rmclhip_status st = field_layout("field_create", map->info.bbox_min, map->info.bbox_max, params, &info, false)) return st;
  rmclhip_field* fd = nullptr;
  if (rmclhip_status st = field_new("field_create", ctx, map, info, &fd)) return st;
  if (rmclhip_status st = field_build(fd)) {
    field_release(fd);   // frees what the build allocated and takes its bytes off the map's device_bytes
    return st;
  }
  *out = fd;
  return RMCLHIP_OK;
}

void rmclhip_field_destroy(rmclhip_field* field) {
  ApiGuard guard_("rmclhip_field_destroy");
  field_release(field);
}

rmclhip_status rmclhip_field_get_info(const rmclhip_field* field, rmclhip_field_info* out) {
  ApiGuard guard_("rmclhip_field_get_info");
  if (!field || !out) return fail(RMCLHIP_ERR_INVALID, "field_get_info: null");
  *out = field->info;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_download(rmclhip_field* field, float* out, size_t capacity) {
  ApiGuard guard_("rmclhip_field_download");
  if (!field || !out) return fail(RMCLHIP_ERR_INVALID, "field_download: null");
  if (field->banded) return fail(RMCLHIP_ERR_INVALID, "field_download: the field is banded (rmclhip_field_download_banded)");
  if (capacity < field->info.n_nodes) return fail(RMCLHIP_ERR_INVALID, "field_download: capacity is smaller than n_nodes");
  HIPCHK(hipSetDevice(field->ctx->device));
  std::lock_guard<std::mutex> lock(field->mtx);
  HIPCHK(upload_on(field->stream, out, field->d_lat.p, field->info.bytes, hipMemcpyDeviceToHost));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_device_view(const rmclhip_field* field, const float** lattice_dev) {
  ApiGuard guard_("rmclhip_field_device_view");
  if (!field || !lattice_dev) return fail(RMCLHIP_ERR_INVALID, "field_device_view: null");
  *lattice_dev = nullptr;
  if (field->banded) return fail(RMCLHIP_ERR_INVALID, "field_device_view: the field is banded, it has no dense lattice");
  *lattice_dev = field->d_lat.p;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_query(rmclhip_field* field, const float* points_xyz, size_t n, int points_on_device, float* distances_out) {
  ApiGuard guard_("rmclhip_field_query");
  if (!field) return fail(RMCLHIP_ERR_INVALID, "field_query: null");
  if (n == 0) return RMCLHIP_OK;
  if (!points_xyz || !distances_out) return fail(RMCLHIP_ERR_INVALID, "field_query: null buffers");
  HIPCHK(hipSetDevice(field->ctx->device));
  std::lock_guard<std::mutex> lock(field->mtx);
  const FieldView fv = field_view(field);
  if (points_on_device) {
    HIPCHK(launch_field_query(fv, points_xyz, n, distances_out, field->stream));
    HIPCHK(hipStreamSynchronize(field->stream));
    return RMCLHIP_OK;
  }
  HIPCHK(field->d_q_points.reserve(3u * n));
  HIPCHK(field->d_q_out.reserve(n));
  HIPCHK(upload_on(field->stream, field->d_q_points.p, points_xyz, 3u * n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(launch_field_query(fv, field->d_q_points.p, n, field->d_q_out.p, field->stream));
  HIPCHK(upload_on(field->stream, distances_out, field->d_q_out.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pf_set_field(rmclhip_pf* f, rmclhip_field* field) {
  ApiGuard guard_("rmclhip_pf_set_field");
  if (!f) return fail(RMCLHIP_ERR_INVALID, "pf_set_field: null");
  if (field && field->map != f->map) return fail(RMCLHIP_ERR_INVALID, "pf_set_field: the field is of another map");
  if (field == f->field) return RMCLHIP_OK;
  // an update in flight on the handle's stream may still read the old lattice
  if (f->field) {
    HIPCHK(hipSetDevice(f->ctx->device));
    HIPCHK(hipStreamSynchronize(f->stream));
  }
  if (field) field->refs.fetch_add(1);
  field_release(f->field);
  f->field = field;
  return RMCLHIP_OK;
}

// rmclhip_pf_update[_async] with a field set (capi_pf.cpp pf_enqueue): the beams are on the device already
RMCL_INTERNAL rmclhip_status pf_field_enqueue(rmclhip_pf* f, const rmclhip_transform* poses, rmclhip_particle_attributes* attrs, uint32_t n, uint32_t n_beams,
                                              const rmclhip_transform* Tsb) {
  if (f->params.correspondence_type != 1u)
    return fail(RMCLHIP_ERR_INVALID, "pf_update: a distance field is set (rmclhip_pf_set_field), which answers correspondence_type 1 only");
  if (n_beams > 8192u) return fail(RMCLHIP_ERR_UNSUPPORTED, "pf_update: more than 8192 beams");
  PfFieldParams p;
  std::memset(&p, 0, sizeof(p));
  p.fv = field_view(f->field);
  p.poses = reinterpret_cast<const xform*>(poses);
  p.attrs = attrs;
  p.n_particles = n;
  p.beams = f->d_beams.p;
  p.n_beams = n_beams;
  p.Tsb = to_x(Tsb);
  p.dist_sigma = f->params.dist_sigma;
  p.max_n_meas = f->params.max_n_meas;
  p.errors = f->errors_dev;
  // particles per workgroup as pf_enqueue deals them: ~2048 beams per workgroup, at most 64 particles; small clouds take fewer until
  // the launch has ~4 workgroups per CU, but never less than one beam per lane
  uint32_t pb = 2048u / n_beams;
  if (pb < 1u) pb = 1u;
  if (pb > 64u) pb = 64u;
  while (pb > 1u && n / pb < 1024u && static_cast<uint64_t>(pb >> 1) * n_beams >= 256u) pb >>= 1;
  p.particles_per_block = pb;
  HIPCHK(launch_pf_update_field(p, f->stream));
  return RMCLHIP_OK;
}
