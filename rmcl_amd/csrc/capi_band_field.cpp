// capi_band_field.cpp -- see capi_internal.h
#include "capi_internal.h"

// ---- the banded distance field (include/rmclhip.h, BANDED DISTANCE FIELD, states the layout; kernels: field_build.hip) ----
void rmclhip_band_field_params_default(rmclhip_band_field_params* out) {
  if (!out) return;
  out->cell = 0.0f;
  out->margin = 0.0f;
  out->max_nodes = 1ull << 26;
  out->band = 0.5f;
  out->reserved = 0u;
}

// the logical lattice and the bricks over [bmin, bmax]; n_stored and bytes stay 0
static rmclhip_status band_layout(const std::string& who, const float* bmin, const float* bmax, const rmclhip_band_field_params* params,
                                  rmclhip_field_info* logical, rmclhip_band_field_info* out) {
  rmclhip_band_field_params p;
  rmclhip_band_field_params_default(&p);
  if (params) p = *params;
  if (!std::isfinite(p.band) || !(p.band > 0.0f)) return fail(RMCLHIP_ERR_INVALID, who + ": band must be finite and > 0");
  const rmclhip_field_params fp = {p.cell, p.margin, p.max_nodes};
  if (rmclhip_status st = field_layout(who, bmin, bmax, &fp, logical, true)) return st;
  std::memset(out, 0, sizeof(*out));
  out->brick_edge = 8u;
  out->n_bricks = 1u;
  out->n_coarse = 1u;
  for (int k = 0; k < 3; ++k) {
    out->nb[k] = (logical->n[k] - 1u + 7u) / 8u;   // <= 2^17: neither product overflows
    out->n_bricks *= out->nb[k];
    out->n_coarse *= static_cast<uint64_t>(out->nb[k]) + 1u;
  }
  out->band = p.band;
  out->reach = p.band + 6.9282032f * logical->cell;
  if (!std::isfinite(out->reach)) return fail(RMCLHIP_ERR_INVALID, who + ": band plus four cell diagonals overflows float32");
  // the coarse lattice alone is over the cap, or the bricks cannot be numbered in a word
  if (out->n_coarse > p.max_nodes || out->n_bricks >= 0xFFFFFFFFull)
    return fail(RMCLHIP_ERR_INVALID, who + ": the coarse lattice has more than max_nodes nodes (a larger cell, a smaller margin, or a larger max_nodes)");
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_band_field_layout_host(const float* bbox_min, const float* bbox_max, const rmclhip_band_field_params* params,
                                              rmclhip_field_info* logical_out, rmclhip_band_field_info* info_out) {
  ApiGuard guard_("rmclhip_band_field_layout_host");
  if (!bbox_min || !bbox_max || !logical_out || !info_out) return fail(RMCLHIP_ERR_INVALID, "band_field_layout_host: null");
  std::memset(logical_out, 0, sizeof(*logical_out));
  std::memset(info_out, 0, sizeof(*info_out));
  rmclhip_field_info logical{};
  rmclhip_band_field_info info{};
  if (rmclhip_status st = band_layout("band_field_layout_host", bbox_min, bbox_max, params, &logical, &info)) return st;
  *logical_out = logical;
  *info_out = info;
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status field_band_check(const std::string& who, const rmclhip_field* field, float max_dist) {
  if (field && field->banded && max_dist > field->band.band)
    return fail(RMCLHIP_ERR_INVALID, who + ": max_dist is larger than the banded field's band (beyond it the field holds no fine values)");
  return RMCLHIP_OK;
}

// Coarse first: every 16th logical node per axis, then every 8th (the coarse lattice, each query started from the level before);
// the bricks are classified and numbered from it, one count is read back, and only then are the fine nodes allocated and filled.
static rmclhip_status band_build(rmclhip_field* fd, uint64_t max_nodes) {
  const std::string who = "field_create_banded";
  rmclhip_band_field_info& bi = fd->band;
  BuildScratch sc;
  hipStream_t s = fd->stream;
  uint32_t *rec16 = nullptr, *rec8 = nullptr, *flags = nullptr, *stored = nullptr;
  unsigned long long *incl = nullptr, *block_tot = nullptr;
  HIPCHK_AS(who, fd->d_coarse.reserve(bi.n_coarse));
  HIPCHK_AS(who, fd->d_table.reserve(bi.n_bricks));
  HIPCHK_AS(who, sc.alloc(&rec8, bi.n_coarse));
  HIPCHK_AS(who, sc.alloc(&flags, bi.n_bricks));
  HIPCHK_AS(who, sc.alloc(&stored, bi.n_bricks));
  HIPCHK_AS(who, sc.alloc(&incl, bi.n_bricks));
  HIPCHK_AS(who, sc.alloc(&block_tot, (bi.n_bricks + 1023u) / 1024u));

  FieldBuildParams p = field_build_params(fd);
  uint32_t cn[3];
  const uint32_t n_max = std::max(fd->info.n[0], std::max(fd->info.n[1], fd->info.n[2]));
  if (n_max > 2u * 16u) {   // (a level of two nodes per axis prunes nothing)
    size_t total = 1;
    for (int k = 0; k < 3; ++k) { cn[k] = (fd->info.n[k] - 1u + 15u) / 16u + 1u; total *= cn[k]; }
    HIPCHK_AS(who, sc.alloc(&rec16, total));
    HIPCHK_AS(who, field_level_step(p, 16u, cn, rec16, nullptr, s));
  }
  for (int k = 0; k < 3; ++k) cn[k] = bi.nb[k] + 1u;
  HIPCHK_AS(who, field_level_step(p, 8u, cn, rec8, fd->d_coarse.p, s));
  HIPCHK_AS(who, launch_band_classify(p.fv, fd->d_coarse.p, bi.reach, flags, s));
  HIPCHK_AS(who, launch_scan_counts(flags, static_cast<uint32_t>(bi.n_bricks), incl, block_tot, s));
  HIPCHK_AS(who, launch_band_table(p.fv, flags, incl, fd->d_table.p, stored, s));
  unsigned long long n_stored = 0;
  HIPCHK_AS(who, upload_on(s, &n_stored, incl + (bi.n_bricks - 1u), sizeof(n_stored), hipMemcpyDeviceToHost));
  bi.n_stored = n_stored;
  if (n_stored > (max_nodes - bi.n_coarse) / kBandBrickNodes)   // 729 n_stored + n_coarse > max_nodes, without the overflow
    return fail(RMCLHIP_ERR_INVALID,
                "field_create_banded: the stored bricks and the coarse lattice have more than max_nodes nodes (a larger cell, a smaller band or "
                "margin, or a larger max_nodes)");
  HIPCHK_AS(who, fd->d_bricks.reserve(std::max<size_t>(static_cast<size_t>(n_stored) * kBandBrickNodes, 1u)));
  BandFillParams f;
  std::memset(&f, 0, sizeof(f));
  f.nodes = p.nodes;
  f.tris = p.tris;
  f.n_tris = p.n_tris;
  f.fv = p.fv;
  f.stored = stored;
  f.n_stored = static_cast<uint32_t>(n_stored);
  f.coarse_rec = rec8;
  f.bricks = fd->d_bricks.p;
  HIPCHK_AS(who, launch_band_fill(f, s));
  HIPCHK_AS(who, hipStreamSynchronize(s));
  bi.bytes = (bi.n_bricks * sizeof(uint32_t) + bi.n_coarse * sizeof(float)) + n_stored * kBandBrickNodes * sizeof(float);
  fd->info.bytes = bi.bytes;
  {
    std::lock_guard<std::mutex> lock(fd->map->grid_mtx);
    fd->map->bytes += bi.bytes;
    fd->accounted = bi.bytes;
  }
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_create_banded(rmclhip_ctx* ctx, rmclhip_map* map, const rmclhip_band_field_params* params, rmclhip_field** out) {
  ApiGuard guard_("rmclhip_field_create_banded");
  if (rmclhip_status st = field_create_check("field_create_banded", ctx, map, out)) return st;
  rmclhip_field_info info{};
  rmclhip_band_field_info band{};
  if (rmclhip_status st = band_layout("field_create_banded", map->info.bbox_min, map->info.bbox_max, params, &info, &band)) return st;
  rmclhip_band_field_params p;
  rmclhip_band_field_params_default(&p);
  if (params) p = *params;
  rmclhip_field* fd = nullptr;
  if (rmclhip_status st = field_new("field_create_banded", ctx, map, info, &fd)) return st;
  fd->banded = true;
  fd->band = band;
  if (rmclhip_status st = band_build(fd, p.max_nodes)) {
    field_release(fd);   // frees what the build allocated; nothing was added to the map's device_bytes
    return st;
  }
  *out = fd;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_get_band_info(const rmclhip_field* field, rmclhip_band_field_info* out) {
  ApiGuard guard_("rmclhip_field_get_band_info");
  if (!field || !out) return fail(RMCLHIP_ERR_INVALID, "field_get_band_info: null");
  if (!field->banded) return fail(RMCLHIP_ERR_INVALID, "field_get_band_info: the field is dense");
  *out = field->band;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_field_download_banded(rmclhip_field* field, uint32_t* table, size_t table_capacity, float* coarse, size_t coarse_capacity,
                                             float* bricks, size_t bricks_capacity) {
  ApiGuard guard_("rmclhip_field_download_banded");
  if (!field) return fail(RMCLHIP_ERR_INVALID, "field_download_banded: null");
  if (!field->banded) return fail(RMCLHIP_ERR_INVALID, "field_download_banded: the field is dense (rmclhip_field_download)");
  const rmclhip_band_field_info& bi = field->band;
  const uint64_t n_fine = bi.n_stored * kBandBrickNodes;
  if ((table && table_capacity < bi.n_bricks) || (coarse && coarse_capacity < bi.n_coarse) || (bricks && bricks_capacity < n_fine))
    return fail(RMCLHIP_ERR_INVALID, "field_download_banded: a capacity is smaller than n_bricks, n_coarse or 729 * n_stored");
  HIPCHK(hipSetDevice(field->ctx->device));
  std::lock_guard<std::mutex> lock(field->mtx);
  if (table) HIPCHK(upload_on(field->stream, table, field->d_table.p, bi.n_bricks * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (coarse) HIPCHK(upload_on(field->stream, coarse, field->d_coarse.p, bi.n_coarse * sizeof(float), hipMemcpyDeviceToHost));
  if (bricks && n_fine != 0u) HIPCHK(upload_on(field->stream, bricks, field->d_bricks.p, n_fine * sizeof(float), hipMemcpyDeviceToHost));
  return RMCLHIP_OK;
}
