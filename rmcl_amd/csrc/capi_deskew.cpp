// capi_deskew.cpp -- motion-compensated PointCloud2 input (include/rmclhip.h, MOTION-COMPENSATED INPUT): the operator form and the
// cloud form of deskew.hip, and the two host helpers -- the scan's motion from base poses, the beam sampler for a moving sensor
// (see capi_internal.h)
#include "capi_internal.h"
#include "deskew_pose.h"

static_assert(sizeof(DeskewKnots) == 2304 && sizeof(DeskewParams) <= 4096, "the knots travel in the launch parameters");
static constexpr size_t kDeskewAuxWords = kDeskewCounters * kDeskewCounterStride, kDeskewAuxBytes = kDeskewAuxWords * sizeof(uint32_t);

// what every entry point checks of the layout, the time field, the filters and the motion before the first HIP call; fills the launch
// parameters that are not pointers, the knots among them
static rmclhip_status deskew_check(const char* who, const uint8_t* data, size_t nbytes, const rmclhip_pointcloud2_layout* L,
                                   const rmclhip_pointcloud2_time* tf, const rmclhip_filter1d* fh, const rmclhip_filter1d* fw,
                                   rmclhip_interval range, const rmclhip_scan_motion* motion, DeskewParams* p) {
  const std::string w(who);
  if (!L) return fail(RMCLHIP_ERR_INVALID, w + ": layout is null");
  if (L->datatype != 7u && L->datatype != 8u)
    return fail(RMCLHIP_ERR_UNSUPPORTED, w + ": Field X has unknown DataType (FLOAT32 / FLOAT64 only)");
  if (tf && tf->datatype != kTimeU32 && tf->datatype != kTimeF32 && tf->datatype != kTimeF64)
    return fail(RMCLHIP_ERR_UNSUPPORTED, w + ": the time field has an unsupported DataType (UINT32 / FLOAT32 / FLOAT64 only)");
  const rmclhip_filter1d none{0u, 0u, 1u};
  const rmclhip_filter1d h = fh ? *fh : none, fwv = fw ? *fw : none;
  if (h.increment == 0u || fwv.increment == 0u || static_cast<uint64_t>(h.skip_begin) + h.skip_end > L->height ||
      static_cast<uint64_t>(fwv.skip_begin) + fwv.skip_end > L->width)
    return fail(RMCLHIP_ERR_INVALID, w + ": bad filter options");
  const uint32_t ow = (L->width - fwv.skip_begin - fwv.skip_end) / fwv.increment;
  const uint32_t oh = (L->height - h.skip_begin - h.skip_end) / h.increment;
  const uint64_t n = static_cast<uint64_t>(ow) * oh;
  if (n > 0x80000000ull) return fail(RMCLHIP_ERR_INVALID, w + ": more than 2^31 points");
  if (n) {
    if (!data || !tf || !motion) return fail(RMCLHIP_ERR_INVALID, w + ": data / time / motion is null");
    const uint64_t fsz = (L->datatype == 8u) ? 8u : 4u, tsz = (tf->datatype == kTimeF64) ? 8u : 4u;
    const uint64_t reach = std::max(std::max<uint64_t>(L->offset_x, std::max(L->offset_y, L->offset_z)) + fsz,
                                    static_cast<uint64_t>(tf->offset) + tsz);
    const uint64_t last = (static_cast<uint64_t>(oh - 1u) * h.increment + h.skip_begin) * L->row_step +
                          (static_cast<uint64_t>(ow - 1u) * fwv.increment + fwv.skip_begin) * L->point_step + reach;
    if (last > nbytes) return fail(RMCLHIP_ERR_INVALID, w + ": cloud data shorter than its layout");
  }
  if (tf && (!std::isfinite(tf->scale) || !std::isfinite(tf->offset_s)))
    return fail(RMCLHIP_ERR_INVALID, w + ": the time field's scale / offset is not finite");
  std::memset(p, 0, sizeof(*p));
  DeskewKnots* knots = &p->knots;
  if (motion) {
    if (motion->n_knots < 2u || motion->n_knots > kDeskewMaxKnots) return fail(RMCLHIP_ERR_INVALID, w + ": the motion needs 2 .. 64 knots");
    if (!motion->knots || !motion->times) return fail(RMCLHIP_ERR_INVALID, w + ": knots / times is null");
    for (uint32_t k = 0; k < motion->n_knots; ++k) {
      const rmclhip_transform& T = motion->knots[k];
      const double t = motion->times[k];
      if (!std::isfinite(t) || (k > 0u && !(t > motion->times[k - 1u])))
        return fail(RMCLHIP_ERR_INVALID, w + ": knot times must be finite and strictly increasing");
      const float v[7] = {T.R.x, T.R.y, T.R.z, T.R.w, T.t.x, T.t.y, T.t.z};
      for (float f : v)
        if (!std::isfinite(f)) return fail(RMCLHIP_ERR_INVALID, w + ": a knot is not finite");
      const double nn = std::sqrt(static_cast<double>(T.R.x) * T.R.x + static_cast<double>(T.R.y) * T.R.y +
                                  static_cast<double>(T.R.z) * T.R.z + static_cast<double>(T.R.w) * T.R.w);
      if (!(std::fabs(nn - 1.0) <= 1e-3)) return fail(RMCLHIP_ERR_INVALID, w + ": a knot's quaternion is not a unit quaternion");
      knots->times[k] = t;
      knots->q[k].x = T.R.x; knots->q[k].y = T.R.y; knots->q[k].z = T.R.z; knots->q[k].w = T.R.w;
      knots->t[k] = mk3(T.t.x, T.t.y, T.t.z);
    }
  }
  p->point_step = L->point_step; p->row_step = L->row_step;
  p->off_x = L->offset_x; p->off_y = L->offset_y; p->off_z = L->offset_z;
  p->is_f64 = (L->datatype == 8u) ? 1u : 0u;
  if (tf) { p->off_t = tf->offset; p->t_type = tf->datatype; p->t_scale = tf->scale; p->t_offset = tf->offset_s; }
  p->h_skip = h.skip_begin; p->h_inc = h.increment; p->w_skip = fwv.skip_begin; p->w_inc = fwv.increment;
  p->out_w = ow; p->out_h = oh;
  p->range_min = range.min; p->range_max = range.max;
  p->n_knots = motion ? motion->n_knots : 0u;
  return RMCLHIP_OK;
}

// counters cleared, the launch, counters down (kDeskewAuxWords words) -- all on s; the caller waits for s before it reads c4
static hipError_t deskew_enqueue(DeskewParams& p, uint8_t* aux, bool cloud_form, uint32_t* c4, hipStream_t s) {
  p.counters = reinterpret_cast<uint32_t*>(aux);
  if (const hipError_t e = hipMemsetAsync(p.counters, 0, kDeskewAuxBytes, s)) return e;
  if (const hipError_t e = launch_deskew(p, cloud_form, s)) return e;
  return hipMemcpyAsync(c4, p.counters, kDeskewAuxBytes, hipMemcpyDeviceToHost, s);
}

static void deskew_stats(const DeskewParams& p, const uint32_t* c, rmclhip_deskew_stats* stats) {
  if (!stats) return;
  stats->n_points = p.out_w * p.out_h;
  stats->n_finite = c[kDeskewFinite * kDeskewCounterStride]; stats->n_valid = c[kDeskewValid * kDeskewCounterStride];
  stats->n_time_clamped = c[kDeskewClamped * kDeskewCounterStride]; stats->n_time_nonfinite = c[kDeskewTimeNonFinite * kDeskewCounterStride];
}

rmclhip_status rmclhip_rcc_set_input_pointcloud2_deskewed(rmclhip_rcc* r, const uint8_t* data, size_t nbytes,
                                                          const rmclhip_pointcloud2_layout* L, const rmclhip_pointcloud2_time* tf,
                                                          const rmclhip_filter1d* fh, const rmclhip_filter1d* fw, rmclhip_interval range,
                                                          int src_is_device, const rmclhip_scan_motion* motion, uint32_t* out_width,
                                                          uint32_t* out_height, rmclhip_deskew_stats* stats) {
  ApiGuard guard_("rmclhip_rcc_set_input_pointcloud2_deskewed");
  if (!r) return fail(RMCLHIP_ERR_INVALID, "rcc_set_input_pointcloud2_deskewed: null");
  DeskewParams p;
  if (rmclhip_status st = deskew_check("rcc_set_input_pointcloud2_deskewed", data, nbytes, L, tf, fh, fw, range, motion, &p)) return st;
  const size_t n = static_cast<size_t>(p.out_w) * p.out_h;
  drop_moment_set(r);
  HIPCHK(hipSetDevice(r->ctx->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  // the handle's state as rmclhip_rcc_set_model_ondn + rmclhip_rcc_set_input_pointcloud2 leave it
  r->kind = kModelOnDn;
  r->ang_aspect = 0.0f;
  r->tile_planes_ok = false;
  r->tuned_kind = r->tuned_batch_kind = 0; r->tuned_frontier = r->tuned_batch_frontier = true; r->tuned_tile = 0; r->tuned_xcd_mapping = 0;
  r->graph_dirty = true;
  r->W = p.out_w; r->H = p.out_h;
  r->range = range;
  r->orig = mk3(0.f, 0.f, 0.f);
  r->n_dataset = static_cast<uint32_t>(n);
  r->cpc_rec_n = 0;
  r->ds_has_mask = true;
  if (out_width) *out_width = p.out_w;
  if (out_height) *out_height = p.out_h;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return RMCLHIP_OK;
  HIPCHK(r->d_model_tab.reserve(6 * n));
  HIPCHK(r->d_ds_points.reserve(3 * n));
  HIPCHK(r->d_ds_mask.reserve(n));
  HIPCHK(r->d_deskew_aux.reserve(kDeskewAuxBytes));
  r->ds_pts = r->d_ds_points.p;
  r->ds_msk = r->d_ds_mask.p;
  p.data = data;
  if (!src_is_device) {
    HIPCHK(r->d_raw.reserve(nbytes));
    HIPCHK(hipMemcpyAsync(r->d_raw.p, data, nbytes, hipMemcpyHostToDevice, r->stream));
    p.data = r->d_raw.p;
  }
  p.origs = r->d_model_tab.p; p.dirs = r->d_model_tab.p + 3 * n;
  p.points = r->d_ds_points.p; p.mask = r->d_ds_mask.p;
  uint32_t c[kDeskewAuxWords] = {};
  const hipError_t e = deskew_enqueue(p, r->d_deskew_aux.p, false, c, r->stream);
  HIPCHK(hipStreamSynchronize(r->stream));   // (also when the enqueue failed half-way: `c` leaves scope)
  if (e != hipSuccess) return fail(RMCLHIP_ERR_HIP, std::string("rcc_set_input_pointcloud2_deskewed: ") + hipGetErrorString(e));
  deskew_stats(p, c, stats);
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_pointcloud2_deskew(rmclhip_ctx* ctx, const uint8_t* data, size_t nbytes, const rmclhip_pointcloud2_layout* L,
                                          const rmclhip_pointcloud2_time* tf, int src_is_device, const rmclhip_scan_motion* motion,
                                          rmclhip_interval range, float* points_out_dev, rmclhip_deskew_stats* stats) {
  ApiGuard guard_("rmclhip_pointcloud2_deskew");
  if (!ctx) return fail(RMCLHIP_ERR_INVALID, "pointcloud2_deskew: null");
  DeskewParams p;
  if (rmclhip_status st = deskew_check("pointcloud2_deskew", data, nbytes, L, tf, nullptr, nullptr, range, motion, &p)) return st;
  const size_t n = static_cast<size_t>(p.out_w) * p.out_h;
  if (n && !points_out_dev) return fail(RMCLHIP_ERR_INVALID, "pointcloud2_deskew: points_out_dev is null");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return RMCLHIP_OK;
  std::lock_guard<std::mutex> lock(ctx->pc2_mtx);
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->pc2_stream == nullptr) HIPCHK(hipStreamCreateWithFlags(&ctx->pc2_stream, hipStreamNonBlocking));
  HIPCHK(ctx->deskew_aux.reserve(kDeskewAuxBytes));
  p.data = data;
  if (!src_is_device) {
    HIPCHK(ctx->pc2_raw.reserve(nbytes));
    HIPCHK(hipMemcpyAsync(ctx->pc2_raw.p, data, nbytes, hipMemcpyHostToDevice, ctx->pc2_stream));
    p.data = ctx->pc2_raw.p;
  }
  p.points = points_out_dev;
  uint32_t c[kDeskewAuxWords] = {};
  const hipError_t e = deskew_enqueue(p, ctx->deskew_aux.p, true, c, ctx->pc2_stream);
  HIPCHK(hipStreamSynchronize(ctx->pc2_stream));
  if (e != hipSuccess) return fail(RMCLHIP_ERR_HIP, std::string("pointcloud2_deskew: ") + hipGetErrorString(e));
  deskew_stats(p, c, stats);
  return RMCLHIP_OK;
}

// ---- host helpers, in double ---------------------------------------------------------------------------------------------------------
namespace {
struct dquat { double x, y, z, w; };
struct dvec { double x, y, z; };
struct dpose { dquat q; dvec t; };

dquat dq_mul(const dquat& a, const dquat& b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
dquat dq_conj(const dquat& q) { return {-q.x, -q.y, -q.z, q.w}; }
dquat dq_unit(const dquat& q) {
  const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return {q.x / n, q.y / n, q.z / n, q.w / n};
}
dvec dq_rot(const dquat& q, const dvec& v) {
  const dquat r = dq_mul(dq_mul(q, dquat{v.x, v.y, v.z, 0.0}), dq_conj(q));
  return {r.x, r.y, r.z};
}
dpose dp_mul(const dpose& a, const dpose& b) {
  const dvec rt = dq_rot(a.q, b.t);
  return {dq_mul(a.q, b.q), {rt.x + a.t.x, rt.y + a.t.y, rt.z + a.t.z}};
}
dpose dp_inv(const dpose& a) {
  const dquat qi = dq_conj(a.q);
  const dvec t = dq_rot(qi, a.t);
  return {qi, {-t.x, -t.y, -t.z}};
}
// slerp on the shorter arc + lerp; u = 0 and u = 1 return the ends themselves
dpose dp_slerp(const dpose& a, const dpose& b, double u) {
  if (u <= 0.0) return a;
  if (u >= 1.0) return b;
  dquat qb = b.q;
  double d = a.q.x * qb.x + a.q.y * qb.y + a.q.z * qb.z + a.q.w * qb.w;
  if (d < 0.0) { qb = {-qb.x, -qb.y, -qb.z, -qb.w}; d = -d; }
  double wa = 1.0 - u, wb = u;
  const double om = std::acos(std::min(1.0, d));
  if (om > 1e-9) {   // (below: the chord IS the arc to double precision)
    const double so = std::sin(om);
    wa = std::sin((1.0 - u) * om) / so; wb = std::sin(u * om) / so;
  }
  dpose r;
  r.q = dq_unit({wa * a.q.x + wb * qb.x, wa * a.q.y + wb * qb.y, wa * a.q.z + wb * qb.z, wa * a.q.w + wb * qb.w});
  r.t = {(1.0 - u) * a.t.x + u * b.t.x, (1.0 - u) * a.t.y + u * b.t.y, (1.0 - u) * a.t.z + u * b.t.z};
  return r;
}
bool dp_from(const rmclhip_transform& T, dpose* out) {
  const float v[7] = {T.R.x, T.R.y, T.R.z, T.R.w, T.t.x, T.t.y, T.t.z};
  for (float f : v)
    if (!std::isfinite(f)) return false;
  const dquat q{T.R.x, T.R.y, T.R.z, T.R.w};
  if (!(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w > 0.0)) return false;
  out->q = dq_unit(q);
  out->t = {T.t.x, T.t.y, T.t.z};
  return true;
}
}  // namespace

rmclhip_status rmclhip_scan_motion_from_base_poses_host(const rmclhip_transform* Tsb, const rmclhip_transform* T_x_b, const double* times,
                                                        uint32_t n, double t_ref, uint32_t subdivide, rmclhip_transform* knots_out,
                                                        double* times_out, uint32_t capacity, uint32_t* n_out) {
  ApiGuard guard_("rmclhip_scan_motion_from_base_poses_host");
  if (n_out) *n_out = 0;
  if (!Tsb || !T_x_b || !times || !knots_out || !times_out || !n_out) return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: null");
  if (n < 2u || subdivide == 0u) return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: needs two poses and subdivide >= 1");
  const uint64_t total = static_cast<uint64_t>(n - 1u) * subdivide + 1u;
  if (total > kDeskewMaxKnots || total > capacity) return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: more than 64 knots, or than capacity");
  dpose sb;
  if (!dp_from(*Tsb, &sb)) return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: Tsb is not a finite pose");
  std::vector<dpose> P(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (!std::isfinite(times[i]) || (i > 0u && !(times[i] > times[i - 1u])))
      return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: times must be finite and strictly increasing");
    if (!dp_from(T_x_b[i], &P[i])) return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: a base pose is not a finite pose");
  }
  if (!(t_ref >= times[0] && t_ref <= times[n - 1u])) return fail(RMCLHIP_ERR_INVALID, "scan_motion_from_base_poses_host: t_ref outside the poses' times");
  uint32_t kr = 0u;
  while (kr + 2u < n && times[kr + 1u] <= t_ref) ++kr;
  const dpose ref = dp_slerp(P[kr], P[kr + 1u], (t_ref - times[kr]) / (times[kr + 1u] - times[kr]));
  const dpose left = dp_mul(dp_inv(sb), dp_inv(ref));   // ~Tsb * ~T_x_b(t_ref)
  uint32_t o = 0u;
  for (uint32_t i = 0; i < n; ++i) {   // the last pose is a knot of its own
    const uint32_t subs = (i == n - 1u) ? 1u : subdivide;
    for (uint32_t m = 0; m < subs; ++m) {
      const double u = static_cast<double>(m) / static_cast<double>(subdivide);
      const dpose b = (m == 0u) ? P[i] : dp_slerp(P[i], P[i + 1u], u);
      const dpose k = dp_mul(dp_mul(left, b), sb);
      const dquat q = dq_unit(k.q);
      rmclhip_transform T;
      std::memset(&T, 0, sizeof(T));
      T.R.x = static_cast<float>(q.x); T.R.y = static_cast<float>(q.y); T.R.z = static_cast<float>(q.z); T.R.w = static_cast<float>(q.w);
      T.t.x = static_cast<float>(k.t.x); T.t.y = static_cast<float>(k.t.y); T.t.z = static_cast<float>(k.t.z);
      knots_out[o] = T;
      times_out[o] = (m == 0u) ? times[i] : times[i] + u * (times[i + 1u] - times[i]);
      ++o;
    }
  }
  *n_out = o;
  return RMCLHIP_OK;
}

// rmclhip_pf_sample_beams_pointcloud2 (capi_pf.cpp) with every beam in its point's own pose: the same draws, retries and index rule
rmclhip_status rmclhip_pf_sample_beams_pointcloud2_deskewed(const uint8_t* data, size_t nbytes, const rmclhip_pointcloud2_layout* L,
                                                            const rmclhip_pointcloud2_time* tf, const rmclhip_scan_motion* motion,
                                                            uint32_t samples, uint64_t seed, rmclhip_range_measurement* beams_out,
                                                            uint32_t* n_out) {
  ApiGuard guard_("rmclhip_pf_sample_beams_pointcloud2_deskewed");
  if (!L || !n_out || (!beams_out && samples)) return fail(RMCLHIP_ERR_INVALID, "pf_sample_beams_pointcloud2_deskewed: null");
  *n_out = 0;
  DeskewParams p;
  const rmclhip_interval any{0.f, 0.f};
  if (rmclhip_status st = deskew_check("pf_sample_beams_pointcloud2_deskewed", data, nbytes, L, tf, nullptr, nullptr, any, motion, &p)) return st;
  if (samples == 0) return RMCLHIP_OK;
  const uint64_t n_points = static_cast<uint64_t>(L->width) * L->height;
  if (n_points == 0 || !data) return fail(RMCLHIP_ERR_INVALID, "pf_sample_beams_pointcloud2_deskewed: empty cloud");
  const bool f64 = p.is_f64 != 0u;
  const DeskewKnots& knots = p.knots;
  std::mt19937 gen(static_cast<uint32_t>(seed));
  auto load = [&](const uint8_t* q) -> float {
    if (f64) { double d; std::memcpy(&d, q, 8); return static_cast<float>(d); }
    float f; std::memcpy(&f, q, 4); return f;
  };
  for (uint32_t sidx = 0; sidx < samples; ++sidx) {
    bool valid = false;
    float x = 0.f, y = 0.f, z = 0.f;
    const uint8_t* ptr = nullptr;
    for (int t = 0; t < 100 && !valid; ++t) {
      const uint64_t id = static_cast<uint64_t>(gen()) % n_points;
      ptr = data + (id / L->width) * L->row_step + (id % L->width) * L->point_step;
      x = load(ptr + L->offset_x); y = load(ptr + L->offset_y); z = load(ptr + L->offset_z);
      valid = (x == x) && (y == y) && (z == z);
    }
    if (!valid) break;
    double raw;
    if (p.t_type == kTimeF64) { std::memcpy(&raw, ptr + p.off_t, 8); }
    else if (p.t_type == kTimeF32) { float f; std::memcpy(&f, ptr + p.off_t, 4); raw = static_cast<double>(f); }
    else { uint32_t u; std::memcpy(&u, ptr + p.off_t, 4); raw = static_cast<double>(u); }
    const double t = p.t_offset + p.t_scale * raw;
    uint32_t k = 0u;
    float s = 0.0f;
    if (deskew_finite(t)) {
      bool clamped;
      k = deskew_segment(knots.times, p.n_knots, t);
      s = deskew_fraction(t, knots.times[k], knots.times[k + 1u], &clamped);
    }
    quat q;
    f3 tr;
    deskew_interp(knots.q[k], knots.t[k], knots.q[k + 1u], knots.t[k + 1u], s, &q, &tr);
    rmclhip_range_measurement m;
    std::memset(&m, 0, sizeof(m));
    const float norm = std::sqrt((x * x + y * y) + z * z);
    const f3 dir = qrot(q, mk3(x / norm, y / norm, z / norm));
    m.orig = {tr.x, tr.y, tr.z};
    m.dir = {dir.x, dir.y, dir.z};
    m.range = norm;
    m.cov[0] = m.cov[4] = m.cov[8] = 0.1f;
    beams_out[(*n_out)++] = m;
  }
  return RMCLHIP_OK;
}
