// deskew_host_loop.cpp -- what a caller does WITHOUT rmclhip_rcc_set_input_pointcloud2_deskewed: one host thread walks the cloud, gives
// every point the pose of its time (segment search, nlerp, rotation: the arithmetic of include/rmclhip.h, MOTION-COMPENSATED INPUT) and
// fills the four arrays set_model_ondn + set_dataset then upload.  FLOAT32 x / y / z / time fields, unorganised or organised without
// filters.  Timed by tools/deskew_time.py beside the device path.
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {
struct Q { float x, y, z, w; };
inline Q qmul(Q a, Q b) {
  Q r;
  r.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
  r.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
  r.y = ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x;
  r.z = ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w;
  return r;
}
}  // namespace

extern "C" uint32_t deskew_host_loop(const uint8_t* data, uint32_t n, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                                     uint32_t off_t, double t_scale, double t_offset, const double* times, const float* knot_q,
                                     const float* knot_t, uint32_t K, float rmin, float rmax, float* origs, float* dirs, float* points,
                                     uint8_t* mask) {
  uint32_t n_valid = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* p = data + static_cast<size_t>(i) * point_step;
    float x, y, z, rawt;
    std::memcpy(&x, p + off_x, 4); std::memcpy(&y, p + off_y, 4); std::memcpy(&z, p + off_z, 4); std::memcpy(&rawt, p + off_t, 4);
    const double t = t_offset + t_scale * static_cast<double>(rawt);
    const bool fin = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
    float range = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (fin) { range = std::sqrt((x * x + y * y) + z * z); dx = x / range; dy = y / range; dz = z / range; }
    const bool t_bad = !std::isfinite(t);
    uint32_t k = 0;
    float s = 0.f;
    if (!t_bad) {
      uint32_t lo = 0, hi = K - 1;
      while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (times[mid] <= t) lo = mid; else hi = mid; }
      k = lo;
      s = static_cast<float>((t - times[k]) / (times[k + 1] - times[k]));
      s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
    }
    const float a = 1.0f - s;
    Q q0, q1;
    std::memcpy(&q0, knot_q + 4 * k, 16); std::memcpy(&q1, knot_q + 4 * (k + 1), 16);
    const float d = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
    if (d < 0.f) { q1.x = -q1.x; q1.y = -q1.y; q1.z = -q1.z; q1.w = -q1.w; }
    Q q{a * q0.x + s * q1.x, a * q0.y + s * q1.y, a * q0.z + s * q1.z, a * q0.w + s * q1.w};
    const float nn = std::sqrt(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    q.x /= nn; q.y /= nn; q.z /= nn; q.w /= nn;
    const float* t0 = knot_t + 3 * k;
    const float* t1 = knot_t + 3 * (k + 1);
    const float tx = a * t0[0] + s * t1[0], ty = a * t0[1] + s * t1[1], tz = a * t0[2] + s * t1[2];
    const Q r = qmul(qmul(q, Q{dx, dy, dz, 0.f}), Q{-q.x, -q.y, -q.z, q.w});
    origs[3 * i] = tx; origs[3 * i + 1] = ty; origs[3 * i + 2] = tz;
    dirs[3 * i] = r.x; dirs[3 * i + 1] = r.y; dirs[3 * i + 2] = r.z;
    points[3 * i] = r.x * range + tx; points[3 * i + 1] = r.y * range + ty; points[3 * i + 2] = r.z * range + tz;
    const bool valid = !((range < rmin) || (range > rmax)) && !t_bad;
    mask[i] = valid ? 1 : 0;
    n_valid += valid ? 1u : 0u;
  }
  return n_valid;
}
