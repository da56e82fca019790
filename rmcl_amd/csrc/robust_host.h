// robust_host.h -- ROBUST MICP of include/rmclhip.h, the parts host and device share: ONE definition of the M-estimator weight
// (robust.hip evaluates it per correspondence, rmclhip_robust_weight_host on the host), the default parameters and the parameter check.
// Plain C++ besides RM_HD: a host compiler alone builds it (tests/robust_host_check.cpp runs it under the sanitizers).
//
// Every weight is +, *, IEEE / and comparisons in f32 -- no transcendental function, no fused operation: the tree is compiled with
// -ffp-contract=off and hipcc's correctly rounded f32 division, so numpy float32 reproduces each weight bit for bit
// (tests/robust_ref.py).  Keep it so: a fast-math flag or an approximate reciprocal here breaks the byte-for-byte tests.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/rmclhip.h"
#include "devmath.h"

namespace rmclhip {

// w(r) at scale c > 0.  r = 0 gives 1 for every kernel and c / 0 is never formed (HUBER divides only where |r| > c > 0).  u * u may
// overflow to +inf for |r| >> c: the weights then are 0 (CAUCHY, GEMAN_MCCLURE) or decided by |r| < c before u is used (TUKEY).
RM_HD float robust_weight(int kernel, float c, float r) {
  const float a = fabsf(r);
  switch (kernel) {
    case RMCLHIP_ROBUST_HUBER:
      return (a <= c) ? 1.0f : c / a;
    case RMCLHIP_ROBUST_CAUCHY: {
      const float u = r / c;
      return 1.0f / (1.0f + u * u);
    }
    case RMCLHIP_ROBUST_TUKEY: {
      if (!(a < c)) return 0.0f;
      const float u = r / c;
      const float t = 1.0f - u * u;
      return t * t;
    }
    case RMCLHIP_ROBUST_GEMAN_MCCLURE: {
      const float u = r / c;
      const float t = 1.0f + u * u;
      return 1.0f / (t * t);
    }
    default:
      return 1.0f;
  }
}

// c of the MAD mode from the exact median: double arithmetic, ONE rounding to f32, then the floor
RM_HD float robust_mad_scale(float tuning, float median, float scale_min) {
  const float c = static_cast<float>(static_cast<double>(tuning) * 1.4826 * static_cast<double>(median));
  return (c > scale_min) ? c : scale_min;   // (max(c, scale_min); c is never NaN: tuning and median are finite)
}

inline void robust_params_default(int kernel, rmclhip_robust_params* out) {
  float k = 1.0f;
  int kk = kernel;
  switch (kernel) {
    case RMCLHIP_ROBUST_HUBER: k = 1.345f; break;
    case RMCLHIP_ROBUST_CAUCHY: k = 2.385f; break;
    case RMCLHIP_ROBUST_TUKEY: k = 4.685f; break;
    case RMCLHIP_ROBUST_GEMAN_MCCLURE: k = 1.0f; break;
    case RMCLHIP_ROBUST_NONE: break;
    default: kk = RMCLHIP_ROBUST_NONE; break;
  }
  out->kernel = kk;
  out->scale_mode = RMCLHIP_ROBUST_SCALE_MAD;
  out->scale = 1.0f;
  out->tuning = k;
  out->scale_min = 1e-3f;
  out->reserved = 0u;
}

// nullptr: the parameters are valid; else a sentence that names the offending field
inline const char* robust_params_error(const rmclhip_robust_params* p) {
  if (p->kernel < RMCLHIP_ROBUST_NONE || p->kernel > RMCLHIP_ROBUST_GEMAN_MCCLURE) return "kernel: not one of RMCLHIP_ROBUST_*";
  if (p->scale_mode != RMCLHIP_ROBUST_SCALE_FIXED && p->scale_mode != RMCLHIP_ROBUST_SCALE_MAD)
    return "scale_mode: not RMCLHIP_ROBUST_SCALE_FIXED or RMCLHIP_ROBUST_SCALE_MAD";
  if (p->scale_mode == RMCLHIP_ROBUST_SCALE_FIXED) {
    if (!std::isfinite(p->scale) || !(p->scale > 0.0f)) return "scale: must be finite and > 0 in FIXED mode";
  } else {
    if (!std::isfinite(p->tuning) || !(p->tuning > 0.0f)) return "tuning: must be finite and > 0 in MAD mode";
    if (!std::isfinite(p->scale_min) || !(p->scale_min > 0.0f)) return "scale_min: must be finite and > 0 in MAD mode";
  }
  return nullptr;
}

}  // namespace rmclhip
