"""POD types of the hot path as numpy dtypes, plus the rmagine-style transform algebra
(evaluated by librmclhip's host entry points, so Python never re-implements arithmetic).

Layouts: rmagine::Transform = {Quaternion{x,y,z,w}, Vector{x,y,z}, uint32 stamp} (32 B,
rmcl_ros/src/nodes/rmcl_localization.cpp:245-249); rmcl::ParticleAttributes (36 B,
ParticleAttributes.hpp:18-34); rmcl::RangeMeasurement (64 B, RangeMeasurement.hpp:10-21).
"""
import ctypes as C
import math

import numpy as np

from . import _capi

VEC3 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
QUAT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")])
TRANSFORM = np.dtype([("R", QUAT), ("t", VEC3), ("stamp", "<u4")])
CROSS_STATISTICS = np.dtype([("dataset_mean", VEC3), ("model_mean", VEC3),
                             ("covariance", "<f4", (9,)), ("n_meas", "<u4")])
GAUSSIAN1D = np.dtype([("mean", "<f4"), ("sigma", "<f4"), ("n_meas", "<u4")])
PARTICLE_ATTRIBUTES = np.dtype([("likelihood", GAUSSIAN1D), ("state_sigma", "<f4", (6,))])
RANGE_MEASUREMENT = np.dtype([("orig", VEC3), ("dir", VEC3), ("range", "<f4"), ("cov", "<f4", (9,))])
# rmclhip_pose_information / rmclhip_pose_covariance (include/rmclhip.h, POSE COVARIANCE): A and covariance row-major 6 x 6 in the
# order x y z rot-x rot-y rot-z; eigenvector k of a block = row k of eigvec_*
POSE_INFORMATION = np.dtype([("A", "<f8", (6, 6)), ("g", "<f8", (6,)), ("rss", "<f8"), ("n_meas", "<u4"), ("pad", "<u4")])
POSE_COVARIANCE = np.dtype([("covariance", "<f8", (6, 6)), ("eig_trans", "<f8", (3,)), ("eigvec_trans", "<f8", (3, 3)),
                            ("eig_rot", "<f8", (3,)), ("eigvec_rot", "<f8", (3, 3)), ("n_degenerate_trans", "<u4"),
                            ("n_degenerate_rot", "<u4"), ("s2", "<f8")])
# rmclhip_robust_statistics (include/rmclhip.h, ROBUST MICP)
ROBUST_STATISTICS = np.dtype([("stats", CROSS_STATISTICS), ("weight_sum", "<f8"), ("wrss", "<f8"), ("rss", "<f8"), ("scale", "<f4"),
                              ("median_abs_residual", "<f4")])
ROBUST_KERNELS = dict(none=_capi.ROBUST_NONE, huber=_capi.ROBUST_HUBER, cauchy=_capi.ROBUST_CAUCHY, tukey=_capi.ROBUST_TUKEY,
                      geman_mcclure=_capi.ROBUST_GEMAN_MCCLURE)
# rmclhip_pose_information_robust (include/rmclhip.h, ROBUST MICP FOR SENSOR RIGS)
POSE_INFORMATION_ROBUST = np.dtype([("info", POSE_INFORMATION), ("weight_sum", "<f8"), ("rss_unweighted", "<f8"), ("scale", "<f4"),
                                    ("median_abs_residual", "<f4")])
assert POSE_INFORMATION_ROBUST.itemsize == 376
assert TRANSFORM.itemsize == 32 and CROSS_STATISTICS.itemsize == 64 and ROBUST_STATISTICS.itemsize == 96
assert POSE_INFORMATION.itemsize == 352 and POSE_COVARIANCE.itemsize == 496
assert PARTICLE_ATTRIBUTES.itemsize == 36 and RANGE_MEASUREMENT.itemsize == 64

MAX_N_MEAS = 10000  # ParticleAttributes.hpp:34


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def transform(q=(0.0, 0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0)):
    """Transform from quaternion (x,y,z,w) and translation."""
    T = np.zeros((), dtype=TRANSFORM)
    T["R"]["x"], T["R"]["y"], T["R"]["z"], T["R"]["w"] = q
    T["t"]["x"], T["t"]["y"], T["t"]["z"] = t
    return T


def identity():
    return transform()


def euler_to_quat(roll, pitch, yaw):
    """rmagine EulerAngles -> Quaternion (ZYX), evaluated in double then rounded to f32."""
    cr, sr = math.cos(roll / 2), math.sin(roll / 2)
    cp, sp = math.cos(pitch / 2), math.sin(pitch / 2)
    cy, sy = math.cos(yaw / 2), math.sin(yaw / 2)
    return (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
            cr * cp * cy + sr * sp * sy)


def transform_from_rpy(t, rpy):
    return transform(euler_to_quat(*rpy), t)


def _one(T, dtype):
    return np.ascontiguousarray(T, dtype=dtype).reshape(1)


def mult(a, b):
    """Transform::operator* (e.g. micp_localization.cpp:963)."""
    a, b, out = _one(a, TRANSFORM), _one(b, TRANSFORM), np.zeros(1, dtype=TRANSFORM)
    _capi.check(_capi.lib().rmclhip_transform_mult(_ptr(a), _ptr(b), _ptr(out)))
    return out[0].copy()


def inv(a):
    """Transform::operator~ (micp_localization.cpp:926)."""
    a, out = _one(a, TRANSFORM), np.zeros(1, dtype=TRANSFORM)
    _capi.check(_capi.lib().rmclhip_transform_inv(_ptr(a), _ptr(out)))
    return out[0].copy()


def cross_statistics_identity():
    return np.zeros((), dtype=CROSS_STATISTICS)


def cross_statistics_merge(a, b):
    """CrossStatistics::operator+= (micp_localization.cpp:936-937)."""
    a, b, out = _one(a, CROSS_STATISTICS), _one(b, CROSS_STATISTICS), np.zeros(1, dtype=CROSS_STATISTICS)
    _capi.check(_capi.lib().rmclhip_cross_statistics_merge(_ptr(a), _ptr(b), _ptr(out)))
    return out[0].copy()


def cross_statistics_merge_weighted(a, wa, b, wb):
    """the merge with real-valued weights where cross_statistics_merge has the counts (rmclhip_cross_statistics_merge_weighted):
    (merged, wa + wb); the counts add whatever the weights are"""
    a, b, out = _one(a, CROSS_STATISTICS), _one(b, CROSS_STATISTICS), np.zeros(1, dtype=CROSS_STATISTICS)
    W = C.c_double(0.0)
    _capi.check(_capi.lib().rmclhip_cross_statistics_merge_weighted(_ptr(a), float(wa), _ptr(b), float(wb), _ptr(out), C.byref(W)))
    return out[0].copy(), W.value


def cross_statistics_transform(T, s):
    """Transform * CrossStatistics (MICPSensor.hpp:182)."""
    T, s, out = _one(T, TRANSFORM), _one(s, CROSS_STATISTICS), np.zeros(1, dtype=CROSS_STATISTICS)
    _capi.check(_capi.lib().rmclhip_cross_statistics_transform(_ptr(T), _ptr(s), _ptr(out)))
    return out[0].copy()


def umeyama_transform(s):
    """rm::umeyama_transform (micp_localization.cpp:952-953)."""
    s, out = _one(s, CROSS_STATISTICS), np.zeros(1, dtype=TRANSFORM)
    _capi.check(_capi.lib().rmclhip_umeyama_transform(_ptr(s), _ptr(out)))
    return out[0].copy()


def pose_information_identity():
    """nothing measured: the neutral element of pose_information_merge"""
    return np.zeros((), dtype=POSE_INFORMATION)


def pose_information_transform(T, info):
    """the frame change of a pose information, the role cross_statistics_transform has (rmclhip_pose_information_transform)"""
    T, info, out = _one(T, TRANSFORM), _one(info, POSE_INFORMATION), np.zeros(1, dtype=POSE_INFORMATION)
    _capi.check(_capi.lib().rmclhip_pose_information_transform(_ptr(T), _ptr(info), _ptr(out)))
    return out[0].copy()


def pose_information_merge(a, b, weight_b=1.0):
    """a + weight_b * b for A, g and rss; the counts add unscaled (rmclhip_pose_information_merge)"""
    a, b, out = _one(a, POSE_INFORMATION), _one(b, POSE_INFORMATION), np.zeros(1, dtype=POSE_INFORMATION)
    _capi.check(_capi.lib().rmclhip_pose_information_merge(_ptr(a), _ptr(b), float(weight_b), _ptr(out)))
    return out[0].copy()


def pose_information_solve(info, rcond=1e-9):
    """the Gauss-Newton step xi = A^+ g = (dt, dtheta) of the dataset in its own frame (rmclhip_pose_information_solve_host)"""
    info, out = _one(info, POSE_INFORMATION), np.zeros(6, dtype=np.float64)
    _capi.check(_capi.lib().rmclhip_pose_information_solve_host(_ptr(info), float(rcond), _ptr(out)))
    return out


def robust_params(kernel="huber", scale=None, tuning=None, scale_min=None, check=True):
    """rmclhip_robust_params for a kernel given by name (ROBUST_KERNELS) or number: the library's defaults
    (rmclhip_robust_params_default: MAD scale, the kernel's customary tuning, scale_min 1e-3); scale=c switches to the FIXED mode.  A
    _capi.RobustParams passes through.  check: refuse invalid parameters here (rmclhip_robust_params_check)."""
    if isinstance(kernel, _capi.RobustParams):
        p = kernel
    else:
        p = _capi.RobustParams()
        _capi.lib().rmclhip_robust_params_default(int(ROBUST_KERNELS[kernel] if isinstance(kernel, str) else kernel), C.byref(p))
        if not isinstance(kernel, str):
            p.kernel = int(kernel)
        if scale is not None:
            p.scale_mode, p.scale = _capi.ROBUST_SCALE_FIXED, float(scale)
        if tuning is not None:
            p.tuning = float(tuning)
        if scale_min is not None:
            p.scale_min = float(scale_min)
    if check:
        _capi.check(_capi.lib().rmclhip_robust_params_check(C.byref(p)))
    return p


def robust_weight(kernel, c, r):
    """the M-estimator weight w(r) at scale c in float32 on the host (rmclhip_robust_weight_host); kernel by name or number"""
    k = int(ROBUST_KERNELS[kernel] if isinstance(kernel, str) else kernel)
    return np.float32(_capi.lib().rmclhip_robust_weight_host(k, float(np.float32(c)), float(np.float32(r))))


def pose_covariance_params(sigma=None, rcond=None, degenerate_variance=None, min_eig_trans=None, min_eig_rot=None):
    """rmclhip_pose_covariance_params; arguments left None keep the library's defaults (rmclhip_pose_covariance_params_default):
    sigma 0 (the noise is estimated from the residuals), rcond 1e-9, degenerate_variance 1e6, min_eig_trans 1e-3, min_eig_rot 1e-3"""
    p = _capi.PoseCovarianceParams()
    _capi.lib().rmclhip_pose_covariance_params_default(C.byref(p))
    for k, v in (("sigma", sigma), ("rcond", rcond), ("degenerate_variance", degenerate_variance), ("min_eig_trans", min_eig_trans),
                 ("min_eig_rot", min_eig_rot)):
        if v is not None:
            setattr(p, k, float(v))
    return p


def pose_covariance(info, params=None, **kw):
    """covariance + degeneracy report of a pose information (rmclhip_pose_covariance_host); params: pose_covariance_params(...) or
    its keyword arguments"""
    p = params if params is not None else pose_covariance_params(**kw)
    info, out = _one(info, POSE_INFORMATION), np.zeros(1, dtype=POSE_COVARIANCE)
    _capi.check(_capi.lib().rmclhip_pose_covariance_host(_ptr(info), C.byref(p), _ptr(out)))
    return out[0].copy()


def pose_covariance_robust(info, params=None, **kw):
    """pose_covariance of a POSE_INFORMATION_ROBUST record: the same algebra on its `info`, the estimated noise
    s2 = rss / (weight_sum - 6) (rmclhip_pose_covariance_robust_host)"""
    p = params if params is not None else pose_covariance_params(**kw)
    info, out = _one(info, POSE_INFORMATION_ROBUST), np.zeros(1, dtype=POSE_COVARIANCE)
    _capi.check(_capi.lib().rmclhip_pose_covariance_robust_host(_ptr(info), C.byref(p), _ptr(out)))
    return out[0].copy()


def debug_solve(ctx, stats, solver):
    """rmclhip_debug_solve (include/rmclhip_lab.h, a test hook): the rotation solve of every CrossStatistics of `stats` by solver
    0 = umeyama() on the host (ctx may be None), 1 = umeyama() on the device, 2 = umeyama_fast() on the device."""
    stats = np.ascontiguousarray(stats, dtype=CROSS_STATISTICS).reshape(-1)
    out = np.zeros(len(stats), dtype=TRANSFORM)
    h = ctx.handle if ctx is not None else None
    _capi.check(_capi.lib().rmclhip_debug_solve(h, _ptr(stats), len(stats), int(solver), _ptr(out)))
    return out


def spherical_model(phi_min, phi_inc, phi_n, theta_min, theta_inc, theta_n, range_min, range_max):
    """rmagine::SphericalModel (fields: rmcl_ros/src/util/conversions.cpp:22-34)."""
    m = _capi.SphericalModel()
    m.phi.min, m.phi.inc, m.phi.size = phi_min, phi_inc, phi_n
    m.theta.min, m.theta.inc, m.theta.size = theta_min, theta_inc, theta_n
    m.range.min, m.range.max = range_min, range_max
    return m


def pf_params(dist_sigma=2.0, real_hit_sim_miss_error=100.0, real_miss_sim_hit_error=100.0,
              real_miss_sim_miss_error=0.0, range_min=0.05, range_max=80.0, max_n_meas=MAX_N_MEAS,
              correspondence_type=0):
    """sensor_update.* defaults of PCDSensorUpdaterEmbree.cpp:122-134."""
    p = _capi.PFParams()
    p.dist_sigma = dist_sigma
    p.real_hit_sim_miss_error = real_hit_sim_miss_error
    p.real_miss_sim_hit_error = real_miss_sim_hit_error
    p.real_miss_sim_miss_error = real_miss_sim_miss_error
    p.sensor_range.min, p.sensor_range.max = range_min, range_max
    p.max_n_meas = max_n_meas
    p.correspondence_type = correspondence_type
    return p


def surface_params(axis=None, height=None, probe_up=None, probe_down=None, min_up_cos=None, align=None, on_miss=None):
    """rmclhip_surface_params: the surface constraint of the motion update (include/rmclhip.h).  Arguments left None keep the library's
    defaults (rmclhip_surface_params_default): axis 0 (map +z; 1 = body z), height 0, probe_up 0.3, probe_down 1.0, min_up_cos 0.7,
    align 0, on_miss 0."""
    p = _capi.SurfaceParams()
    _capi.lib().rmclhip_surface_params_default(C.byref(p))
    for k, v in (("axis", axis), ("height", height), ("probe_up", probe_up), ("probe_down", probe_down), ("min_up_cos", min_up_cos),
                 ("align", align), ("on_miss", on_miss)):
        if v is not None:
            setattr(p, k, int(v) if k in ("axis", "align", "on_miss") else float(v))
    return p


def kld_params(bin_xyz=None, bin_rpy=None, min_likelihood_rel=None, epsilon=None, z=None, n_min=None, n_max=None):
    """rmclhip_kld_params: the bins of pose space and the KLD-sampling bound of the adaptive resampler (include/rmclhip.h).  Arguments
    left None keep the library's defaults (rmclhip_kld_params_default): bins of 0.5 m and 10 degrees (0 ignores a dimension; x, y and
    yaw alone is AMCL's form), likelihood floor 0.01 of the maximum, epsilon 0.01, z 2.3263479 (delta 0.01), n_min 500, n_max 2^32 - 1."""
    p = _capi.KldParams()
    _capi.lib().rmclhip_kld_params_default(C.byref(p))
    for k, v in (("bin_xyz", bin_xyz), ("bin_rpy", bin_rpy)):
        if v is not None:
            setattr(p, k, (C.c_float * 3)(*[float(x) for x in v]))
    for k, v in (("min_likelihood_rel", min_likelihood_rel), ("epsilon", epsilon), ("z", z)):
        if v is not None:
            setattr(p, k, float(v))
    for k, v in (("n_min", n_min), ("n_max", n_max)):
        if v is not None:
            setattr(p, k, int(v))
    return p


def gladiator_config(min_noise_tx=0.03, min_noise_ty=0.03, min_noise_tz=0.0, min_noise_roll=0.0, min_noise_pitch=0.0,
                     min_noise_yaw=0.01, likelihood_forget_per_meter=0.3, likelihood_forget_per_radian=0.2,
                     trans_dist_metric=0):
    """resampling.* parameters with the defaults of GladiatorResamplerGPU::updateParams (GladiatorResamplerGPU.cpp:34-44);
    trans_dist_metric 0 = |t| like the reference's GPU kernel, 1 = |t|^2 like its CPU implementation."""
    return _capi.GladiatorConfig(min_noise_tx, min_noise_ty, min_noise_tz, min_noise_roll, min_noise_pitch,
                                 min_noise_yaw, likelihood_forget_per_meter, likelihood_forget_per_radian,
                                 trans_dist_metric)
