"""Particle-filter sensor update, mirror of rmcl::SensorUpdater<MemT> over the C ABI.

Reference: SensorUpdaterBase{init,reset} + ParticleUpdater<MemT>::update(poses, attrs, cfg)
(rmcl_ros/include/rmcl_ros/rmcl/SensorUpdater.hpp:18-42, ParticleUpdater.hpp:24-44), implemented by
PCDSensorUpdaterEmbree / PCDSensorUpdaterOptix (rmcl_ros/src/rmcl/PCDSensorUpdater*.cpp).
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from .registration import _as_ptr
from .types import RANGE_MEASUREMENT, TRANSFORM, _ptr, gladiator_config, kld_params, pf_params


def beams_from_points(points):
    """PCDSensorUpdaterEmbree.cpp:313-327: meas_s = {orig 0, dir = p/|p|, range = |p|, cov = 0.1 I}."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(p), dtype=RANGE_MEASUREMENT)
    # rmagine Vector3::l2norm / normalize in float32
    nrm = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(np.float32)
    out["dir"]["x"], out["dir"]["y"], out["dir"]["z"] = p[:, 0] / nrm, p[:, 1] / nrm, p[:, 2] / nrm
    out["range"] = nrm
    out["cov"][:, 0] = out["cov"][:, 4] = out["cov"][:, 8] = np.float32(0.1)
    return out


def sample_beams_pointcloud2(data, width, height, point_step, row_step, offset_x, offset_y, offset_z, samples, seed,
                             datatype=7):
    """PCDSensorUpdaterEmbree.cpp:276-327 on the raw sensor_msgs/PointCloud2 bytes, through the C ABI
    (rmclhip_pf_sample_beams_pointcloud2, a host function): `samples` uniformly random points -- std::mt19937(seed),
    index = draw % (width * height), up to 100 retries for a point without NaN -- as RangeMeasurements."""
    buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8)) if isinstance(data, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    L = _capi.PointCloud2Layout(int(width), int(height), int(point_step), int(row_step), int(offset_x), int(offset_y),
                                int(offset_z), int(datatype))
    out = np.zeros(int(samples), dtype=RANGE_MEASUREMENT)
    n = C.c_uint32(0)
    _capi.check(_capi.lib().rmclhip_pf_sample_beams_pointcloud2(_ptr(buf), buf.size, C.byref(L), int(samples), int(seed),
                                                               _ptr(out), C.byref(n)))
    return out[: n.value].copy()


def sample_beams(cloud_xyz, samples, seed):
    """the same sampling on an [n, 3] float32 array (an unorganised cloud: width n, height 1, point_step 12)"""
    pts = np.ascontiguousarray(cloud_xyz, dtype=np.float32).reshape(-1, 3)
    return sample_beams_pointcloud2(pts.view(np.uint8).reshape(-1), len(pts), 1, 12, 12 * len(pts), 0, 4, 8, samples, seed)


def combined_forget_rate(forget_rate_per_meter, forget_rate_per_second, dist_travelled, dt):
    """TFMotionUpdaterCPU.cpp:172-174: per-meter and per-second rates turned absolute (exponential) and multiplied."""
    space = 1.0 - math.pow(1.0 - forget_rate_per_meter, dist_travelled)
    tim = 1.0 - math.pow(1.0 - forget_rate_per_second, dt)
    return space * tim


def _count_of(poses, first, count):
    if count is not None:
        return int(count)
    n = poses.count if hasattr(poses, "count") else poses.shape[0]
    return int(n)


def init_particles_uniform(ctx, poses, attrs, bb_min, bb_max, seed, epoch=0, first=0, count=None):
    """RmclNode::initSamplesUniform (rmcl_localization.cpp:277-342) on the device (rmclhip_particles_init_uniform): poses / attrs are
    device views of `count` particles (default: all of `poses`) that receive the GLOBAL particles first .. first+count-1 of the cloud
    (seed, epoch) selects -- uniform in [bb_min, bb_max] over x y z roll pitch yaw, likelihood {1, 0, 0}.  The reference's defaults:
    [-50, -50, 0, 0, 0, -pi] .. [50, 50, 0, 0, 0, pi], 50 000 particles."""
    lo = np.ascontiguousarray(bb_min, dtype=np.float32).reshape(6)
    hi = np.ascontiguousarray(bb_max, dtype=np.float32).reshape(6)
    _capi.check(_capi.lib().rmclhip_particles_init_uniform(ctx.handle, _as_ptr(poses), _as_ptr(attrs), int(first),
                                                           _count_of(poses, first, count), _ptr(lo), _ptr(hi), int(seed), int(epoch)))


def init_particles_pose(ctx, poses, attrs, pose, covariance, seed, epoch=0, first=0, count=None):
    """RmclNode::initSamples(PoseWithCovarianceStamped) (rmcl_localization.cpp:165-275) on the device (rmclhip_particles_init_pose):
    particles pose * {EulerAngles(x3, x4, x5), (x0, x1, x2)} with x = L z, L L^T = covariance (6x6 over x y z roll pitch yaw, positive
    semidefinite).  Returns the "Cholesky Err" of the factor (chol6)."""
    T = np.ascontiguousarray(pose, dtype=TRANSFORM).reshape(1)
    cov = np.ascontiguousarray(covariance, dtype=np.float64).reshape(36)
    err = C.c_double(0.0)
    _capi.check(_capi.lib().rmclhip_particles_init_pose(ctx.handle, _as_ptr(poses), _as_ptr(attrs), int(first),
                                                        _count_of(poses, first, count), _ptr(T), _ptr(cov), int(seed), int(epoch),
                                                        C.byref(err)))
    return err.value


def surface_sample_params(**kwargs):
    """rmclhip_surface_sample_params with the library's defaults (min_up_cos 0.7, height 0, align 0, region unbounded, yaw in
    [-pi, pi]); keyword arguments replace fields (region_min / region_max: three floats)"""
    p = _capi.SurfaceSampleParams()
    _capi.lib().rmclhip_surface_sample_params_default(C.byref(p))
    for k, v in kwargs.items():
        if k in ("region_min", "region_max"):
            setattr(p, k, (C.c_float * 3)(*[float(x) for x in v]))
        elif k == "align":
            p.align = int(v)
        elif hasattr(p, k):
            setattr(p, k, float(v))
        else:
            raise TypeError("surface_sample_params: unknown field %r" % k)
    return p


class SurfaceSamplerHip:
    """Poses drawn uniformly by area on the drivable faces of a map (rmclhip_surface_sampler): the global initialisation of a ground
    robot and the fresh draws of the recovery injection.  Built once per (map, parameters); keeps the map alive."""

    def __init__(self, hip_map, params=None, **kwargs):
        self.map = hip_map
        self.params = surface_sample_params(**kwargs) if params is None else params
        self._h = C.c_void_p()
        _capi.check(_capi.lib().rmclhip_surface_sampler_create(hip_map.handle, C.byref(self.params), C.byref(self._h)))

    def info(self):
        """{n_faces, n_eligible, n_weighted, area_eligible, weight_total}"""
        out = _capi.SurfaceSampleInfo()
        _capi.check(_capi.lib().rmclhip_surface_sampler_get_info(self._h, C.byref(out)))
        return out.as_dict()

    def init(self, poses, attrs, seed, epoch=0, first=0, count=None):
        """rmclhip_particles_init_surface: poses / attrs (device views of `count` particles, default all of `poses`) receive the GLOBAL
        particles first .. first+count-1 of the cloud (seed, epoch) selects, likelihood {1, 0, 0}"""
        _capi.check(_capi.lib().rmclhip_particles_init_surface(self._h, _as_ptr(poses), _as_ptr(attrs), int(first),
                                                               _count_of(poses, first, count), int(seed), int(epoch)))

    def inject(self, poses, attrs, p, seed, step, first=0, count=None):
        """rmclhip_particles_inject_surface: every slot of the cloud is replaced with probability p by a fresh draw, in place;
        returns how many were"""
        n = C.c_uint32(0)
        _capi.check(_capi.lib().rmclhip_particles_inject_surface(self._h, _as_ptr(poses), _as_ptr(attrs), int(first),
                                                                 _count_of(poses, first, count), float(p), int(seed), int(step),
                                                                 C.byref(n)))
        return int(n.value)

    def close(self):
        if self._h:
            _capi.lib().rmclhip_surface_sampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def init_particles_surface(sampler, poses, attrs, seed, epoch=0, first=0, count=None):
    """the third initialisation, beside init_particles_uniform and init_particles_pose: every particle on a drivable face of the map,
    uniform by area (SurfaceSamplerHip.init)"""
    sampler.init(poses, attrs, seed, epoch=epoch, first=first, count=count)


class RecoveryHip:
    """The augmented-MCL recovery rule as AMCL runs it (rmclhip_recovery_update_host, a host function): a slow and a fast running
    average of the cloud's mean likelihood; update() returns the fraction of the cloud to replace by fresh draws, reset() is called
    after an injection.  The defaults are AMCL's recovery_alpha_slow / recovery_alpha_fast."""

    def __init__(self, alpha_slow=0.001, alpha_fast=0.1, p_max=1.0):
        self.params = _capi.RecoveryParams(float(alpha_slow), float(alpha_fast), float(p_max))
        self.state = _capi.RecoveryState(0.0, 0.0)

    def update(self, stats, n):
        """stats: {"sum": ...} of the cloud's likelihoods (compute_stats), or the sum itself; n: the particles it covers"""
        total = stats["sum"] if isinstance(stats, dict) else stats
        p = C.c_double(0.0)
        _capi.check(_capi.lib().rmclhip_recovery_update_host(C.byref(self.state), C.byref(self.params), float(total), int(n), C.byref(p)))
        return p.value

    def reset(self):
        _capi.check(_capi.lib().rmclhip_recovery_reset_host(C.byref(self.state)))


VISUALIZATION_CHANNELS = ("x", "y", "z", "likelihood", "likelihood_sigma", "likelihood_n_meas", "badness")


def pack_visualization(ctx, poses, attrs, n, max_n_meas=10000, out_dev=None):
    """RmclNode::visualize's per-particle loop (rmcl_localization.cpp:856-874) on the device (rmclhip_particles_pack_visualization):
    a dict of seven float32 arrays of n -- the point cloud's x y z and its four channels.  out_dev: a device buffer of 7 * n floats
    that receives them instead (the dict then holds nothing: returns None)."""
    if out_dev is not None:
        _capi.check(_capi.lib().rmclhip_particles_pack_visualization(ctx.handle, _as_ptr(poses), _as_ptr(attrs), int(n), int(max_n_meas),
                                                                     _as_ptr(out_dev), 1))
        return None
    out = np.zeros((7, int(n)), dtype=np.float32)
    _capi.check(_capi.lib().rmclhip_particles_pack_visualization(ctx.handle, _as_ptr(poses), _as_ptr(attrs), int(n), int(max_n_meas),
                                                                 _ptr(out), 0))
    return {k: out[i] for i, k in enumerate(VISUALIZATION_CHANNELS)}


def chol6(covariance):
    """rmclhip_chol6_host (no device needed): (L, err) -- the float32 lower-triangular factor of a positive semidefinite 6x6
    covariance, as the pose initialisation uses it, and sum |L L^T - C| / 36."""
    cov = np.ascontiguousarray(covariance, dtype=np.float64).reshape(36)
    L = np.zeros(36, dtype=np.float32)
    err = C.c_double(0.0)
    _capi.check(_capi.lib().rmclhip_chol6_host(_ptr(cov), _ptr(L), C.byref(err)))
    return L.reshape(6, 6), err.value


def constrain_to_surface(updater_or_map, poses, attrs, n, params):
    """the standalone surface pass (rmclhip_pf_constrain_to_surface), e.g. after init_particles_uniform or a resampler's noise: every
    one of the n particles is put `params.height` above the mesh below it (and, with align, its body z on the face normal), in place.
    updater_or_map: a TFMotionUpdaterHip / PCDSensorUpdaterHip (its handle, and its max_n_meas for on_miss, are used) or a HipMap (a
    handle is made for the call).  Returns the counts {n_particles, n_snapped, n_missed, n_steep}."""
    st = _capi.SurfaceStats()
    own = None
    if hasattr(updater_or_map, "_h") and hasattr(updater_or_map, "init"):
        updater_or_map.init()
        h = updater_or_map._h
    else:
        own = C.c_void_p()
        _capi.check(_capi.lib().rmclhip_pf_create(updater_or_map.ctx.handle, updater_or_map.handle, C.byref(own)))
        h = own
    try:
        _capi.check(_capi.lib().rmclhip_pf_constrain_to_surface(h, _as_ptr(poses), _as_ptr(attrs), int(n),
                                                                None if params is None else C.byref(params), C.byref(st)))
    finally:
        if own is not None:
            _capi.lib().rmclhip_pf_destroy(own)
    return st.as_dict()


_NOISE_FIELDS = ("alpha_trans_trans", "alpha_trans_rot", "alpha_rot_trans", "alpha_rot_rot")


def motion_noise_params(**kwargs):
    """rmclhip_motion_noise_params with the library's defaults (0.2 throughout, AMCL's alpha1..4); keyword arguments replace fields:
    alpha_trans_trans (m per m) and alpha_trans_rot (m per rad) for body x y z, alpha_rot_trans (rad per m) and alpha_rot_rot (rad per
    rad) for roll pitch yaw -- three floats each, or one float for all three"""
    p = _capi.MotionNoiseParams()
    _capi.lib().rmclhip_motion_noise_params_default(C.byref(p))
    for k, v in kwargs.items():
        if k not in _NOISE_FIELDS:
            raise TypeError("motion_noise_params: unknown field %r" % k)
        v3 = [float(v)] * 3 if np.ndim(v) == 0 else [float(x) for x in v]
        if len(v3) != 3:
            raise TypeError("motion_noise_params: %s takes one float or three" % k)
        setattr(p, k, (C.c_float * 3)(*v3))
    return p


def motion_noise_sigma(params, T_bnew_bold):
    """rmclhip_motion_noise_sigma_host (no device needed): the six standard deviations (body x y z in metres, roll pitch yaw in radians)
    of the sampled odometry model for the step T_bnew_bold; an identity step gives zeros"""
    T = np.ascontiguousarray(T_bnew_bold, dtype=TRANSFORM).reshape(1)
    out = np.zeros(6, dtype=np.float32)
    _capi.check(_capi.lib().rmclhip_motion_noise_sigma_host(None if params is None else C.byref(params), _ptr(T), _ptr(out)))
    return out


def _noise_sigma(noise, T_bnew_bold):
    """noise of an update call -> six float32 sigmas: a MotionNoiseParams (sigma of this step) or six sigmas as they are"""
    if isinstance(noise, _capi.MotionNoiseParams):
        return motion_noise_sigma(noise, T_bnew_bold)
    return np.ascontiguousarray(noise, dtype=np.float32).reshape(6)


class TFMotionUpdaterHip:
    """rmcl::TFMotionUpdaterGPU on gfx950 + the wall-collision test of TFMotionUpdaterCPU (MotionUpdater<MemT>).
    surface: None, or types.surface_params(...) -- update() then keeps the particles on the mesh in the same launch."""

    def __init__(self, hip_map, check_collision=True):
        if hip_map is None:
            raise RuntimeError("NO MAP")
        self.map, self.ctx, self.check_collision = hip_map, hip_map.ctx, check_collision
        self.surface = None
        self.config = pf_params()   # (max_n_meas of a killed particle)
        self._h = C.c_void_p()

    def init(self):
        if not self._h:
            _capi.check(_capi.lib().rmclhip_pf_create(self.ctx.handle, self.map.handle, C.byref(self._h)))

    def reset(self):
        """TFMotionUpdaterCPU::reset forgets the previous odometry pose (host-side state of the caller)."""

    def update(self, particle_poses, particle_attrs, n_particles, T_bnew_bold, forget_rate, noise=None, seed=0, step=0, first=0):
        """noise: None (the deterministic update), motion_noise_params(...) (sigma follows this step) or six sigmas -- every particle's
        step is then composed with its own Gaussian draw of (seed, step, first + i) (rmclhip_pf_motion_update_noisy)"""
        self.init()
        T = np.ascontiguousarray(T_bnew_bold, dtype=TRANSFORM).reshape(1)
        _capi.check(_capi.lib().rmclhip_pf_set_params(self._h, C.byref(self.config)))
        _capi.check(_capi.lib().rmclhip_pf_set_surface(self._h, None if self.surface is None else C.byref(self.surface)))
        if noise is not None:
            sigma = _noise_sigma(noise, T)
            _capi.check(_capi.lib().rmclhip_pf_motion_update_noisy(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs),
                                                                   int(n_particles), _ptr(T), float(forget_rate),
                                                                   int(bool(self.check_collision)), _ptr(sigma), int(seed), int(step),
                                                                   int(first)))
            return {}
        _capi.check(_capi.lib().rmclhip_pf_motion_update(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs),
                                                         int(n_particles), _ptr(T), float(forget_rate),
                                                         int(bool(self.check_collision))))
        return {}

    def surface_stats(self):
        """{n_particles, n_snapped, n_missed, n_steep} of the last constrained call on this updater (zeros before the first)"""
        self.init()
        st = _capi.SurfaceStats()
        _capi.check(_capi.lib().rmclhip_pf_get_surface_stats(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            _capi.lib().rmclhip_pf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PCDSensorUpdaterHip:
    """rmcl::PCDSensorUpdaterOptix on gfx950: update() mutates attrs in place on the device."""

    def __init__(self, hip_map):
        if hip_map is None:
            raise RuntimeError("NO MAP")  # PCDSensorUpdaterOptix.cpp:179-182
        self.map = hip_map
        self.ctx = hip_map.ctx
        self.config = pf_params()
        self._h = C.c_void_p()
        self._beams = None
        self._Tsb = None

    def init(self):
        """SensorUpdaterBase::init (PCDSensorUpdaterEmbree.cpp:107-114)."""
        if not self._h:
            _capi.check(_capi.lib().rmclhip_pf_create(self.ctx.handle, self.map.handle, C.byref(self._h)))
        self._push_params()

    def reset(self):
        """SensorUpdaterBase::reset (PCDSensorUpdaterEmbree.cpp:116-119): nothing to reset."""

    def setInput(self, beams, Tsb):
        """Input<>::setInput analogue: the sampled measurements (sensor frame) and the sensor->base TF."""
        self._beams = np.ascontiguousarray(beams, dtype=RANGE_MEASUREMENT).reshape(-1)
        self._Tsb = np.ascontiguousarray(Tsb, dtype=TRANSFORM).reshape(1)

    def update(self, particle_poses, particle_attrs, n_particles=None, sync=True):
        """ParticleUpdater::update(poses, attrs): device views of n Transform / ParticleAttributes."""
        if not self._h:
            self.init()
        if self._beams is None:
            raise RuntimeError("setInput() first")
        if n_particles is None:
            n_particles = particle_poses.count if hasattr(particle_poses, "count") else particle_poses.shape[0]
        self._push_params()
        fn = _capi.lib().rmclhip_pf_update if sync else _capi.lib().rmclhip_pf_update_async
        _capi.check(fn(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles),
                       _ptr(self._beams), len(self._beams), _ptr(self._Tsb)))
        return {}

    def sync(self):
        _capi.check(_capi.lib().rmclhip_pf_sync(self._h))

    def set_error_output(self, errors_dev):
        if not self._h:
            self.init()
        _capi.check(_capi.lib().rmclhip_pf_set_error_output(self._h, _as_ptr(errors_dev)))

    def set_field(self, field):
        """answer correspondence_type 1 from a DistanceFieldHip (dense or DistanceFieldHip.banded) of this updater's map
        (rmclhip_pf_set_field); None: off.  The handle keeps the field alive: the field object may be closed afterwards."""
        if not self._h:
            self.init()
        _capi.check(_capi.lib().rmclhip_pf_set_field(self._h, None if field is None else field.handle))

    def refine(self, particle_poses, n_particles=None, params=None, results_dev=None, **kwargs):
        """rmclhip_pf_refine: damped Gauss-Newton of every pose (device memory, in place) on the field set with set_field, with the
        beams and Tsb of setInput.  Attributes are not touched: follow with update().  Returns the counts as a dict."""
        from .field import _refine_call
        if not self._h:
            self.init()
        if self._beams is None:
            raise RuntimeError("setInput() first")
        return _refine_call(_capi.lib().rmclhip_pf_refine, self._h, particle_poses, n_particles, self._beams, self._Tsb, params, results_dev, kwargs)

    def stein_step(self, particle_poses, n_particles=None, params=None, results_dev=None, **kwargs):
        """rmclhip_pf_stein_step: Stein variational steps of the cloud (device memory, in place) on the field set with set_field, with
        the beams and Tsb of setInput -- every particle moves by the kernel-weighted average of its neighbours' Gauss-Newton steps and
        away from its neighbours.  Attributes are not touched: follow with update().  params: a stein_params(), or its keywords
        directly; results_dev: device memory for one STEIN_RESULT row per particle (optional).  Returns the counts as a dict."""
        from .field import stein_params
        if not self._h:
            self.init()
        if self._beams is None:
            raise RuntimeError("setInput() first")
        if params is None:
            params = stein_params(**kwargs)
        elif kwargs:
            raise TypeError("stein_step: give params or keywords, not both")
        if n_particles is None:
            n_particles = particle_poses.count if hasattr(particle_poses, "count") else particle_poses.shape[0]
        st = _capi.SteinStats()
        _capi.check(_capi.lib().rmclhip_pf_stein_step(self._h, _as_ptr(particle_poses), int(n_particles), _ptr(self._beams), len(self._beams),
                                                      _ptr(self._Tsb), C.byref(params), _as_ptr(results_dev), C.byref(st)))
        return st.as_dict()

    def extract_weights(self, particle_attrs, n_particles, weights_dev):
        _capi.check(_capi.lib().rmclhip_pf_extract_weights(self._h, _as_ptr(particle_attrs), int(n_particles),
                                                           _as_ptr(weights_dev)))

    def time_update(self, particle_poses, particle_attrs, n_particles, iters=5):
        if not self._h:
            self.init()
        self._push_params()
        ms = C.c_float(0)
        _capi.check(_capi.lib().rmclhip_pf_time_update(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs),
                                                       int(n_particles), _ptr(self._beams), len(self._beams),
                                                       _ptr(self._Tsb), int(iters), C.byref(ms)))
        return ms.value

    def time_update_unfused(self, particle_poses, particle_attrs, n_particles, sync_each_beam=True, iters=2):
        """the reference's GPU schedule as a comparator (PCDSensorUpdaterOptix.cpp:319-338): one single-beam update per beam, synchronised
        after each (or only at the end); host-clock ms per sequence of all beams (rmclhip_pf_time_update_unfused)"""
        if not self._h:
            self.init()
        self._push_params()
        ms = C.c_float(0)
        _capi.check(_capi.lib().rmclhip_pf_time_update_unfused(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles),
                                                               _ptr(self._beams), len(self._beams), _ptr(self._Tsb),
                                                               1 if sync_each_beam else 0, int(iters), C.byref(ms)))
        return ms.value

    def set_variant(self, v):
        if not self._h:
            self.init()
        _capi.check(_capi.lib().rmclhip_pf_set_variant(self._h, int(v)))

    def set_schedule(self, refill_idle_lanes=0, tail_lanes=8):
        if not self._h:
            self.init()
        _capi.check(_capi.lib().rmclhip_pf_set_schedule(self._h, int(refill_idle_lanes), int(tail_lanes)))

    def set_mapping(self, mapping, particles_per_block=0, order=None):
        """ray dealing of the update (rmclhip_pf_set_mapping): 0 beam-minor (default), 1 particle-minor (converged clouds); order: a
        DeviceArray of uint32 slot -> particle indices (kept alive by this object) or None"""
        if not self._h:
            self.init()
        self._order = order
        _capi.check(_capi.lib().rmclhip_pf_set_mapping(self._h, int(mapping), int(particles_per_block),
                                                       order.ptr if order is not None else None, order.count if order is not None else 0))

    def _push_params(self):
        _capi.check(_capi.lib().rmclhip_pf_set_params(self._h, C.byref(self.config)))

    def close(self):
        if self._h:
            _capi.lib().rmclhip_pf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GladiatorResamplerHip:
    """rmcl::GladiatorResamplerGPU on gfx950 (Resampler<MemT>: init / reset / update(poses, attrs, poses_new,
    attrs_new) -> {n_particles}; GladiatorResamplerGPU.cpp:46-81).  The tournament is out of place (the node's
    particle double buffer, rmcl_localization.cpp:600-640); `seed` and the running step counter select the
    Philox stream, so a run is reproducible."""

    def __init__(self, ctx, seed=1234):
        self.ctx = ctx
        self.config = gladiator_config()
        self.seed = int(seed)
        self.step = 0
        self._h = C.c_void_p()

    def init(self):
        if not self._h:
            _capi.check(_capi.lib().rmclhip_resampler_create(self.ctx.handle, C.byref(self._h)))

    def reset(self):
        self.step = 0

    def compute_stats(self, particle_attrs, n_particles):
        """compute_stats (resampling.cu:83-92): {sum, max} of the particle likelihoods."""
        self.init()
        out = _capi.LikelihoodStats()
        _capi.check(_capi.lib().rmclhip_resampler_compute_stats(self._h, _as_ptr(particle_attrs), int(n_particles),
                                                                C.byref(out)))
        return {"sum": out.sum, "max": out.max}

    def compute_stats_weights(self, weights, n):
        """{sum, max} of a dense float32 weight vector on the device (the all-gathered likelihood.mean of a sharded cloud): the bits
        compute_stats gives for attributes holding the same values (rmclhip_resampler_compute_stats_weights)"""
        self.init()
        out = _capi.LikelihoodStats()
        _capi.check(_capi.lib().rmclhip_resampler_compute_stats_weights(self._h, _as_ptr(weights), int(n), C.byref(out)))
        return {"sum": out.sum, "max": out.max}

    def update(self, particle_poses, particle_attrs, particle_poses_new, particle_attrs_new, n_particles,
               first=0, count=None):
        """champions first..first+count-1 (default: all) vs random enemies out of all n_particles; results in
        particle_*_new[0..count)."""
        self.init()
        if count is None:
            count = int(n_particles) - int(first)
        _capi.check(_capi.lib().rmclhip_resampler_gladiator(
            self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles), _as_ptr(particle_poses_new),
            _as_ptr(particle_attrs_new), int(first), int(count), C.byref(self.config), self.seed, self.step))
        self.step += 1
        return {"n_particles": int(count)}

    def close(self):
        if self._h:
            _capi.lib().rmclhip_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidualResamplerHip(GladiatorResamplerHip):
    """rmcl::ResidualResamplerCPU on gfx950 (ResidualResamplerCPU.cpp:55-203), the PF node's second resampler plugin: random
    particles are inserted floor(L / sum(L) * N_new) times each, perturbed, until the new cloud is full.  Same interface and
    parameters as the gladiator (`config.trans_dist_metric` is ignored: this resampler measures |dt|^2); `last_draws` = the
    iterations the reference's sequential loop would have run."""

    def __init__(self, ctx, seed=1234):
        super().__init__(ctx, seed)
        self.last_draws = 0

    def update(self, particle_poses, particle_attrs, particle_poses_new, particle_attrs_new, n_particles, n_particles_new=None,
               first=0, count=None):
        """slots first..first+count-1 (default: all) of a new cloud of n_particles_new (default n_particles) particles; results in
        particle_*_new[0..count)."""
        self.init()
        n_new = int(n_particles if n_particles_new is None else n_particles_new)
        if count is None:
            count = n_new - int(first)
        nd = C.c_uint64(0)
        _capi.check(_capi.lib().rmclhip_resampler_residual(
            self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles), _as_ptr(particle_poses_new),
            _as_ptr(particle_attrs_new), n_new, int(first), int(count), C.byref(self.config), self.seed, self.step, C.byref(nd)))
        self.step += 1
        self.last_draws = int(nd.value)
        return {"n_particles": int(count)}


def kld_bound(k, epsilon=0.01, z=2.3263479, n_min=500, n_max=0xFFFFFFFF):
    """rmclhip_kld_bound_host (no device needed): the KLD-sampling bound (Fox 2003) on the particle count for k occupied bins,
    clamped to [n_min, n_max]"""
    n = C.c_uint32(0)
    _capi.check(_capi.lib().rmclhip_kld_bound_host(int(k), float(epsilon), float(z), int(n_min), int(n_max), C.byref(n)))
    return int(n.value)


class AdaptiveResamplerHip(GladiatorResamplerHip):
    """A resampler that chooses the particle count: the KLD-sampling bound on the occupied bins of pose space, then systematic
    (low-variance) resampling to that size -- the reference's open item "reduce the number of particles more intelligently"
    (docs/RMCL.md); its node adopts the returned count (rmcl_localization.cpp:633-639).  `config`: the gladiator's noise (every copy
    of a particle after the first is perturbed as the gladiator perturbs a winner); `kld`: types.kld_params()."""

    def __init__(self, ctx, seed=1234):
        super().__init__(ctx, seed)
        self.kld = kld_params()

    def count_bins(self, particle_poses, particle_attrs, n_particles):
        """{"bins": occupied bins of pose space, "counted": particles above the likelihood floor} (rmclhip_particles_count_bins)"""
        self.init()
        k, c = C.c_uint32(0), C.c_uint32(0)
        _capi.check(_capi.lib().rmclhip_particles_count_bins(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles),
                                                             C.byref(self.kld), C.byref(k), C.byref(c)))
        return {"bins": int(k.value), "counted": int(c.value)}

    def kld_bound(self, k, capacity=None):
        """the bound for k bins with this resampler's parameters; capacity limits n_max (and n_min) as update() does"""
        n_max = int(self.kld.n_max) if capacity is None else min(int(self.kld.n_max), int(capacity))
        return kld_bound(k, self.kld.epsilon, self.kld.z, min(int(self.kld.n_min), n_max), n_max)

    def update_systematic(self, particle_poses, particle_attrs, particle_poses_new, particle_attrs_new, n_particles, n_particles_new=None,
                          first=0, count=None):
        """slots first..first+count-1 (default: all) of a new cloud of n_particles_new (default n_particles) particles by systematic
        resampling (rmclhip_resampler_systematic); results in particle_*_new[0..count)."""
        self.init()
        n_new = int(n_particles if n_particles_new is None else n_particles_new)
        if count is None:
            count = n_new - int(first)
        _capi.check(_capi.lib().rmclhip_resampler_systematic(
            self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles), _as_ptr(particle_poses_new),
            _as_ptr(particle_attrs_new), n_new, int(first), int(count), C.byref(self.config), self.seed, self.step))
        self.step += 1
        return {"n_particles": int(count)}

    def update(self, particle_poses, particle_attrs, particle_poses_new, particle_attrs_new, n_particles, capacity_new=None,
               recovery=None, sampler=None):
        """Resampler::update with a count of its own: particle_*_new (room for capacity_new particles, default n_particles) receive
        n_new particles; returns {"n_particles": n_new, "bins": k} (rmclhip_resampler_adaptive).
        recovery= (a RecoveryHip) with sampler= (a SurfaceSamplerHip): the likelihood statistics of the old cloud feed the recovery
        averages, and after the resampler the fraction they ask for is replaced in the new cloud by fresh draws from the sampler
        (same seed and step); the averages are reset when anything was injected.  The dict then also holds "injected" and
        "p_inject"."""
        if (recovery is None) != (sampler is None):
            raise ValueError("AdaptiveResamplerHip.update: recovery= and sampler= come as a pair")
        self.init()
        if recovery is not None:
            p_inject = recovery.update(self.compute_stats(particle_attrs, n_particles), n_particles)
            step = self.step
            out = self.update(particle_poses, particle_attrs, particle_poses_new, particle_attrs_new, n_particles, capacity_new)
            out["injected"] = sampler.inject(particle_poses_new, particle_attrs_new, p_inject, self.seed, step, count=out["n_particles"])
            out["p_inject"] = p_inject
            if out["injected"]:
                recovery.reset()
            return out
        cap = int(n_particles if capacity_new is None else capacity_new)
        n_new, k = C.c_uint32(0), C.c_uint32(0)
        _capi.check(_capi.lib().rmclhip_resampler_adaptive(
            self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles), _as_ptr(particle_poses_new),
            _as_ptr(particle_attrs_new), cap, C.byref(self.kld), C.byref(self.config), self.seed, self.step, C.byref(n_new), C.byref(k)))
        self.step += 1
        return {"n_particles": int(n_new.value), "bins": int(k.value)}


def _estimate_dict(e):
    """rmclhip_pose_estimate -> the dict RmclNode::estimateStats' message maps to"""
    pose = np.frombuffer(bytes(bytearray(memoryview(e.pose))), dtype=TRANSFORM)[0].copy()
    return {"pose": pose, "covariance": np.array(e.covariance, dtype=np.float64).reshape(6, 6),
            "likelihood": {"mean": e.likelihood_mean, "sigma": e.likelihood_sigma, "min": e.likelihood_min, "max": e.likelihood_max},
            "trans_bb_min": np.array(e.trans_bb_min), "trans_bb_max": np.array(e.trans_bb_max), "nparticles": e.n_particles}


def _hypotheses_dict(out, n_out, n_clusters):
    hyps = []
    for k in range(int(n_out)):
        d = _estimate_dict(out[k].estimate)
        d.update(key_min=int(out[k].key_min), weight=int(out[k].weight), weight_share=float(out[k].weight_share), n_bins=int(out[k].n_bins))
        hyps.append(d)
    return {"n_clusters": int(n_clusters), "hypotheses": hyps}


class PoseEstimatorHip:
    """RmclNode::estimateStats for a cloud on one device, and the answer to a posterior with several modes: pose hypotheses -- the
    connected components of the cloud's occupied bins (the bins of AdaptiveResamplerHip.count_bins), weighed, ranked, each with a mean
    and covariance of its own.  Owns a rmclhip_resampler (stream + scratch); `kld`: types.kld_params(), of which bin_xyz, bin_rpy and
    min_likelihood_rel are read."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.kld = kld_params()
        self._h = C.c_void_p()

    def init(self):
        if not self._h:
            _capi.check(_capi.lib().rmclhip_resampler_create(self.ctx.handle, C.byref(self._h)))

    def estimate(self, particle_poses, particle_attrs, n_particles, max_induction_particles=0xFFFFFFFF):
        """the one mean and covariance over the first min(n_particles, max_induction_particles) particles
        (rmclhip_particles_pose_estimate): ShardedParticleFilterHip.pose_estimate on one rank, bit for bit"""
        self.init()
        e = _capi.PoseEstimate()
        _capi.check(_capi.lib().rmclhip_particles_pose_estimate(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles),
                                                                int(min(max_induction_particles, 0xFFFFFFFF)), C.byref(e)))
        return _estimate_dict(e)

    def hypotheses(self, particle_poses, particle_attrs, n_particles, max_hypotheses=8, labels=None):
        """{"n_clusters", "hypotheses": [estimate dict + key_min, weight, weight_share, n_bins, ...]}, heaviest first
        (rmclhip_particles_pose_hypotheses); labels: optional device uint32[n_particles], the rank of every particle's cluster"""
        self.init()
        out = (_capi.PoseHypothesis * max(1, min(int(max_hypotheses), 64)))()
        n_out, n_clusters = C.c_uint32(0), C.c_uint32(0)
        _capi.check(_capi.lib().rmclhip_particles_pose_hypotheses(self._h, _as_ptr(particle_poses), _as_ptr(particle_attrs), int(n_particles),
                                                                  C.byref(self.kld), int(max_hypotheses), out, C.byref(n_out),
                                                                  C.byref(n_clusters), _as_ptr(labels)))
        return _hypotheses_dict(out, n_out.value, n_clusters.value)

    def close(self):
        if self._h:
            _capi.lib().rmclhip_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedParticleFilterHip:
    """A particle cloud block-partitioned over the devices of ONE process (rmclhip_comm / rmclhip_pf_sharded: RCCL
    ncclCommInitAll + all-gather / all-reduce over xGMI) -- the multi-GPU form of PCDSensorUpdater + GladiatorResampler +
    RmclNode::estimateStats for the single-process node (rmcl_localization.cpp:482-552, 642-731)."""

    def __init__(self, vertices, faces, devices=(0,), loopback=False):
        """loopback=True: the in-process stand-in for RCCL (rmclhip_comm_create_loopback) -- `devices` may then repeat a device, which
        lets a one-GPU box run and check the ndev > 1 code paths; never a production configuration."""
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._comm = C.c_void_p()
        create = _capi.lib().rmclhip_comm_create_loopback if loopback else _capi.lib().rmclhip_comm_create
        _capi.check(create(devs, len(devices), C.byref(self._comm)))
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
        self._h = C.c_void_p()
        try:
            _capi.check(_capi.lib().rmclhip_pf_sharded_create(self._comm, _ptr(v), len(v), _ptr(f), len(f), C.byref(self._h)))
        except Exception:
            _capi.lib().rmclhip_comm_destroy(self._comm)
            self._comm = C.c_void_p()
            raise
        self.world = len(devices)
        self.n_total = 0
        self.config_ = pf_params()

    def set_particles(self, poses, attrs):
        p = np.ascontiguousarray(poses, dtype=TRANSFORM).reshape(-1)
        a = np.ascontiguousarray(attrs).reshape(-1)
        assert a.dtype.itemsize == 36 and len(a) == len(p)
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_particles(self._h, _ptr(p), _ptr(a), len(p)))
        self.n_total = len(p)

    def init_uniform(self, n, bb_min, bb_max, seed, epoch=0):
        """(re)create the cloud on its devices, uniform in the box (rmclhip_pf_sharded_init_uniform): every device fills its own block;
        the single-device cloud of init_particles_uniform bit for bit"""
        lo = np.ascontiguousarray(bb_min, dtype=np.float32).reshape(6)
        hi = np.ascontiguousarray(bb_max, dtype=np.float32).reshape(6)
        _capi.check(_capi.lib().rmclhip_pf_sharded_init_uniform(self._h, int(n), _ptr(lo), _ptr(hi), int(seed), int(epoch)))
        self.n_total = int(n)

    def init_pose(self, n, pose, covariance, seed, epoch=0):
        """(re)create the cloud around a pose guess with covariance (rmclhip_pf_sharded_init_pose); returns the "Cholesky Err" """
        T = np.ascontiguousarray(pose, dtype=TRANSFORM).reshape(1)
        cov = np.ascontiguousarray(covariance, dtype=np.float64).reshape(36)
        err = C.c_double(0.0)
        _capi.check(_capi.lib().rmclhip_pf_sharded_init_pose(self._h, int(n), _ptr(T), _ptr(cov), int(seed), int(epoch), C.byref(err)))
        self.n_total = int(n)
        return err.value

    def set_surface_sampler(self, params=None, **kwargs):
        """one surface sampler per map replica (rmclhip_pf_sharded_set_surface_sampler): params (surface_sample_params()), or the
        library's defaults with the keyword arguments replacing fields"""
        p = surface_sample_params(**kwargs) if params is None else params
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_surface_sampler(self._h, C.byref(p)))

    def drop_surface_sampler(self):
        """take the replicas' samplers off (the C ABI's NULL)"""
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_surface_sampler(self._h, None))

    def init_surface(self, n, seed, epoch=0):
        """(re)create the cloud on the surface: every device fills its own block (rmclhip_pf_sharded_init_surface)"""
        _capi.check(_capi.lib().rmclhip_pf_sharded_init_surface(self._h, int(n), int(seed), int(epoch)))
        self.n_total = int(n)

    def inject_surface(self, p, seed, step):
        """the recovery injection on every device's block; returns the replaced slots (rmclhip_pf_sharded_inject_surface)"""
        n = C.c_uint32(0)
        _capi.check(_capi.lib().rmclhip_pf_sharded_inject_surface(self._h, float(p), int(seed), int(step), C.byref(n)))
        return int(n.value)

    def download(self):
        from .types import PARTICLE_ATTRIBUTES
        p, a = np.zeros(self.n_total, TRANSFORM), np.zeros(self.n_total, PARTICLE_ATTRIBUTES)
        _capi.check(_capi.lib().rmclhip_pf_sharded_download(self._h, _ptr(p), _ptr(a)))
        return p, a

    def update(self, beams, Tsb):
        """sensor update on every device's block + the weight all-gather; returns the dense weights as rank 0 holds them"""
        b = np.ascontiguousarray(beams, dtype=RANGE_MEASUREMENT).reshape(-1)
        T = np.ascontiguousarray(Tsb, dtype=TRANSFORM).reshape(1)
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_params(self._h, C.byref(self.config_)))
        _capi.check(_capi.lib().rmclhip_pf_update_sharded(self._h, _ptr(b), len(b), _ptr(T)))
        return self.weights(0)

    def motion_update(self, T_bnew_bold, forget_rate, check_collision=True, noise=None, seed=0, step=0):
        """TFMotionUpdater*::update on every device's block, in place (rmclhip_pf_sharded_motion_update): pose <- pose * T_bnew_bold,
        n_meas -= forget_rate * n_meas, and with check_collision the wall-collision ray of the CPU updater.  noise (None,
        motion_noise_params(...) or six sigmas), seed, step: as TFMotionUpdaterHip.update (rmclhip_pf_sharded_motion_update_noisy)"""
        T = np.ascontiguousarray(T_bnew_bold, dtype=TRANSFORM).reshape(1)
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_params(self._h, C.byref(self.config_)))   # (max_n_meas of a collided particle)
        if noise is not None:
            sigma = _noise_sigma(noise, T)
            _capi.check(_capi.lib().rmclhip_pf_sharded_motion_update_noisy(self._h, _ptr(T), float(forget_rate), int(bool(check_collision)),
                                                                           _ptr(sigma), int(seed), int(step)))
            return
        _capi.check(_capi.lib().rmclhip_pf_sharded_motion_update(self._h, _ptr(T), float(forget_rate), int(bool(check_collision))))

    def set_motion_noise(self, params):
        """step() with a T_bnew_bold then draws the sampled odometry model's noise with its own seed and step
        (rmclhip_pf_sharded_set_motion_noise); None: off"""
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_motion_noise(self._h, None if params is None else C.byref(params)))

    def set_surface(self, params):
        """the surface constraint of motion_update and step on every device's block (rmclhip_pf_sharded_set_surface); None: off"""
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_surface(self._h, None if params is None else C.byref(params)))

    def set_field(self, cell=0.0, margin=0.0, max_nodes=1 << 26):
        """every device builds the distance field of its copy of the map and answers correspondence_type 1 from it
        (rmclhip_pf_sharded_set_field); set_field(None): off"""
        if cell is None:
            _capi.check(_capi.lib().rmclhip_pf_sharded_set_field(self._h, None))
            return
        p = _capi.FieldParams(float(cell), float(margin), int(max_nodes))
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_field(self._h, C.byref(p)))

    def set_field_banded(self, cell=0.0, margin=0.0, band=0.5, max_nodes=1 << 26):
        """set_field with a banded field on every device (rmclhip_pf_sharded_set_field_banded)"""
        p = _capi.BandFieldParams(float(cell), float(margin), int(max_nodes), float(band), 0)
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_field_banded(self._h, C.byref(p)))

    def refine(self, beams, Tsb, params=None, **kwargs):
        """every device refines its own block on its own field (rmclhip_pf_sharded_refine; set_field first), no collective; attributes
        and weights are not touched.  Returns the counts summed over the devices."""
        from .field import refine_params
        if params is None:
            params = refine_params(**kwargs)
        elif kwargs:
            raise TypeError("refine: give params or keywords, not both")
        b = np.ascontiguousarray(beams, dtype=RANGE_MEASUREMENT).reshape(-1)
        T = np.ascontiguousarray(Tsb, dtype=TRANSFORM).reshape(1)
        st = _capi.RefineStats()
        _capi.check(_capi.lib().rmclhip_pf_sharded_refine(self._h, _ptr(b), len(b), _ptr(T), C.byref(params), C.byref(st)))
        return st.as_dict()

    def constrain_to_surface(self, params):
        """the standalone surface pass on every device's own block, no collective; returns the counts summed over the devices"""
        st = _capi.SurfaceStats()
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_params(self._h, C.byref(self.config_)))   # (max_n_meas of on_miss)
        _capi.check(_capi.lib().rmclhip_pf_sharded_constrain_to_surface(self._h, None if params is None else C.byref(params), C.byref(st)))
        return st.as_dict()

    def surface_stats(self):
        """counts of the last constrained motion_update / step / constrain_to_surface, summed over the devices"""
        st = _capi.SurfaceStats()
        _capi.check(_capi.lib().rmclhip_pf_sharded_get_surface_stats(self._h, C.byref(st)))
        return st.as_dict()

    def step(self, beams, Tsb, T_bnew_bold=None, forget_rate=0.0, check_collision=True, resample=None, cfg=None, seed=42, step=0):
        """one cycle of the filter node (rmcl_localization.cpp:84, 432-552) behind ONE C call: motion (skipped when T_bnew_bold is None)
        -> sensor update -> weight all-gather -> {sum, max} -> resampling (None, "gladiator" or "residual"); returns {sum, max} of the
        likelihoods after the sensor update"""
        b = np.ascontiguousarray(beams, dtype=RANGE_MEASUREMENT).reshape(-1)
        T = np.ascontiguousarray(Tsb, dtype=TRANSFORM).reshape(1)
        Tm = None if T_bnew_bold is None else np.ascontiguousarray(T_bnew_bold, dtype=TRANSFORM).reshape(1)
        cfg = cfg if cfg is not None else gladiator_config()
        st = _capi.LikelihoodStats()
        _capi.check(_capi.lib().rmclhip_pf_sharded_set_params(self._h, C.byref(self.config_)))
        _capi.check(_capi.lib().rmclhip_pf_sharded_step(self._h, None if Tm is None else _ptr(Tm), float(forget_rate), int(bool(check_collision)),
                                                       _ptr(b), len(b), _ptr(T), {None: 0, "gladiator": 1, "residual": 2}[resample],
                                                       C.byref(cfg), int(seed), int(step), C.byref(st)))
        return {"sum": st.sum, "max": st.max}

    def weights(self, rank=0):
        w = np.zeros(self.n_total, np.float32)
        _capi.check(_capi.lib().rmclhip_pf_sharded_get_weights(self._h, int(rank), _ptr(w)))
        return w

    def stats(self):
        """{sum, max} of the likelihoods: every device reduces ITS copy of the gathered weights in the single-device kernel's order
        (no collective since round 6: rmclhip_pf_allreduce_stats)"""
        st = _capi.LikelihoodStats()
        _capi.check(_capi.lib().rmclhip_pf_allreduce_stats(self._h, C.byref(st)))
        return {"sum": st.sum, "max": st.max}

    def collective_ranks(self):
        """(ranks the collective library itself reports for this communicator -- ncclCommCount --, "rccl" | "loopback")"""
        n, is_rccl = C.c_uint32(0), C.c_int(0)
        _capi.check(_capi.lib().rmclhip_comm_collective_ranks(self._comm, C.byref(n), C.byref(is_rccl)))
        return n.value, ("rccl" if is_rccl.value else "loopback")

    def set_loopback_reduce_rotation(self, first_rank):
        """TEST knob (loopback communicators): the all-reduce adds the ranks starting at first_rank (include/rmclhip_lab.h)"""
        _capi.check(_capi.lib().rmclhip_comm_loopback_set_reduce_rotation(self._comm, int(first_rank)))

    def pose_estimate(self, max_induction_particles=0xFFFFFFFF):
        e = _capi.PoseEstimate()
        _capi.check(_capi.lib().rmclhip_pf_allreduce_pose_estimate(self._h, int(min(max_induction_particles, 0xFFFFFFFF)), C.byref(e)))
        return _estimate_dict(e)

    def pose_hypotheses(self, kld, max_hypotheses=8):
        """PoseEstimatorHip.hypotheses of the whole sharded cloud (rmclhip_pf_sharded_pose_hypotheses): the records are gathered, rank 0
        runs the single-device path; the cloud is not changed.  kld: types.kld_params()"""
        out = (_capi.PoseHypothesis * max(1, min(int(max_hypotheses), 64)))()
        n_out, n_clusters = C.c_uint32(0), C.c_uint32(0)
        _capi.check(_capi.lib().rmclhip_pf_sharded_pose_hypotheses(self._h, C.byref(kld), int(max_hypotheses), out, C.byref(n_out),
                                                                   C.byref(n_clusters)))
        return _hypotheses_dict(out, n_out.value, n_clusters.value)

    def resample(self, cfg=None, seed=42, step=0, residual=False):
        """all-gather the cloud, then every device resamples its shard: the gladiator tournament (default) or the residual resampler"""
        cfg = cfg if cfg is not None else gladiator_config()
        fn = _capi.lib().rmclhip_pf_sharded_resample_residual if residual else _capi.lib().rmclhip_pf_sharded_resample
        _capi.check(fn(self._h, C.byref(cfg), int(seed), int(step)))

    def close(self):
        if self._h:
            _capi.lib().rmclhip_pf_sharded_destroy(self._h)
            self._h = C.c_void_p()
        if self._comm:
            _capi.lib().rmclhip_comm_destroy(self._comm)
            self._comm = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
