"""ctypes binding of librmclhip.so (include/rmclhip.h).

The library is the product; this module only loads it.  It fails loudly when the
shared object is missing -- there is no Python/CPU fallback of the hot path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librmclhip.so")

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_UNSUPPORTED = range(6)


class RmclHipError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws (micp_localization.cpp:613)."""

    def __init__(self, status, msg):
        super().__init__("rmclhip status %d: %s" % (status, msg))
        self.status = status


class NoDeviceError(RmclHipError):
    pass


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Interval(C.Structure):
    _fields_ = [("min", C.c_float), ("max", C.c_float)]


class DiscreteInterval(C.Structure):
    _fields_ = [("min", C.c_float), ("inc", C.c_float), ("size", C.c_uint32)]


class SphericalModel(C.Structure):
    _fields_ = [("phi", DiscreteInterval), ("theta", DiscreteInterval), ("range", Interval)]


class PFParams(C.Structure):
    _fields_ = [("dist_sigma", C.c_float), ("real_hit_sim_miss_error", C.c_float),
                ("real_miss_sim_hit_error", C.c_float), ("real_miss_sim_miss_error", C.c_float),
                ("sensor_range", Interval), ("max_n_meas", C.c_uint32),
                ("correspondence_type", C.c_uint32)]


class MicpFastInfo(C.Structure):
    _fields_ = [("attempts", C.c_uint32), ("done", C.c_uint32), ("cap_exits", C.c_uint32), ("overflows", C.c_uint32),
                ("last_code", C.c_uint32), ("last_uncertain", C.c_uint32), ("last_rho", C.c_float), ("last_tau", C.c_float),
                ("rho_cap", C.c_float), ("tau_cap", C.c_float), ("last_setup_clocks", C.c_uint32), ("last_loop_clocks", C.c_uint32),
                ("host_loops", C.c_uint32)]


class CcsInfo(C.Structure):
    _fields_ = [("calls", C.c_uint32), ("from_moments", C.c_uint32), ("passes", C.c_uint32), ("speculative_finds", C.c_uint32)]


class FindLaunchShape(C.Structure):
    _fields_ = [("exists", C.c_uint32), ("in_product", C.c_uint32), ("tiles_per_block", C.c_uint32), ("grid_x", C.c_uint32),
                ("grid_y", C.c_uint32), ("lds_bytes", C.c_uint32), ("clock_dwords", C.c_uint32), ("has_moments", C.c_uint32)]


class PointCloud2Layout(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("offset_x", C.c_uint32), ("offset_y", C.c_uint32), ("offset_z", C.c_uint32), ("datatype", C.c_uint32)]


class Filter1D(C.Structure):
    _fields_ = [("skip_begin", C.c_uint32), ("skip_end", C.c_uint32), ("increment", C.c_uint32)]


class GladiatorConfig(C.Structure):
    _fields_ = [("min_noise_tx", C.c_float), ("min_noise_ty", C.c_float), ("min_noise_tz", C.c_float),
                ("min_noise_roll", C.c_float), ("min_noise_pitch", C.c_float), ("min_noise_yaw", C.c_float),
                ("likelihood_forget_per_meter", C.c_float), ("likelihood_forget_per_radian", C.c_float),
                ("trans_dist_metric", C.c_uint32)]


class SurfaceParams(C.Structure):
    """rmclhip_surface_params (the surface constraint of the motion update)"""
    _fields_ = [("axis", C.c_uint32), ("height", C.c_float), ("probe_up", C.c_float), ("probe_down", C.c_float),
                ("min_up_cos", C.c_float), ("align", C.c_uint32), ("on_miss", C.c_uint32)]


class MotionNoiseParams(C.Structure):
    """rmclhip_motion_noise_params (the sampled odometry model of the motion update)"""
    _fields_ = [("alpha_trans_trans", C.c_float * 3), ("alpha_trans_rot", C.c_float * 3), ("alpha_rot_trans", C.c_float * 3),
                ("alpha_rot_rot", C.c_float * 3)]


class SurfaceStats(C.Structure):
    """rmclhip_surface_stats"""
    _fields_ = [("n_particles", C.c_uint32), ("n_snapped", C.c_uint32), ("n_missed", C.c_uint32), ("n_steep", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SurfaceSampleParams(C.Structure):
    """rmclhip_surface_sample_params (the surface sampler)"""
    _fields_ = [("min_up_cos", C.c_float), ("height", C.c_float), ("align", C.c_int), ("region_min", C.c_float * 3),
                ("region_max", C.c_float * 3), ("yaw_min", C.c_float), ("yaw_max", C.c_float)]


class SurfaceSampleInfo(C.Structure):
    """rmclhip_surface_sample_info"""
    _fields_ = [("n_faces", C.c_uint32), ("n_eligible", C.c_uint32), ("n_weighted", C.c_uint32), ("reserved", C.c_uint32),
                ("area_eligible", C.c_double), ("weight_total", C.c_uint64)]

    def as_dict(self):
        return {"n_faces": int(self.n_faces), "n_eligible": int(self.n_eligible), "n_weighted": int(self.n_weighted),
                "area_eligible": float(self.area_eligible), "weight_total": int(self.weight_total)}


class RecoveryState(C.Structure):
    """rmclhip_recovery_state"""
    _fields_ = [("w_slow", C.c_double), ("w_fast", C.c_double)]


class RecoveryParams(C.Structure):
    """rmclhip_recovery_params"""
    _fields_ = [("alpha_slow", C.c_double), ("alpha_fast", C.c_double), ("p_max", C.c_double)]


class KldParams(C.Structure):
    """rmclhip_kld_params (occupied bins of pose space + the KLD-sampling bound)"""
    _fields_ = [("bin_xyz", C.c_float * 3), ("bin_rpy", C.c_float * 3), ("min_likelihood_rel", C.c_float), ("epsilon", C.c_double),
                ("z", C.c_double), ("n_min", C.c_uint32), ("n_max", C.c_uint32)]


class LikelihoodStats(C.Structure):
    _fields_ = [("sum", C.c_float), ("max", C.c_float)]


class PoseEstimate(C.Structure):
    _fields_ = [("pose", C.c_float * 8), ("covariance", C.c_double * 36), ("likelihood_mean", C.c_double),
                ("likelihood_sigma", C.c_double), ("likelihood_min", C.c_double), ("likelihood_max", C.c_double),
                ("trans_bb_min", C.c_float * 3), ("trans_bb_max", C.c_float * 3), ("n_particles", C.c_uint32),
                ("reserved", C.c_uint32)]


class PoseHypothesis(C.Structure):
    """rmclhip_pose_hypothesis: one cluster of the cloud's occupied bins"""
    _fields_ = [("estimate", PoseEstimate), ("key_min", C.c_uint64), ("weight", C.c_uint64), ("weight_share", C.c_double),
                ("n_bins", C.c_uint32), ("reserved", C.c_uint32)]


class PoseCovarianceParams(C.Structure):
    """rmclhip_pose_covariance_params"""
    _fields_ = [("sigma", C.c_double), ("rcond", C.c_double), ("degenerate_variance", C.c_double), ("min_eig_trans", C.c_double),
                ("min_eig_rot", C.c_double)]


class RobustParams(C.Structure):
    """rmclhip_robust_params (include/rmclhip.h, ROBUST MICP)"""
    _fields_ = [("kernel", C.c_int32), ("scale_mode", C.c_int32), ("scale", C.c_float), ("tuning", C.c_float), ("scale_min", C.c_float),
                ("reserved", C.c_uint32)]


class RobustStatistics(C.Structure):
    """rmclhip_robust_statistics (types.ROBUST_STATISTICS is its numpy twin, which the entry points fill): `stats` holds the 64 bytes
    of a CROSS_STATISTICS record"""
    _fields_ = [("stats", C.c_uint8 * 64), ("weight_sum", C.c_double), ("wrss", C.c_double), ("rss", C.c_double), ("scale", C.c_float),
                ("median_abs_residual", C.c_float)]


ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY, ROBUST_GEMAN_MCCLURE = 0, 1, 2, 3, 4
ROBUST_SCALE_FIXED, ROBUST_SCALE_MAD = 0, 1


class MapInfo(C.Structure):
    _fields_ = [("n_faces", C.c_uint32), ("n_vertices", C.c_uint32), ("n_nodes", C.c_uint32),
                ("n_tri_records", C.c_uint32), ("max_depth", C.c_uint32), ("stack_need", C.c_uint32),
                ("device_bytes", C.c_uint64), ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3),
                ("height_fallbacks", C.c_uint32), ("guarded_nodes", C.c_uint32), ("spatial_splits", C.c_uint32), ("reserved", C.c_uint32)]


class BundleViews(C.Structure):
    """rmclhip_bundle_views: a rmagine Bundle over caller-owned device memory, one nullable pointer per attribute"""
    _fields_ = [("hits_dev", C.c_void_p), ("ranges_dev", C.c_void_p), ("points_xyz_dev", C.c_void_p),
                ("normals_xyz_dev", C.c_void_p), ("face_ids_dev", C.c_void_p)]


class SegmentationParams(C.Structure):
    """rmclhip_segmentation_params (map_segmentation.cpp:25-41: the node's two thresholds, stored as float)"""
    _fields_ = [("min_dist_outlier_scan", C.c_float), ("min_dist_outlier_map", C.c_float), ("flags", C.c_uint32)]


class SegmentationViews(C.Structure):
    """rmclhip_segmentation_views: caller-owned device memory, every pointer nullable"""
    _fields_ = [("labels_dev", C.c_void_p), ("outlier_scan_xyz_dev", C.c_void_p), ("outlier_map_xyz_dev", C.c_void_p),
                ("counts_dev", C.c_void_p)]


class Pc2ScanStats(C.Structure):
    """rmclhip_pc2scan_stats"""
    _fields_ = [("n_points", C.c_uint32), ("n_finite", C.c_uint32), ("n_in_image", C.c_uint32), ("n_in_range", C.c_uint32),
                ("n_cells_filled", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PointCloud2Time(C.Structure):
    """rmclhip_pointcloud2_time: the per-point time field, t = offset_s + scale * raw"""
    _fields_ = [("offset", C.c_uint32), ("datatype", C.c_uint32), ("scale", C.c_double), ("offset_s", C.c_double)]


class ScanMotion(C.Structure):
    """rmclhip_scan_motion: K knots T_sref_s(t_k) (TRANSFORM records) and their times (doubles), host memory"""
    _fields_ = [("knots", C.c_void_p), ("times", C.c_void_p), ("n_knots", C.c_uint32)]


class DeskewStats(C.Structure):
    """rmclhip_deskew_stats"""
    _fields_ = [("n_points", C.c_uint32), ("n_finite", C.c_uint32), ("n_valid", C.c_uint32), ("n_time_clamped", C.c_uint32),
                ("n_time_nonfinite", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class FieldParams(C.Structure):
    """rmclhip_field_params (the distance field's lattice: cell 0 = automatic)"""
    _fields_ = [("cell", C.c_float), ("margin", C.c_float), ("max_nodes", C.c_uint64)]


class FieldInfo(C.Structure):
    """rmclhip_field_info"""
    _fields_ = [("n", C.c_uint32 * 3), ("origin", C.c_float * 3), ("cell", C.c_float), ("inv_cell", C.c_float),
                ("n_nodes", C.c_uint64), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {"n": tuple(int(x) for x in self.n), "origin": tuple(float(x) for x in self.origin), "cell": float(self.cell),
                "inv_cell": float(self.inv_cell), "n_nodes": int(self.n_nodes), "bytes": int(self.bytes)}


class BandFieldParams(C.Structure):
    """rmclhip_band_field_params (a banded distance field: fine nodes within `band` of the surface; max_nodes counts stored nodes)"""
    _fields_ = [("cell", C.c_float), ("margin", C.c_float), ("max_nodes", C.c_uint64), ("band", C.c_float), ("reserved", C.c_uint32)]


class BandFieldInfo(C.Structure):
    """rmclhip_band_field_info"""
    _fields_ = [("nb", C.c_uint32 * 3), ("brick_edge", C.c_uint32), ("n_bricks", C.c_uint64), ("n_stored", C.c_uint64),
                ("n_coarse", C.c_uint64), ("band", C.c_float), ("reach", C.c_float), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {"nb": tuple(int(x) for x in self.nb), "brick_edge": int(self.brick_edge), "n_bricks": int(self.n_bricks),
                "n_stored": int(self.n_stored), "n_coarse": int(self.n_coarse), "band": float(self.band), "reach": float(self.reach),
                "bytes": int(self.bytes)}


class RefineParams(C.Structure):
    """rmclhip_refine_params (the damped Gauss-Newton refinement on the distance field)"""
    _fields_ = [("iterations", C.c_uint32), ("dof_mask", C.c_uint32), ("max_dist", C.c_float), ("max_step_trans", C.c_float),
                ("max_step_rot", C.c_float), ("lambda0", C.c_float)]


class SteinParams(C.Structure):
    """rmclhip_stein_params (the Stein variational step on a filter handle's field)"""
    _fields_ = [("iterations", C.c_uint32), ("dof_mask", C.c_uint32), ("max_dist", C.c_float), ("max_step_trans", C.c_float),
                ("max_step_rot", C.c_float), ("lambda0", C.c_float), ("h_trans", C.c_float), ("h_rot", C.c_float), ("repulsion", C.c_float),
                ("max_per_bin", C.c_uint32), ("seed", C.c_uint64), ("step", C.c_uint32)]


class SteinStats(C.Structure):
    """rmclhip_stein_stats"""
    _fields_ = [("n_particles", C.c_uint32), ("n_not_finite", C.c_uint32), ("n_no_beams", C.c_uint32), ("n_bins", C.c_uint32),
                ("n_thinned_bins", C.c_uint32), ("reserved", C.c_uint32), ("cost_sum", C.c_double)]

    def as_dict(self):
        return {k: (float if k.startswith("cost") else int)(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class RefineStats(C.Structure):
    """rmclhip_refine_stats"""
    _fields_ = [("n_particles", C.c_uint32), ("n_moved", C.c_uint32), ("n_no_beams", C.c_uint32), ("n_not_finite", C.c_uint32),
                ("cost_before_sum", C.c_double), ("cost_after_sum", C.c_double)]

    def as_dict(self):
        return {k: (float if k.startswith("cost") else int)(getattr(self, k)) for k, _ in self._fields_}


PC2SCAN_TRUE_ELEVATION, PC2SCAN_FLOOR, PC2SCAN_WRAP_THETA, PC2SCAN_NEAREST = 1, 2, 4, 8
SEG_PINT_WITH_ORIGIN = 1
SEG_NONE, SEG_INLIER, SEG_OUTLIER_SCAN, SEG_OUTLIER_MAP = 0, 1, 2, 3

OUT_HITS, OUT_RANGES, OUT_POINTS, OUT_NORMALS, OUT_FACE_IDS = 1, 2, 4, 8, 16
OUT_ALL = 31
OUT_MICP = OUT_HITS | OUT_POINTS | OUT_NORMALS   # Correspondences_::model_buffers_ (Correspondences.hpp:81-85)


class Mesh(C.Structure):
    _fields_ = [("vertices_xyz", C.c_void_p), ("faces_ijk", C.c_void_p), ("n_vertices", C.c_uint32), ("n_faces", C.c_uint32)]


class Instance(C.Structure):
    _fields_ = [("transform", C.c_float * 12), ("mesh", C.c_uint32), ("reserved", C.c_uint32 * 3)]


# name -> (restype, argtypes); every symbol declared in include/rmclhip.h
_vp, _u32, _f32, _i32, _sz, _dbl = C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_size_t, C.c_double
_pp = C.POINTER(C.c_void_p)
SIGNATURES = {
    "rmclhip_last_error": (C.c_char_p, []),
    "rmclhip_version": (C.c_char_p, []),
    "rmclhip_ctx_create": (_i32, [_i32, _pp]),
    "rmclhip_ctx_destroy": (None, [_vp]),
    "rmclhip_ctx_device_name": (_i32, [_vp, C.c_char_p, _sz]),
    "rmclhip_map_create": (_i32, [_vp, _vp, _u32, _vp, _u32, _pp]),
    "rmclhip_map_create_scene": (_i32, [_vp, _vp, _u32, _vp, _u32, _pp]),
    "rmclhip_map_scene_instances": (_i32, [_vp, _vp, _sz, C.POINTER(_u32)]),
    "rmclhip_map_scene_locate": (_i32, [_vp, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_scene_flatten_host": (_i32, [_vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _sz, C.POINTER(_u32),
                                           C.POINTER(_u32)]),
    "rmclhip_map_retain": (_i32, [_vp]),
    "rmclhip_map_release": (None, [_vp]),
    "rmclhip_map_get_info": (_i32, [_vp, C.POINTER(MapInfo)]),
    "rmclhip_bvh_build_host": (_i32, [_vp, _u32, _vp, _u32, C.POINTER(MapInfo), _vp, _sz, _vp, _sz]),
    "rmclhip_bvh_build_host_quantised": (_i32, [_vp, _u32, _vp, _u32, _vp, _sz]),
    "rmclhip_bvh_build_host_pf": (_i32, [_vp, _u32, _vp, _u32, C.POINTER(MapInfo), _vp, _sz, _vp, _sz]),
    "rmclhip_bvh_build_host_frontier": (_i32, [_vp, _u32, _vp, _u32, _i32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "rmclhip_rcc_create": (_i32, [_vp, _vp, _pp]),
    "rmclhip_rcc_destroy": (None, [_vp]),
    "rmclhip_rcc_set_tsb": (_i32, [_vp, _vp]),
    "rmclhip_rcc_set_model_spherical": (_i32, [_vp, C.POINTER(SphericalModel)]),
    "rmclhip_rcc_set_model_o1dn": (_i32, [_vp, _u32, _u32, Interval, Vec3, _vp]),
    "rmclhip_rcc_set_model_pinhole": (_i32, [_vp, _u32, _u32, Interval, _f32, _f32, _f32, _f32]),
    "rmclhip_rcc_set_model_ondn": (_i32, [_vp, _u32, _u32, Interval, _vp, _vp]),
    "rmclhip_rcc_set_params": (_i32, [_vp, _f32, _f32]),
    "rmclhip_rcc_set_dataset": (_i32, [_vp, _vp, _vp, _u32, _i32]),
    "rmclhip_rcc_set_dataset_view": (_i32, [_vp, _vp, _vp, _u32]),
    "rmclhip_rcc_set_dataset_from_ranges": (_i32, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "rmclhip_rcc_find": (_i32, [_vp, _vp]),
    "rmclhip_rcc_find_async": (_i32, [_vp, _vp]),
    "rmclhip_rcc_sync": (_i32, [_vp]),
    "rmclhip_rcc_find_cpc": (_i32, [_vp, _vp]),
    "rmclhip_rcc_set_input_pointcloud2": (_i32, [_vp, _vp, _sz, C.POINTER(PointCloud2Layout), C.POINTER(Filter1D),
                                                  C.POINTER(Filter1D), Interval, _i32, C.POINTER(_u32),
                                                  C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_pointcloud2_to_scan": (_i32, [_vp, _vp, _sz, C.POINTER(PointCloud2Layout), _i32, _vp, C.POINTER(SphericalModel), _u32,
                                            _vp, _i32, C.POINTER(Pc2ScanStats)]),
    "rmclhip_rcc_set_input_pointcloud2_scan": (_i32, [_vp, _vp, _sz, C.POINTER(PointCloud2Layout), _i32, _vp, _u32, _pp,
                                                       C.POINTER(Pc2ScanStats)]),
    "rmclhip_rcc_set_input_pointcloud2_deskewed": (_i32, [_vp, _vp, _sz, C.POINTER(PointCloud2Layout), C.POINTER(PointCloud2Time),
                                                           C.POINTER(Filter1D), C.POINTER(Filter1D), Interval, _i32,
                                                           C.POINTER(ScanMotion), C.POINTER(_u32), C.POINTER(_u32),
                                                           C.POINTER(DeskewStats)]),
    "rmclhip_pointcloud2_deskew": (_i32, [_vp, _vp, _sz, C.POINTER(PointCloud2Layout), C.POINTER(PointCloud2Time), _i32,
                                           C.POINTER(ScanMotion), Interval, _vp, C.POINTER(DeskewStats)]),
    "rmclhip_scan_motion_from_base_poses_host": (_i32, [_vp, _vp, _vp, _u32, _dbl, _u32, _vp, _vp, _u32, C.POINTER(_u32)]),
    "rmclhip_pf_sample_beams_pointcloud2_deskewed": (_i32, [_vp, _sz, C.POINTER(PointCloud2Layout), C.POINTER(PointCloud2Time),
                                                             C.POINTER(ScanMotion), _u32, C.c_uint64, _vp, C.POINTER(_u32)]),
    "rmclhip_rcc_input_views": (_i32, [_vp, _pp, C.POINTER(_u32), C.POINTER(_u32), _pp, _pp, C.POINTER(_u32)]),
    "rmclhip_rcc_compute_cross_statistics": (_i32, [_vp, _vp, _dbl, _vp]),
    "rmclhip_rcc_download": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rmclhip_rcc_device_views": (_i32, [_vp, _pp, _pp, _pp, _pp, _pp, C.POINTER(_u32)]),
    "rmclhip_rcc_set_outputs": (_i32, [_vp, _u32]),
    "rmclhip_rcc_get_outputs": (_i32, [_vp, C.POINTER(_u32)]),
    "rmclhip_rcc_simulate": (_i32, [_vp, _vp, _u32, _i32, C.POINTER(BundleViews)]),
    "rmclhip_rcc_simulate_async": (_i32, [_vp, _vp, _u32, _i32, C.POINTER(BundleViews)]),
    "rmclhip_rcc_segment": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(SegmentationParams), C.POINTER(SegmentationViews),
                                   C.POINTER(_u32)]),
    "rmclhip_rcc_segment_async": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(SegmentationParams), C.POINTER(SegmentationViews)]),
    "rmclhip_statistics_p2l": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _f32, _vp]),
    "rmclhip_rcc_correct_once": (_i32, [_vp, _vp, _vp, _u32, _dbl, _i32, _vp, _vp]),
    "rmclhip_micp_correct_once": (_i32, [_vp, _u32, _vp, _vp, _vp, _u32, _dbl, _vp, _vp]),
    "rmclhip_rcc_correct_batch": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "rmclhip_rcc_sharded_create": (_i32, [_vp, _u32, _vp, _u32, _vp, _u32, _pp]),
    "rmclhip_rcc_sharded_destroy": (None, [_vp]),
    "rmclhip_rcc_sharded_size": (_u32, [_vp]),
    "rmclhip_rcc_sharded_replica": (_i32, [_vp, _u32, _pp]),
    "rmclhip_rcc_sharded_correct_batch": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "rmclhip_rcc_last_kernel_ms": (_i32, [_vp, C.POINTER(_f32), C.POINTER(_f32)]),
    "rmclhip_rcc_set_kernel_timing": (_i32, [_vp, _i32]),
    "rmclhip_rcc_time_find_sync": (_i32, [_vp, _vp, _u32, C.POINTER(_f32)]),
    "rmclhip_rcc_time_find": (_i32, [_vp, _vp, _u32, C.POINTER(_f32)]),
    "rmclhip_rcc_autotune": (_i32, [_vp, _vp, C.POINTER(_i32), C.POINTER(_f32)]),
    "rmclhip_rcc_autotune_batch": (_i32, [_vp, _vp, _u32, C.POINTER(_i32), C.POINTER(_f32)]),
    "rmclhip_rcc_time_reduce": (_i32, [_vp, _vp, _u32, C.POINTER(_f32)]),
    "rmclhip_rcc_time_correct_once": (_i32, [_vp, _vp, _vp, _u32, _dbl, _i32, _u32, C.POINTER(_f32)]),
    "rmclhip_rcc_time_caller_loop": (_i32, [_vp, _vp, _vp, _u32, _dbl, _u32, _vp, _vp, C.POINTER(_f32)]),
    "rmclhip_rcc_set_variant": (_i32, [_vp, _i32]),
    "rmclhip_rcc_find_variant": (_i32, [_vp, _u32, C.POINTER(_i32)]),
    "rmclhip_rcc_set_descent": (_i32, [_vp, _u32, _u32]),
    "rmclhip_rcc_set_batch_order": (_i32, [_vp, C.c_int]),
    "rmclhip_debug_batch_order": (_i32, [_vp, _vp, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_rcc_set_micp_fast": (_i32, [_vp, _i32]),
    "rmclhip_rcc_micp_fast_info": (_i32, [_vp, C.POINTER(MicpFastInfo)]),
    "rmclhip_rcc_ccs_info": (_i32, [_vp, C.POINTER(CcsInfo)]),
    "rmclhip_host_moment_statistics": (_i32, [_vp, _vp, _vp, _vp, _u32, _f32, _f32, _f32, _f32, _vp, _f32, _vp, C.POINTER(_u32),
                                               C.POINTER(_i32)]),
    "rmclhip_debug_wave_clock": (_i32, [_vp, _vp, _vp, _sz, C.POINTER(_u32)]),
    "rmclhip_debug_find_launch_shape": (_i32, [_i32, _i32, _u32, _u32, _u32, _u32, _u32, C.POINTER(FindLaunchShape)]),
    "rmclhip_debug_micp_moments": (_i32, [_vp, _vp, C.POINTER(_u32), C.POINTER(C.c_uint64)]),
    "rmclhip_debug_probe_find": (_i32, [_vp, _vp, _i32, _vp, _sz, C.POINTER(_u32)]),
    "rmclhip_rcc_find_batch": (_i32, [_vp, _vp, _u32]),
    "rmclhip_rcc_time_find_batch": (_i32, [_vp, _vp, _u32, _u32, C.POINTER(_f32)]),
    "rmclhip_umeyama_transform": (_i32, [_vp, _vp]),
    "rmclhip_cross_statistics_merge": (_i32, [_vp, _vp, _vp]),
    "rmclhip_cross_statistics_transform": (_i32, [_vp, _vp, _vp]),
    "rmclhip_transform_mult": (_i32, [_vp, _vp, _vp]),
    "rmclhip_transform_inv": (_i32, [_vp, _vp]),
    "rmclhip_pf_create": (_i32, [_vp, _vp, _pp]),
    "rmclhip_pf_destroy": (None, [_vp]),
    "rmclhip_pf_set_params": (_i32, [_vp, C.POINTER(PFParams)]),
    "rmclhip_pf_update": (_i32, [_vp, _vp, _vp, _u32, _vp, _u32, _vp]),
    "rmclhip_pf_update_async": (_i32, [_vp, _vp, _vp, _u32, _vp, _u32, _vp]),
    "rmclhip_pf_sync": (_i32, [_vp]),
    "rmclhip_pf_set_error_output": (_i32, [_vp, _vp]),
    "rmclhip_pf_motion_update": (_i32, [_vp, _vp, _vp, _u32, _vp, _dbl, _i32]),
    "rmclhip_pf_extract_weights": (_i32, [_vp, _vp, _u32, _vp]),
    "rmclhip_pf_time_update": (_i32, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _u32, C.POINTER(_f32)]),
    "rmclhip_pf_time_update_unfused": (_i32, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _i32, _u32, C.POINTER(_f32)]),
    "rmclhip_pf_set_variant": (_i32, [_vp, _i32]),
    "rmclhip_pf_set_schedule": (_i32, [_vp, _u32, _u32]),
    "rmclhip_pf_set_mapping": (_i32, [_vp, _i32, _u32, _vp, _u32]),
    "rmclhip_ctx_set_wait_mode": (_i32, [_vp, _i32]),
    "rmclhip_rcc_set_cpc_tracking": (_i32, [_vp, _i32]),
    "rmclhip_rcc_set_cpc_bounded": (_i32, [_vp, _i32]),
    "rmclhip_rcc_set_cpc_grid": (_i32, [_vp, _i32]),
    "rmclhip_pf_sample_beams_pointcloud2": (_i32, [_vp, _sz, C.POINTER(PointCloud2Layout), _u32, C.c_uint64, _vp, C.POINTER(_u32)]),
    "rmclhip_resampler_create": (_i32, [_vp, _pp]),
    "rmclhip_resampler_destroy": (None, [_vp]),
    "rmclhip_resampler_compute_stats": (_i32, [_vp, _vp, _u32, C.POINTER(LikelihoodStats)]),
    "rmclhip_resampler_compute_stats_weights": (_i32, [_vp, _vp, _u32, C.POINTER(LikelihoodStats)]),
    "rmclhip_resampler_gladiator": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, C.POINTER(GladiatorConfig),
                                            C.c_uint64, _u32]),
    "rmclhip_resampler_residual": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _u32, C.POINTER(GladiatorConfig),
                                           C.c_uint64, _u32, C.POINTER(C.c_uint64)]),
    "rmclhip_kld_params_default": (None, [_vp]),
    "rmclhip_particles_count_bins": (_i32, [_vp, _vp, _vp, _u32, C.POINTER(KldParams), C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_kld_bound_host": (_i32, [_u32, _dbl, _dbl, _u32, _u32, C.POINTER(_u32)]),
    "rmclhip_resampler_systematic": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _u32, C.POINTER(GladiatorConfig),
                                             C.c_uint64, _u32]),
    "rmclhip_resampler_adaptive": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, C.POINTER(KldParams), C.POINTER(GladiatorConfig),
                                           C.c_uint64, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_particles_pose_estimate": (_i32, [_vp, _vp, _vp, _u32, _u32, C.POINTER(PoseEstimate)]),
    "rmclhip_particles_pose_hypotheses": (_i32, [_vp, _vp, _vp, _u32, C.POINTER(KldParams), _u32, C.POINTER(PoseHypothesis), C.POINTER(_u32),
                                                  C.POINTER(_u32), _vp]),
    "rmclhip_chol6_host": (_i32, [_vp, _vp, C.POINTER(_dbl)]),
    "rmclhip_particles_init_uniform": (_i32, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, C.c_uint64, _u32]),
    "rmclhip_particles_init_pose": (_i32, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, C.c_uint64, _u32, C.POINTER(_dbl)]),
    "rmclhip_surface_sample_params_default": (None, [C.POINTER(SurfaceSampleParams)]),
    "rmclhip_surface_sampler_create": (_i32, [_vp, C.POINTER(SurfaceSampleParams), _pp]),
    "rmclhip_surface_sampler_destroy": (None, [_vp]),
    "rmclhip_surface_sampler_get_info": (_i32, [_vp, C.POINTER(SurfaceSampleInfo)]),
    "rmclhip_particles_init_surface": (_i32, [_vp, _vp, _vp, _u32, _u32, C.c_uint64, _u32]),
    "rmclhip_recovery_params_default": (None, [C.POINTER(RecoveryParams)]),
    "rmclhip_recovery_update_host": (_i32, [C.POINTER(RecoveryState), C.POINTER(RecoveryParams), _dbl, _u32, C.POINTER(_dbl)]),
    "rmclhip_recovery_reset_host": (_i32, [C.POINTER(RecoveryState)]),
    "rmclhip_particles_inject_surface": (_i32, [_vp, _vp, _vp, _u32, _u32, _dbl, C.c_uint64, _u32, C.POINTER(_u32)]),
    "rmclhip_pf_sharded_set_surface_sampler": (_i32, [_vp, C.POINTER(SurfaceSampleParams)]),
    "rmclhip_pf_sharded_init_surface": (_i32, [_vp, _u32, C.c_uint64, _u32]),
    "rmclhip_pf_sharded_inject_surface": (_i32, [_vp, _dbl, C.c_uint64, _u32, C.POINTER(_u32)]),
    "rmclhip_particles_pack_visualization": (_i32, [_vp, _vp, _vp, _u32, _u32, _vp, _i32]),
    "rmclhip_comm_create": (_i32, [_vp, _u32, _pp]),
    "rmclhip_comm_create_loopback": (_i32, [_vp, _u32, _pp]),
    "rmclhip_comm_collective_ranks": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_i32)]),
    "rmclhip_comm_loopback_set_reduce_rotation": (_i32, [_vp, _u32]),
    "rmclhip_debug_tag_retries": (_i32, [C.POINTER(C.c_ulonglong)]),
    "rmclhip_debug_trace": (_i32, [_i32, _vp, _sz]),
    "rmclhip_debug_particles_timing": (_i32, [_vp, _i32, C.POINTER(_f32)]),
    "rmclhip_debug_stein_timing": (_i32, [_vp, _i32, C.POINTER(_f32)]),
    "rmclhip_debug_live_bytes": (_i32, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rmclhip_debug_solve": (_i32, [_vp, _vp, _u32, _i32, _vp]),
    "rmclhip_comm_destroy": (None, [_vp]),
    "rmclhip_comm_size": (_u32, [_vp]),
    "rmclhip_shard_bounds": (None, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_pf_sharded_create": (_i32, [_vp, _vp, _u32, _vp, _u32, _pp]),
    "rmclhip_pf_sharded_destroy": (None, [_vp]),
    "rmclhip_pf_sharded_set_params": (_i32, [_vp, C.POINTER(PFParams)]),
    "rmclhip_pf_sharded_set_particles": (_i32, [_vp, _vp, _vp, _u32]),
    "rmclhip_pf_sharded_init_uniform": (_i32, [_vp, _u32, _vp, _vp, C.c_uint64, _u32]),
    "rmclhip_pf_sharded_init_pose": (_i32, [_vp, _u32, _vp, _vp, C.c_uint64, _u32, C.POINTER(_dbl)]),
    "rmclhip_pf_sharded_download": (_i32, [_vp, _vp, _vp]),
    "rmclhip_pf_update_sharded": (_i32, [_vp, _vp, _u32, _vp]),
    "rmclhip_pf_sharded_motion_update": (_i32, [_vp, _vp, _dbl, _i32]),
    "rmclhip_motion_noise_params_default": (None, [C.POINTER(MotionNoiseParams)]),
    "rmclhip_motion_noise_sigma_host": (_i32, [C.POINTER(MotionNoiseParams), _vp, _vp]),
    "rmclhip_pf_motion_update_noisy": (_i32, [_vp, _vp, _vp, _u32, _vp, _dbl, _i32, _vp, C.c_uint64, _u32, _u32]),
    "rmclhip_pf_sharded_motion_update_noisy": (_i32, [_vp, _vp, _dbl, _i32, _vp, C.c_uint64, _u32]),
    "rmclhip_pf_sharded_set_motion_noise": (_i32, [_vp, C.POINTER(MotionNoiseParams)]),
    "rmclhip_surface_params_default": (None, [_vp]),
    "rmclhip_pf_set_surface": (_i32, [_vp, _vp]),
    "rmclhip_pf_get_surface_stats": (_i32, [_vp, _vp]),
    "rmclhip_pf_constrain_to_surface": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "rmclhip_pf_sharded_set_surface": (_i32, [_vp, _vp]),
    "rmclhip_pf_sharded_constrain_to_surface": (_i32, [_vp, _vp, _vp]),
    "rmclhip_pf_sharded_get_surface_stats": (_i32, [_vp, _vp]),
    "rmclhip_debug_surface_faces": (_i32, [_vp, _vp]),
    "rmclhip_pf_sharded_step": (_i32, [_vp, _vp, _dbl, _i32, _vp, _u32, _vp, _i32, C.POINTER(GladiatorConfig), C.c_uint64, _u32,
                                       C.POINTER(LikelihoodStats)]),
    "rmclhip_pf_allgather_weights": (_i32, [_vp]),
    "rmclhip_pf_sharded_get_weights": (_i32, [_vp, _u32, _vp]),
    "rmclhip_pf_allreduce_stats": (_i32, [_vp, C.POINTER(LikelihoodStats)]),
    "rmclhip_pf_allreduce_pose_estimate": (_i32, [_vp, _u32, C.POINTER(PoseEstimate)]),
    "rmclhip_pf_sharded_pose_hypotheses": (_i32, [_vp, C.POINTER(KldParams), _u32, C.POINTER(PoseHypothesis), C.POINTER(_u32), C.POINTER(_u32)]),
    "rmclhip_pf_sharded_resample": (_i32, [_vp, C.POINTER(GladiatorConfig), C.c_uint64, _u32]),
    "rmclhip_pf_sharded_resample_residual": (_i32, [_vp, C.POINTER(GladiatorConfig), C.c_uint64, _u32]),
    "rmclhip_pose_information_p2l": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _f32, _vp]),
    "rmclhip_rcc_pose_information": (_i32, [_vp, _vp, _dbl, _vp]),
    "rmclhip_rcc_pose_information_batch": (_i32, [_vp, _u32, _dbl, _vp]),
    "rmclhip_pose_information_transform": (_i32, [_vp, _vp, _vp]),
    "rmclhip_pose_information_merge": (_i32, [_vp, _vp, _dbl, _vp]),
    "rmclhip_pose_information_solve_host": (_i32, [_vp, _dbl, _vp]),
    "rmclhip_pose_covariance_params_default": (None, [C.POINTER(PoseCovarianceParams)]),
    "rmclhip_pose_covariance_host": (_i32, [_vp, C.POINTER(PoseCovarianceParams), _vp]),
    "rmclhip_robust_params_default": (None, [C.c_int, C.POINTER(RobustParams)]),
    "rmclhip_robust_params_check": (_i32, [C.POINTER(RobustParams)]),
    "rmclhip_robust_weight_host": (_f32, [C.c_int, _f32, _f32]),
    "rmclhip_statistics_p2l_robust": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _f32, C.POINTER(RobustParams), _vp, _vp]),
    "rmclhip_rcc_compute_robust_statistics": (_i32, [_vp, _vp, _dbl, C.POINTER(RobustParams), _vp]),
    "rmclhip_rcc_robust_weights": (_i32, [_vp, _vp, _dbl, C.POINTER(RobustParams), _vp, C.c_int]),
    "rmclhip_rcc_residual_scale": (_i32, [_vp, _vp, _dbl, C.POINTER(RobustParams), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_u32)]),
    "rmclhip_rcc_correct_once_robust": (_i32, [_vp, _vp, _vp, _u32, _dbl, C.POINTER(RobustParams), _vp, _vp]),
    "rmclhip_debug_robust_select_recompute": (_i32, [C.c_int]),
    "rmclhip_cross_statistics_merge_weighted": (_i32, [_vp, _dbl, _vp, _dbl, _vp, C.POINTER(_dbl)]),
    "rmclhip_micp_correct_once_robust": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _u32, _dbl, _vp, _vp, C.POINTER(_dbl), _vp]),
    "rmclhip_rcc_pose_information_robust": (_i32, [_vp, _vp, _dbl, C.POINTER(RobustParams), _vp]),
    "rmclhip_pose_covariance_robust_host": (_i32, [_vp, C.POINTER(PoseCovarianceParams), _vp]),
    "rmclhip_field_params_default": (None, [C.POINTER(FieldParams)]),
    "rmclhip_field_layout_host": (_i32, [_vp, _vp, C.POINTER(FieldParams), C.POINTER(FieldInfo)]),
    "rmclhip_field_create": (_i32, [_vp, _vp, C.POINTER(FieldParams), _pp]),
    "rmclhip_field_destroy": (None, [_vp]),
    "rmclhip_field_get_info": (_i32, [_vp, C.POINTER(FieldInfo)]),
    "rmclhip_field_download": (_i32, [_vp, _vp, _sz]),
    "rmclhip_field_device_view": (_i32, [_vp, _pp]),
    "rmclhip_field_query": (_i32, [_vp, _vp, _sz, _i32, _vp]),
    "rmclhip_pf_set_field": (_i32, [_vp, _vp]),
    "rmclhip_pf_sharded_set_field": (_i32, [_vp, C.POINTER(FieldParams)]),
    "rmclhip_band_field_params_default": (None, [C.POINTER(BandFieldParams)]),
    "rmclhip_band_field_layout_host": (_i32, [_vp, _vp, C.POINTER(BandFieldParams), C.POINTER(FieldInfo), C.POINTER(BandFieldInfo)]),
    "rmclhip_field_create_banded": (_i32, [_vp, _vp, C.POINTER(BandFieldParams), _pp]),
    "rmclhip_field_get_band_info": (_i32, [_vp, C.POINTER(BandFieldInfo)]),
    "rmclhip_field_download_banded": (_i32, [_vp, _vp, _sz, _vp, _sz, _vp, _sz]),
    "rmclhip_pf_sharded_set_field_banded": (_i32, [_vp, C.POINTER(BandFieldParams)]),
    "rmclhip_refine_params_default": (None, [C.POINTER(RefineParams)]),
    "rmclhip_field_refine": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp, C.POINTER(RefineParams), _vp, C.POINTER(RefineStats)]),
    "rmclhip_pf_refine": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp, C.POINTER(RefineParams), _vp, C.POINTER(RefineStats)]),
    "rmclhip_pf_sharded_refine": (_i32, [_vp, _vp, _u32, _vp, C.POINTER(RefineParams), C.POINTER(RefineStats)]),
    "rmclhip_stein_params_default": (None, [C.POINTER(SteinParams)]),
    "rmclhip_pf_stein_step": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp, C.POINTER(SteinParams), _vp, C.POINTER(SteinStats)]),
    "rmclhip_malloc": (_i32, [_vp, _sz, _pp]),
    "rmclhip_free": (_i32, [_vp, _vp]),
    "rmclhip_memcpy_h2d": (_i32, [_vp, _vp, _vp, _sz]),
    "rmclhip_memcpy_d2h": (_i32, [_vp, _vp, _vp, _sz]),
}

_lib = None


def lib():
    """Load librmclhip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "librmclhip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C rmcl_amd/csrc`. rmcl_amd has no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the ABI symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


LAB_PATH = os.path.join(os.path.dirname(LIB_PATH), "librmclhip_lab.so")
_lab = None


def load_lab():
    """Load librmclhip_lab.so (EXPERIMENTS: rejected traversal kinds, probes, older particle-filter kernels; see
    include/rmclhip_lab.h).  Its static initialiser registers the experiments' launchers with librmclhip.so.  Only tools/
    and the `lab` test group call this; the product never does."""
    global _lab
    if _lab is not None:
        return _lab
    lib()
    if not os.path.exists(LAB_PATH):
        raise ImportError("librmclhip_lab.so is missing (%s): `make -C rmcl_amd/csrc`" % LAB_PATH)
    _lab = C.CDLL(LAB_PATH, mode=C.RTLD_GLOBAL)
    _lab.rmclhip_lab_version.restype = C.c_char_p
    return _lab


def check(status):
    if status == OK:
        return
    msg = lib().rmclhip_last_error().decode("utf-8", "replace")
    if status == ERR_NO_DEVICE:
        raise NoDeviceError(status, msg)
    raise RmclHipError(status, msg)
