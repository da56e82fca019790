"""rmcl_amd -- MI355X (gfx950) implementation of RMCL / MICP-L's ray-casting-correspondence +
pose-correction hot path.  Host-side mirror of the reference's operator interfaces over the C ABI
of librmclhip.so (include/rmclhip.h).  No CPU fallback: importing works anywhere the shared
library is built, computing needs a HIP device.
"""
from . import _capi, types, synthetic, wire  # noqa: F401
from ._capi import NoDeviceError, RmclHipError  # noqa: F401
from .micp import MICPLocalization, MICPSensor  # noqa: F401
from . import pf  # noqa: F401
from .pf import (AdaptiveResamplerHip, GladiatorResamplerHip, PCDSensorUpdaterHip, PoseEstimatorHip, ResidualResamplerHip, ShardedParticleFilterHip,  # noqa: F401
                 TFMotionUpdaterHip, beams_from_points, chol6, combined_forget_rate, constrain_to_surface, init_particles_pose,
                 init_particles_uniform, kld_bound, kld_params, pack_visualization, sample_beams,
                 RecoveryHip, SurfaceSamplerHip, init_particles_surface, surface_sample_params, motion_noise_params, motion_noise_sigma)
from .registration import (CPCHip, Context, CorrespondencesHIP, DeviceArray, HipMap, MapMap, RCCHipO1Dn,  # noqa: F401
                           RCCHipOnDn, RCCHipPinhole, RCCHipSpherical, ShardedCorrectorHip, build_bvh_host, build_bvh_host_frontier, build_bvh_host_pf, build_bvh_host_quantised,
                           flatten_scene_host, import_hip_map, import_hip_scene, micp_correct_once_robust, pose_information_p2l, statistics_p2l,
                           statistics_p2l_robust)

from . import field  # noqa: F401
from .field import DistanceFieldHip, band_field_layout, band_field_params, field_layout, field_params, refine_params, stein_params  # noqa: F401

from ._capi import load_lab  # noqa: F401  (experiments library; tools/ and the `lab` tests only)

__version__ = "0.1.0"
