"""Wire-format adapters: the ROS message layouts the reference's sensors and updaters
consume, restated as plain field mappings so a host without ROS bindings (or a bag reader) can drive the operators.

Reference: rmcl_ros/src/util/conversions.cpp:22-120 (ScanInfo / CameraInfo / DepthInfo / O1DnInfo / OnDnInfo ->
rmagine models), :869-1002 (PointCloud2 -> O1Dn), PCDSensorUpdaterEmbree.cpp:290-327 (beam sampling from a
PointCloud2), rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213 (PointCloud2 -> spherical scan).  The device-side PointCloud2
paths are RCCHipO1Dn.setInputPointCloud2 (cloud -> O1Dn model + dataset), RCCHipSpherical.setInputPointCloud2 (cloud -> the dataset
of a spherical model) and pointcloud2_to_scan below.
"""
import ctypes as C

import numpy as np

from . import _capi
from .pf import beams_from_points

FLOAT32, FLOAT64 = 7, 8   # sensor_msgs/PointField datatypes
UINT32 = 6                # ... of a per-point time field (Ouster t, ns); FLOAT32 (Velodyne time) and FLOAT64 are the others


def spherical_from_scan_info(info):
    """rmcl_msgs/ScanInfo -> rm::SphericalModel (conversions.cpp:22-34). `info`: mapping or object with
    phi_min, phi_inc, phi_n, theta_min, theta_inc, theta_n, range_min, range_max."""
    g = (lambda k: info[k]) if isinstance(info, dict) else (lambda k: getattr(info, k))
    m = _capi.SphericalModel()
    m.phi.min, m.phi.inc, m.phi.size = g("phi_min"), g("phi_inc"), g("phi_n")
    m.theta.min, m.theta.inc, m.theta.size = g("theta_min"), g("theta_inc"), g("theta_n")
    m.range.min, m.range.max = g("range_min"), g("range_max")
    return m


def pinhole_from_camera_info(width, height, k, range_min=0.0, range_max=1e30):
    """sensor_msgs/CameraInfo -> rm::PinholeModel (conversions.cpp:36-46): f = (K[0], K[4]), c = (K[2], K[5]);
    the message carries no range, so the caller supplies it.  Returns RCCHipPinhole.setModel keyword arguments."""
    k = [float(x) for x in np.asarray(k).reshape(-1)]
    if len(k) != 9:
        raise ValueError("CameraInfo.k must have 9 entries")
    return dict(width=int(width), height=int(height), range_min=float(range_min), range_max=float(range_max),
                fx=k[0], fy=k[4], cx=k[2], cy=k[5])


def pinhole_from_depth_info(info):
    """rmcl_msgs/DepthInfo -> rm::PinholeModel (conversions.cpp:48-60)."""
    g = (lambda k: info[k]) if isinstance(info, dict) else (lambda k: getattr(info, k))
    return dict(width=int(g("width")), height=int(g("height")), range_min=float(g("range_min")),
                range_max=float(g("range_max")), fx=float(g("fx")), fy=float(g("fy")), cx=float(g("cx")), cy=float(g("cy")))


def xyz_from_pointcloud2(data, n_points, point_step, offset_x, offset_y, offset_z, datatype=FLOAT32):
    """the x / y / z fields of a PointCloud2 byte buffer as an [n, 3] float32 array (host side; used for beam
    sampling, where only `samples` random points are touched)."""
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    if datatype not in (FLOAT32, FLOAT64):
        raise ValueError("Field X has unknown DataType. Check Topic of PC")   # conversions.cpp:994
    ft = "<f4" if datatype == FLOAT32 else "<f8"
    size = 4 if datatype == FLOAT32 else 8
    if n_points and (n_points - 1) * point_step + max(offset_x, offset_y, offset_z) + size > buf.size:
        raise ValueError("cloud data shorter than its layout")
    out = np.empty((n_points, 3), np.float32)
    for c, off in enumerate((offset_x, offset_y, offset_z)):
        col = np.lib.stride_tricks.as_strided(buf[off:], shape=(n_points, size), strides=(point_step, 1))
        out[:, c] = np.ascontiguousarray(col).view(ft).reshape(-1).astype(np.float32)
    return out


def sample_beams_pointcloud2(data, n_points, point_step, offset_x, offset_y, offset_z, samples, seed, datatype=FLOAT32):
    """PCDSensorUpdaterEmbree.cpp:290-327 on the raw message bytes (cloud treated as n_points x 1 like the reference's
    `random_point_id * point_step` addressing), through the C ABI sampler (rmclhip_pf_sample_beams_pointcloud2)."""
    from .pf import sample_beams_pointcloud2 as _sample
    return _sample(data, n_points, 1, point_step, point_step * n_points, offset_x, offset_y, offset_z, samples, seed, datatype)


def pointcloud2_to_scan(ctx, data, width, height, point_step, row_step, offset_x, offset_y, offset_z, model, datatype=FLOAT32,
                        T=None, flags=0, device=False, nbytes=None, into=None):
    """Pc2ToScanNode::convert (pc2_to_scan.cpp:105-213) on the device, without an operator (rmclhip_pointcloud2_to_scan): the cloud's
    bytes (or a device pointer with device=True and nbytes) binned into `model` (a SphericalModel).  T: T_sensor_cloud or None;
    flags: an OR of _capi.PC2SCAN_*.  into=None: returns (ranges as a (phi.size, theta.size) float32 array, stats dict);
    into=device memory of phi.size * theta.size floats: fills it and returns the stats dict."""
    from .registration import _as_ptr, _cloud_bytes
    from .types import TRANSFORM, _ptr
    L = _capi.PointCloud2Layout(int(width), int(height), int(point_step), int(row_step), int(offset_x), int(offset_y),
                                int(offset_z), int(datatype))
    ptr, nb, _keep = _cloud_bytes(data, device, nbytes)
    Tarr = None if T is None else np.ascontiguousarray(T, dtype=TRANSFORM).reshape(1)   # (kept alive over the call)
    Tp = _ptr(Tarr)
    st = _capi.Pc2ScanStats()
    H, W = int(model.phi.size), int(model.theta.size)
    out = np.zeros((H, W), np.float32) if into is None else None
    optr = _ptr(out) if into is None else _as_ptr(into)
    _capi.check(_capi.lib().rmclhip_pointcloud2_to_scan(ctx.handle, ptr, nb, C.byref(L), int(bool(device)), Tp, C.byref(model),
                                                        int(flags), optr, 0 if into is None else 1, C.byref(st)))
    return (out, st.as_dict()) if into is None else st.as_dict()


def scan_motion(Tsb, base_poses, times, t_ref, subdivide=1, capacity=64):
    """The motion of a scan from base poses T_x_b (TRANSFORM[n], base in a fixed frame such as odometry) at strictly increasing
    `times` (seconds): knots T_sref_s(t_k) = ~Tsb * ~T_x_b(t_ref) * T_x_b(t_k) * Tsb with `subdivide` - 1 slerp knots inserted per
    segment, in double on the host (rmclhip_scan_motion_from_base_poses_host).  Returns (knots TRANSFORM[K], times float64[K]): what
    the deskewing calls take as `motion`.  The device interpolates between knots by nlerp; 16 knots per 0.3 rad keep that below
    float resolution (include/rmclhip.h)."""
    from .types import TRANSFORM, _ptr
    sb = np.ascontiguousarray(Tsb, dtype=TRANSFORM).reshape(1)
    P = np.ascontiguousarray(base_poses, dtype=TRANSFORM).reshape(-1)
    t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
    if len(P) != len(t):
        raise ValueError("one time per base pose")
    knots, kt, n = np.zeros(int(capacity), TRANSFORM), np.zeros(int(capacity), np.float64), C.c_uint32(0)
    _capi.check(_capi.lib().rmclhip_scan_motion_from_base_poses_host(_ptr(sb), _ptr(P), _ptr(t), len(P), float(t_ref), int(subdivide),
                                                                     _ptr(knots), _ptr(kt), int(capacity), C.byref(n)))
    return knots[:n.value].copy(), kt[:n.value].copy()


def pointcloud2_deskew(ctx, data, width, height, point_step, row_step, offset_x, offset_y, offset_z, time_field, motion,
                       datatype=FLOAT32, range_min=0.0, range_max=1e30, device=False, nbytes=None, into=None):
    """A cloud taken in motion -> the cloud in the sensor frame of the reference time, on the device, without an operator
    (rmclhip_pointcloud2_deskew): width * height xyz float32 records, NaN where the point is out of range or has no time.
    time_field: (offset, datatype[, scale[, offset_s]]); motion: (knots, times) as scan_motion returns them.  into=None: returns
    (a DeviceArray of 3 * n floats, stats dict); into=device memory of that size: fills it and returns the stats dict.  The records
    are what RCCHipSpherical.setInputPointCloud2(device=True, point_step=12) and CPCHip.set_dataset(device=True) accept."""
    from .registration import DeviceArray, _as_ptr, _cloud_bytes, _motion_arg, _time_arg
    L = _capi.PointCloud2Layout(int(width), int(height), int(point_step), int(row_step), int(offset_x), int(offset_y),
                                int(offset_z), int(datatype))
    ptr, nb, _keep = _cloud_bytes(data, device, nbytes)
    tf = _time_arg(time_field)
    mo, _keep_motion = _motion_arg(motion)
    st = _capi.DeskewStats()
    n = int(width) * int(height)
    out = DeviceArray(ctx, np.float32, max(3 * n, 1)) if into is None else None
    optr = C.c_void_p(out.ptr) if into is None else _as_ptr(into)
    _capi.check(_capi.lib().rmclhip_pointcloud2_deskew(ctx.handle, ptr, nb, C.byref(L), C.byref(tf), int(bool(device)), C.byref(mo),
                                                       _capi.Interval(range_min, range_max), optr, C.byref(st)))
    return (out, st.as_dict()) if into is None else st.as_dict()


def sample_beams_pointcloud2_deskewed(data, width, height, point_step, row_step, offset_x, offset_y, offset_z, time_field, motion,
                                      samples, seed, datatype=FLOAT32):
    """pf.sample_beams_pointcloud2 for a scan taken in motion (rmclhip_pf_sample_beams_pointcloud2_deskewed, a host function): the
    same draws, every beam with the origin and rotated direction of its point's own pose; an identity motion returns the plain
    sampler's bytes."""
    from .registration import _cloud_bytes, _motion_arg, _time_arg
    from .types import RANGE_MEASUREMENT, _ptr
    ptr, nb, _keep = _cloud_bytes(data, False, None)
    L = _capi.PointCloud2Layout(int(width), int(height), int(point_step), int(row_step), int(offset_x), int(offset_y),
                                int(offset_z), int(datatype))
    tf = _time_arg(time_field)
    mo, _keep_motion = _motion_arg(motion)
    out = np.zeros(int(samples), dtype=RANGE_MEASUREMENT)
    n = C.c_uint32(0)
    _capi.check(_capi.lib().rmclhip_pf_sample_beams_pointcloud2_deskewed(ptr, nb, C.byref(L), C.byref(tf), C.byref(mo), int(samples),
                                                                         int(seed), _ptr(out), C.byref(n)))
    return out[: n.value].copy()
