"""The map's distance field over the C ABI (include/rmclhip.h, DISTANCE FIELD): a lattice of float32 distances to the closest
triangle, built on the device.  Set on a PCDSensorUpdaterHip, it answers sensor_update.correspondence_type 1 by lookup.
"""
import ctypes as C

import numpy as np

from . import _capi
from .registration import _as_ptr
from .types import _ptr

DEFAULT_MAX_NODES = 1 << 26


def field_params(cell=0.0, margin=0.0, max_nodes=DEFAULT_MAX_NODES):
    """rmclhip_field_params: cell 0 = automatic (the near grid's size rule)"""
    p = _capi.FieldParams()
    _capi.lib().rmclhip_field_params_default(C.byref(p))
    p.cell, p.margin, p.max_nodes = float(cell), float(margin), int(max_nodes)
    return p


def field_layout(bbox_min, bbox_max, cell=0.0, margin=0.0, max_nodes=DEFAULT_MAX_NODES):
    """rmclhip_field_layout_host (no device needed): the geometry a field over this box gets, as FieldInfo.as_dict()"""
    lo = np.ascontiguousarray(bbox_min, dtype=np.float32).reshape(3)
    hi = np.ascontiguousarray(bbox_max, dtype=np.float32).reshape(3)
    info = _capi.FieldInfo()
    p = field_params(cell, margin, max_nodes)
    _capi.check(_capi.lib().rmclhip_field_layout_host(_ptr(lo), _ptr(hi), C.byref(p), C.byref(info)))
    return info.as_dict()


def band_field_params(cell=0.0, margin=0.0, band=0.5, max_nodes=DEFAULT_MAX_NODES):
    """rmclhip_band_field_params: max_nodes counts the stored nodes (729 per stored brick, plus the coarse lattice)"""
    p = _capi.BandFieldParams()
    _capi.lib().rmclhip_band_field_params_default(C.byref(p))
    p.cell, p.margin, p.band, p.max_nodes = float(cell), float(margin), float(band), int(max_nodes)
    return p


def band_field_layout(bbox_min, bbox_max, cell=0.0, margin=0.0, band=0.5, max_nodes=DEFAULT_MAX_NODES):
    """rmclhip_band_field_layout_host (no device needed): (the logical lattice as FieldInfo.as_dict(), the bricks as
    BandFieldInfo.as_dict()) of a banded field over this box; n_stored and the bytes depend on the map and are 0"""
    lo = np.ascontiguousarray(bbox_min, dtype=np.float32).reshape(3)
    hi = np.ascontiguousarray(bbox_max, dtype=np.float32).reshape(3)
    logical, info = _capi.FieldInfo(), _capi.BandFieldInfo()
    p = band_field_params(cell, margin, band, max_nodes)
    _capi.check(_capi.lib().rmclhip_band_field_layout_host(_ptr(lo), _ptr(hi), C.byref(p), C.byref(logical), C.byref(info)))
    return logical.as_dict(), info.as_dict()


REFINE_RESULT = np.dtype([("cost_before", np.float32), ("cost_after", np.float32), ("n_used", np.uint32), ("accepted", np.uint32)])


def refine_params(iterations=None, dof_mask=None, max_dist=None, max_step_trans=None, max_step_rot=None, lambda0=None):
    """rmclhip_refine_params: the library's defaults (rmclhip_refine_params_default), overridden by the keywords that are given"""
    p = _capi.RefineParams()
    _capi.lib().rmclhip_refine_params_default(C.byref(p))
    for k, v in (("iterations", iterations), ("dof_mask", dof_mask)):
        if v is not None:
            setattr(p, k, int(v))
    for k, v in (("max_dist", max_dist), ("max_step_trans", max_step_trans), ("max_step_rot", max_step_rot), ("lambda0", lambda0)):
        if v is not None:
            setattr(p, k, float(v))
    return p


def _refine_call(fn, handle, poses_dev, n_particles, beams, Tsb, params, results_dev, kwargs):
    """the argument handling DistanceFieldHip.refine and PCDSensorUpdaterHip.refine share: returns the counts as a dict"""
    from .types import RANGE_MEASUREMENT, TRANSFORM
    if params is None:
        params = refine_params(**kwargs)
    elif kwargs:
        raise TypeError("refine: give params or keywords, not both")
    if n_particles is None:
        n_particles = poses_dev.count if hasattr(poses_dev, "count") else poses_dev.shape[0]
    b = np.ascontiguousarray(beams, dtype=RANGE_MEASUREMENT).reshape(-1)
    T = np.ascontiguousarray(Tsb, dtype=TRANSFORM).reshape(1)
    st = _capi.RefineStats()
    _capi.check(fn(handle, _as_ptr(poses_dev), int(n_particles), _ptr(b), len(b), _ptr(T), C.byref(params), _as_ptr(results_dev), C.byref(st)))
    return st.as_dict()


STEIN_RESULT = np.dtype([("cost", np.float32), ("n_used", np.uint32), ("n_neighbours", np.uint32), ("kernel_weight", np.float32)])


def stein_params(iterations=None, dof_mask=None, max_dist=None, max_step_trans=None, max_step_rot=None, lambda0=None, h_trans=None, h_rot=None,
                 repulsion=None, max_per_bin=None, seed=None, step=None):
    """rmclhip_stein_params: the library's defaults (rmclhip_stein_params_default), overridden by the keywords that are given"""
    p = _capi.SteinParams()
    _capi.lib().rmclhip_stein_params_default(C.byref(p))
    for k, v in (("iterations", iterations), ("dof_mask", dof_mask), ("max_per_bin", max_per_bin), ("seed", seed), ("step", step)):
        if v is not None:
            setattr(p, k, int(v))
    for k, v in (("max_dist", max_dist), ("max_step_trans", max_step_trans), ("max_step_rot", max_step_rot), ("lambda0", lambda0),
                 ("h_trans", h_trans), ("h_rot", h_rot), ("repulsion", repulsion)):
        if v is not None:
            setattr(p, k, float(v))
    return p


class DistanceFieldHip:
    """rmclhip_field: built once from a HipMap, immutable.  An updater it is set on keeps it alive past close()."""

    def __init__(self, hip_map, cell=0.0, margin=0.0, max_nodes=DEFAULT_MAX_NODES):
        self._create(hip_map, _capi.lib().rmclhip_field_create, field_params(cell, margin, max_nodes))

    @classmethod
    def banded(cls, hip_map, cell=0.0, margin=0.0, band=0.5, max_nodes=DEFAULT_MAX_NODES):
        """rmclhip_field_create_banded: the same logical lattice, fine nodes stored only in the bricks within `band` (plus four cell
        diagonals) of the surface, the rest answered from a coarse lattice; max_nodes counts the stored nodes.  Query, refine and
        set_field work as on a dense field (refine / stein_step with max_dist > band are refused); download() is download_banded()."""
        self = cls.__new__(cls)
        self._create(hip_map, _capi.lib().rmclhip_field_create_banded, band_field_params(cell, margin, band, max_nodes))
        return self

    def _create(self, hip_map, create, params):
        if hip_map is None:
            raise RuntimeError("NO MAP")
        self.map, self.ctx = hip_map, hip_map.ctx
        self._h = C.c_void_p()
        _capi.check(create(self.ctx.handle, hip_map.handle, C.byref(params), C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def info(self):
        """the (logical) lattice; bytes is what the field holds on the device"""
        fi = _capi.FieldInfo()
        _capi.check(_capi.lib().rmclhip_field_get_info(self._h, C.byref(fi)))
        return fi.as_dict()

    def band_info(self):
        """rmclhip_field_get_band_info as a dict; a dense field raises"""
        bi = _capi.BandFieldInfo()
        _capi.check(_capi.lib().rmclhip_field_get_band_info(self._h, C.byref(bi)))
        return bi.as_dict()

    def download_banded(self):
        """(table uint32 [nb_z, nb_y, nb_x], coarse float32 [nb_z + 1, nb_y + 1, nb_x + 1], bricks float32 [n_stored, 9, 9, 9]) of a
        banded field, x fastest everywhere"""
        b = self.band_info()
        nb = b["nb"]
        table = np.zeros(b["n_bricks"], dtype=np.uint32)
        coarse = np.zeros(b["n_coarse"], dtype=np.float32)
        bricks = np.zeros(max(b["n_stored"], 1) * 729, dtype=np.float32)
        _capi.check(_capi.lib().rmclhip_field_download_banded(self._h, _ptr(table), table.size, _ptr(coarse), coarse.size, _ptr(bricks),
                                                              bricks.size))
        return (table.reshape(nb[2], nb[1], nb[0]), coarse.reshape(nb[2] + 1, nb[1] + 1, nb[0] + 1),
                bricks[:b["n_stored"] * 729].reshape(b["n_stored"], 9, 9, 9))

    def download(self):
        """the node values as a float32 array [n_z, n_y, n_x] (x fastest)"""
        i = self.info()
        out = np.zeros(i["n_nodes"], dtype=np.float32)
        _capi.check(_capi.lib().rmclhip_field_download(self._h, _ptr(out), out.size))
        return out.reshape(i["n"][2], i["n"][1], i["n"][0])

    def query(self, points, out_dev=None, n=None):
        """the lookup at points in map coordinates: an [n, 3] array on the host -> float32 array of n; or device memory of 3 n floats
        together with out_dev (n floats on the device), which then receives the distances"""
        if out_dev is not None:
            _capi.check(_capi.lib().rmclhip_field_query(self._h, _as_ptr(points), int(n), 1, _as_ptr(out_dev)))
            return None
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(p), dtype=np.float32)
        _capi.check(_capi.lib().rmclhip_field_query(self._h, _ptr(p), len(p), 0, _ptr(out)))
        return out

    def refine(self, poses_dev, beams, Tsb, n_particles=None, params=None, results_dev=None, **kwargs):
        """rmclhip_field_refine: damped Gauss-Newton of every pose (device memory, in place) on this field; likelihood attributes are
        not touched -- follow with a sensor update.  params: a refine_params(), or its keywords directly; results_dev: device memory for
        one REFINE_RESULT row per particle (optional).  Returns the counts (rmclhip_refine_stats) as a dict."""
        return _refine_call(_capi.lib().rmclhip_field_refine, self._h, poses_dev, n_particles, beams, Tsb, params, results_dev, kwargs)

    def close(self):
        if self._h:
            _capi.lib().rmclhip_field_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
