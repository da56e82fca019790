"""The rigs of the robust rig loop's tests (tests/test_robust_rig_cpu.py, tests/test_gpu_robust_rig.py), from fixed seeds.

THE RIG.  The lidar is robust_cases.contaminated_scan's: 32 x 32 rays on the cube room, columns 5..11 shortened by 0.3 - 0.8 m (a pallet
in front of the wall), the estimate 0.2 m / 2 degrees off, SCAN_ITER = 10 iterations under SCAN_MAX_DIST = 1.0.  A second, CLEAN sensor
is micp_multi_cases.o1dn_pf16() on another mount, measured at the truth on the same room.  Multipliers 1.0 and 0.37.  Tom is the
identity, every Tbo the estimate (robust_cases.pose_error's convention).

EDGE RIGS come from micp_multi_cases.cases(): EDGE_NAMES."""
import numpy as np

import micp_multi_cases as mmc
import oracle_micp as om
import robust_cases as rc
import robust_ref as rr

F = np.float32
CLEAN_MOUNT = mmc.MOUNTS[1]
MULTIPLIERS = (1.0, 0.37)
EDGE_NAMES = ("mixed4", "one", "empty_member", "all_empty", "all_weight_zero", "short_dataset")
NONE_MULTIPLIERS = (1.0, 2.0, 2.0, 1.0)      # mixed4's, replaced by 1 and 2: n_meas * multiplier is an integer, nothing to truncate

_RIG = None


def rig(orc):
    """dict scan (contaminated_scan), sensors: two entries as micp_multi_cases.sensor makes them (name, model, Tsb, Tbo, ds, mask, w,
    max_dist, adaptive_min), each with the oracle's buffers of the find at the estimate (points, normals, hits)"""
    global _RIG
    if _RIG is not None:
        return _RIG
    from rmcl_amd import synthetic as syn
    s = rc.contaminated_scan(orc)
    pts, mask = s["dataset"]
    lidar = {"name": "lidar", "model": mmc.spherical(syn.model_c1()), "Tsb": s["Tsb"], "Tbo": s["estimate"], "ds": pts, "mask": mask,
             "w": MULTIPLIERS[0], "max_dist": rc.SCAN_MAX_DIST, "adaptive_min": rc.SCAN_MAX_DIST,
             "points": s["points"], "normals": s["normals"], "hits": s["hits"]}
    model = mmc.o1dn_pf16()
    ds, dmask = mmc.measure(s["mesh"], model, CLEAN_MOUNT, s["truth"])
    sim = om.simulate_model(s["mesh"], model, CLEAN_MOUNT, s["estimate"])
    clean = {"name": "clean", "model": model, "Tsb": CLEAN_MOUNT, "Tbo": s["estimate"], "ds": ds, "mask": dmask, "w": MULTIPLIERS[1],
             "max_dist": rc.SCAN_MAX_DIST, "adaptive_min": rc.SCAN_MAX_DIST,
             "points": sim["points"], "normals": sim["normals"], "hits": np.asarray(sim["hits"]).astype(np.uint8)}
    _RIG = dict(scan=s, sensors=[lidar, clean])
    return _RIG


def spec(sensors):
    """the sensors as oracle_micp.correct_once_multi takes them"""
    return [(s["model"], s["Tsb"], s["Tbo"], s["ds"], s["mask"], s["max_dist"], s["adaptive_min"], s["w"]) for s in sensors]


def ref_sensors(sensors, params, buffers=None, multipliers=None):
    """the sensors as robust_rig_ref.rig_loop takes them: params one robust_ref.params per sensor (or one for all); buffers: per sensor a
    dict points / normals / hits (a modelView()) replacing the entry's own, cut to the dataset's length"""
    out = []
    for k, s in enumerate(sensors):
        b = s if buffers is None else buffers[k]
        n = min(len(np.asarray(s["ds"]).reshape(-1, 3)), len(np.asarray(b["hits"]).reshape(-1)))
        out.append(dict(p=params[k] if isinstance(params, (list, tuple)) else params, Tsb=s["Tsb"], Tbo=s["Tbo"],
                        ds=np.asarray(s["ds"], F).reshape(-1, 3)[:n], mask=None if s["mask"] is None else np.asarray(s["mask"]).reshape(-1)[:n],
                        points=np.asarray(b["points"], F).reshape(-1, 3)[:n], normals=np.asarray(b["normals"], F).reshape(-1, 3)[:n],
                        hits=np.asarray(b["hits"]).reshape(-1)[:n], max_dist=s["max_dist"],
                        w=s["w"] if multipliers is None else multipliers[k]))
    return out


def params_of(ra, p):
    """the ctypes twin of a restatement's parameter dict"""
    q = ra._capi.RobustParams()
    q.kernel, q.scale_mode, q.scale, q.tuning, q.scale_min, q.reserved = p["kernel"], p["scale_mode"], p["scale"], p["tuning"], p["scale_min"], 0
    return q


def delta(orc, a, b):
    d = orc.tmult(orc.tinv(a), b)
    return max(max(abs(float(d["t"][k])) for k in "xyz"), max(abs(float(d["R"][k])) for k in "xyz"))


KERNELS = (rr.TUKEY, rr.HUBER)
