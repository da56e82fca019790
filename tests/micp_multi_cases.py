"""Rigs of the N-sensor MICP correction (rmclhip_micp_correct_once), shared by tests/test_micp_multi_cases_cpu.py (the oracle alone)
and tests/test_gpu_micp_multi.py (the three loop forms of the library against the oracle).

A case is a rig on one map -- up to eight sensors of the four models (spherical, O1Dn, OnDn, pinhole), each with its mount Tsb, its
odometry stamp Tbo, its dataset (measured at the truth) and mask, its gate (max_dist, adaptive_min) and its merge weight -- plus the
localisation state Tom = truth * perturbation, n_iter and convergence_progress, and the loop form a call on sensors in the default
mode is meant to end in:

    host           iterations on the host from the published moments (every sensor <= 1024 undecided correspondences)
    device         the host form hands over to the device's moment loop (a sensor above 1024, the rig at most 4096)
    per-iteration  both moment forms overflow

Every model is small (256 ... 14 400 rays): a case costs the oracle well under a second.  Everything is deterministic.

near / mid / far are three perturbations of ONE rig, scaled along one direction; the scales were chosen on the device by the
undecided counts they give there (profiles/micp_multi_forms.txt), which depend on the caps the sensors have learnt by the third call.
"""
import math

import numpy as np

import oracle as orc
import oracle_micp as om

rpy = orc.transform_from_rpy

FORMS = ("host", "device", "per-iteration")


# ---- sensor models ---------------------------------------------------------------------------------------------------
def spherical(model):
    return {"kind": "spherical", "model": model}


def _grid_directions(H, W, phi0, phi1):
    from rmcl_amd import synthetic as syn, types as T
    sm = T.spherical_model(np.float32(phi0), np.float32((phi1 - phi0) / (H - 1)), H, np.float32(-math.pi), np.float32(2 * math.pi / W), W,
                           np.float32(0.1), np.float32(25.0))
    return syn.model_directions(sm).copy()


def o1dn_pf16(orig=(0.05, -0.02, 0.1), range_max=80.0):
    """model_pf16's 16 x 16 directions from ONE origin that is not the sensor's"""
    from rmcl_amd import synthetic as syn
    return {"kind": "o1dn", "width": 16, "height": 16, "range_min": 0.05, "range_max": range_max, "orig": tuple(orig),
            "dirs": syn.model_directions(syn.model_pf16()).copy()}


def ondn_48x10(seed=3):
    """tests/test_gpu_models.py's multi-emitter rig: 48 x 10 directions, every ray with an origin of its own"""
    W, H = 48, 10
    dirs = _grid_directions(H, W, -0.3, 0.3)
    origs = np.random.RandomState(seed).uniform(-0.2, 0.2, size=dirs.shape).astype(np.float32)
    return {"kind": "ondn", "width": W, "height": H, "range_min": 0.1, "range_max": 25.0, "origs": origs, "dirs": dirs}


def pinhole_64x48():
    return {"kind": "pinhole", "width": 64, "height": 48, "range_min": 0.3, "range_max": 12.0, "f": (52.5, 52.5), "c": (31.5, 23.5)}


def model_shape(model):
    """(H, W)"""
    if model["kind"] == "spherical":
        return int(model["model"].phi.size), int(model["model"].theta.size)
    return model["height"], model["width"]


def model_range(model):
    if model["kind"] == "spherical":
        return float(model["model"].range.min), float(model["model"].range.max)
    return float(model["range_min"]), float(model["range_max"])


def measure(mesh, model, Tsb, Tbm):
    """dataset and mask of one scan at Tbm (MICP*SensorCPU::unpackMessage: point = origin + direction * range; mask = range within
    the model's interval); points outside the mask are NaN"""
    sim = om.simulate_model(mesh, model, Tsb, Tbm)
    r = np.asarray(sim["ranges"], np.float32).reshape(-1)
    k = model["kind"]
    if k == "spherical":
        dirs, orig = orc.spherical_directions(model["model"]), 0.0
    elif k == "pinhole":
        dirs, orig = orc.pinhole_directions(model["width"], model["height"], model["f"], model["c"]), 0.0
    elif k == "o1dn":
        dirs, orig = np.asarray(model["dirs"], np.float32), np.asarray(model["orig"], np.float32)[None, :]
    else:
        dirs, orig = np.asarray(model["dirs"], np.float32), np.asarray(model["origs"], np.float32)
    lo, hi = model_range(model)
    mask = ((r >= np.float32(lo)) & (r <= np.float32(hi)) & (np.asarray(sim["hits"]).reshape(-1) > 0)).astype(np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        pts = (dirs * r[:, None] + orig).astype(np.float32)
    pts[mask == 0] = np.nan
    return pts, mask


# ---- cases -----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, mesh_name, sensors, truth, pert, n_iter=5, convergence_progress=0.0, form="host", identity=False):
        self.name, self.mesh_name, self.sensors, self.truth = name, mesh_name, sensors, truth
        self.Tom = orc.tmult(truth, pert)
        self.n_iter, self.convergence_progress, self.form, self.identity = n_iter, convergence_progress, form, identity
        assert form in FORMS and 1 <= len(sensors) <= 8

    def spec(self, order=None):
        """the sensors as oracle_micp.correct_once_multi takes them"""
        ss = self.sensors if order is None else [self.sensors[i] for i in order]
        return [(s["model"], s["Tsb"], s["Tbo"], s["ds"], s["mask"], s["max_dist"], s["adaptive_min"], s["w"]) for s in ss]

    def with_state(self, Tom=None, n_iter=None, convergence_progress=None):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        if Tom is not None:
            c.Tom = Tom
        if n_iter is not None:
            c.n_iter = n_iter
        if convergence_progress is not None:
            c.convergence_progress = convergence_progress
        return c


_MESH = {}


def mesh_arrays(name):
    from rmcl_amd import synthetic as syn
    if name not in _MESH:
        v, f = syn.noisy_room(30000) if name == "room30k" else syn.cube_room()
        _MESH[name] = (v, f, orc.Mesh(v, f))
    return _MESH[name]


def sensor(mesh, truth, name, model, Tsb, Tbo, w=1.0, max_dist=0.8, adaptive_min=0.2, measured_with=None, keep=None, use_mask=True,
           zero_mask=False):
    """measured_with: another model (same directions) the dataset is measured with; keep: the dataset's length; use_mask=False: the
    dataset goes without a mask (its invalid points are NaN and fall to the gate's own comparison)"""
    ds, mask = measure(mesh, measured_with or model, Tsb, orc.tmult(truth, Tbo))
    if zero_mask:
        mask = np.zeros_like(mask)
        ds = np.nan_to_num(ds, nan=1.0)        # finite points: only the mask keeps them out
    if keep is not None:
        ds, mask = ds[:keep].copy(), mask[:keep].copy()
    return {"name": name, "model": model, "Tsb": Tsb, "Tbo": Tbo, "ds": ds, "mask": mask if use_mask else None, "w": w,
            "max_dist": max_dist, "adaptive_min": adaptive_min}


ROOM_TRUTH = rpy((1.0, -2.0, 1.4), (0.02, -0.03, 0.4))
CUBE_TRUTH = rpy((0.5, -0.3, 0.2), (0.02, -0.03, 0.4))
SMALL = rpy((0.03, -0.02, 0.01), (0.002, 0.0, 0.006))

MOUNTS = [rpy((0.1, 0.0, 0.3), (0.0, 0.0, 10.0 * math.pi / 180)), rpy((-0.2, 0.1, 0.5), (0.0, 0.1, -1.0)),
          rpy((0.0, -0.25, 0.2), (0.05, 0.0, 2.0)), rpy((0.3, 0.0, 0.1), (0.0, -0.05, 0.1)),
          rpy((-0.1, -0.1, 0.4), (0.0, 0.0, 3.0)), rpy((0.2, 0.2, 0.0), (0.02, 0.02, -2.2)),
          rpy((0.0, 0.3, 0.35), (0.0, 0.08, 1.3)), rpy((-0.3, 0.0, 0.25), (-0.04, 0.0, -0.4))]
STAMPS = [orc.transform(), rpy((0.01, 0.0, 0.0), (0.0, 0.0, 0.002)), rpy((-0.005, 0.008, 0.0), (0.0, 0.0, -0.003)),
          rpy((0.0, -0.01, 0.002), (0.0, 0.001, 0.001)), rpy((0.004, 0.004, 0.0), (0.0, 0.0, 0.0015)),
          rpy((-0.008, 0.0, 0.001), (0.0, 0.0, -0.001)), rpy((0.002, -0.006, 0.0), (0.001, 0.0, 0.0025)),
          rpy((0.0, 0.009, -0.001), (0.0, 0.0, -0.002))]

# near / mid / far: Tom = truth * bracket_pert(scale); the scales come from the device (module docstring).  With fresh operators in
# the default mode, three identical calls go (code, undecided):
#   near 0.2     cap exit (1, 51), host (0, 71), host (0, 66 = 49 + 8 + 9 over the three sensors)
#   mid  0.45    cap exit (1, 263), overflow (2, 11990), host -> device hand-over (0, 3100)
#   far  1.04    overflow at the first sensor already (2, 4882 of its 14 400), again, then held off
# 0.05 leaves 9 undecided, all in one sensor; 0.3 hands its second call over (1576) and serves the third on the host (878); 0.6 and
# above overflow from the second call on.  far sits at 1.04 and not at 1.0 for the gate margin test_micp_multi_cases_cpu.py asks for.
BRACKET_SCALES = {"near": 0.2, "mid": 0.45, "far": 1.04}
BRACKET_GATE = (0.8, 0.8)       # max_dist, adaptive_min of the bracket rig
TINY_SCALE = 0.005              # calls at this error teach the sensors small caps (x 0.9 per completed call, down to twice what it met)


def bracket_pert(scale):
    return rpy((0.55 * scale, -0.45 * scale, 0.12 * scale), (0.004 * scale, 0.0, 0.05 * scale))


# six calls in a row on cube6's ONE set of operators: (order or subset of its sensors, the error of that call's Tom).  Another state
# every call, so that rows, flags or a call block left over from the call before give another answer
ORDER_CALLS = [((0, 1, 2, 3, 4, 5), ((0.02, -0.015, 0.01), (0.001, 0.0, 0.004))), ((3, 0, 1, 2, 4, 5), ((-0.03, 0.01, 0.02), (0.0, 0.002, -0.005))),
               ((5, 4, 3), ((0.01, 0.03, -0.02), (-0.002, 0.0, 0.006))), ((1, 5, 0, 4, 2, 3), ((-0.015, -0.025, 0.005), (0.001, -0.001, -0.003))),
               ((2, 4), ((0.035, 0.0, -0.01), (0.0, 0.0, 0.008))), ((0, 1, 2, 3, 4, 5), ((-0.01, 0.02, 0.03), (0.002, 0.001, -0.007)))]


def order_calls():
    """[(order, cube6 at that call's state)]"""
    base = cases()["cube6"]
    return [(order, base.with_state(Tom=orc.tmult(base.truth, rpy(*pert)))) for order, pert in ORDER_CALLS]


_CASES = None


def cases():
    """name -> Case"""
    global _CASES
    if _CASES is not None:
        return _CASES
    from rmcl_amd import synthetic as syn
    room, cube = mesh_arrays("room30k")[2], mesh_arrays("cube")[2]
    c1, pf16, vlp = spherical(syn.model_c1()), spherical(syn.model_pf16()), spherical(syn.model_vlp16_900(0.3))
    M, S = MOUNTS, STAMPS
    C = {}

    def room_sensor(*a, **k):
        return sensor(room, ROOM_TRUTH, *a, **k)

    C["mixed4"] = Case("mixed4", "room30k", [room_sensor("sph", c1, M[0], S[0], 1.0), room_sensor("o1dn", o1dn_pf16(), M[1], S[1], 0.37),
                                             room_sensor("ondn", ondn_48x10(), M[2], S[2], 2.0),
                                             room_sensor("pin", pinhole_64x48(), M[3], S[3], 0.0)], ROOM_TRUTH, SMALL)
    kinds = [c1, o1dn_pf16(), ondn_48x10(), pinhole_64x48(), pf16, c1, o1dn_pf16((-0.03, 0.04, 0.0)), ondn_48x10(11)]
    weights = [1.0, 0.37, 2.0, 0.0, 1.0, 0.5, 1.5, 0.25]
    C["eight"] = Case("eight", "room30k", [room_sensor("s%d" % k, kinds[k], M[k], S[k], weights[k]) for k in range(8)], ROOM_TRUTH, SMALL,
                      n_iter=4)
    C["one"] = Case("one", "room30k", [room_sensor("sph", c1, M[0], S[1], 0.37)], ROOM_TRUTH, SMALL, n_iter=6)
    blind = spherical(syn.model_pf16(0.05, 0.4))       # range limit below the nearest wall: every ray of the find misses
    C["empty_member"] = Case("empty_member", "room30k", [room_sensor("masked", c1, M[0], S[0], 1.0, zero_mask=True),
                                                         room_sensor("sees", o1dn_pf16(), M[1], S[1], 1.0),
                                                         room_sensor("blind", blind, M[2], S[2], 2.0, measured_with=pf16)], ROOM_TRUTH, SMALL)
    C["all_empty"] = Case("all_empty", "room30k", [room_sensor("masked", c1, M[0], S[0], 1.0, zero_mask=True),
                                                   room_sensor("blind", blind, M[2], S[2], 2.0, measured_with=pf16)], ROOM_TRUTH, SMALL,
                          identity=True)
    C["all_weight_zero"] = Case("all_weight_zero", "room30k", [room_sensor("sph", c1, M[0], S[0], 0.0),
                                                               room_sensor("o1dn", o1dn_pf16(), M[1], S[1], 0.0)], ROOM_TRUTH, SMALL,
                                identity=True)
    C["short_dataset"] = Case("short_dataset", "room30k", [room_sensor("short", c1, M[0], S[0], 1.0, keep=1024 // 2 + 7),
                                                           room_sensor("unmasked", o1dn_pf16(), M[1], S[1], 1.0, use_mask=False)],
                              ROOM_TRUTH, SMALL)
    # six sensors in the bare cube, a small error and a wide gate: no correspondence anywhere near the gate
    six = [c1, pf16, o1dn_pf16(), ondn_48x10(), c1, pf16]
    C["cube6"] = Case("cube6", "cube", [sensor(cube, CUBE_TRUTH, "s%d" % k, six[k], M[k], S[k], weights[k], max_dist=1.5, adaptive_min=1.5)
                                        for k in range(6)], CUBE_TRUTH, rpy((0.02, -0.015, 0.01), (0.001, 0.0, 0.004)), n_iter=4)
    g0, g1 = BRACKET_GATE
    rig = [room_sensor("vlp", vlp, M[0], S[0], 1.0, g0, g1), room_sensor("sph", c1, M[1], S[1], 0.37, g0, g1),
           room_sensor("pin", pinhole_64x48(), M[3], S[3], 2.0, g0, g1)]
    for name, form in (("near", "host"), ("mid", "device"), ("far", "per-iteration")):
        C[name] = Case(name, "room30k", rig, ROOM_TRUTH, bracket_pert(BRACKET_SCALES[name]), n_iter=5, form=form)
    _CASES = C
    return C


# ---- the oracle's answer, computed once per (case, order, state) ------------------------------------------------------
_ORACLE = {}


def oracle(case, order=None):
    """(T_onew_oold, merged unweighted statistics, solved weighted statistics per iteration, T_onew_oold per iteration)"""
    key = (case.name, None if order is None else tuple(order), case.Tom.tobytes(), case.n_iter, case.convergence_progress)
    if key not in _ORACLE:
        _ORACLE[key] = om.correct_once_multi(mesh_arrays(case.mesh_name)[2], case.spec(order), case.Tom, case.n_iter,
                                             case.convergence_progress, want_traj=True)
    return _ORACLE[key]


def gate_margins(case, order=None):
    """the smallest | |signed plane distance| - gate | / max_dist over every sensor, iteration and masked, hit correspondence, in
    float64 numpy at the oracle's pre-transforms -- the condition under which n_meas is the same number in every arithmetic"""
    mesh = mesh_arrays(case.mesh_name)[2]
    _, _, _, traj = oracle(case, order)
    worst = np.inf
    pre = [orc.transform()] + traj[:-1]
    for model, Tsb, Tbo, ds, mask, max_dist, adaptive_min, _ in case.spec(order):
        sim, ds, mask = om.reduced(om.simulate_model(mesh, model, Tsb, orc.tmult(case.Tom, Tbo)), ds, mask)
        md = float(orc.adaptive_max_dist(max_dist, adaptive_min, case.convergence_progress))
        ok = np.asarray(sim["hits"]).reshape(-1) > 0
        if mask is not None:
            ok &= mask > 0
        D0 = ds.astype(np.float64)
        ok &= np.isfinite(D0).all(1)
        I, N = sim["points"].astype(np.float64)[ok], sim["normals"].astype(np.float64)[ok]
        for T_onew_oold in pre:
            Ts = orc.tmult(orc.tmult(orc.tinv(Tsb), orc.tmult(orc.tmult(orc.tinv(Tbo), T_onew_oold), Tbo)), Tsb)
            q = np.array([Ts["R"][k] for k in "xyzw"], np.float64)
            x, y, z, w = q / np.linalg.norm(q)
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            t = np.array([Ts["t"][k] for k in "xyz"], np.float64)
            dist = np.einsum("ij,ij->i", I - (D0[ok] @ R.T + t), N)
            if len(dist):
                worst = min(worst, float(np.abs(np.abs(dist) - md).min()) / max_dist)
    return worst


# ---- the library side ------------------------------------------------------------------------------------------------
def make_operator(ra, hm, s):
    """the correspondence operator of one sensor entry"""
    m = s["model"]
    k = m["kind"]
    if k == "spherical":
        rcc = ra.RCCHipSpherical(hm)
        rcc.setModel(m["model"])
    elif k == "o1dn":
        rcc = ra.RCCHipO1Dn(hm)
        rcc.setModel(m["width"], m["height"], m["range_min"], m["range_max"], m["orig"], m["dirs"])
    elif k == "ondn":
        rcc = ra.RCCHipOnDn(hm)
        rcc.setModel(m["width"], m["height"], m["range_min"], m["range_max"], m["origs"], m["dirs"])
    else:
        rcc = ra.RCCHipPinhole(hm)
        rcc.setModel(m["width"], m["height"], m["range_min"], m["range_max"], m["f"][0], m["f"][1], m["c"][0], m["c"][1])
    rcc.set_dataset(s["ds"], s["mask"])
    rcc.params.max_dist, rcc.adaptive_max_dist_min = s["max_dist"], s["adaptive_min"]
    return rcc


def make_localization(ra, hm, case, mode=None, order=None):
    """MICPLocalization over fresh operators of the case's sensors (in `order`), every operator in moment-form `mode` (an int, or one
    per sensor; None: the default)"""
    ss = case.sensors if order is None else [case.sensors[i] for i in order]
    sensors = []
    for i, s in enumerate(ss):
        rcc = make_operator(ra, hm, s)
        if mode is not None:
            rcc.set_micp_fast(mode if isinstance(mode, int) else mode[i])
        sensors.append(ra.MICPSensor(s["name"], rcc, Tsb=s["Tsb"], Tbo=s["Tbo"], merge_weight_multiplier=s["w"]))
    loc = ra.MICPLocalization(sensors, optimization_iterations=case.n_iter)
    loc.Tom_, loc.convergence_progress_ = case.Tom, case.convergence_progress
    return loc


def call(loc, case):
    """one rmclhip_micp_correct_once on the case's state -> (T_onew_oold, merged unweighted statistics)"""
    loc.optimization_iterations_, loc.convergence_progress_ = case.n_iter, case.convergence_progress
    return loc._device_loop(case.Tom)


def infos(loc):
    return [s.correspondences_.micp_fast_info() for s in loc.sensors_vec_]


def close(loc):
    for s in loc.sensors_vec_:
        s.correspondences_.close()
