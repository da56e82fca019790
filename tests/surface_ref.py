"""The surface constraint of the motion update (include/rmclhip.h, "surface-constrained motion") restated in numpy float32 -- every
operation in the header's order.  The ray goes through the oracle's intersector (orc.Mesh.intersect: Embree's Moeller-Trumbore, tie
rule min t then min face id), the face normal is the oracle's record normal (face_normals()), and quaternion rotate / multiply are the
oracle's exported orc_quat_rotate / orc_quat_mult -- the arithmetic the GPU tests already hold bit-exact.  Not a test module.
"""
import numpy as np

import oracle as orc

F = np.float32
SNAP, MISS, STEEP = 0, 1, 2
CLASS_NAMES = ("snap", "miss", "steep")


def params(axis=0, height=0.0, probe_up=0.3, probe_down=1.0, min_up_cos=0.7, align=0, on_miss=0):
    """rmclhip_surface_params with the defaults of rmclhip_surface_params_default"""
    return dict(axis=int(axis), height=F(height), probe_up=F(probe_up), probe_down=F(probe_down), min_up_cos=F(min_up_cos),
                align=int(align), on_miss=int(on_miss))


def qrot(q, v):
    r = orc.lib().orc_quat_rotate(orc.Quat(*[float(x) for x in q]), orc.Vec3(*[float(x) for x in v]))
    return np.array([r.x, r.y, r.z], F)


def qmul(a, b):
    r = orc.lib().orc_quat_mult(orc.Quat(*[float(x) for x in a]), orc.Quat(*[float(x) for x in b]))
    return np.array([r.x, r.y, r.z, r.w], F)


def qnormalise(q):
    q = np.asarray(q, F)
    nrm = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return np.array([q[0] / nrm, q[1] / nrm, q[2] / nrm, q[3] / nrm], F)


def pose_Rt(pose):
    return (np.array([pose["R"][k] for k in "xyzw"], F), np.array([pose["t"][k] for k in "xyz"], F))


def set_pose(pose, R=None, t=None):
    if R is not None:
        for k, v in zip("xyzw", R):
            pose["R"][k] = v
    if t is not None:
        for k, v in zip("xyz", t):
            pose["t"][k] = v


def axis_of(R, p):
    return np.array([0, 0, 1], F) if p["axis"] == 0 else qrot(R, (0, 0, 1))


def origin_of(t, a, p):
    """O = (t - height a) + probe_up a: the probe's origin, and an end point of the lifted collision segment"""
    with np.errstate(all="ignore"):
        c = t - p["height"] * a
        return c + p["probe_up"] * a


def probe_one(mesh, normals, R, t, p, bvh=True):
    """steps 1-3 for one particle -- what depends on axis, height, probe_up, probe_down and min_up_cos only:
    (class, a, O, t_hit, n flipped towards a, face or -1, flipped)"""
    finite = bool(np.isfinite(R).all() and np.isfinite(t).all())
    if not finite:
        return MISS, None, None, None, None, -1, False
    a = axis_of(R, p)
    O = origin_of(t, a, p)
    tfar = p["probe_up"] + p["probe_down"]
    hit, th, face = mesh.intersect(O, -a, 0.0, float(tfar), bvh=bvh)
    if not hit:
        return MISS, a, O, None, None, -1, False
    n = normals[face].astype(F)
    d = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]
    flipped = bool(d < 0)
    if flipped:
        n, d = -n, -d
    return (SNAP if d >= p["min_up_cos"] else STEEP), a, O, F(th), n, face, flipped


def snap_one(R, t, probe, p):
    """steps 4-5 for a particle of class snap: (R', t')"""
    _, a, O, th, n, _, _ = probe
    pt = O + (-a) * th
    t2 = (pt + p["height"] * a).astype(F)
    if not p["align"]:
        return R, t2
    zb = qrot(R, (0, 0, 1))
    w = F(1) + ((zb[0] * n[0] + zb[1] * n[1]) + zb[2] * n[2])
    if w < F(1e-6):
        xb = qrot(R, (1, 0, 0))
        q = np.array([xb[0], xb[1], xb[2], 0], F)
    else:
        q = np.array([zb[1] * n[2] - zb[2] * n[1], zb[2] * n[0] - zb[0] * n[2], zb[0] * n[1] - zb[1] * n[0], w], F)
    return qnormalise(qmul(qnormalise(q), R)), t2


def constrain_one(mesh, normals, R, t, p, bvh=True, probe=None):
    """steps 1-5 for one particle: (class, R', t', face or -1, flipped)"""
    probe = probe_one(mesh, normals, R, t, p, bvh) if probe is None else probe
    if probe[0] != SNAP:
        return probe[0], R, t, probe[5], probe[6]
    R2, t2 = snap_one(R, t, probe, p)
    return SNAP, R2, t2, probe[5], probe[6]


def _kill(attr, max_n_meas):
    attr["likelihood"]["mean"], attr["likelihood"]["sigma"], attr["likelihood"]["n_meas"] = 0.0, 0.0, max_n_meas


def probes_of(mesh, poses, p, bvh=True, normals=None):
    """probe_one for every particle: computed once, shared by the calls that differ in align and on_miss only"""
    normals = mesh.face_normals() if normals is None else normals
    return [probe_one(mesh, normals, *pose_Rt(poses[i]), p, bvh) for i in range(len(poses))]


def constrain(mesh, poses, attrs, p, max_n_meas=10000, bvh=True, normals=None, probes=None):
    """rmclhip_pf_constrain_to_surface: returns (poses', attrs', stats, info) without touching its inputs;
    info = {"cls", "face", "flipped"} per particle.  probes: probes_of(mesh, poses, p) of the same poses and probe parameters."""
    normals = mesh.face_normals() if normals is None else normals
    poses, attrs = poses.copy(), attrs.copy()
    n = len(poses)
    cls, face, flipped = np.zeros(n, np.int32), np.full(n, -1, np.int64), np.zeros(n, bool)
    for i in range(n):
        R, t = pose_Rt(poses[i])
        cls[i], R2, t2, face[i], flipped[i] = constrain_one(mesh, normals, R, t, p, bvh, None if probes is None else probes[i])
        if cls[i] == SNAP:
            set_pose(poses[i], R2, t2)
        elif p["on_miss"]:
            _kill(attrs[i], max_n_meas)
    stats = dict(n_particles=n, n_snapped=int((cls == SNAP).sum()), n_missed=int((cls == MISS).sum()), n_steep=int((cls == STEEP).sum()))
    return poses, attrs, stats, dict(cls=cls, face=face, flipped=flipped)


def collides(mesh, p_from, p_to, bvh=True):
    """collision_in_between (TFMotionUpdaterCPU.cpp:17-50) as the motion kernel runs it: (moving and hit)"""
    with np.errstate(all="ignore"):
        vec = (p_to - p_from).astype(F)
        length = np.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2])
        moving = not (float(length) < 0.00001)
        if not (length >= 0) or not moving:      # (a NaN length gets no ray)
            return False
        vec = np.array([vec[0] / length, vec[1] / length, vec[2] / length], F)
    hit, _, _ = mesh.intersect(p_from, vec, 0.0, float(length), bvh=bvh)
    return bool(hit)


def motion_update(mesh, poses, attrs, T_bnew_bold, forget_rate, check_collision, p, max_n_meas=10000, bvh=True, normals=None):
    """rmclhip_pf_motion_update with the constraint set: move -> forget -> collision on the LIFTED segment (from the probe origin of the
    old pose to that of the moved pose) -> the constraint on the moved pose, killed or not.  Returns (poses', attrs', stats, killed)."""
    normals = mesh.face_normals() if normals is None else normals
    poses, attrs = poses.copy(), attrs.copy()
    n = len(poses)
    killed = np.zeros(n, bool)
    cls = np.zeros(n, np.int32)
    for i in range(n):
        old = poses[i].copy()
        new = orc.tmult(old, T_bnew_bold)
        nm = float(attrs[i]["likelihood"]["n_meas"])
        attrs[i]["likelihood"]["n_meas"] = np.uint32(int(nm - float(forget_rate) * nm))
        Ro, to = pose_Rt(old)
        Rn, tn = pose_Rt(new)
        if check_collision:
            killed[i] = collides(mesh, origin_of(to, axis_of(Ro, p), p), origin_of(tn, axis_of(Rn, p), p), bvh)
            if killed[i]:
                _kill(attrs[i], max_n_meas)
        cls[i], R2, t2, _, _ = constrain_one(mesh, normals, Rn, tn, p, bvh)
        poses[i] = new
        if cls[i] == SNAP:
            set_pose(poses[i], R2, t2)
        elif p["on_miss"]:
            _kill(attrs[i], max_n_meas)
    stats = dict(n_particles=n, n_snapped=int((cls == SNAP).sum()), n_missed=int((cls == MISS).sum()), n_steep=int((cls == STEEP).sum()))
    return poses, attrs, stats, killed


def to_capi(ra, p):
    """the same parameters as the library's struct"""
    return ra.types.surface_params(axis=p["axis"], height=float(p["height"]), probe_up=float(p["probe_up"]), probe_down=float(p["probe_down"]),
                                   min_up_cos=float(p["min_up_cos"]), align=p["align"], on_miss=p["on_miss"])
