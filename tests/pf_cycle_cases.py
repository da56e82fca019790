"""Every input of the particle-filter cycle tests (tests/test_gpu_pf_cycle.py): motion-update cases, pose-estimate clouds and the
residual-resampling cloud, made deterministically from fixed seeds -- and proved non-vacuous on the CPU oracle alone by
tests/test_pf_cycle_cases_cpu.py.

Motion cases (motion_case): a map, a cloud, a step T_delta and a forget rate.  On the deep maps (chain200, nested200: 56 / 57 stack
entries against the 16 LDS rows of the collision ray; fan20k: massively overlapping boxes) every particle is AIMED: its step, turned
into the world by its own orientation, is laid through a point on a random face so that it crosses the face, ends before it, or
starts beyond it.  The wall cases are constructed float by float on a quad of two triangles (quad_wall), the gate cases put the
step length on both sides of the `length < 0.00001` gate.

Estimate cases (estimate_case): clouds for RmclNode::estimateStats and the induction counts to run them at.  estimate_ref restates
oracle.estimate_stats vectorised in float64 (the oracle loops in Python and extracts the Euler angles in float32).
"""
import math

import numpy as np

MAX_N_MEAS = 10000
DEEP_MAPS = ("chain200", "nested200", "fan20k")
N_MEAS_EDGES = (0, 1, 3, 9999, MAX_N_MEAS, MAX_N_MEAS + 1, 1 << 31, (1 << 32) - 1)     # 0, 1, odd, max_n_meas, past it, 2^32 - 1
F32_1E5 = np.float32(1e-5)                                                               # 9.99999975e-06: itself BELOW the double 0.00001
GATE_STEPS = (0.0, 0.9e-5, float(np.nextafter(F32_1E5, np.float32(0))), float(F32_1E5), float(np.nextafter(F32_1E5, np.float32(1))), 1.1e-5)
FORGET_RATES = (0.0, 1.0, 1e-12, 0.5)
BLOCK_EDGE_COUNTS = (1, 63, 64, 255, 256, 257, 1023)
BAD_FORGET_RATES = (-1e-9, -1.0, 1.0 + 1e-9, 2.0, 1e300, float("inf"), float("-inf"), float("nan"))

MOTION_CASES = (["%s_%s" % (m, s) for m in DEEP_MAPS for s in ("short", "long")] + ["chain200_far", "wall_x", "wall_inplane"] +
                ["gate_%d" % i for i in range(len(GATE_STEPS))] + ["rollpitch", "nan"] + ["forget_%d" % i for i in range(len(FORGET_RATES))])
DEEP_CASES = tuple(c for c in MOTION_CASES if c.split("_")[0] in DEEP_MAPS)
WALL_CASES = ("wall_x", "wall_inplane")
GATE_CASES = tuple(c for c in MOTION_CASES if c.startswith("gate_"))


# ---- maps -----------------------------------------------------------------------------------------------------------------------
def quad_wall(x0=1.0):
    """one axis-aligned wall of two triangles in the plane x = x0: A (x0, -1, 0), B (x0, 1, 0), C (x0, 1, 2), D (x0, -1, 2), faces
    (A, B, C) and (A, C, D): the shared edge A-C is the diagonal z = y + 1; A and C belong to both faces, B and D to one"""
    v = np.array([[x0, -1, 0], [x0, 1, 0], [x0, 1, 2], [x0, -1, 2]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def build_map(name, meshes):
    if name == "quad":
        return quad_wall(1.0)
    if name == "quad0":
        return quad_wall(0.0)
    return meshes(name)


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
def quats_from_rpy(roll, pitch, yaw):
    """ZYX Euler angles -> (n, 4) quaternions x y z w in float64"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], -1)


def make_poses(q, t, stamp_seed=0):
    from rmcl_amd.types import TRANSFORM
    n = len(q)
    p = np.zeros(n, TRANSFORM)
    for i, k in enumerate("xyzw"):
        p["R"][k] = q[:, i]
    for i, k in enumerate("xyz"):
        p["t"][k] = t[:, i]
    p["stamp"] = np.random.RandomState(1000 + stamp_seed).randint(0, 1 << 30, n)
    return p


def make_attrs(n, seed, n_meas=None):
    from rmcl_amd.types import PARTICLE_ATTRIBUTES
    rng = np.random.RandomState(seed)
    a = np.zeros(n, PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = rng.uniform(0.01, 1, n)
    a["likelihood"]["sigma"] = rng.uniform(0, 0.1, n)
    a["likelihood"]["n_meas"] = rng.randint(0, MAX_N_MEAS + 1, n) if n_meas is None else np.resize(np.asarray(n_meas, np.uint32), n)
    a["state_sigma"] = rng.uniform(0, 1, (n, 6))
    return a


def quat_mul(a, b):
    """Hamilton product of (..., 4) arrays in x y z w order (oracle: orc_quat_mult), in the arrays' own precision"""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def quat_conj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def quat_rotate(q, p):
    """q (p, 0) ~q, NOT normalised -- as orc_quat_rotate"""
    P = np.concatenate([p, np.zeros(p.shape[:-1] + (1,))], -1)
    return quat_mul(quat_mul(q, P), quat_conj(q))[..., :3]


def _step(t, rpy=(0.0, 0.0, 0.0)):
    from rmcl_amd import types as T
    return T.transform_from_rpy(tuple(float(x) for x in t), tuple(float(x) for x in rpy))


def _aimed_cloud(v, f, n, seed, step_t, rp=0.3):
    """n particles whose step (step_t in the body frame, turned by the particle's own orientation) is laid through a point on a random
    face: the point sits at 0.5 (the step crosses the face), 1.5 (ends before it), -0.5 (starts beyond it), 0.999 or 1.001 of the step"""
    rng = np.random.RandomState(seed)
    q = quats_from_rpy(rng.uniform(-rp, rp, n), rng.uniform(-rp, rp, n), rng.uniform(-math.pi, math.pi, n))
    q = q.astype(np.float32).astype(np.float64)
    step_w = quat_rotate(q, np.broadcast_to(np.asarray(step_t, np.float64), (n, 3)))
    tri = v.astype(np.float64)[f[rng.randint(0, len(f), n)]]
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    target = (tri * b[:, :, None]).sum(1)
    frac = np.resize(np.array([0.5, 1.5, -0.5, 0.999, 1.001, 0.5, 0.25, 0.75]), n)
    return make_poses(q, target - frac[:, None] * step_w, seed), make_attrs(n, seed + 1)


def _wall_cloud():
    """identity (or half-turn: q = (0, 0, 1, 0), exact) orientations in front of, on and behind quad_wall(1.0); with the step
    (0.25, 0, 0) the identity particles move +x and the half-turn ones -x, with (0, 0.25, 0) they move along the wall"""
    f32 = np.float32

    def up(x, k=1):
        for _ in range(k):
            x = np.nextafter(f32(x), f32(np.inf))
        return float(x)

    def dn(x, k=1):
        for _ in range(k):
            x = np.nextafter(f32(x), f32(-np.inf))
        return float(x)

    rows = []      # (x, y, z, half_turn)
    for y, z in ((0.25, 0.5), (-0.5, 1.5), (0.25, 1.25), (-0.75, 0.25)):         # inside face 0, inside face 1, two ON the diagonal z = y + 1
        rows += [(dn(0.75, k), y, z, 0) for k in (1, 2, 3, 8)]                    # ends a few ulps short of the wall
        rows += [(0.75, y, z, 0)]                                                 # ends exactly on it: t == tfar
        rows += [(up(0.75, k), y, z, 0) for k in (1, 2, 3)]                       # crosses by a few ulps
        rows += [(0.875, y, z, 0), (0.5, y, z, 0)]                                # crosses in the middle; ends 0.25 short
        rows += [(1.0, y, z, 0), (1.0, y, z, 1)]                                  # starts exactly on it, moving either way
        rows += [(up(1.0), y, z, 0), (1.5, y, z, 0), (dn(1.0), y, z, 1), (0.5, y, z, 1)]   # starts behind / in front of it and moves away
        rows += [(1.125, y, z, 1), (1.25, y, z, 1), (up(1.25), y, z, 1), (dn(1.25), y, z, 1)]   # the same wall from the other side
    for y, z in ((-1, 0), (1, 2), (1, 0), (-1, 2)):                               # through the corner vertices A, C (both faces), B, D (one)
        rows += [(0.875, y, z, 0), (1.125, y, z, 1), (0.75, y, z, 0), (1.0, y, z, 0)]
    for y, z in ((0.0, 0.0), (1.0, 1.0), (-1.0, 1.0), (0.0, 2.0), (up(1.0), 1.0), (0.0, dn(0.0))):   # through the outer edges and just past them
        rows += [(0.875, y, z, 0), (1.0, y, z, 0)]
    for y in (-1.5, -1.25, -1.125, -1.0, -0.875, 0.75, 0.875, 1.0, 1.125):        # (in-plane step +y: into, inside, along and out of the wall)
        rows += [(1.0, y, 1.0, 0), (1.0, y, 0.0, 0), (1.0, y, y + 1.0, 0), (up(1.0), y, 1.0, 0), (dn(1.0), y, 1.0, 0)]
    r = np.array(rows, np.float64)
    q = np.where(r[:, 3:4] > 0, np.array([[0.0, 0.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 0.0, 1.0]]))
    rng = np.random.RandomState(71)       # ... and an ordinary cloud around the wall, every orientation
    n = 400
    q2 = quats_from_rpy(rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-math.pi, math.pi, n))
    t2 = np.stack([rng.uniform(0.7, 1.3, n), rng.uniform(-1.3, 1.3, n), rng.uniform(-0.3, 2.3, n)], -1)
    q, t = np.concatenate([q, q2]), np.concatenate([r[:, :3], t2])
    return make_poses(q, t, 70), make_attrs(len(q), 72)


def _gate_cloud():
    """particles on, just in front of and just behind quad_wall(0.0) -- around the origin, where float32 resolves a step of 1e-5 to
    1e-12 -- moving +x (identity), -x (half turn) and every other way"""
    xs = [0.0, -1e-7, -1e-6, -5e-6, -8.9e-6, -9.5e-6, -9.99e-6, -1.0e-5, -1.05e-5, -1.2e-5, -1e-4, 1e-7, 5e-6, 1.05e-5]
    rows = [(x, y, z, h) for x in xs for y, z in ((0.25, 0.5), (0.25, 1.25), (-1.0, 0.0), (0.5, 1.0)) for h in (0, 1)]
    rows += [(-x, y, z, 1) for x in xs for y, z in ((0.25, 0.5),)]
    r = np.array(rows, np.float64)
    q = np.where(r[:, 3:4] > 0, np.array([[0.0, 0.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 0.0, 1.0]]))
    rng = np.random.RandomState(73)
    n = 300
    q2 = quats_from_rpy(rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-math.pi, math.pi, n))
    t2 = np.stack([rng.uniform(-1.5e-5, 1.5e-5, n), rng.uniform(-1.1, 1.1, n), rng.uniform(-0.1, 2.1, n)], -1)
    q, t = np.concatenate([q, q2]), np.concatenate([r[:, :3], t2])
    return make_poses(q, t, 74), make_attrs(len(q), 75)


def _room_cloud(n, seed, n_meas=None):
    """a cloud in the cube room (walls at +-5) with roll and pitch; every third quaternion has w < 0 (the same rotation), every fifth
    is denormalised by up to 1e-3 (nothing normalises: the step stretches with |q|^2, on the device as in the oracle)"""
    rng = np.random.RandomState(seed)
    q = quats_from_rpy(rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-math.pi, math.pi, n))
    q[::3] *= -np.sign(q[::3, 3:4])
    q[::5] *= rng.uniform(1 - 1e-3, 1 + 1e-3, (len(q[::5]), 1))
    t = rng.uniform(-4.99, 4.99, (n, 3))
    return make_poses(q, t, seed), make_attrs(n, seed + 1, n_meas)


_cache = {}


def motion_case(name, meshes):
    """-> dict(name, map, v, f, poses, attrs, T_delta, rate); poses / attrs are the INPUT: copy before an in-place update"""
    if name in _cache:
        return _cache[name]
    head, _, tail = name.partition("_")
    rate = 0.05
    if head in DEEP_MAPS:
        mp = head
        v, f = build_map(mp, meshes)
        # chain200: triangles along +x, 4e-18 .. 3e17 m; nested200: a stack of coaxial triangles up z, 2 m tall; fan20k: a disc of radius 10
        step_t = {"short": (0.05, 0.0, 0.0), "long": {"chain200": (30.0, 1.0, 0.5), "nested200": (0.3, 0.2, 3.0), "fan20k": (12.0, 0.0, 0.4)}[mp],
                  "far": (1e5, 2e3, 1e3)}[tail]
        poses, attrs = _aimed_cloud(v, f, 2000, 100 + 7 * MOTION_CASES.index(name), step_t)
        T_delta = _step(step_t, (0.01, -0.02, 0.03))
    elif name in WALL_CASES:
        mp = "quad"
        v, f = build_map(mp, meshes)
        poses, attrs = _wall_cloud()
        T_delta = _step((0.25, 0.0, 0.0) if name == "wall_x" else (0.0, 0.25, 0.0))
    elif head == "gate":
        mp = "quad0"
        v, f = build_map(mp, meshes)
        poses, attrs = _gate_cloud()
        T_delta = _step((GATE_STEPS[int(tail)], 0.0, 0.0))
    elif name in ("rollpitch", "nan"):
        mp = "cube"
        v, f = build_map(mp, meshes)
        poses, attrs = _room_cloud(1500, 81)
        T_delta = _step((0.6, -0.1, 0.05), (0.1, -0.2, 0.3))
        if name == "nan":
            poses = poses[:300].copy()
            attrs = attrs[:300].copy()
            poses["t"]["x"][7] = np.nan
            poses["t"]["z"][70] = np.nan
    elif head == "forget":
        mp = "cube"
        v, f = build_map(mp, meshes)
        poses, attrs = _room_cloud(640, 91, N_MEAS_EDGES)
        T_delta = _step((0.3, 0.0, 0.0), (0.0, 0.0, 0.05))
        rate = FORGET_RATES[int(tail)]
    else:
        raise KeyError(name)
    c = dict(name=name, map=mp, v=v, f=f, poses=poses, attrs=attrs, T_delta=T_delta, rate=rate)
    _cache[name] = c
    return c


def motion_reference(case, orc, collision, bvh=False):
    """the oracle's update of the case (brute force by default), cached: -> (poses, attrs), not to be modified"""
    key = (case["name"], "ref", bool(collision), bool(bvh))
    if key not in _cache:
        if "mesh" not in case:
            case["mesh"] = orc.Mesh(case["v"], case["f"])
        p, a = case["poses"].copy(), case["attrs"].copy()
        case["mesh"].pf_motion_update(p, a, case["T_delta"], case["rate"], collision=collision, max_n_meas=MAX_N_MEAS, bvh=bvh)
        _cache[key] = (p, a)
    return _cache[key]


def killed(attrs_ref):
    L = attrs_ref["likelihood"]
    return (L["n_meas"] == MAX_N_MEAS) & (L["mean"] == 0) & (L["sigma"] == 0)


def step_lengths(case, poses_ref):
    """the float32 length the collision test computes: sqrtf((dx dx + dy dy) + dz dz) of new - old"""
    d = [poses_ref["t"][k] - case["poses"]["t"][k] for k in "xyz"]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=np.float32)


def first_difference(name, what, got, want, n=None):
    """None, or a message naming the case, the first differing records and both values"""
    n = len(want) if n is None else n
    g, w = got[:n], want[:n]
    if g.tobytes() == w.tobytes():
        return None
    rec = g.dtype.itemsize
    bad = np.flatnonzero((g.view(np.uint8).reshape(n, rec) != w.view(np.uint8).reshape(n, rec)).any(1))
    return "%s: %s differ on %d of %d particles, first %s:\n" % (name, what, bad.size, n, bad[:6].tolist()) + "\n".join(
        "  particle %d: got %s\n%s want %s" % (i, g[i], " " * (12 + len(str(i))), w[i]) for i in bad[:4])


# ---- pose-estimate clouds ---------------------------------------------------------------------------------------------------------
ESTIMATE_CASES = ("uniform_rp", "converged_pi", "converged_pi_flipped", "wide_weights", "single_weight",
                  "n1", "n255", "n256", "n257", "n1023", "n1025", "big")
CONCENTRATED = ("converged_pi", "converged_pi_flipped", "single_weight", "n1")     # covariance floor derived from float32, see the GPU test
BIG_N = 262144 + 1025


def _uniform_rp(n, seed):
    """uniform in a box with roll and pitch from +-0.2; yaw from +-2.5, not the full circle: a yaw uniform on the circle has no mean
    (the two largest eigenvalues of sum w q q^T meet)"""
    rng = np.random.RandomState(seed)
    q = quats_from_rpy(rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-2.5, 2.5, n))
    t = np.stack([rng.uniform(-9, 9, n), rng.uniform(-9, 9, n), rng.uniform(0.2, 3.0, n)], -1)
    a = make_attrs(n, seed + 1)
    a["likelihood"]["mean"] = rng.uniform(0, 1, n)
    return make_poses(q, t, seed), a


def _converged_pi(n, seed):
    """sigma 1 cm / 0.01 rad around (3, -2, 1), yaw pi - 0.005: half of the yaws wrap to -pi + ..."""
    rng = np.random.RandomState(seed)
    q = quats_from_rpy(rng.normal(0, 0.01, n), rng.normal(0, 0.01, n), math.pi - 0.005 + rng.normal(0, 0.01, n))
    t = np.array([3.0, -2.0, 1.0]) + rng.normal(0, 0.01, (n, 3))
    a = make_attrs(n, seed + 1)
    a["likelihood"]["mean"] = rng.uniform(0.2, 1, n)
    return make_poses(q, t, seed), a


def estimate_case(name):
    """-> dict(name, poses, attrs, n_inductions): all particles, 1, 1000, one particle into rank 1 of three, more than there are"""
    key = ("est", name)
    if key in _cache:
        return _cache[key]
    if name == "uniform_rp":
        poses, attrs = _uniform_rp(4099, 201)
    elif name in ("converged_pi", "converged_pi_flipped"):
        poses, attrs = _converged_pi(3001, 203)
        if name.endswith("flipped"):
            for k in "xyzw":
                poses["R"][k][1::2] *= -1
    elif name == "wide_weights":
        poses, attrs = _uniform_rp(2500, 205)
        attrs["likelihood"]["mean"] = 10.0 ** np.random.RandomState(206).uniform(-30, 0, len(poses))
    elif name == "single_weight":
        poses, attrs = _uniform_rp(1501, 207)
        attrs["likelihood"]["mean"] = 0.0
        attrs["likelihood"]["mean"][1000] = 0.7
    elif name == "big":
        poses, attrs = _uniform_rp(BIG_N, 209)
    elif name[0] == "n":
        poses, attrs = _uniform_rp(int(name[1:]), 211 + int(name[1:]))
    else:
        raise KeyError(name)
    n = len(poses)
    from rmcl_amd.distributed import shard_bounds
    want = [n, 1, 1000, shard_bounds(n, 0, 3)[1] + 1, n + 7]
    if name == "single_weight":
        want = [n, 1001, shard_bounds(n, 1, 3)[1] + 1, n + 7]      # (the first 1000 likelihoods sum to zero: refused, see the zero-sum test)
    n_ind = []
    for k in want:                          # (a small cloud: counts that mean the same particles are run once, one of them past n)
        if (min(k, n), k > n) not in [(min(x, n), x > n) for x in n_ind]:
            n_ind.append(k)
    c = dict(name=name, poses=poses, attrs=attrs, n_inductions=tuple(n_ind))
    _cache[key] = c
    return c


def euler_zyx(q):
    """ZYX extraction of orc_quat_to_euler, in float64: (n, 4) x y z w -> (n, 3) roll pitch yaw"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    sinp = 2.0 * (w * y - z * x)
    pitch = np.where(np.abs(sinp) >= 1.0, np.copysign(math.pi / 2, sinp), np.arcsin(np.clip(sinp, -1.0, 1.0)))
    return np.stack([np.arctan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)), pitch,
                     np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))], -1)


def estimate_ref(poses, attrs, n_induction=None, mean_pose=None):
    """oracle.estimate_stats restated vectorised in float64: likelihood statistics, bounding box, Markley mean (eigenvector of the
    largest eigenvalue of M = sum w q q^T, w >= 0 sign), mean translation and the 6x6 covariance sum w d d^T, d = (translation, roll,
    pitch, yaw) of ~Tbm * T_i.  Tbm is `mean_pose` (a TRANSFORM record) if given, else the mean rounded to float32 as the oracle and the
    device round it.  Adds "eigenvalues" (of M, ascending) and "q", "t" (the mean before rounding)."""
    from rmcl_amd.types import TRANSFORM
    n = len(poses) if n_induction is None else min(len(poses), int(n_induction))
    P, A = poses[:n], attrs[:n]
    L = A["likelihood"]["mean"].astype(np.float64)
    L_sum = L.sum()
    L_mean = L_sum / n
    t = np.stack([P["t"][k] for k in "xyz"], 1).astype(np.float64)
    q = np.stack([P["R"][k] for k in "xyzw"], 1).astype(np.float64)
    out = {"likelihood": {"mean": L_mean, "sigma": float(np.sqrt(max((L * L).sum() / n - L_mean * L_mean, 0.0))),
                          "min": float(L.min()), "max": float(max(L.max(), 0.0))},
           "trans_bb_min": t.min(0), "trans_bb_max": t.max(0), "nparticles": n}
    w = L / L_sum
    M = (q * w[:, None]).T @ q
    ev, evec = np.linalg.eigh(M)
    qm = evec[:, -1] * (-1.0 if evec[3, -1] < 0 else 1.0)
    tm = (t * w[:, None]).sum(0)
    out["eigenvalues"], out["q"], out["t"] = ev, qm, tm
    if mean_pose is None:
        mean_pose = np.zeros((), TRANSFORM)
        for i, k in enumerate("xyzw"):
            mean_pose["R"][k] = qm[i]
        for i, k in enumerate("xyz"):
            mean_pose["t"][k] = tm[i]
    out["pose"] = mean_pose
    qb = np.array([mean_pose["R"][k] for k in "xyzw"], np.float64)
    tb = np.array([mean_pose["t"][k] for k in "xyz"], np.float64)
    qi = quat_conj(qb)                                           # ~Tbm = (~R, -(~R t)), ~R the conjugate (orc_transform_inv: no normalisation)
    ti = -quat_rotate(qi, tb)
    d = np.concatenate([quat_rotate(qi[None, :], t) + ti, euler_zyx(quat_mul(qi[None, :], q))], 1)
    out["covariance"] = (d * w[:, None]).T @ d
    return out


# ---- the residual resampler's cloud --------------------------------------------------------------------------------------------
RESIDUAL_N = 300007
RESIDUAL_SEED = 0xC0FFEE7654321
RESIDUAL_NOISE = dict(min_noise_tz=0.01, min_noise_roll=0.005, min_noise_pitch=0.005)
SCAN_TRIP = 256 * 1024          # draws one trip of k_scan_totals covers: 256 block totals of 1024 draws


def residual_case():
    """n = n_new = 300007, likelihoods uniform(0.5, 1): a share L / sum * N of 0.67 .. 1.33, so about every second draw inserts one
    copy and the sequential loop needs ~2 N draws -- more than one trip of the scan of the block totals"""
    if "residual" not in _cache:
        poses, attrs = _uniform_rp(RESIDUAL_N, 301)
        attrs["likelihood"]["mean"] = np.random.RandomState(302).uniform(0.5, 1.0, RESIDUAL_N)
        _cache["residual"] = (poses, attrs)
    return _cache["residual"]
