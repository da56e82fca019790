"""Host restatement (numpy only) of the sampled odometry model of the motion update (include/rmclhip.h, MOTION NOISE) -- what
rmclhip_motion_noise_sigma_host, pf_random.hip.h: motion_noise_compose and k_pf_motion<., ., true> compute, operation by operation in
their order (transcendentals in double, rounded to float, on both sides: nearly always the same bits).

    sigma_host        the six standard deviations of a step, in Python doubles
    noise_words       A, B of global particle g: philox((g, step, 0, 2), seed), philox((g, step, 1, 2), seed) -- stream 2
    noise_transforms  N_i = {EulerAngles(z3 s3, z4 s4, z5 s5), (z0 s0, z1 s1, z2 s2)}
    xmul              float32 a * b of TRANSFORM arrays in devmath.h's operation order
    motion_update     the whole call without the surface constraint: (poses, attrs), the kill by oracle.Mesh.intersect on the segment
    kill_flags        the kill alone, on given old and new positions (the device's, in the GPU tests)
    exclusions        the particles a last-bit difference of the pose may flip: endpoint within 1e-3 m of a face, or segment length
                      within 1e-6 of the 1e-5 moving threshold
and the wall scene the CPU and the GPU tests share (wall_scene).
"""
import math

import numpy as np

import particle_init_ref as pref
from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM

F = np.float32
SEED = 0x5EED0D0123456
FIELDS = ("alpha_trans_trans", "alpha_trans_rot", "alpha_rot_trans", "alpha_rot_rot")
MOVING = 0.00001          # the kernel's threshold on the segment length
NEAR_FACE = 1e-3          # exclusions: endpoint this close to a face
NEAR_MOVING = 1e-6        # ... or segment length this close to MOVING


def default_params():
    return {k: [0.2, 0.2, 0.2] for k in FIELDS}


def sigma_host(params, T):
    """params: dict of four float triples; T: one TRANSFORM -> [6] float32.  ValueError where the library returns RMCLHIP_ERR_INVALID"""
    a = {k: [float(F(x)) for x in params[k]] for k in FIELDS}
    for k in FIELDS:
        if len(a[k]) != 3 or not all(math.isfinite(x) and x >= 0.0 for x in a[k]):
            raise ValueError("every alpha must be finite and >= 0")
    T = np.asarray(T, dtype=TRANSFORM).reshape(())
    q = [float(T["R"][k]) for k in "xyzw"]
    t = [float(T["t"][k]) for k in "xyz"]
    if not all(math.isfinite(x) for x in q + t):
        raise ValueError("non-finite step")
    s_t = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    s_r = 2.0 * math.atan2(math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]), abs(q[3]))
    out = np.zeros(6, dtype=F)
    for k in range(3):
        tt, tr = a["alpha_trans_trans"][k] * s_t, a["alpha_trans_rot"][k] * s_r
        rt, rr = a["alpha_rot_trans"][k] * s_t, a["alpha_rot_rot"][k] * s_r
        out[k] = F(math.sqrt(tt * tt + tr * tr))
        out[3 + k] = F(math.sqrt(rt * rt + rr * rr))
    return out


def noise_words(first, count, seed, step):
    """[count, 6] uint32: A0..A3, B0, B1 of global particles first .. first+count-1"""
    g = (np.arange(count, dtype=np.uint64) + np.uint64(first)).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    ctr = np.zeros((count, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 3] = g, np.uint32(step), 2
    a = pref.philox4x32_10(ctr, key)
    ctr[:, 2] = 1
    b = pref.philox4x32_10(ctr, key)
    return np.concatenate([a, b[:, :2]], axis=1)


def noise_components(first, count, sigma, seed, step):
    """[count, 6] float32: z_k * sigma_k -- N's translation and its three Euler angles"""
    z = pref.gaussians(noise_words(first, count, seed, step))
    return z * np.asarray(sigma, dtype=F).reshape(1, 6)


def _R(p):
    return tuple(np.ascontiguousarray(p["R"][k]) for k in "xyzw")


def _t(p):
    return tuple(np.ascontiguousarray(p["t"][k]) for k in "xyz")


def xmul(a, b):
    """a * b, TRANSFORM arrays (either may be a single record): t = qrot(a.R, b.t) + a.t, R = qmul(a.R, b.R), stamp = a's"""
    a, b = np.atleast_1d(np.asarray(a, dtype=TRANSFORM)), np.atleast_1d(np.asarray(b, dtype=TRANSFORM))
    n = max(len(a), len(b))
    qa, qb = [np.broadcast_to(c, n) for c in _R(a)], [np.broadcast_to(c, n) for c in _R(b)]
    ta, tb = [np.broadcast_to(c, n) for c in _t(a)], [np.broadcast_to(c, n) for c in _t(b)]
    qi = (-qa[0], -qa[1], -qa[2], qa[3])
    PT = pref._qmul(pref._qmul(qa, (tb[0], tb[1], tb[2], np.zeros(n, dtype=F))), qi)
    out = np.zeros(n, dtype=TRANSFORM)
    for k, c in zip("xyzw", pref._qmul(qa, qb)):
        out["R"][k] = c
    for i, k in enumerate("xyz"):
        out["t"][k] = PT[i] + ta[i]
    out["stamp"] = np.broadcast_to(a["stamp"], n)
    return out


def xinv(a):
    a = np.atleast_1d(np.asarray(a, dtype=TRANSFORM))
    n = len(a)
    q = _R(a)
    qi = (-q[0], -q[1], -q[2], q[3])
    t = _t(a)
    PT = pref._qmul(pref._qmul(qi, (t[0], t[1], t[2], np.zeros(n, dtype=F))), q)
    out = np.zeros(n, dtype=TRANSFORM)
    for k, c in zip("xyzw", qi):
        out["R"][k] = c
    for i, k in enumerate("xyz"):
        out["t"][k] = -PT[i]
    out["stamp"] = a["stamp"]
    return out


def noise_transforms(first, count, sigma, seed, step):
    c = noise_components(first, count, sigma, seed, step)
    N = np.zeros(count, dtype=TRANSFORM)
    for k, q in zip("xyzw", pref.euler_to_quat(c[:, 3], c[:, 4], c[:, 5])):
        N["R"][k] = q
    for i, k in enumerate("xyz"):
        N["t"][k] = c[:, i]
    return N


def _q64(p):
    return np.stack([p["R"][k].astype(np.float64) for k in "xyzw"], axis=1)


def _t64(p):
    return np.stack([p["t"][k].astype(np.float64) for k in "xyz"], axis=1)


def _qmul64(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=1)


def relative_f64(moved, new):
    """inv(moved) * new in float64 from the float32 records: (q [n, 4] in x y z w order, t [n, 3] in the body frame of `moved`)"""
    qm = _q64(moved)
    qm = qm / np.linalg.norm(qm, axis=1, keepdims=True)
    qi = qm * np.array([-1.0, -1.0, -1.0, 1.0])
    d = _t64(new) - _t64(moved)
    P = np.concatenate([d, np.zeros((len(d), 1))], axis=1)
    return _qmul64(qi, _q64(new)), _qmul64(_qmul64(qi, P), qm)[:, :3]


def euler_f64(q):
    x, y, z, w = q.T
    return np.stack([np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), np.arcsin(np.clip(2 * (w * y - z * x), -1, 1)),
                     np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))], axis=1)


def components_f64(N):
    """[n, 6] float64: the translation of the TRANSFORM records N and the ZYX Euler angles of their rotations"""
    return np.concatenate([_t64(N), euler_f64(_q64(N))], axis=1)


def relative_components_f64(moved, new):
    q, t = relative_f64(moved, new)
    return np.concatenate([t, euler_f64(q)], axis=1)


def segments(t_old, t_new):
    """the kernel's segment of every particle: (direction [n, 3], length [n], moving [n]) in float32"""
    vec = [t_new[k] - t_old[k] for k in "xyz"]
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]).astype(F)
        moving = ~(length.astype(np.float64) < MOVING)
        d = np.stack([vec[0] / length, vec[1] / length, vec[2] / length], axis=1).astype(F)
    return d, length, moving


def kill_flags(mesh, t_old, t_new, bvh=True):
    """[n] bool: the segment old -> new crosses the mesh (oracle.Mesh.intersect on (0, length]); t_old / t_new: the "t" fields"""
    d, length, moving = segments(t_old, t_new)
    O = np.stack([t_old[k] for k in "xyz"], axis=1)
    out = np.zeros(len(length), dtype=bool)
    for i in np.nonzero(moving)[0]:
        out[i] = mesh.intersect(O[i], d[i], 0.0, float(length[i]), bvh=bvh)[0]
    return out


def exclusions(mesh, t_old, t_new):
    """[n] bool: the noisy endpoint lies within NEAR_FACE of a face, or the segment length within NEAR_MOVING of the threshold"""
    _, length, _ = segments(t_old, t_new)
    P = np.stack([t_new[k] for k in "xyz"], axis=1)
    ident = np.zeros((), dtype=TRANSFORM)
    ident["R"]["w"] = 1.0
    near = mesh.cpc_find(ident, ident, P, NEAR_FACE, bvh=True)["hits"].astype(bool)
    return near | (np.abs(length.astype(np.float64) - MOVING) <= NEAR_MOVING)


def forget(attrs, rate):
    a = np.array(attrs, dtype=PARTICLE_ATTRIBUTES, copy=True)
    n0 = a["likelihood"]["n_meas"].astype(np.float64)
    a["likelihood"]["n_meas"] = (n0 - float(rate) * n0).astype(np.uint32)
    return a


def kill(attrs, flags, max_n_meas=10000):
    attrs["likelihood"]["mean"][flags] = 0.0
    attrs["likelihood"]["sigma"][flags] = 0.0
    attrs["likelihood"]["n_meas"][flags] = max_n_meas
    return attrs


def motion_update(mesh, poses, attrs, T, rate, sigma, seed, step, first=0, collision=True, max_n_meas=10000, bvh=True):
    """rmclhip_pf_motion_update_noisy without the surface constraint: (poses_new, attrs_new, killed)"""
    poses = np.asarray(poses, dtype=TRANSFORM)
    moved = xmul(poses, T)
    new = xmul(moved, noise_transforms(first, len(poses), sigma, seed, step)) if np.any(np.asarray(sigma) != 0) else moved
    a = forget(attrs, rate)
    flags = kill_flags(mesh, poses["t"], new["t"], bvh=bvh) if collision else np.zeros(len(poses), dtype=bool)
    return new, kill(a, flags, max_n_meas), flags


def randomised_attrs(n, seed):
    rng = np.random.RandomState(seed)
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["n_meas"] = rng.randint(0, 10001, n)
    a["likelihood"]["mean"] = rng.uniform(0.1, 1, n)
    a["likelihood"]["sigma"] = rng.uniform(0, 0.1, n)
    a["state_sigma"] = rng.uniform(0, 1, (n, 6))
    return a


# ---- the wall scene: the cube room (walls at +-5 m), a cloud 0.1 .. 0.7 m in front of the +x wall that heads towards it within 0.5 rad,
# a 0.4 m step forward and sigmas of 0.25 m: without noise the particles nearer than about 0.4 m cross the wall, with it either may ----
WALL_STEP_T = (0.4, 0.0, 0.0)
WALL_SIGMA = np.array([0.25, 0.25, 0.0, 0.0, 0.0, 0.1], dtype=F)
WALL_STEP = 3


def wall_step():
    T = np.zeros((), dtype=TRANSFORM)
    T["R"]["w"] = 1.0
    T["t"]["x"], T["t"]["y"], T["t"]["z"] = WALL_STEP_T
    T["stamp"] = 5
    return T


def wall_cloud(n, seed=17):
    rng = np.random.RandomState(seed)
    p = np.zeros(n, dtype=TRANSFORM)
    yaw = rng.uniform(-0.5, 0.5, n).astype(F)
    zero = np.zeros(n, dtype=F)
    for k, q in zip("xyzw", pref.euler_to_quat(zero, zero, yaw)):
        p["R"][k] = q
    p["t"]["x"] = rng.uniform(4.3, 4.9, n)
    p["t"]["y"] = rng.uniform(-4.0, 4.0, n)
    p["t"]["z"] = rng.uniform(-1.0, 1.0, n)
    p["stamp"] = rng.randint(0, 1000, n)
    return p, randomised_attrs(n, seed + 1)
