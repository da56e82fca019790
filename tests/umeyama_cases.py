"""Inputs of the rotation solve (rm::umeyama_transform) where it can go wrong, shared by the CPU and the GPU tests, and its
third, independent statement in float64 numpy.

Three solvers serve the MICP correction: umeyama() of devmath.h (host and device), umeyama_fast() of micp.hip (the moment-form
loops) and the oracle's orc_umeyama_transform.  umeyama_ref() below is the definition they are all measured against:

    n_meas = 0                      identity transform
    C = 0                           identity rotation
    s2 <= 1e-6 s1  (rank <= 1)      the SHORTEST rotation taking v1 to u1 = C v1 / |C v1|; for u1 = -v1 (u1 . v1 <= -1 + 1e-12) the
                                    half turn about the axis perpendicular to v1 built from the coordinate axis of v1's smallest
                                    |component| (components within 1e-6 of each other are tied: first of x, y, z)
    otherwise                       R = U diag(1, 1, sign(det U det V)) V^T
    t = model_mean - R dataset_mean

with C the float32 covariance taken in float64.  No case here has s2 / s1 inside (1e-7, 1e-5): solver and reference classify from
the same float32 numbers, and the empty band keeps the rounding of either detector out of the tests.

Everything is deterministic from fixed seeds.  crafted_cases() returns [(family, name, stats)]; scenes() the degenerate scans.
"""
import math

import numpy as np

import oracle as orc

RANK1_RATIO = 1e-6          # s2 <= RANK1_RATIO * s1: rank <= 1
BAND = (1e-7, 1e-5)         # no case has s2 / s1 inside
Q_TOL, T_TOL = 2e-6, 2e-5   # crafted cases: quaternion per component (up to sign), translation (test_abi's bars)


# ---- the reference -------------------------------------------------------------------------------------------
def cov64(stats):
    return np.asarray(stats["covariance"], dtype=np.float32).astype(np.float64).reshape(3, 3)


def singular_values(stats):
    return np.linalg.svd(cov64(stats), compute_uv=False)


def _quat_from_matrix(R):
    """unit quaternion (x, y, z, w) of a rotation matrix, float64"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    return v[:, 3] / np.linalg.norm(v[:, 3])


def _matrix_from_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def shortest_arc(v, u):
    """unit quaternion (x, y, z, w) of the rank-one rule for unit vectors v -> u"""
    d = float(np.dot(u, v))
    if d <= -1.0 + 1e-12:
        k = 0
        if abs(v[1]) < abs(v[k]) - 1e-6:
            k = 1
        if abs(v[2]) < abs(v[k]) - 1e-6:
            k = 2
        a = -v[k] * v
        a[k] += 1.0
        q = np.array([a[0], a[1], a[2], 0.0])
    else:
        c = np.cross(v, u)
        q = np.array([c[0], c[1], c[2], 1.0 + d])
    return q / np.linalg.norm(q)


def umeyama_ref(stats):
    """(quaternion xyzw, translation) in float64: the definition of the module docstring"""
    dm = np.array([stats["dataset_mean"][k] for k in "xyz"], dtype=np.float64)
    mm = np.array([stats["model_mean"][k] for k in "xyz"], dtype=np.float64)
    if int(stats["n_meas"]) == 0:
        return np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    C = cov64(stats)
    U, S, Vt = np.linalg.svd(C)
    if S[0] == 0.0:
        q = np.array([0.0, 0.0, 0.0, 1.0])
    elif S[1] <= RANK1_RATIO * S[0]:
        v = Vt[0]
        u = C @ v
        q = shortest_arc(v, u / np.linalg.norm(u))
    else:
        D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0])
        q = _quat_from_matrix(U @ D @ Vt)
    return q, mm - _matrix_from_quat(q) @ dm


def quat_of(T):
    return np.array([T["R"][k] for k in "xyzw"], dtype=np.float64)


def trans_of(T):
    return np.array([T["t"][k] for k in "xyz"], dtype=np.float64)


def rotation_angle(q):
    q = np.asarray(q, dtype=np.float64)
    return 2.0 * math.atan2(np.linalg.norm(q[:3]), abs(q[3]))


def assert_matches_ref(T, stats, what=""):
    """a solver's transform against umeyama_ref at the crafted cases' bars"""
    q, t = umeyama_ref(stats)
    qs = quat_of(T)
    assert abs(np.linalg.norm(qs) - 1.0) < 1e-6, (what, qs)
    assert min(np.abs(qs - q).max(), np.abs(qs + q).max()) < Q_TOL, (what, qs, q, cov64(stats))
    assert np.abs(trans_of(T) - t).max() < T_TOL, (what, trans_of(T), t)


def ulp_sensitivity(stats):
    """how far ONE ulp in ONE float32 covariance entry -- what another order of summation can move it by -- takes umeyama_ref: the
    largest change of the rotation's angle, the largest angle of the residual rotation, the largest change of the translation"""
    q0, t0 = umeyama_ref(stats)
    d_ang = d_res = d_t = 0.0
    for k in range(9):
        for toward in (-np.inf, np.inf):
            s = stats.copy()
            s["covariance"][k] = np.nextafter(np.float32(stats["covariance"][k]), np.float32(toward))
            q, t = umeyama_ref(s)
            if np.dot(q, q0) < 0:
                q = -q
            vec = q0[3] * q[:3] - q[3] * q0[:3] - np.cross(q0[:3], q[:3])
            d_res = max(d_res, 2.0 * math.atan2(np.linalg.norm(vec), abs(np.dot(q, q0))))
            d_ang = max(d_ang, abs(rotation_angle(q) - rotation_angle(q0)))
            d_t = max(d_t, float(np.linalg.norm(t - t0)))
    return d_ang, d_res, d_t


# ---- crafted covariances ---------------------------------------------------------------------------------------
def make_stats(C, dm=(0.3, -0.2, 0.1), mm=(1.0, 2.0, -0.5), n=100):
    s = np.zeros((), orc.CROSS_STATISTICS)
    for k, a, b in zip("xyz", dm, mm):
        s["dataset_mean"][k], s["model_mean"][k] = a, b
    s["covariance"] = np.asarray(C, np.float64).reshape(9)
    s["n_meas"] = n
    return s


def rot(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _ratio32(C):
    s = np.linalg.svd(np.asarray(C, np.float64).astype(np.float32).astype(np.float64), compute_uv=False)
    return s[1] / s[0]


def _orthonormal_pair(u):
    """two unit vectors completing the unit vector u to a right-handed basis"""
    k = int(np.argmin(np.abs(u)))
    a = np.zeros(3)
    a[k] = 1.0
    b = a - np.dot(a, u) * u
    b /= np.linalg.norm(b)
    return b, np.cross(u, b)


def _with_second(base, u, v, s1, ratio, below):
    """base + ratio s1 u2 v2^T, the size of the second term adjusted until the FLOAT32 matrix -- what the solvers see -- sits on the
    intended side of the band: s2 / s1 <= 1e-7 (below; rounding a rank-one matrix to float32 alone leaves up to 6e-8, so a
    target of 1e-12 or 1e-9 is the size of the term added, not of the result) or >= ratio (not below)"""
    u2, v2 = _orthonormal_pair(u)[0], _orthonormal_pair(v)[1]
    f = 1.0
    for _ in range(400):
        C = base + f * ratio * s1 * np.outer(u2, v2)
        r = _ratio32(C)
        if (r <= BAND[0]) if below else (r >= max(ratio, BAND[1])):
            return C
        f *= 0.98 if below else 1.02
    raise AssertionError("could not place s2 / s1 at %g" % ratio)


def general_cases():
    """test_abi's list: rotations 0 ... pi about four axes, noise-free and noisy; planar; a line; scales; random with det < 0"""
    rng = np.random.RandomState(5)
    cases = []
    for angle in (0.0, 1e-4, 0.5, math.pi / 2, math.pi - 1e-3, math.pi):
        for axis in ((1, 0, 0), (0, 0, 1), (1, 2, 3), (-1, 1, 0.1)):
            d = rng.normal(size=(60, 3)) * (2.0, 1.0, 0.5)
            m = d @ rot(axis, angle).T
            for noise in (0.0, 0.02):
                mn = m + rng.normal(size=m.shape) * noise
                cases.append(((mn - mn.mean(0)).T @ (d - d.mean(0))) / len(d))
    planar = rng.normal(size=(40, 3)) * (1.0, 1.0, 0.0)
    cases.append(((planar @ rot((0, 0, 1), 0.7).T).T @ planar) / 40)                 # rank 2
    line = np.outer(rng.normal(size=40), (1.0, 2.0, -1.0))
    cases.append((line.T @ line) / 40)                                               # rank 1
    cases += [c * s for c in cases[:6] for s in (1e-8, 1e6)]                         # scales
    cases += [rng.normal(size=(3, 3)) * (1, 1, -1) for _ in range(20)]               # arbitrary, many with det < 0
    return cases


def crafted_cases():
    """[(family, name, CrossStatistics)].  Families: general (rank 3 and test_abi's planar / line), rank1 (shortest arc), rank1_half
    (u1 = -v1: the half turn), near_rank1 (s2 / s1 of 1e-5 and 1e-3: unique), rank2 (s3 = 0 exactly), zero, empty."""
    out = []
    for i, C in enumerate(general_cases()):
        out.append(("general", "g%d" % i, make_stats(C)))
    dirs = [("x", (1.0, 0.0, 0.0)), ("y", (0.0, 1.0, 0.0)), ("z", (0.0, 0.0, 1.0)), ("d121", (1.0, 2.0, -1.0))]
    scales = (("", 1.0), ("_s1e-8", 1e-8), ("_s1e6", 1e6))
    for dname, e in dirs:
        e = np.asarray(e) / np.linalg.norm(e)
        for fam, sign in (("rank1", 1.0), ("rank1_half", -1.0)):
            for sname, scale in scales:
                s1 = 7.5 * scale
                base = sign * s1 * np.outer(e, e)
                out.append((fam, "%s%s_exact" % (dname, sname), make_stats(base)))
                for ratio in (1e-12, 1e-9, 1e-7):
                    out.append((fam, "%s%s_%g" % (dname, sname, ratio), make_stats(_with_second(base, sign * e, e, s1, ratio, True))))
    # rank one with u1 != v1: a wall seen from a pose that is off by a rotation (what the scenes produce), exact and noisy
    rng = np.random.RandomState(17)
    for i, (axis, angle) in enumerate((((0, 0, 1), 0.02), ((1, 2, 3), 0.5), ((-1, 1, 0.1), math.pi / 2), ((0.3, -1, 2), 2.5),
                                       ((0, 1, 0), math.pi - 0.01))):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        u = rot(axis, angle) @ v
        for sname, scale in scales:
            s1 = 3.25 * scale
            base = s1 * np.outer(u, v)
            out.append(("rank1", "arc%d%s_exact" % (i, sname), make_stats(base)))
            out.append(("rank1", "arc%d%s_1e-9" % (i, sname), make_stats(_with_second(base, u, v, s1, 1e-9, True))))
    for i, (axis, angle) in enumerate((((0, 0, 1), 0.02), ((1, 2, 3), 0.5), ((-1, 1, 0.1), 2.0), ((1, 0, 0), 0.0), ((0, 1, 0), 3.0))):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        u = rot(axis, angle) @ v
        u2, v2 = _orthonormal_pair(u)[0], _orthonormal_pair(v)[1]
        for ratio in (1e-5, 1e-3):
            out.append(("near_rank1", "n%d_%g" % (i, ratio), make_stats(_with_second(4.0 * np.outer(u, v), u, v, 4.0, ratio, False))))
        # rank two, s3 = 0 exactly: proper (u3 = u1 x u2 goes with v3 = v1 x v2) and reflected (u2 flipped)
        for k, s2 in enumerate((2.0, 0.01)):
            for refl, sg in (("proper", 1.0), ("reflected", -1.0)):
                out.append(("rank2", "r%d_%d_%s" % (i, k, refl), make_stats(4.0 * np.outer(u, v) + sg * s2 * np.outer(u2, v2))))
    means = [((0.3, -0.2, 0.1), (1.0, 2.0, -0.5)), ((0, 0, 0), (0, 0, 0)), ((5, 0, 0), (5.05, 0.02, 0))]
    means += [(tuple(rng.uniform(-5, 5, 3)), tuple(rng.uniform(-5, 5, 3))) for _ in range(7)]
    for i, (dm, mm) in enumerate(means):
        out.append(("zero", "z%d" % i, make_stats(np.zeros((3, 3)), dm, mm, n=1)))
        out.append(("empty", "e%d" % i, make_stats(rot((1, 2, 3), 0.5) * (i + 1.0), dm, mm, n=0)))
    return out


# ---- degenerate scenes -------------------------------------------------------------------------------------------
def _quad(p0, eu, ev):
    p0, eu, ev = (np.asarray(a, np.float64) for a in (p0, eu, ev))
    v = np.array([p0, p0 + eu, p0 + eu + ev, p0 + ev], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _join(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + np.uint32(base))
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def line_model(range_max=130.0):
    """a 2-D lidar: H = 1, W = 900, phi = 0"""
    from rmcl_amd.types import spherical_model
    f = np.float32
    return spherical_model(f(0.0), f(1.0), 1, f(-math.pi), f(2 * math.pi / 900), 900, f(0.0), f(range_max))


class Scene:
    """map (v, f), model, Tsb, Tbo, truth (base in map), Tom (estimate: odom in map), dataset + mask (measured at the truth)"""

    def __init__(self, name, mesh, model, truth, pert, keep=None, Tsb=None, Tbo=None, max_dist=1.0):
        self.name, self.v, self.f, self.model, self.max_dist = name, mesh[0], mesh[1], model, max_dist
        ident = orc.transform()
        self.Tsb = ident if Tsb is None else Tsb
        self.Tbo = ident if Tbo is None else Tbo
        self.truth = truth
        # Tom * Tbo = truth * pert
        self.Tom = orc.tmult(orc.tmult(truth, pert), orc.tinv(self.Tbo))
        self.mesh = orc.Mesh(self.v, self.f)
        self.keep = keep
        self.ds, self.mask = self.measure(self.Tsb)

    def measure(self, Tsb):
        """dataset and mask of a sensor mounted at Tsb, measured at the truth (MICPSphericalSensorCPU::unpackMessage); with `keep`,
        only that many valid measurements, taken at a fixed stride through the scan, stay in the mask"""
        meas = self.mesh.simulate_spherical(self.model, Tsb, self.truth, bvh=True)
        r = np.asarray(meas["ranges"], np.float32).reshape(-1)
        ds = (orc.spherical_directions(self.model) * r[:, None]).astype(np.float32)
        mask = np.where((r < np.float32(self.model.range.min)) | (r > np.float32(self.model.range.max)), 0, 1).astype(np.uint8)
        if self.keep is not None:
            valid = np.flatnonzero(mask)[7::131][:self.keep]
            mask = np.zeros_like(mask)
            mask[valid] = 1
        return ds, mask

    def oracle_correct_once(self, n_iter=4, refind=False):
        import oracle_micp as om
        return om.correct_once(self.mesh, self.model, self.Tsb, self.Tbo, self.Tom, self.ds, self.mask, n_iter, self.max_dist,
                               refind=refind)


# Floors of the scene comparisons: tests/test_gpu_reduce.py _transform_close's own (2e-7 rad, 1e-6 m) unless a scene is listed here.
# A listed scene missed them on the device, and its floor is 4 x the reference's own sensitivity to ONE ulp in one covariance entry
# (ulp_sensitivity of the first iteration's statistics; one ulp is what another order of summation moves an entry by, x 4 for the
# four iterations) -- measured, not chosen: tests/test_umeyama_cases_cpu.py recomputes it; profiles/umeyama_degenerate.txt.
#   two sensors on cube_3 (3 + 3 correspondences, the second sensor's merged at weight 0.5 -> count 1): s = 7.18, 0.52, 0.093;
#   one ulp moves the angle by 2.04e-7 rad and t by 1.26e-6 m; the host loop was off by 1.15e-6 rad and 5.2e-6 m
TWO_SENSOR_SENSITIVITY = {"cube_3": (2.04e-7, 1.26e-6)}   # scene -> (rad, m) per ulp
TWO_SENSOR_FLOORS = {k: (4.0 * r, 4.0 * t) for k, (r, t) in TWO_SENSOR_SENSITIVITY.items()}


def two_sensor_spec(sc):
    """the scene's sensor and a second one of the same model mounted 1.5 m beside it, merged at half weight:
    [(model, Tsb, Tbo, dataset, mask, max_dist, adaptive_min, merge_weight_multiplier)] for oracle_micp.correct_once_multi"""
    spec = []
    for Tsb, w in ((sc.Tsb, 1.0), (orc.tmult(sc.Tsb, orc.transform_from_rpy((0.0, 1.5, 0.0), (0, 0, 0))), 0.5)):
        ds, mask = sc.measure(Tsb)
        spec.append((sc.model, Tsb, sc.Tbo, ds, mask, sc.max_dist, sc.max_dist, w))
    return spec


_SCENES = None


def scenes():
    """name -> Scene.  Maps of 2..12 triangles, at most 14 400 rays."""
    global _SCENES
    if _SCENES is not None:
        return _SCENES
    from rmcl_amd import synthetic as syn
    rpy = orc.transform_from_rpy
    S = {}
    S["floor"] = Scene("floor", _quad((-40, -40, 0), (80, 0, 0), (0, 80, 0)), syn.model_vlp16_900(0.0),
                       rpy((0, 0, 1.5), (0, 0, 0)), rpy((0.0, 0.0, 0.05), (0.01, -0.015, 0.02)))
    S["corridor2d"] = Scene("corridor2d", _join(_quad((-20, 3, -1), (40, 0, 0), (0, 0, 2)), _quad((-20, -3, -1), (0, 0, 2), (40, 0, 0))),
                            line_model(), rpy((0, 0, 0), (0, 0, 0)), rpy((0.05, 0.02, 0.0), (0, 0, 0.018)))
    wall = _quad((5, -40, -30), (0, 0, 60), (0, 80, 0))
    S["wall_line"] = Scene("wall_line", wall, line_model(), rpy((0, 0, 0), (0, 0, 0)), rpy((0.05, 0.02, 0.0), (0, 0, 0.02)))
    # the same wall through a sensor that is tilted against it (pitch of the true pose), an estimate that is off in all three
    # angles, a mount and an odometry stamp that are not the identity.  Mount and stamp are translations: the oracle turns the
    # covariance into the odometry frame in float32, and a rotation there would leave 1e-8 of rounding in s2 -- still of rank one
    # for every solver, but no longer the exactly singular matrix this scene is here for
    S["wall_line_tilt"] = Scene("wall_line_tilt", wall, line_model(), rpy((0, 0, 0), (0, 0.2, 0)), rpy((0.05, 0.02, 0.0), (0.03, -0.02, 0.02)),
                                Tsb=rpy((0.2, -0.1, 0.3), (0, 0, 0)), Tbo=rpy((0.1, 0.3, 0.0), (0, 0, 0)))
    cube = syn.cube_room(grid=1)
    for k in range(4):
        S["cube_%d" % k] = Scene("cube_%d" % k, cube, syn.model_c1(), syn.pose_c2_truth(), syn.pose_c2_perturbation(), keep=k,
                                 Tsb=syn.tsb_offset())
    S["nothing"] = Scene("nothing", _quad((500, -40, -30), (0, 0, 60), (0, 80, 0)), line_model(),
                         rpy((0, 0, 0), (0, 0, 0)), rpy((0.05, 0.02, 0.0), (0, 0, 0.02)))
    _SCENES = S
    return S
