"""Inputs of the surface constraint's edge tests (include/rmclhip.h, "surface-constrained motion"): hand-built maps of two to six
triangles and the clouds that reach what random clouds on scanned rooms do not -- the ends of the hit interval, min_up_cos at equality,
the upside-down branch of step 5 and its threshold, every attitude, non-unit quaternions, a map 5 km out, ragged and dead waves, the
kerb.  Everything is built from fixed seeds.  tests/test_surface_cases_cpu.py proves with the restatement alone that every case reaches
what it is for; tests/test_gpu_surface_edges.py holds the kernels to the restatement on them, byte for byte.  Not a test module.

A case is a dict: map (a name of MAPS), p (surface_ref.params), poses, attrs, and where the answer is known in closed form want (the
class per particle, -1: no claim).
"""
import math

import numpy as np

import surface_ref as sr
from rmcl_amd import types as T

F = np.float32
PROBE = dict(height=0.1, probe_up=0.5, probe_down=1.0, min_up_cos=0.7)     # the probe of the cube room and of most hand maps
OFFSET = (5000.0, -5000.0, 300.0)
ATTITUDE_SEED = 5


# ---- mesh helpers (shared with tests/test_surface_cases_cpu.py) ----------------------------------------------------------------------
def quad(p00, p10, p11, p01):
    """two triangles of a quadrilateral, wound p00 -> p10 -> p11 -> p01"""
    v = np.array([p00, p10, p11, p01], F)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def join(*parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + np.uint32(base))
        base += len(v)
    return np.concatenate(vs).astype(F), np.concatenate(fs).astype(np.uint32)


def plane_z0(down=False):
    """the square [-4, 4]^2 at z = 0 (legs of 8: the geometric normal is (0, 0, +-64), every product with it exact)"""
    if down:
        return quad((-4, -4, 0), (-4, 4, 0), (4, 4, 0), (4, -4, 0))
    return quad((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))


def one(ra_types, q=(0, 0, 0, 1), t=(0, 0, 0)):
    poses = np.zeros(1, ra_types.TRANSFORM)
    sr.set_pose(poses[0], np.array(q, F), np.array(t, F))
    attrs = np.zeros(1, ra_types.PARTICLE_ATTRIBUTES)
    attrs["likelihood"]["mean"], attrs["likelihood"]["n_meas"] = 1.0, 7
    attrs["state_sigma"] = np.arange(6, dtype=F)
    return poses, attrs


# ---- the maps ------------------------------------------------------------------------------------------------------------------------
def ramp30():
    k = math.tan(math.radians(30.0))
    return quad((-4, -4, -4 * k), (4, -4, 4 * k), (4, 4, 4 * k), (-4, 4, -4 * k))


def face80():
    k = math.tan(math.radians(80.0))
    return quad((-1, -4, -k), (1, -4, k), (1, 4, k), (-1, 4, -k))


def wall_x1():
    return quad((1, -4, -4), (1, 4, -4), (1, 4, 4), (1, -4, 4))


def hole():
    return join(quad((-4, -4, 0), (-1, -4, 0), (-1, 4, 0), (-4, 4, 0)), quad((1, -4, 0), (4, -4, 0), (4, 4, 0), (1, 4, 0)))


def kerb():
    """floor z = 0 for x < 1, top z = 0.3 for x > 1, the riser x = 1 between them"""
    return join(quad((-4, -4, 0), (1, -4, 0), (1, 4, 0), (-4, 4, 0)), quad((1, -4, 0.3), (4, -4, 0.3), (4, 4, 0.3), (1, 4, 0.3)),
                quad((1, -4, 0), (1, 4, 0), (1, 4, 0.3), (1, -4, 0.3)))


def stack():
    """two level squares within one probe's reach: z = 0 wound upwards (faces 0, 1), z = 0.75 wound downwards (faces 2, 3)"""
    v, f = plane_z0(down=True)
    return join(plane_z0(), (v + np.array([0, 0, 0.75], F), f))


def ramp30_far():
    v, f = ramp30()
    return (v + np.array(OFFSET, F)).astype(F), f


MAPS = dict(plane=plane_z0, plane_down=lambda: plane_z0(down=True), ramp30=ramp30, face80=face80, wall_x1=wall_x1, hole=hole, kerb=kerb,
            stack=stack, ramp30_far=ramp30_far)

_meshes = {}


def oracle_mesh(name):
    """(oracle mesh, its record normals) of a hand map, built once"""
    if name not in _meshes:
        import oracle as orc
        m = orc.Mesh(*MAPS[name]())
        _meshes[name] = (m, m.face_normals())
    return _meshes[name]


# ---- cloud helpers -------------------------------------------------------------------------------------------------------------------
def cloud(quats, ts, seed):
    """poses from quaternions (x, y, z, w) and positions, rounded to float32; attributes drawn from `seed`"""
    quats, ts = np.asarray(quats, np.float64).reshape(-1, 4), np.asarray(ts, np.float64).reshape(-1, 3)
    n = len(ts)
    assert len(quats) == n
    poses = np.zeros(n, T.TRANSFORM)
    for j, k in enumerate("xyzw"):
        poses["R"][k] = quats[:, j]
    for j, k in enumerate("xyz"):
        poses["t"][k] = ts[:, j]
    rng = np.random.RandomState(seed)
    attrs = np.zeros(n, T.PARTICLE_ATTRIBUTES)
    attrs["likelihood"]["n_meas"] = rng.randint(0, 10001, n)
    attrs["likelihood"]["mean"] = rng.uniform(0.1, 1, n)
    attrs["likelihood"]["sigma"] = rng.uniform(0, 0.1, n)
    attrs["state_sigma"] = rng.uniform(0, 1, (n, 6))
    return poses, attrs


def pose_arrays(poses):
    """(quaternions [n, 4], positions [n, 3]) of a pose array"""
    return (np.column_stack([poses["R"][k] for k in "xyzw"]).astype(np.float64), np.column_stack([poses["t"][k] for k in "xyz"]).astype(np.float64))


def case(map_name, p, poses_attrs, want=None, note=""):
    poses, attrs = poses_attrs
    want = np.full(len(poses), -1, np.int32) if want is None else np.asarray(want, np.int32)
    assert len(want) == len(poses)
    return dict(map=map_name, p=p, poses=poses, attrs=attrs, want=want, note=note)


def rpy_quats(rng, n, tilt):
    return [T.euler_to_quat(rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-math.pi, math.pi)) for _ in range(n)]


def next_up(x):
    return np.nextafter(F(x), F(np.inf))


def next_down(x):
    return np.nextafter(F(x), F(-np.inf))


IDENT = (0.0, 0.0, 0.0, 1.0)
# (x, y) of the interval cloud: inside a triangle, on the shared diagonal, on the square's edge and on its corner
INTERVAL_XY = ((0.3, -1.2), (1.5, 1.5), (4.0, 0.25), (-4.0, -4.0), (0.0, 0.0))


def interval_cloud(map_name="plane"):
    """the ends of the hit interval (0, tfar] on a level plane at z = 0, axis 0: t_hit == O.z == (t.z - height) + probe_up, every
    operation exact for the values below.  Groups of [below, at, above] per (x, y)."""
    S, M = sr.SNAP, sr.MISS
    out = []

    def group(p, zs, want, note):
        qs, ts, ws = [], [], []
        for x, y in INTERVAL_XY:
            for z, w in zip(zs, want):
                qs.append(IDENT)
                ts.append((x, y, float(z)))
                ws.append(w)
        out.append(case(map_name, p, cloud(qs, ts, 31 + len(out)), ws, note))

    p = sr.params(height=0.25, probe_up=0.5, probe_down=1.0)
    group(p, (next_down(1.25), F(1.25), next_up(1.25)), (S, S, M), "t_hit == tfar")
    # t.z = -0.25 gives c.z = -0.5 and O.z = 0.  Its float32 neighbours give c.z = -0.5 - 2^-25 and -0.5 + 2^-26, ties that round back
    # to -0.5: t_hit == 0 again.  The nearest origins off the plane are -0.25 - 2^-24 (O.z = -2^-24, below) and -0.25 + 2^-25 (O.z = 2^-25)
    group(p, (F(-0.3), F(-0.25) - F(2.0 ** -24), next_down(-0.25), F(-0.25), next_up(-0.25), F(-0.25) + F(2.0 ** -25)), (M, M, M, M, M, S),
          "t_hit == 0")
    group(sr.params(height=0.25, probe_up=0.0, probe_down=0.0), (F(0.25), F(0.5)), (M, M), "no length: on the plane and above it")
    group(sr.params(height=0.25, probe_up=0.0, probe_down=1.0), (next_down(0.25), F(0.25), next_up(0.25), F(1.25), next_up(1.25)),
          (M, M, S, S, M), "probe_up == 0: a contact point exactly on the plane has t_hit == 0")
    group(sr.params(height=0.0, probe_up=0.5, probe_down=1.0), (next_down(-0.5), F(-0.5), next_up(-0.5), F(0.0), F(1.0), next_up(1.0)),
          (M, M, S, S, S, M), "height == 0")
    group(sr.params(height=0.0, probe_up=0.0, probe_down=1.0), (F(0.0), F(2.0 ** -140), F(1.0), next_up(1.0)), (M, S, S, M),
          "height == probe_up == 0")
    return out


def face_d(map_name, pose, axis, probe=PROBE):
    """the d of step 3 as the restatement computes it for the face this pose's probe hits (after the flip)"""
    mesh, normals = oracle_mesh(map_name)
    R, t = sr.pose_Rt(pose)
    cls, a, O, th, n, face, flipped = sr.probe_one(mesh, normals, R, t, sr.params(axis=axis, **dict(probe, min_up_cos=0.0)), bvh=False)
    assert cls == sr.SNAP
    return F((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2])


def threshold_cloud():
    """min_up_cos at exactly the d of the face, one float either side of it, at 0 and at 1.  The rule is !(d >= min_up_cos)."""
    S, X = sr.SNAP, sr.STEEP
    k = math.tan(math.radians(30.0))
    out = []
    ramp_pose = cloud([IDENT], [(0.5, 0.25, 0.5 * k + 0.2)], 41)
    tilted = cloud([T.euler_to_quat(0.15, -0.1, 0.8)], [(-1.3, 0.25, -1.3 * k + 0.2)], 42)
    for axis, pa in ((0, ramp_pose), (1, ramp_pose), (1, tilted)):
        d = face_d("ramp30", pa[0][0], axis)
        assert F(0.7) < d < F(1.0)
        for muc, want in ((next_down(d), S), (d, S), (next_up(d), X)):
            for align in (0, 1):
                out.append(case("ramp30", sr.params(axis=axis, align=align, **dict(PROBE, min_up_cos=muc)), pa, [want], "ramp30 d = %r" % float(d)))
    flat = cloud([IDENT], [(0.3, -1.2, 0.77)], 43)
    assert face_d("plane", flat[0][0], 0) == F(1.0)
    for muc in (next_down(1.0), F(1.0)):
        out.append(case("plane", sr.params(axis=0, align=1, **dict(PROBE, min_up_cos=muc)), flat, [S], "plane d == 1"))
    out.append(case("ramp30", sr.params(axis=0, align=1, **dict(PROBE, min_up_cos=1.0)), ramp_pose, [X], "min_up_cos == 1 on a ramp"))
    # min_up_cos == 0: whatever is hit snaps -- the wall x = 1 under the body-axis ray of a particle pitched by 30 degrees
    pitched = cloud([(0, math.sin(math.radians(-15.0)), 0, math.cos(math.radians(-15.0)))], [(0.9, 0.0, 0.0)], 44)
    wall = dict(height=0.0, probe_up=0.5, probe_down=1.0)
    for align in (0, 1):
        out.append(case("wall_x1", sr.params(axis=1, align=align, min_up_cos=0.0, **wall), pitched, [S], "min_up_cos == 0 on a wall"))
    d = face_d("wall_x1", pitched[0][0], 1, wall)
    assert abs(float(d) - 0.5) < 1e-6
    for muc, want in ((d, S), (next_up(d), X)):
        out.append(case("wall_x1", sr.params(axis=1, align=1, min_up_cos=muc, **wall), pitched, [want], "wall d = %r" % float(d)))
    return out


# ---- the upside-down branch of step 5 --------------------------------------------------------------------------------------------------
def align_w(R, n=(0, 0, 1)):
    """the w of step 5 for a body rotated by R under the (flipped) normal n, in the restatement's arithmetic"""
    zb = sr.qrot(np.asarray(R, F), (0, 0, 1))
    n = np.asarray(n, F)
    return F(1) + ((zb[0] * n[0] + zb[1] * n[1]) + zb[2] * n[2])


def about_x(eps):
    """the rotation about x by pi - eps, computed in double and rounded to float32"""
    h = (math.pi - eps) / 2.0
    return np.array([math.sin(h), 0.0, 0.0, math.cos(h)], F)


def _about_x_from_w(c):
    """the float32 rotation about x whose w component is the float32 c (a unit quaternion to rounding)"""
    c = F(c)
    return np.array([F(math.sqrt(1.0 - float(c) * float(c))), 0.0, 0.0, c], F)


def threshold_rotations():
    """the two rotations about x by nearly pi, ADJACENT in float32 (their w components are neighbouring floats), between which the
    restatement's branch w < 1e-6 flips: bisection over the bit pattern of the w component between eps = 1.4142e-3 (taken) and
    eps = 1.5e-3 (not taken).  Returns (taken, not_taken)."""
    lo, hi = about_x(1.4142e-3)[3], about_x(1.5e-3)[3]
    assert align_w(_about_x_from_w(lo)) < F(1e-6) and not align_w(_about_x_from_w(hi)) < F(1e-6)
    lo, hi = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    assert lo < hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if align_w(_about_x_from_w(np.uint32(mid).view(F))) < F(1e-6):
            lo = mid
        else:
            hi = mid
    return _about_x_from_w(np.uint32(lo).view(F)), _about_x_from_w(np.uint32(hi).view(F))


def yaw_quat(deg):
    h = math.radians(deg) / 2.0
    return np.array([0, 0, math.sin(h), math.cos(h)], F)


N_HALF_TURNS = 4
UPSIDE_EPS = (0.0, 2e-4, 1.4142e-3, 1.5e-3, 2e-3, 1e-2)


def upside_down_quats():
    """[x half turn, y half turn, x after a yaw of 90 deg, x after a yaw of 37 deg] + the sweep about x by pi - eps + the two adjacent
    rotations either side of the threshold"""
    half_x = np.array([1, 0, 0, 0], F)
    qs = [half_x, np.array([0, 1, 0, 0], F), sr.qmul(yaw_quat(90.0), half_x), sr.qmul(yaw_quat(37.0), half_x)]
    qs += [about_x(e) for e in UPSIDE_EPS]
    qs += list(threshold_rotations())
    return qs


def upside_down_cloud(map_name="plane"):
    """align = 1, axis 0 on a level plane: the particle at index k has rotation upside_down_quats()[k]; the last two are the threshold
    pair (taken, not taken).  The same cloud runs on plane_down, where the flip of step 3 comes first."""
    qs = upside_down_quats()
    rng = np.random.RandomState(47)
    ts = np.column_stack([rng.uniform(-3.5, 3.5, len(qs)), rng.uniform(-3.5, 3.5, len(qs)), rng.uniform(0.0, 0.6, len(qs))])
    ts[0] = (0.5, 0.5, 0.3)
    return case(map_name, sr.params(axis=0, align=1, **PROBE), cloud(qs, ts, 48), [sr.SNAP] * len(qs), "upside down")


# ---- every attitude ------------------------------------------------------------------------------------------------------------------
def attitude_cloud(n=1025, seed=ATTITUDE_SEED):
    """uniformly random unit quaternions, positions uniform in the cube room's interior (+-4.9)"""
    rng = np.random.RandomState(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    return cloud(q, rng.uniform(-4.9, 4.9, (n, 3)), seed + 1)


# ---- non-unit quaternions --------------------------------------------------------------------------------------------------------------
NONUNIT_SCALES = (0.5, 2.0, 1.0 + 1e-3, 1.0 - 1e-3, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23)


def nonunit_base():
    """{map: (quaternions, positions)}: the poses of the plane's and the ramp's closed-form tests, and two tilted ones on the ramp"""
    k = math.tan(math.radians(30.0))
    q = np.array([0.1, -0.05, 0.3, 0.94], np.float64)
    q = q / np.linalg.norm(q)
    plane = ([q] * 3, [(0.3, -1.2, 0.77), (-3.9, 3.9, -0.2), (0.0, 0.0, 0.25)])
    xs = (0.5, 0.25, 1.0, -1.3, 2.0)
    ramp = ([IDENT] * 5 + [T.euler_to_quat(0.1, -0.2, 0.5), T.euler_to_quat(-0.15, 0.1, -2.0)],
            [(x, 0.25, x * k + 0.2) for x in xs] + [(0.7, -1.0, 0.7 * k + 0.15), (-2.0, 2.0, -2.0 * k + 0.3)])
    return dict(plane=plane, ramp30=ramp)


def nonunit_cloud():
    """the motion update never renormalises: a = R * (0, 0, 1) is then no unit vector, and D, t_hit and tfar are in its units.  One case
    per (map, axis, align); the particles are scale-major: index = i_scale * n_base + i_pose."""
    out = []
    for name, (qs, ts) in nonunit_base().items():
        quats = np.concatenate([np.asarray(qs, np.float64) * s for s in NONUNIT_SCALES])
        pos = np.concatenate([np.asarray(ts, np.float64)] * len(NONUNIT_SCALES))
        pa = cloud(quats, pos, 53)
        for axis in (0, 1):
            for align in (0, 1):
                out.append(case(name, sr.params(axis=axis, align=align, **PROBE), pa, None, "non-unit, %d poses per scale" % len(ts)))
    return out


# ---- a map five kilometres out -------------------------------------------------------------------------------------------------------
FAR_SEED = 59


def far_cloud(n=257, seed=FAR_SEED):
    """(near, far): poses on and around ramp30 -- x and y within +-4.5 of its centre (the ramp ends at +-4), z within +-0.6 of the
    surface, roll and pitch +-0.3 -- and the same poses moved by OFFSET onto ramp30_far; the same attributes"""
    rng = np.random.RandomState(seed)
    k = math.tan(math.radians(30.0))
    xy = rng.uniform(-4.5, 4.5, (n, 2))
    z = xy[:, 0] * k + rng.uniform(-0.6, 0.6, n)
    qs = rpy_quats(rng, n, 0.3)
    local = np.column_stack([xy, z])
    near = cloud(qs, local, seed + 1)
    far = cloud(qs, local + np.array(OFFSET), seed + 1)
    return near, far


# ---- ragged and dead waves -----------------------------------------------------------------------------------------------------------
WAVE_SEED = 61
WAVE_COUNTS = (63, 64, 65, 129)


def wave_base(n=192, seed=WAVE_SEED):
    """the attitude cloud's positions in x and y, z around the reach of the cube room's floor (z = -5), roll and pitch
    +-0.2: most snap, some start below the floor and some too high above it"""
    rng = np.random.RandomState(seed)
    ts = np.column_stack([rng.uniform(-4.9, 4.9, n), rng.uniform(-4.9, 4.9, n), rng.uniform(-5.5, -3.6, n)])
    return cloud(rpy_quats(rng, n, 0.2), ts, seed + 1)


def _kill_pose(poses, i, j):
    """make pose i non-finite, pattern j: NaN and +-inf in t and in R"""
    grp, k, val = (("t", "x", np.nan), ("t", "y", np.inf), ("t", "z", -np.inf), ("R", "x", np.nan), ("R", "y", np.inf), ("R", "z", -np.inf),
                   ("R", "w", np.nan), ("R", "w", np.inf))[j % 8]
    poses[grp][k][i] = val
    if j % 16 >= 8:      # ... and more than one field
        poses["t"]["z"][i] = np.nan
        poses["R"]["x"][i] = -np.inf


def wave_clouds():
    """{name: (poses, attrs, dead)}: prefixes of wave_base at the counts around one wave; "dead_middle": 192 particles whose wave 1
    (indices 64..127) is entirely non-finite; "one_live": 128 particles whose wave 0 has one finite pose, at lane 37.  dead: bool mask."""
    bp, ba = wave_base()
    out = {"n%d" % n: (bp[:n].copy(), ba[:n].copy(), np.zeros(n, bool)) for n in WAVE_COUNTS}
    p = bp.copy()
    dead = np.zeros(192, bool)
    dead[64:128] = True
    for i in range(64, 128):
        _kill_pose(p, i, i - 64)
    out["dead_middle"] = (p, ba.copy(), dead)
    p = bp[:128].copy()
    dead = np.zeros(128, bool)
    dead[:64] = True
    dead[37] = False
    for i in np.nonzero(dead)[0]:
        _kill_pose(p, i, int(i))
    out["one_live"] = (p, ba[:128].copy(), dead)
    return out


# ---- the kerb ------------------------------------------------------------------------------------------------------------------------
def kerb_steps():
    """drives over the kerb through the motion update with collision on: dicts of name, p, poses, attrs, step, and the closed-form
    answers want_killed / want (class) / want_z per particle.  A particle stands height = 0.1 above what it stands on."""
    out = []
    ys = np.linspace(-3.9, 3.9, 65)
    fwd, back, along = T.transform(IDENT, (1.0, 0, 0)), T.transform(IDENT, (-1.0, 0, 0)), T.transform(IDENT, (0, 1.0, 0))

    def add(name, probe_up, ts, step, killed, cls, z):
        n = len(ts)
        poses, attrs = cloud([IDENT] * n, ts, 67)
        out.append(dict(name="%s, probe_up %g" % (name, probe_up), map="kerb", p=sr.params(height=0.1, probe_up=probe_up, probe_down=1.0),
                        poses=poses, attrs=attrs, step=step, want_killed=np.full(n, killed, bool), want=np.full(n, cls, np.int32),
                        want_z=np.full(n, z, np.float64)))

    for probe_up in (0.5, 0.2):
        climbed = probe_up == 0.5
        # up the kerb, x = 0.5 -> 1.5: the lifted segment passes over the riser (0.5 > 0.3) or crosses it; the kerb's top is above the
        # probe of the lower one, which finds no ground
        add("up", probe_up, [(0.5, 0.0, 0.1)], fwd, not climbed, sr.SNAP if climbed else sr.MISS, 0.4 if climbed else 0.1)
        add("up, a row of 65", probe_up, [(0.5, y, 0.1) for y in ys], fwd, not climbed, sr.SNAP if climbed else sr.MISS, 0.4 if climbed else 0.1)
        # down the kerb, x = 1.5 -> 0.5 from z = 0.4: the lifted segment runs at z = 0.3 + probe_up, above the top it leaves and parallel
        # to it; the probe of the moved pose starts there and finds the floor
        add("down", probe_up, [(1.5, y, 0.4) for y in ys[::8]], back, False, sr.SNAP, 0.1)
        # along the riser, x = 1 exactly, y -> y + 1: the segment lies IN the riser's plane (den == 0: no hit) whether it runs above the
        # top or between floor and top; the vertical probe runs down the shared edges: the top's (min t) from 0.5, the floor's from 0.2
        add("along the riser", probe_up, [(1.0, y, 0.1) for y in (-3.0, -0.5, 0.25)], along, False, sr.SNAP, 0.4 if climbed else 0.1)
    return out


# ---- one small cloud per hand map ------------------------------------------------------------------------------------------------------
def hand_clouds():
    """cases on every map of MAPS (at most 65 particles each): the poses of the closed-form CPU tests first (with their classes), then
    random ones around the map"""
    S, M, X = sr.SNAP, sr.MISS, sr.STEEP
    k30 = math.tan(math.radians(30.0))
    out = []

    def around(seed, n, lo, hi, tilt):
        rng = np.random.RandomState(seed)
        return rpy_quats(rng, n, tilt), rng.uniform(lo, hi, (n, 3)).tolist()

    def add(name, axis, align, fixed_q, fixed_t, want, rand, probe=PROBE):
        rq, rt = rand
        qs, ts = list(fixed_q) + list(rq), list(fixed_t) + list(rt)
        assert len(ts) <= 65
        out.append(case(name, sr.params(axis=axis, align=align, **probe), cloud(qs, ts, 71 + len(out)), list(want) + [-1] * len(rt), name))

    q1 = np.array([0.1, -0.05, 0.3, 0.94], np.float64)
    q1 /= np.linalg.norm(q1)
    q2 = np.array([0.15, 0.1, -0.4, 0.9], np.float64)
    q2 /= np.linalg.norm(q2)
    plane_t = [(0.3, -1.2, 0.77), (-3.9, 3.9, -0.2), (0.0, 0.0, 0.25), (0.7, -0.2, 0.5)]
    for name in ("plane", "plane_down"):
        for axis in (0, 1):
            add(name, axis, 1, [q1, q1, q1, q2], plane_t, [S, S, S, S] if axis == 0 else [-1] * 4, around(73, 56, (-4.4, -4.4, -0.5), (4.4, 4.4, 1.2), 0.5))
    ramp_t = [(x, 0.25, x * k30 + 0.2) for x in (0.5, 0.25, 1.0, -1.3, 2.0)]
    for axis in (0, 1):
        add("ramp30", axis, 1, [IDENT] * 5, ramp_t, [S] * 5, around(79, 58, (-4.4, -4.4, -2.6), (4.4, 4.4, 2.9), 0.3))
    add("ramp30_far", 1, 1, [], [], [], pose_arrays(far_cloud()[1][0][:64]))
    # the 80 degree face under a vertical ray: steep; random positions along it
    add("face80", 0, 0, [IDENT], [(0.01, 0.0, 0.3)], [X], around(83, 40, (-1.1, -4.2, -6.0), (1.1, 4.2, 6.0), 0.3))
    add("face80", 1, 1, [IDENT], [(0.01, 0.0, 0.3)], [X], around(83, 40, (-1.1, -4.2, -6.0), (1.1, 4.2, 6.0), 0.3))
    # the wall x = 1: a vertical ray runs inside its plane (x == 1 exactly, too); the body-axis ray of a pitched particle meets it
    pitched = (0, math.sin(math.radians(-15.0)), 0, math.cos(math.radians(-15.0)))
    wall_probe = dict(height=0.0, probe_up=0.5, probe_down=1.0, min_up_cos=0.7)
    wall_q, wall_t = [pitched, pitched, IDENT], [(0.9, 0.0, 0.0), (0.9, -3.5, 3.0), (1.0, 0.5, 0.2)]
    add("wall_x1", 0, 0, wall_q, wall_t, [M, M, M], around(89, 40, (0.4, -4.2, -4.2), (1.6, 4.2, 4.2), 1.0), wall_probe)
    add("wall_x1", 1, 1, wall_q, wall_t, [X, X, M], around(89, 40, (0.4, -4.2, -4.2), (1.6, 4.2, 4.2), 1.0), wall_probe)
    # the hole: snap / miss / snap, the strips' edges x = +-1 exactly, and one float inside the gap (no claim: the test is not watertight)
    hole_t = [(-2.0, 0.3, 0.4), (0.0, 0.3, 0.4), (2.0, 0.3, 0.4), (-1.0, 0.3, 0.4), (1.0, -2.0, 0.4), (float(next_up(-1.0)), 0.3, 0.4)]
    for axis in (0, 1):
        add("hole", axis, 1, [IDENT] * 6, hole_t, [S, M, S, S, S, -1], around(97, 50, (-4.4, -4.4, -0.3), (4.4, 4.4, 1.0), 0.3))
    # the kerb: on the floor, on the top, on the riser's line (the top wins: min t), and a body-axis ray into the riser
    kerb_t = [(0.5, 0.0, 0.1), (1.5, 0.0, 0.4), (1.0, 0.0, 0.2), (1.0, 0.0, -0.25)]
    for axis in (0, 1):
        add("kerb", axis, 1, [IDENT] * 4, kerb_t, [S, S, S, S], around(101, 56, (-0.5, -4.2, -0.3), (2.5, 4.2, 1.0), 0.6))
    # the stack (height 0.125: every origin below is exact): from above both floors the upper one (min t), flipped; from between them
    # the lower one; from exactly ON the upper one (t == 0 there) the lower one
    stack_probe = dict(height=0.125, probe_up=0.5, probe_down=1.0, min_up_cos=0.7)
    for axis in (0, 1):
        add("stack", axis, 1, [IDENT] * 3, STACK_T, [S, S, S], around(103, 56, (-4.2, -4.2, -0.4), (4.2, 4.2, 1.9), 0.3), stack_probe)
    return out


STACK_T = [(0.5, -1.0, 1.0), (0.5, -1.0, 0.25), (0.5, -1.0, 0.375)]     # above both, between, origin exactly on the upper floor
STACK_FACES = ((2, 3), (0, 1), (0, 1))
STACK_Z = (0.875, 0.125, 0.125)


def hex32(x):
    return "0x%08X" % int(np.asarray(x, F).view(np.uint32))
