"""CPU tests of the surface constraint's restatement (tests/surface_ref.py) against answers known in closed form, on hand-built meshes
of a few triangles; the POD layout of its two structs; the C++ example compiles and prints its usage.  The GPU tests
(tests/test_gpu_surface.py) hold the kernels to this restatement bit for bit.
"""
import ctypes as C
import math
import subprocess
import time

import numpy as np
import pytest

import surface_ref as sr

F = np.float32


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


@pytest.fixture(scope="module")
def T(ra):
    return ra.types


def test_plane_height_is_exact_and_xy_and_R_untouched(orc, T):
    m = orc.Mesh(*plane_z0())
    q = np.array([0.1, -0.05, 0.3, 0.94], np.float64)
    q = (q / np.linalg.norm(q)).astype(F)
    for axis0_t in ((0.3, -1.2, 0.77), (-3.9, 3.9, -0.2), (0.0, 0.0, 0.25)):
        poses, attrs = one(T, q, axis0_t)
        p = sr.params(height=0.25, probe_up=0.5, probe_down=1.0)
        po, ao, st, info = sr.constrain(m, poses, attrs, p)
        assert st == dict(n_particles=1, n_snapped=1, n_missed=0, n_steep=0)
        assert po["t"]["z"][0] == F(0.25)
        assert po["t"]["x"][0] == poses["t"]["x"][0] and po["t"]["y"][0] == poses["t"]["y"][0]
        assert po["R"].tobytes() == poses["R"].tobytes() and ao.tobytes() == attrs.tobytes()


def test_ramp_align_puts_body_z_on_the_normal_and_is_idempotent(orc, T):
    """a 30 degree ramp rising along x.  Body z against the ramp normal: components of a unit vector, bounded by 2 ulp of a number just
    below one (2 * 2^-24) each.  A second application leaves the rotation bit for bit -- the aligned body z is a fixed point of step 5.
    The position is NOT a fixed point of the float32 rule on a sloped face: it is re-derived through a ray intersection, whose
    C = v0 - O (|C_k| <= 8 here: half an ulp of 8 is 4.8e-7 per component) enters t = (Ng . C) / (Ng . D); x and y stay (axis 0), z moves
    by that rounding -- measured: up to 10 ulp of z = 1.5e-7 m at five positions on this ramp -- and is bounded here by
    3 * 4.8e-7 / cos(30 deg) + the five roundings of steps 1 and 4 < 2e-6 m."""
    k = math.tan(math.radians(30.0))
    m = orc.Mesh(*quad((-4, -4, -4 * k), (4, -4, 4 * k), (4, 4, 4 * k), (-4, 4, -4 * k)))
    p = sr.params(height=0.1, probe_up=0.5, probe_down=1.0, align=1)
    for x in (0.5, 0.25, 1.0, -1.3, 2.0):
        poses, attrs = one(T, (0, 0, 0, 1), (x, 0.25, x * k + 0.2))
        po, ao, st, info = sr.constrain(m, poses, attrs, p)
        assert st["n_snapped"] == 1
        n = m.face_normals()[info["face"][0]]
        n = -n if n[2] < 0 else n
        assert abs(float(n[0]) + 0.5) < 1e-6 and abs(float(n[2]) - math.cos(math.radians(30.0))) < 1e-6
        R1, t1 = sr.pose_Rt(po[0])
        zb = sr.qrot(R1, (0, 0, 1))
        print("ramp x = %g: body z - normal =" % x, (zb.astype(np.float64) - n.astype(np.float64)))
        assert np.all(np.abs(zb.astype(np.float64) - n.astype(np.float64)) <= 2.0 * 2.0 ** -24)
        assert abs(float(t1[2]) - (x * k + 0.1)) < 1e-6        # axis 0: height is measured along map z
        po2, ao2, st2, _ = sr.constrain(m, po, ao, p)
        assert st2["n_snapped"] == 1
        assert po2["R"].tobytes() == po["R"].tobytes() and ao2.tobytes() == ao.tobytes()
        assert po2["t"]["x"][0] == po["t"]["x"][0] and po2["t"]["y"][0] == po["t"]["y"][0]
        print("   second application: dz = %.3g m" % (float(po2["t"]["z"][0]) - float(po["t"]["z"][0])))
        assert abs(float(po2["t"]["z"][0]) - float(po["t"]["z"][0])) < 2e-6
    # on a level floor the whole pose is a fixed point, position included
    flat = orc.Mesh(*plane_z0())
    poses, attrs = one(T, (0, 0, 0, 1), (0.3, -1.2, 0.77))
    po, ao, _, _ = sr.constrain(flat, poses, attrs, p)
    po2, ao2, _, _ = sr.constrain(flat, po, ao, p)
    assert po2.tobytes() == po.tobytes() and ao2.tobytes() == ao.tobytes()


def test_walls_are_steep(orc, T):
    # an 80 degree face under a vertical ray
    k = math.tan(math.radians(80.0))
    m = orc.Mesh(*quad((-1, -4, -k), (1, -4, k), (1, 4, k), (-1, 4, -k)))
    poses, attrs = one(T, (0, 0, 0, 1), (0.01, 0.0, 0.3))
    for on_miss in (0, 1):
        po, ao, st, info = sr.constrain(m, poses, attrs, sr.params(height=0.1, probe_up=0.5, probe_down=1.0, on_miss=on_miss), max_n_meas=123)
        assert st == dict(n_particles=1, n_snapped=0, n_missed=0, n_steep=1) and po.tobytes() == poses.tobytes()
        if on_miss:
            assert (float(ao["likelihood"]["mean"][0]), float(ao["likelihood"]["sigma"][0]), int(ao["likelihood"]["n_meas"][0])) == (0.0, 0.0, 123)
            assert np.array_equal(ao["state_sigma"], attrs["state_sigma"])
        else:
            assert ao.tobytes() == attrs.tobytes()
    # a truly vertical wall (the plane x = 1): a vertical ray runs inside its plane and cannot hit it -- the body-axis ray of a
    # particle pitched by 30 degrees does, at |n . a| = 0.5
    wall = orc.Mesh(*quad((1, -4, -4), (1, 4, -4), (1, 4, 4), (1, -4, 4)))
    poses, attrs = one(T, (0, math.sin(math.radians(-15.0)), 0, math.cos(math.radians(-15.0))), (0.9, 0.0, 0.0))
    a = sr.axis_of(sr.pose_Rt(poses[0])[0], sr.params(axis=1))
    assert abs(abs(float(a[0])) - 0.5) < 1e-6
    _, _, st, _ = sr.constrain(wall, poses, attrs, sr.params(axis=0, height=0.0, probe_up=0.5, probe_down=1.0))
    assert st["n_missed"] == 1
    _, _, st, _ = sr.constrain(wall, poses, attrs, sr.params(axis=1, height=0.0, probe_up=0.5, probe_down=1.0))
    assert st["n_steep"] == 1


def test_hole_and_zero_probe_miss(orc, T):
    m = orc.Mesh(*join(quad((-4, -4, 0), (-1, -4, 0), (-1, 4, 0), (-4, 4, 0)), quad((1, -4, 0), (4, -4, 0), (4, 4, 0), (1, 4, 0))))
    p = sr.params(height=0.1, probe_up=0.5, probe_down=1.0)
    for x, want in ((-2.0, "n_snapped"), (0.0, "n_missed"), (2.0, "n_snapped")):
        poses, attrs = one(T, (0, 0, 0, 1), (x, 0.3, 0.4))
        po, ao, st, _ = sr.constrain(m, poses, attrs, p)
        assert st[want] == 1
        if want == "n_missed":
            assert po.tobytes() == poses.tobytes() and ao.tobytes() == attrs.tobytes()
    # probe_up = probe_down = 0: the ray has no length -- on the plane (t = 0 is not a hit) and above it
    for z in (0.1, 0.4):
        poses, attrs = one(T, (0, 0, 0, 1), (-2.0, 0.3, z))
        _, _, st, _ = sr.constrain(m, poses, attrs, sr.params(height=0.1, probe_up=0.0, probe_down=0.0))
        assert st["n_missed"] == 1


def test_a_face_wound_downward_is_flipped(orc, T):
    up, down = orc.Mesh(*plane_z0()), orc.Mesh(*plane_z0(down=True))
    assert up.face_normals()[0][2] * down.face_normals()[0][2] < 0
    q = np.array([0.15, 0.1, -0.4, 0.9], np.float64)
    q = (q / np.linalg.norm(q)).astype(F)
    for axis in (0, 1):
        for align in (0, 1):
            poses, attrs = one(T, q, (0.7, -0.2, 0.5))
            p = sr.params(axis=axis, height=0.2, probe_up=0.5, probe_down=1.0, align=align)
            pu, au, su, iu = sr.constrain(up, poses, attrs, p)
            pd, ad, sd, idn = sr.constrain(down, poses, attrs, p)
            assert su["n_snapped"] == 1 and sd["n_snapped"] == 1
            assert bool(iu["flipped"][0]) != bool(idn["flipped"][0])
            assert pu.tobytes() == pd.tobytes() and au.tobytes() == ad.tobytes()
            if align:
                zb = sr.qrot(sr.pose_Rt(pu[0])[0], (0, 0, 1))
                assert np.all(np.abs(zb.astype(np.float64) - np.array([0, 0, 1.0])) <= 2.0 * 2.0 ** -24)


def test_upside_down_takes_the_half_turn_about_body_x(orc, T):
    m = orc.Mesh(*plane_z0())
    poses, attrs = one(T, (1, 0, 0, 0), (0.5, 0.5, 0.3))                # half turn about x: body z = -map z
    assert np.array_equal(sr.qrot(sr.pose_Rt(poses[0])[0], (0, 0, 1)), np.array([0, 0, -1], F))
    po, _, st, _ = sr.constrain(m, poses, attrs, sr.params(height=0.1, probe_up=0.5, probe_down=1.0, align=1))
    assert st["n_snapped"] == 1
    R1 = sr.pose_Rt(po[0])[0]
    assert np.array_equal(sr.qrot(R1, (0, 0, 1)), np.array([0, 0, 1], F))
    assert np.array_equal(sr.qrot(R1, (1, 0, 0)), np.array([1, 0, 0], F))    # the heading (body x) is kept
    assert np.array_equal(np.abs(R1), np.array([0, 0, 0, 1], F))
    # with a yaw of 90 degrees first: body x = map y stays
    s = math.sqrt(0.5)
    Ryaw = np.array([0, 0, s, s], F)
    poses, attrs = one(T, sr.qmul(Ryaw, np.array([1, 0, 0, 0], F)), (0.5, 0.5, 0.3))
    po, _, st, _ = sr.constrain(m, poses, attrs, sr.params(height=0.1, probe_up=0.5, probe_down=1.0, align=1))
    R1 = sr.pose_Rt(po[0])[0]
    assert np.allclose(sr.qrot(R1, (0, 0, 1)), [0, 0, 1], atol=3e-7) and np.allclose(sr.qrot(R1, (1, 0, 0)), [0, 1, 0], atol=3e-7)


def test_kerb_is_climbed_below_the_step_height_and_a_wall_above_it(orc, T):
    """a kerb of 0.3 m at x = 1: floor z = 0 for x < 1, top z = 0.3 for x > 1, the riser between them.  A particle drives from x = 0.5 to
    x = 1.5: with probe_up 0.5 the lifted segment passes over the riser and the particle lands on the kerb; with probe_up 0.2 the segment
    crosses the riser and the particle is killed (and finds no ground: the kerb's top is above its probe)."""
    m = orc.Mesh(*join(quad((-4, -4, 0), (1, -4, 0), (1, 4, 0), (-4, 4, 0)), quad((1, -4, 0.3), (4, -4, 0.3), (4, 4, 0.3), (1, 4, 0.3)),
                       quad((1, -4, 0), (1, 4, 0), (1, 4, 0.3), (1, -4, 0.3))))
    step = T.transform((0, 0, 0, 1), (1.0, 0, 0))
    for probe_up, want_killed in ((0.5, False), (0.2, True)):
        poses, attrs = one(T, (0, 0, 0, 1), (0.5, 0.0, 0.1))
        p = sr.params(height=0.1, probe_up=probe_up, probe_down=1.0)
        po, ao, st, killed = sr.motion_update(m, poses, attrs, step, 0.0, True, p, max_n_meas=10000)
        assert bool(killed[0]) == want_killed
        assert float(po["t"]["x"][0]) == 1.5
        if want_killed:
            assert st["n_missed"] == 1 and float(po["t"]["z"][0]) == float(F(0.1))
            assert (float(ao["likelihood"]["mean"][0]), int(ao["likelihood"]["n_meas"][0])) == (0.0, 10000)
        else:
            assert st["n_snapped"] == 1 and abs(float(po["t"]["z"][0]) - 0.4) < 1e-6
            assert ao.tobytes() == attrs.tobytes()
        # the unlifted segment of the unconstrained update (old.t -> new.t at z = 0.1) crosses the riser in both cases
        assert sr.collides(m, np.array([0.5, 0, 0.1], F), np.array([1.5, 0, 0.1], F))


@pytest.mark.parametrize("name,lo,hi,probe_down", [("room30k", (-9.9, -9.9, -0.3), (9.9, 9.9, 2.5), 1.0),
                                                   ("sphere20k", (-6, -6, -9.5), (6, 6, -4), 3.0)])
def test_restatement_is_quick_and_its_two_intersectors_agree(orc, T, meshes, name, lo, hi, probe_down):
    """1 500 particles take under a second per mesh through the BVH, and brute force gives the same class, face and pose for every one"""
    v, f = meshes(name)
    m = orc.Mesh(v, f)
    rng = np.random.RandomState(11)
    n = 1500
    poses = np.zeros(n, T.TRANSFORM)
    attrs = np.zeros(n, T.PARTICLE_ATTRIBUTES)
    t = rng.uniform(lo, hi, (n, 3)).astype(F)
    for i in range(n):
        poses[i] = T.transform_from_rpy(t[i], (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-math.pi, math.pi)))
    p = sr.params(height=0.1, probe_up=0.5, probe_down=probe_down, min_up_cos=0.7, align=1)
    normals = m.face_normals()
    t0 = time.perf_counter()
    pa, aa, sa, ia = sr.constrain(m, poses, attrs, p, bvh=True, normals=normals)
    dt = time.perf_counter() - t0
    pb, ab, sb, ib = sr.constrain(m, poses, attrs, p, bvh=False, normals=normals)
    print(name, sa, "flipped", int(ia["flipped"].sum()), "%.2f s" % dt)
    assert dt < 1.0
    assert sa == sb and np.array_equal(ia["face"], ib["face"]) and pa.tobytes() == pb.tobytes()
    assert sa["n_snapped"] >= n // 10 and sa["n_missed"] >= n // 10


def test_pod_sizes_and_defaults(ra):
    assert C.sizeof(ra._capi.SurfaceParams) == 28 and C.sizeof(ra._capi.SurfaceStats) == 16
    assert [n for n, _ in ra._capi.SurfaceParams._fields_] == ["axis", "height", "probe_up", "probe_down", "min_up_cos", "align", "on_miss"]
    assert ra._capi.SurfaceParams.min_up_cos.offset == 16 and ra._capi.SurfaceStats.n_steep.offset == 12
    p = ra.types.surface_params()
    assert (p.axis, p.align, p.on_miss) == (0, 0, 0)
    assert (p.height, p.probe_up, p.probe_down, p.min_up_cos) == (0.0, float(F(0.3)), 1.0, float(F(0.7)))
    ref = sr.params()
    assert all(float(ref[k]) == float(getattr(p, k)) for k in ("height", "probe_up", "probe_down", "min_up_cos"))
    q = ra.types.surface_params(axis=1, height=0.1, align=1, on_miss=1)
    assert (q.axis, q.align, q.on_miss, q.height) == (1, 1, 1, float(F(0.1)))
    # the argument check needs no device: a null handle and bad parameters are refused
    L = ra._capi.lib()
    assert L.rmclhip_pf_set_surface(None, C.byref(p)) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_constrain_to_surface(None, None, None, 0, C.byref(p), None) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_sharded_set_surface(None, None) == ra._capi.ERR_INVALID


def test_surface_example_compiles_and_prints_usage(ra, tmp_path):
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "surface_motion_cpp_example.cpp")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
