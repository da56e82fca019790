"""CPU tests of the surface constraint's restatement (tests/surface_ref.py) against answers known in closed form, on hand-built meshes
of a few triangles; the POD layout of its two structs; the C++ example compiles and prints its usage.  The GPU tests
(tests/test_gpu_surface.py) hold the kernels to this restatement bit for bit.  The second half proves that every case of
tests/surface_cases.py reaches what it was built for -- counts per class, both sides of each threshold, the branch taken and not taken --
so that tests/test_gpu_surface_edges.py, which runs the same cases on the device, cannot pass vacuously.
"""
import ctypes as C
import math
import subprocess
import time

import numpy as np
import pytest

import surface_cases as sc
import surface_ref as sr
from surface_cases import join, one, plane_z0, quad

F = np.float32


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


# ---- the cases of tests/surface_cases.py: each is proved fit for its purpose here, with the restatement alone; the GPU tests
# (tests/test_gpu_surface_edges.py) rely on these conditions ----------------------------------------------------------------------------
def run_case(c, bvh=False):
    mesh, normals = sc.oracle_mesh(c["map"])
    return sr.constrain(mesh, c["poses"], c["attrs"], c["p"], bvh=bvh, normals=normals)


def assert_wanted_classes(c, info):
    claimed = c["want"] >= 0
    assert np.array_equal(info["cls"][claimed], c["want"][claimed]), (c["map"], c["note"], info["cls"].tolist(), c["want"].tolist())


def class_counts(cls):
    return tuple(int((cls == k).sum()) for k in (sr.SNAP, sr.MISS, sr.STEEP))


@pytest.fixture(scope="module")
def cube(orc, meshes):
    m = orc.Mesh(*meshes("cube"))
    return m, m.face_normals()


def test_interval_cloud_sits_on_both_ends_of_the_hit_interval():
    cases = sc.interval_cloud()
    mesh, normals = sc.oracle_mesh("plane")
    n_xy = len(sc.INTERVAL_XY)
    for c in cases:
        _, _, st, info = run_case(c)
        print("interval,", c["note"], st)
        assert_wanted_classes(c, info)
        assert np.all(c["want"] >= 0)
    # the far end: [below, at, above] per (x, y) are snap, snap, miss, and the middle one has t_hit == tfar in float32
    far = cases[0]
    assert far["want"].reshape(n_xy, 3).tolist() == [[sr.SNAP, sr.SNAP, sr.MISS]] * n_xy
    tfar = far["p"]["probe_up"] + far["p"]["probe_down"]
    for i in range(n_xy):
        below, at, above = (sr.probe_one(mesh, normals, *sr.pose_Rt(far["poses"][3 * i + j]), far["p"], bvh=False) for j in range(3))
        assert at[3] == tfar and at[2][2] == tfar and below[3] == np.nextafter(tfar, F(0)) and above[2][2] == np.nextafter(tfar, F(2))
    # the near end: [well below, below, the three that round onto the plane, above]: only the last one snaps; t_hit == 0 for the three
    near = cases[1]
    assert near["want"].reshape(n_xy, 6).tolist() == [[sr.MISS] * 5 + [sr.SNAP]] * n_xy
    for i in range(n_xy):
        pr = [sr.probe_one(mesh, normals, *sr.pose_Rt(near["poses"][6 * i + j]), near["p"], bvh=False) for j in range(6)]
        assert [float(q[2][2]) for q in pr] == [float(F(-0.3) - F(0.25) + F(0.5)), -2.0 ** -24, 0.0, 0.0, 0.0, 2.0 ** -25]
        for q in pr[2:5]:      # with the near end opened the same ray reports t == 0: it is the strict near side that refuses it
            assert mesh.intersect(q[2], -q[1], -1.0, float(tfar), bvh=False)[:2] == (True, 0.0)
        assert float(pr[5][3]) == 2.0 ** -25
    # zero-length probes and the cases with a zero parameter reach both classes
    for c in cases[3:]:
        assert class_counts(run_case(c)[3]["cls"])[0] >= n_xy and class_counts(run_case(c)[3]["cls"])[1] >= n_xy


def test_threshold_cloud_is_snap_at_equality_and_steep_one_float_above():
    cases = sc.threshold_cloud()
    seen = {sr.SNAP: 0, sr.STEEP: 0}
    for c in cases:
        _, _, st, info = run_case(c)
        assert_wanted_classes(c, info)
        seen[int(info["cls"][0])] += 1
    print("threshold cases:", seen)
    # the trios on the ramp: min_up_cos one float below d, d itself, one float above
    ramp = [c for c in cases if c["note"].startswith("ramp30 d")]
    assert len(ramp) == 18
    for k in range(0, 18, 6):
        lo, at, hi = (ramp[k + j]["p"]["min_up_cos"] for j in (0, 2, 4))
        assert np.nextafter(lo, F(2)) == at and np.nextafter(at, F(2)) == hi
        assert [int(ramp[k + j]["want"][0]) for j in range(6)] == [sr.SNAP] * 4 + [sr.STEEP] * 2
    assert {float(c["p"]["min_up_cos"]) for c in cases} >= {0.0, 1.0}
    assert seen[sr.SNAP] >= 10 and seen[sr.STEEP] >= 5


def test_upside_down_cloud_takes_the_branch_and_straddles_its_threshold():
    up, down = sc.upside_down_cloud("plane"), sc.upside_down_cloud("plane_down")
    assert up["poses"].tobytes() == down["poses"].tobytes()
    n = len(up["poses"])
    w = np.array([sc.align_w(sr.pose_Rt(up["poses"][i])[0]) for i in range(n)], F)
    taken = w < F(1e-6)
    print("upside down: w =", w.tolist(), "taken", int(taken.sum()), "of", n)
    assert int(taken.sum()) >= 6 and int((~taken).sum()) >= 4 and int((w == 0).sum()) >= 2
    # the last two are adjacent float32 rotations, either side of the threshold
    qa, qb = sr.pose_Rt(up["poses"][n - 2])[0], sr.pose_Rt(up["poses"][n - 1])[0]
    print("threshold pair: w components", sc.hex32(qa[3]), sc.hex32(qb[3]), "x components", sc.hex32(qa[0]), sc.hex32(qb[0]), "w =", w[n - 2], w[n - 1])
    assert int(qb[3].view(np.uint32)) - int(qa[3].view(np.uint32)) == 1 and np.array_equal(qa[:3], qb[:3])
    assert taken[n - 2] and not taken[n - 1]
    pu, au, su, iu = run_case(up)
    pd, ad, sd, idn = run_case(down)
    assert su["n_snapped"] == n and sd["n_snapped"] == n and not iu["flipped"].any() and idn["flipped"].all()
    assert pu.tobytes() == pd.tobytes() and au.tobytes() == ad.tobytes()
    # the exact half turns: body z ends on +z and the heading (body x) is kept
    for k, xb_want, exact in ((0, (1, 0, 0), True), (1, (-1, 0, 0), True), (2, (0, 1, 0), False),
                              (3, (math.cos(math.radians(37.0)), math.sin(math.radians(37.0)), 0), False)):
        assert taken[k]
        R1 = sr.pose_Rt(pu[k])[0]
        zb, xb = sr.qrot(R1, (0, 0, 1)), sr.qrot(R1, (1, 0, 0))
        if exact:
            assert np.array_equal(zb, np.array([0, 0, 1], F)) and np.array_equal(xb, np.array(xb_want, F))
        else:
            assert np.allclose(zb, [0, 0, 1], atol=3e-7) and np.allclose(xb, xb_want, atol=3e-7)
    assert np.array_equal(np.abs(sr.pose_Rt(pu[0])[0]), np.array([0, 0, 0, 1], F))
    # outside the branch the body z ends on the normal too, as well as float32 allows: q = (zb x n, w) turns by 2 atan(|zb x n| / w) with
    # |zb x n| = sqrt(2 w) to first order, so an error dw of w turns the result by 2 dw / sqrt(2 w).  w = 1 + zb.z, and zb.z (magnitude
    # below one) comes out of two quaternion products of seven roundings per component each, from an R that was itself rounded: at most
    # sixteen roundings of 2^-25, dw <= 2^-21 -- 6.7e-4 rad at the threshold w = 1e-6, less beyond it.  (Seen: 1e-5 to 3e-5.)
    for k in np.nonzero(~taken)[0]:
        off = sr.qrot(sr.pose_Rt(pu[k])[0], (0, 0, 1)).astype(np.float64) - np.array([0, 0, 1.0])
        print("   w = %.4g: body z off the normal by %.3g" % (w[k], np.abs(off).max()))
        assert np.abs(off).max() <= 2.0 * 2.0 ** -21 / math.sqrt(2.0 * float(w[k]))


def test_attitude_cloud_reaches_every_class_on_both_axes(cube):
    mesh, normals = cube
    poses, attrs = sc.attitude_cloud(1025)
    for axis, want_steep in ((0, 0), (1, 50)):
        _, _, st, info = sr.constrain(mesh, poses, attrs, sr.params(axis=axis, align=1, **sc.PROBE), bvh=False, normals=normals)
        print("attitudes, seed %d, axis %d:" % (sc.ATTITUDE_SEED, axis), st, "flipped", int(info["flipped"].sum()))
        assert st["n_snapped"] >= 50 and st["n_missed"] >= 50 and st["n_steep"] >= want_steep and int(info["flipped"].sum()) >= 20


def test_nonunit_cloud_changes_the_reach_of_the_body_axis_ray():
    ns = len(sc.NONUNIT_SCALES)
    assert sc.NONUNIT_SCALES[:2] == (0.5, 2.0)
    differ = 0
    for c in sc.nonunit_cloud():
        _, _, st, info = run_case(c)
        cls = info["cls"].reshape(ns, -1)
        R = np.column_stack([c["poses"]["R"][k] for k in "xyzw"]).astype(np.float64)
        norms = np.linalg.norm(R, axis=1).reshape(ns, -1)
        assert np.allclose(norms, np.array(sc.NONUNIT_SCALES)[:, None], rtol=1e-6) and len(set(norms[:, 0].tolist())) == ns
        print("non-unit,", c["map"], "axis %d align %d:" % (c["p"]["axis"], c["p"]["align"]), [class_counts(r) for r in cls])
        if c["p"]["axis"] == 0:
            assert np.all(cls == sr.SNAP)
        else:
            differ += int((cls[0] != cls[1]).sum())
            assert np.all(cls[1] == sr.SNAP)      # norm 2: sixteen times the reach of norm 0.5, and d = 4 cos
    assert differ >= 1


def test_far_cloud_is_the_near_cloud_five_kilometres_out():
    near, far = sc.far_cloud()
    assert len(near[0]) == 257 and near[0]["R"].tobytes() == far[0]["R"].tobytes() and near[1].tobytes() == far[1].tobytes()
    assert np.all(far[0]["t"]["x"] > 4990) and np.all(far[0]["t"]["y"] < -4990) and np.all(far[0]["t"]["z"] > 290)
    for axis, want_steep in ((0, 0), (1, 5)):
        p = sr.params(axis=axis, align=1, **sc.PROBE)
        cls = {}
        for name, (poses, attrs) in (("ramp30", near), ("ramp30_far", far)):
            mesh, normals = sc.oracle_mesh(name)
            _, _, st, info = sr.constrain(mesh, poses, attrs, p, bvh=False, normals=normals)
            print("far cloud on %s, axis %d:" % (name, axis), st)
            assert st["n_snapped"] >= 100 and st["n_missed"] >= 30 and st["n_steep"] >= want_steep
            cls[name] = info["cls"]
        assert int((cls["ramp30"] != cls["ramp30_far"]).sum()) <= 257 * 2 // 100


def test_stack_takes_the_nearer_floor_and_not_the_one_it_starts_on():
    c = [h for h in sc.hand_clouds() if h["map"] == "stack" and h["p"]["axis"] == 0][0]
    po, _, st, info = run_case(c)
    assert info["cls"][:3].tolist() == [sr.SNAP] * 3 and info["flipped"][:3].tolist() == [True, False, False]
    for i in range(3):
        assert int(info["face"][i]) in sc.STACK_FACES[i] and float(po["t"]["z"][i]) == sc.STACK_Z[i]
    # the third probe starts exactly on the upper floor: O.z == 0.75
    R, t = sr.pose_Rt(c["poses"][2])
    assert float(sr.origin_of(t, sr.axis_of(R, c["p"]), c["p"])[2]) == 0.75


def test_hand_clouds_have_their_closed_form_classes_and_stay_small():
    seen = set()
    for c in sc.hand_clouds():
        assert len(c["poses"]) <= 65
        _, _, st, info = run_case(c)
        print("hand map %-10s axis %d:" % (c["map"], c["p"]["axis"]), st, "flipped", int(info["flipped"].sum()))
        assert_wanted_classes(c, info)
        seen.add(c["map"])
    assert seen == set(sc.MAPS)
    by = {(c["map"], c["p"]["axis"]): run_case(c)[3]["cls"] for c in sc.hand_clouds()}
    assert by[("hole", 0)][:3].tolist() == [sr.SNAP, sr.MISS, sr.SNAP] and by[("face80", 0)][0] == sr.STEEP
    assert by[("wall_x1", 0)][0] == sr.MISS and by[("wall_x1", 1)][0] == sr.STEEP


def test_kerb_steps_up_down_and_along_the_riser():
    """up: the existing answers (climbed with probe_up 0.5, killed and without ground with 0.2).  Down: the lifted segment runs above
    the top the particle leaves, nobody is killed and the probe finds the floor.  Along the riser at x == 1 exactly: the segment lies
    in the riser's plane (den == 0 is no hit), nobody is killed; the vertical probe runs down the edges the faces share and takes the
    top from probe_up 0.5 (min t) and the floor from 0.2, where the top is above its origin."""
    mesh, normals = sc.oracle_mesh("kerb")
    for c in sc.kerb_steps():
        po, ao, st, killed = sr.motion_update(mesh, c["poses"], c["attrs"], c["step"], 0.0, True, c["p"], bvh=False, normals=normals)
        print("kerb,", c["name"], st, "killed", int(killed.sum()))
        n = len(po)
        assert np.array_equal(killed, c["want_killed"])
        assert class_counts(c["want"]) == (st["n_snapped"], st["n_missed"], st["n_steep"])
        assert np.all(np.abs(po["t"]["z"].astype(np.float64) - c["want_z"]) < 1e-6)
        assert np.all(ao["likelihood"]["mean"][killed] == 0) and ao[~killed].tobytes() == c["attrs"][~killed].tobytes()
        if c["name"].startswith("up"):      # the unlifted segment of the unconstrained update crosses the riser in both cases
            for i in range(n):
                _, t0 = sr.pose_Rt(c["poses"][i])
                assert sr.collides(mesh, t0, t0 + np.array([1, 0, 0], F), bvh=False)


def test_brute_force_and_bvh_agree_on_every_case(cube):
    def same(mesh, normals, poses, attrs, p):
        pa, aa, sa, ia = sr.constrain(mesh, poses, attrs, p, bvh=True, normals=normals)
        pb, ab, sb, ib = sr.constrain(mesh, poses, attrs, p, bvh=False, normals=normals)
        assert sa == sb and np.array_equal(ia["cls"], ib["cls"]) and np.array_equal(ia["face"], ib["face"])
        assert pa.tobytes() == pb.tobytes() and aa.tobytes() == ab.tobytes()

    cases = sc.interval_cloud() + sc.threshold_cloud() + [sc.upside_down_cloud("plane"), sc.upside_down_cloud("plane_down")]
    cases += sc.nonunit_cloud() + sc.hand_clouds()
    for c in cases:
        same(*sc.oracle_mesh(c["map"]), c["poses"], c["attrs"], c["p"])
    near, far = sc.far_cloud()
    for axis in (0, 1):
        p = sr.params(axis=axis, align=1, **sc.PROBE)
        same(*sc.oracle_mesh("ramp30"), *near, p)
        same(*sc.oracle_mesh("ramp30_far"), *far, p)
        same(*cube, *sc.attitude_cloud(1025), p)
        for poses, attrs, _ in sc.wave_clouds().values():
            same(*cube, poses, attrs, p)
    mesh, normals = sc.oracle_mesh("kerb")
    for c in sc.kerb_steps():
        a = sr.motion_update(mesh, c["poses"], c["attrs"], c["step"], 0.0, True, c["p"], bvh=True, normals=normals)
        b = sr.motion_update(mesh, c["poses"], c["attrs"], c["step"], 0.0, True, c["p"], bvh=False, normals=normals)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_wave_clouds_have_their_dead_lanes_where_they_say(cube):
    mesh, normals = cube
    clouds = sc.wave_clouds()
    assert [len(clouds["n%d" % n][0]) for n in sc.WAVE_COUNTS] == [63, 64, 65, 129]
    for name, (poses, attrs, dead) in clouds.items():
        finite = np.ones(len(poses), bool)
        for grp, keys in (("R", "xyzw"), ("t", "xyz")):
            for k in keys:
                finite &= np.isfinite(poses[grp][k])
        assert np.array_equal(~finite, dead)
        _, _, st, info = sr.constrain(mesh, poses, attrs, sr.params(axis=1, align=1, **sc.PROBE), bvh=False, normals=normals)
        print("wave cloud", name, st, "dead", int(dead.sum()))
        assert np.all(info["cls"][dead] == sr.MISS) and st["n_snapped"] >= int((~dead).sum()) * 6 // 10 and st["n_missed"] > int(dead.sum())
    assert np.nonzero(clouds["dead_middle"][2])[0].tolist() == list(range(64, 128))
    assert np.nonzero(~clouds["one_live"][2][:64])[0].tolist() == [37] and not clouds["one_live"][2][64:].any()
    t = clouds["dead_middle"][0]
    assert np.isnan(t["t"]["x"]).any() and np.isposinf(t["t"]["y"]).any() and np.isneginf(t["R"]["z"]).any() and np.isnan(t["R"]["w"]).any()


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
