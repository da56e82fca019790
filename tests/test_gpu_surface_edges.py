"""GPU tests of the surface constraint at its edges (include/rmclhip.h, "surface-constrained motion"): the cases of tests/surface_cases.py
-- hand-built maps of two to six triangles through the product's own builder, the ends of the hit interval, min_up_cos at equality, the
upside-down branch of step 5 and its threshold, every attitude, non-unit quaternions, a map 5 km out, ragged and dead waves, the kerb's
lifted collision segment, sharded clouds smaller than the communicator -- through k_surface_constrain and the fused case of the motion
kernel.  The rule of tests/test_gpu_surface.py holds: poses, attributes, the four counts and the face of every probe are compared BYTE
FOR BYTE with the numpy float32 restatement (tests/surface_ref.py) on the brute-force oracle; no field has a tolerance.
tests/test_surface_cases_cpu.py proves that every case reaches what it is for.  Each test prints the class counts it saw.
"""
import ctypes as C
import math

import numpy as np
import pytest

import surface_cases as sc
import surface_ref as sr
from test_gpu_surface import NO_FACE, gpu_constrain, ref_faces

pytestmark = pytest.mark.gpu

F = np.float32


class Map:
    """a map on the device (through the product's builder) and in the oracle, with a standalone handle and fused updaters"""

    def __init__(self, ra, ctx, name, v, f, mesh, normals):
        self.ra, self.ctx, self.name, self.v, self.f, self.mesh, self.normals = ra, ctx, name, v, f, mesh, normals
        self.hm = ra.import_hip_map(ctx, v, f)
        self.upd = ra.TFMotionUpdaterHip(self.hm, check_collision=False)
        self.upd.init()
        self._fused = {}

    def fused(self, collision):
        if collision not in self._fused:
            self._fused[collision] = self.ra.TFMotionUpdaterHip(self.hm, check_collision=collision)
        return self._fused[collision]

    def ref(self, poses, attrs, p, max_n_meas=10000, probes=None):
        return sr.constrain(self.mesh, poses, attrs, p, max_n_meas=max_n_meas, bvh=False, normals=self.normals, probes=probes)

    def check(self, poses, attrs, p, upd=None, max_n_meas=10000, probes=None):
        """the standalone pass against the restatement: counts, faces, pose and attribute bytes.  Returns the restatement's result."""
        upd = self.upd if upd is None else upd
        pr, ar, sref, info = self.ref(poses, attrs, p, max_n_meas, probes)
        pg, ag, sg, faces = gpu_constrain(self.ra, self.ctx, upd, poses, attrs, p)
        assert sg == sref, (self.name, sg, sref)
        assert np.array_equal(faces, ref_faces(info)), (self.name, np.nonzero(faces != ref_faces(info))[0][:8])
        assert pg.tobytes() == pr.tobytes(), (self.name, [i for i in range(len(pg)) if pg[i].tobytes() != pr[i].tobytes()][:8])
        assert ag.tobytes() == ar.tobytes(), (self.name, [i for i in range(len(ag)) if ag[i].tobytes() != ar[i].tobytes()][:8])
        assert upd.surface_stats() == sref
        return pr, ar, sref, info

    def check_fused(self, poses, attrs, p, step, rate, collision, max_n_meas=10000):
        """the motion update with the constraint set against the restatement: counts, pose and attribute bytes"""
        pr, ar, sref, killed = sr.motion_update(self.mesh, poses, attrs, step, rate, collision, p, max_n_meas=max_n_meas, bvh=False, normals=self.normals)
        upd = self.fused(collision)
        upd.surface = sr.to_capi(self.ra, p)
        d_p, d_a = self.ra.DeviceArray.from_host(self.ctx, poses), self.ra.DeviceArray.from_host(self.ctx, attrs)
        upd.update(d_p, d_a, len(poses), step, rate)
        pg, ag = d_p.download(), d_a.download()
        assert upd.surface_stats() == sref, (self.name, upd.surface_stats(), sref)
        assert pg.tobytes() == pr.tobytes(), (self.name, [i for i in range(len(pg)) if pg[i].tobytes() != pr[i].tobytes()][:8])
        assert ag.tobytes() == ar.tobytes(), (self.name, [i for i in range(len(ag)) if ag[i].tobytes() != ar[i].tobytes()][:8])
        return pr, ar, sref, killed


@pytest.fixture(scope="module")
def maps(ra, orc, ctx, meshes):
    """every hand map of surface_cases.MAPS and the cube room, built once"""
    out = {}
    for name in sc.MAPS:
        v, f = sc.MAPS[name]()
        out[name] = Map(ra, ctx, name, v, f, *sc.oracle_mesh(name))
    v, f = meshes("cube")
    m = orc.Mesh(v, f)
    out["cube"] = Map(ra, ctx, "cube", v, f, m, m.face_normals())
    return out


def counts(info, dead=None):
    c = "snap %d miss %d steep %d flipped %d" % (int((info["cls"] == sr.SNAP).sum()), int((info["cls"] == sr.MISS).sum()),
                                                 int((info["cls"] == sr.STEEP).sum()), int(info["flipped"].sum()))
    return c if dead is None else c + " non-finite %d" % int(dead.sum())


def test_interval_ends(ra, maps):
    """the hit interval is (0, tfar]: t_hit == tfar snaps and the next float misses; t_hit == 0 misses and the next origin above the
    plane snaps -- at points inside a triangle, on the shared diagonal, on the map's edge and on its corner; zero-length probes.  Through
    the standalone pass and through the fused launch (identity step, forget_rate 0, collision off)."""
    from rmcl_amd import types as T
    M = maps["plane"]
    for c in sc.interval_cloud():
        for on_miss in (0, 1):
            p = dict(c["p"], on_miss=on_miss)
            _, _, sref, info = M.check(c["poses"], c["attrs"], p)
            assert np.array_equal(info["cls"], c["want"])
            M.check_fused(c["poses"], c["attrs"], p, T.identity(), 0.0, False)
        print("interval, %s:" % c["note"], counts(info))


def test_min_up_cos_at_equality_zero_and_one(ra, maps):
    """!(d >= min_up_cos): snap at equality and one float below, steep one float above; 0 takes a wall, 1 takes only d == 1"""
    seen = np.zeros(3, int)
    for c in sc.threshold_cloud():
        for on_miss in (0, 1):
            _, _, sref, info = maps[c["map"]].check(c["poses"], c["attrs"], dict(c["p"], on_miss=on_miss))
            assert np.array_equal(info["cls"], c["want"])
        seen += np.bincount(info["cls"], minlength=3)
        print("threshold, %s, axis %d, min_up_cos %s:" % (c["note"], c["p"]["axis"], sc.hex32(c["p"]["min_up_cos"])), counts(info))
    print("threshold cases: snap %d miss %d steep %d" % tuple(seen))
    assert seen[sr.SNAP] >= 10 and seen[sr.STEEP] >= 5


def test_upside_down_branch_and_its_threshold(ra, maps):
    """step 5 with w < 1e-6: exact half turns, the sweep about x by pi - eps, and the two adjacent float32 rotations either side of the
    threshold; on the plane and on the plane wound downwards, where the flip of step 3 comes first -- the same bytes"""
    up, down = sc.upside_down_cloud("plane"), sc.upside_down_cloud("plane_down")
    n = len(up["poses"])
    w = np.array([sc.align_w(sr.pose_Rt(up["poses"][i])[0]) for i in range(n)], F)
    taken = w < F(1e-6)
    qa, qb = sr.pose_Rt(up["poses"][n - 2])[0], sr.pose_Rt(up["poses"][n - 1])[0]
    pu, au, su, iu = maps["plane"].check(up["poses"], up["attrs"], up["p"])
    pd, ad, sd, idn = maps["plane_down"].check(down["poses"], down["attrs"], down["p"])
    print("upside down:", counts(iu), "| wound downwards:", counts(idn), "| branch taken by %d of %d, w == 0 for %d" % (taken.sum(), n, (w == 0).sum()))
    print("threshold pair: R.w %s (w = %.8g, taken) and %s (w = %.8g, not taken), R.x %s" % (sc.hex32(qa[3]), w[n - 2], sc.hex32(qb[3]), w[n - 1], sc.hex32(qa[0])))
    assert taken.sum() >= 6 and (~taken).sum() >= 4 and taken[n - 2] and not taken[n - 1]
    assert su["n_snapped"] == n and sd["n_snapped"] == n and idn["flipped"].all() and not iu["flipped"].any()
    # (check() held the device to pu and pd; they are each other's bytes too)
    assert pu.tobytes() == pd.tobytes() and au.tobytes() == ad.tobytes()
    pg = gpu_constrain(ra, maps["plane"].ctx, maps["plane"].upd, up["poses"], up["attrs"], up["p"])[0]
    R0 = sr.pose_Rt(pg[0])[0]
    assert np.array_equal(np.abs(R0), np.array([0, 0, 0, 1], F))                            # the pure x half turn ends on the identity
    R1 = sr.pose_Rt(pg[1])[0]
    assert np.array_equal(sr.qrot(R1, (0, 0, 1)), np.array([0, 0, 1], F)) and np.array_equal(sr.qrot(R1, (1, 0, 0)), np.array([-1, 0, 0], F))
    R2, R3 = sr.pose_Rt(pg[2])[0], sr.pose_Rt(pg[3])[0]
    assert np.allclose(sr.qrot(R2, (0, 0, 1)), [0, 0, 1], atol=3e-7) and np.allclose(sr.qrot(R2, (1, 0, 0)), [0, 1, 0], atol=3e-7)
    assert np.allclose(sr.qrot(R3, (1, 0, 0)), [math.cos(math.radians(37.0)), math.sin(math.radians(37.0)), 0], atol=3e-7)
    # the fused launch runs the same text
    from rmcl_amd import types as T
    maps["plane"].check_fused(up["poses"], up["attrs"], up["p"], T.identity(), 0.0, False)


def test_every_attitude_both_axes(ra, maps):
    """uniformly random attitudes in the cube room: body-axis rays in every direction reach walls and the ceiling, steep faces and
    normals flipped on the underside; 1 025 particles (five workgroups, a ragged last wave) and the first 65 of them"""
    M = maps["cube"]
    poses, attrs = sc.attitude_cloud(1025)
    for axis in (0, 1):
        probes = sr.probes_of(M.mesh, poses, sr.params(axis=axis, **sc.PROBE), bvh=False, normals=M.normals)
        for align in (0, 1):
            for on_miss in (0, 1):
                p = sr.params(axis=axis, align=align, on_miss=on_miss, **sc.PROBE)
                for n in (1025, 65):
                    _, _, sref, info = M.check(poses[:n], attrs[:n], p, probes=probes[:n])
                    if n == 1025 and align == 1 and on_miss == 0:
                        print("attitudes axis %d:" % axis, counts(info))
                        assert sref["n_snapped"] >= 50 and sref["n_missed"] >= 50 and info["flipped"].sum() >= 20
                        assert sref["n_steep"] >= (50 if axis else 0)


def test_non_unit_quaternions(ra, maps):
    """the motion update never renormalises: a = R * (0, 0, 1) is no unit vector, and D, t_hit and tfar are in its units"""
    ns = len(sc.NONUNIT_SCALES)
    for c in sc.nonunit_cloud():
        for on_miss in (0, 1):
            _, _, sref, info = maps[c["map"]].check(c["poses"], c["attrs"], dict(c["p"], on_miss=on_miss))
        cls = info["cls"].reshape(ns, -1)
        print("non-unit, %s axis %d align %d:" % (c["map"], c["p"]["axis"], c["p"]["align"]), counts(info),
              "| class differs between norm 0.5 and norm 2 for %d poses" % int((cls[0] != cls[1]).sum()))


def test_hand_maps(ra, maps):
    """every hand map with a small cloud of its own: zero-extent boxes, axis-parallel rays in box planes and along shared edges"""
    cases = sc.hand_clouds()
    small = {}
    for name in sc.MAPS:      # a handle with a max_n_meas of its own per map
        small[name] = ra.TFMotionUpdaterHip(maps[name].hm, check_collision=False)
        small[name].config.max_n_meas = 777
        small[name].init()
        ra._capi.check(ra._capi.lib().rmclhip_pf_set_params(small[name]._h, C.byref(small[name].config)))
    by = {}
    for c in cases:
        M = maps[c["map"]]
        _, _, sref, info = M.check(c["poses"], c["attrs"], c["p"])
        print("hand map %-10s axis %d:" % (c["map"], c["p"]["axis"]), counts(info))
        claimed = c["want"] >= 0
        assert np.array_equal(info["cls"][claimed], c["want"][claimed])
        by[(c["map"], c["p"]["axis"])] = (c, sref, info)
        _, a1, s1, _ = M.check(c["poses"], c["attrs"], dict(c["p"], on_miss=1), upd=small[c["map"]], max_n_meas=777)
        lost = info["cls"] != sr.SNAP
        assert s1 == sref and np.all(a1["likelihood"]["n_meas"][lost] == 777) and np.all(a1["likelihood"]["mean"][lost] == 0)
        assert a1[~lost].tobytes() == c["attrs"][~lost].tobytes() and np.array_equal(a1["state_sigma"], c["attrs"]["state_sigma"])
    assert by[("hole", 0)][2]["cls"][:3].tolist() == [sr.SNAP, sr.MISS, sr.SNAP]
    assert by[("face80", 0)][2]["cls"][0] == sr.STEEP
    assert by[("wall_x1", 0)][2]["cls"][0] == sr.MISS and by[("wall_x1", 1)][2]["cls"][0] == sr.STEEP
    c, _, info = by[("stack", 0)]
    assert info["flipped"][:3].tolist() == [True, False, False] and [int(x) in fs for x, fs in zip(info["face"][:3], sc.STACK_FACES)] == [True] * 3
    pg = gpu_constrain(ra, maps["stack"].ctx, maps["stack"].upd, c["poses"], c["attrs"], c["p"])[0]
    assert [float(z) for z in pg["t"]["z"][:3]] == list(sc.STACK_Z)
    # the counts belong to the call: a second call on the same handle returns its own, and a call on another map's handle in between
    # leaves them alone
    ch, sh, _ = by[("hole", 0)]
    ck, sk, _ = by[("kerb", 1)]
    assert sh != sk
    H, K = maps["hole"], maps["kerb"]
    assert gpu_constrain(ra, H.ctx, H.upd, ch["poses"], ch["attrs"], ch["p"])[2] == sh
    assert gpu_constrain(ra, K.ctx, K.upd, ck["poses"], ck["attrs"], ck["p"])[2] == sk
    assert H.upd.surface_stats() == sh and K.upd.surface_stats() == sk
    first = gpu_constrain(ra, H.ctx, H.upd, ch["poses"][:7], ch["attrs"][:7], ch["p"])[2]
    assert first == H.ref(ch["poses"][:7], ch["attrs"][:7], ch["p"])[2] and first["n_particles"] == 7 and K.upd.surface_stats() == sk


def test_map_five_kilometres_out(ra, maps):
    """particles ON a map 5 km from the origin: the quantised boxes stay conservative there and the guarded slab test keeps the
    axis-parallel rays; the same cloud at the origin"""
    near, far = sc.far_cloud()
    for name, (poses, attrs) in (("ramp30", near), ("ramp30_far", far)):
        for axis in (0, 1):
            for align, on_miss in ((1, 0), (0, 1)):
                _, _, sref, info = maps[name].check(poses, attrs, sr.params(axis=axis, align=align, on_miss=on_miss, **sc.PROBE))
            print("far cloud on %-10s axis %d:" % (name, axis), counts(info))
            assert sref["n_snapped"] >= 100 and sref["n_missed"] >= 30 and sref["n_steep"] >= (5 if axis else 0)


def test_ragged_and_dead_waves(ra, maps):
    """the traversal votes and every lane must call it: counts around one wave, a wave whose 64 poses are all non-finite, a wave with
    one finite pose.  Non-finite particles come back untouched, count as missed and have no face; their neighbours get the bytes they
    get in a cloud without them."""
    M = maps["cube"]
    base_p, base_a = sc.wave_base()
    for axis in (0, 1):
        p = sr.params(axis=axis, align=1, on_miss=0, **sc.PROBE)
        full_p, full_a, _, _ = M.ref(base_p, base_a, p)
        for name, (poses, attrs, dead) in sc.wave_clouds().items():
            n = len(poses)
            pr, ar, sref, info = M.check(poses, attrs, p)
            print("wave cloud %-11s axis %d:" % (name, axis), counts(info, dead))
            live = ~dead
            assert pr[live].tobytes() == full_p[:n][live].tobytes() and ar[live].tobytes() == full_a[:n][live].tobytes()
            assert pr[dead].tobytes() == poses[dead].tobytes() and ar[dead].tobytes() == attrs[dead].tobytes()
            assert np.all(info["cls"][dead] == sr.MISS) and np.all(ref_faces(info)[dead] == NO_FACE)
            assert sref["n_missed"] >= int(dead.sum()) and sref["n_snapped"] + sref["n_missed"] + sref["n_steep"] == n
            M.check(poses, attrs, dict(p, on_miss=1))


def test_kerb_lifted_segment(ra, maps):
    """the one case with a known answer for "climbed" against "wall": a kerb of 0.3 m driven up with probe_up 0.5 and 0.2, by one
    particle and by a row of 65, down again, and along the riser's plane"""
    M = maps["kerb"]
    for c in sc.kerb_steps():
        for rate in (0.0, 0.25):
            pr, ar, sref, killed = M.check_fused(c["poses"], c["attrs"], c["p"], c["step"], rate, True)
            assert np.array_equal(killed, c["want_killed"]) and np.array_equal(ar["likelihood"]["n_meas"][killed], np.full(int(killed.sum()), 10000))
            assert (sref["n_snapped"], sref["n_missed"], sref["n_steep"]) == tuple(int((c["want"] == k).sum()) for k in range(3))
        print("kerb, %s:" % c["name"], sref, "killed %d" % int(killed.sum()))
        if c["name"].startswith("up"):
            # the constraint off: the unlifted segment at z = 0.1 crosses the riser, whatever probe_up says
            plain = M.fused(True)
            plain.surface = None
            d_p, d_a = ra.DeviceArray.from_host(M.ctx, c["poses"]), ra.DeviceArray.from_host(M.ctx, c["attrs"])
            plain.update(d_p, d_a, len(c["poses"]), c["step"], 0.0)
            pg, ag = d_p.download(), d_a.download()
            assert np.all(ag["likelihood"]["mean"] == 0) and np.all(ag["likelihood"]["sigma"] == 0) and np.all(ag["likelihood"]["n_meas"] == 10000)
            assert np.all(pg["t"]["x"] == 1.5) and np.array_equal(pg["t"]["z"], c["poses"]["t"]["z"])
            po, ao = c["poses"].copy(), c["attrs"].copy()
            M.mesh.pf_motion_update(po, ao, c["step"], 0.0, collision=True, bvh=False)      # the oracle's unconstrained update, in place
            assert pg.tobytes() == po.tobytes() and ag.tobytes() == ao.tobytes()


def test_sharded_small_clouds(ra, maps):
    """a loopback communicator of 3 ranks and clouds of 2 (one rank holds none), 3, 65 and 192 particles (the last with a dead wave):
    the standalone pass, the motion update with the constraint and the counts equal the single-device calls byte for byte"""
    from rmcl_amd import types as T
    M = maps["cube"]
    base_p, base_a = sc.wave_base()
    waves = sc.wave_clouds()
    clouds = [(base_p[:2], base_a[:2], True), (base_p[:3], base_a[:3], True), waves["n65"][:2] + (True,), waves["dead_middle"][:2] + (False,)]
    p = sr.params(axis=1, align=1, on_miss=1, **sc.PROBE)
    cp = sr.to_capi(ra, p)
    step = T.transform_from_rpy((0.3, 0.05, 0.0), (0.0, 0.0, 0.1))
    sh = ra.ShardedParticleFilterHip(M.v, M.f, devices=(0, 0, 0), loopback=True)
    try:
        for poses, attrs, finite in clouds:
            n = len(poses)
            # the standalone pass
            sh.set_particles(poses, attrs)
            st_sh = sh.constrain_to_surface(cp)
            pr, ar, sref, info = M.check(poses, attrs, p)
            ps, as_ = sh.download()
            print("sharded, %d particles on 3 ranks:" % n, counts(info))
            assert st_sh == sref and sh.surface_stats() == sref
            assert ps.tobytes() == pr.tobytes() and as_.tobytes() == ar.tobytes()
            # the motion update with the constraint, collision on
            upd = M.fused(True)
            upd.surface = cp
            d_p, d_a = ra.DeviceArray.from_host(M.ctx, poses), ra.DeviceArray.from_host(M.ctx, attrs)
            upd.update(d_p, d_a, n, step, 0.01)
            sh.set_particles(poses, attrs)
            sh.set_surface(cp)
            sh.motion_update(step, 0.01, check_collision=True)
            ps, as_ = sh.download()
            assert sh.surface_stats() == upd.surface_stats() and upd.surface_stats()["n_particles"] == n
            assert ps.tobytes() == d_p.download().tobytes() and as_.tobytes() == d_a.download().tobytes()
            if finite:
                M.check_fused(poses, attrs, p, step, 0.01, True)
            sh.set_surface(None)
    finally:
        sh.close()
