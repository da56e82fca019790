"""GPU tests of the surface constraint (include/rmclhip.h, "surface-constrained motion"): the standalone kernel (k_surface_constrain) and
the fused case of the motion kernel against the numpy float32 restatement (tests/surface_ref.py) -- BIT FOR BIT on poses, attributes and
counts; the face every probe hit (rmclhip_debug_surface_faces) against the oracle's.  Every operation of the rule is + - * / or sqrt,
correctly rounded on both sides: no field is given a tolerance.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import surface_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32
NO_FACE = 0xFFFFFFFF
ROOM = dict(height=0.1, probe_up=0.5, probe_down=1.0, min_up_cos=0.7)


class Scene:
    """a map on the device and in the oracle, a cloud, and the restatement's probes of it per axis (computed once, never changed)"""

    def __init__(self, ra, orc, ctx, meshes, name, n, bb_min, bb_max, seed, probe):
        from rmcl_amd import synthetic as syn
        self.ra, self.ctx = ra, ctx
        self.v, self.f = meshes(name)
        self.mesh = orc.Mesh(self.v, self.f)
        self.normals = self.mesh.face_normals()
        self.hm = ra.import_hip_map(ctx, self.v, self.f)
        self.poses, self.attrs = syn.uniform_particles(n, seed=seed, bb_min=bb_min, bb_max=bb_max)
        rng = np.random.RandomState(seed + 1)
        self.attrs["likelihood"]["n_meas"] = rng.randint(0, 10001, n)
        self.attrs["likelihood"]["mean"] = rng.uniform(0.1, 1, n)
        self.attrs["likelihood"]["sigma"] = rng.uniform(0, 0.1, n)
        self.attrs["state_sigma"] = rng.uniform(0, 1, (n, 6))
        self.probe = probe
        self._probes = {}
        self.upd = ra.TFMotionUpdaterHip(self.hm, check_collision=False)
        self.upd.init()

    def probes(self, axis, bvh=True):
        if (axis, bvh) not in self._probes:
            self._probes[(axis, bvh)] = sr.probes_of(self.mesh, self.poses, sr.params(axis=axis, **self.probe), bvh=bvh, normals=self.normals)
        return self._probes[(axis, bvh)]


def gpu_constrain(ra, ctx, upd, poses, attrs, p, want_faces=True):
    """rmclhip_pf_constrain_to_surface on a copy of the cloud: (poses', attrs', stats, faces)"""
    n = len(poses)
    upd.init()
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_faces = ra.DeviceArray.from_host(ctx, np.full(max(n, 1), 0xABABABAB, np.uint32)) if want_faces else None
    ra._capi.check(ra._capi.lib().rmclhip_debug_surface_faces(upd._h, d_faces.ptr if want_faces else None))
    try:
        st = ra.constrain_to_surface(upd, d_poses, d_attrs, n, sr.to_capi(ra, p))
    finally:
        ra._capi.check(ra._capi.lib().rmclhip_debug_surface_faces(upd._h, None))
    return d_poses.download(), d_attrs.download(), st, (d_faces.download()[:n] if want_faces else None)


def ref_faces(info):
    return np.where(info["face"] < 0, NO_FACE, info["face"]).astype(np.uint32)


@pytest.fixture(scope="module")
def room(ra, orc, ctx, meshes):
    return Scene(ra, orc, ctx, meshes, "room30k", 4099, (-9.9, -9.9, -0.3, -0.2, -0.2, -math.pi), (9.9, 9.9, 2.5, 0.2, 0.2, math.pi), 23, ROOM)


@pytest.fixture(scope="module")
def sphere(ra, orc, ctx, meshes):
    return Scene(ra, orc, ctx, meshes, "sphere20k", 1500, (-6, -6, -9.5, -0.2, -0.2, -math.pi), (6, 6, -4, 0.2, 0.2, math.pi), 29,
                 dict(height=0.1, probe_up=0.5, probe_down=3.0, min_up_cos=0.7))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("on_miss", [0, 1])
def test_room_matches_restatement(ra, room, axis, align, on_miss):
    """room30k, 4 099 particles (17 workgroups, ragged last wave), and the first 257 and the first one of them"""
    p = sr.params(axis=axis, align=align, on_miss=on_miss, **ROOM)
    probes = room.probes(axis)
    for n in (4099, 257, 1):
        pr, ar, sref, info = sr.constrain(room.mesh, room.poses[:n], room.attrs[:n], p, normals=room.normals, probes=probes[:n])
        if n == 4099:
            print("room30k axis %d:" % axis, sref, "flipped", int(info["flipped"].sum()))
            assert sref["n_snapped"] >= n // 10 and sref["n_missed"] >= n // 10
        pg, ag, sg, faces = gpu_constrain(ra, room.ctx, room.upd, room.poses[:n], room.attrs[:n], p)
        assert sg == sref
        assert np.array_equal(faces, ref_faces(info))
        assert pg.tobytes() == pr.tobytes()
        assert ag.tobytes() == ar.tobytes()
        moved = pr.tobytes() != room.poses[:n].tobytes()
        assert moved == (sref["n_snapped"] > 0)
        assert room.upd.surface_stats() == sref


@pytest.mark.parametrize("axis", [0, 1])
def test_sphere_from_inside_flips_normals_and_finds_steep_faces(ra, sphere, axis):
    """sphere20k seen from inside: its normals point outward, so the flip is the normal case; towards the equator the faces get steep"""
    n = len(sphere.poses)
    probes = sphere.probes(axis)
    for align, on_miss in ((1, 0), (0, 1)):
        p = sr.params(axis=axis, align=align, on_miss=on_miss, **sphere.probe)
        pr, ar, sref, info = sr.constrain(sphere.mesh, sphere.poses, sphere.attrs, p, normals=sphere.normals, probes=probes)
        print("sphere20k axis %d:" % axis, sref, "flipped", int(info["flipped"].sum()))
        assert sref["n_steep"] >= n // 100 and int(info["flipped"].sum()) >= n // 4
        pg, ag, sg, faces = gpu_constrain(ra, sphere.ctx, sphere.upd, sphere.poses, sphere.attrs, p)
        assert sg == sref and np.array_equal(faces, ref_faces(info))
        assert pg.tobytes() == pr.tobytes() and ag.tobytes() == ar.tobytes()


def test_cube_rays_along_edges_and_through_vertices_hit_the_oracles_faces(ra, orc, ctx, meshes):
    """particles at exact grid coordinates of the cube's floor: x and y on the vertex lines of cube_room (and half way between them), so
    the ray runs along shared edges, through vertices, in the planes of the walls and in BVH box planes.  The faces must be the
    brute-force oracle's (min t, then min face id)."""
    from rmcl_amd import types as T
    v, f = meshes("cube")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    lin = np.linspace(-5.0, 5.0, 10)
    half = np.concatenate([lin, (lin[:-1] + lin[1:]) / 2])
    xy = [(x, y) for x in lin for y in half] + [(x, y) for x in half for y in lin]
    poses = np.zeros(len(xy), T.TRANSFORM)
    attrs = np.zeros(len(xy), T.PARTICLE_ATTRIBUTES)
    poses["R"]["w"] = 1.0
    poses["t"]["x"], poses["t"]["y"] = np.array(xy, np.float64).T
    poses["t"]["z"] = -5.0 + 0.3
    attrs["likelihood"]["mean"] = 1.0
    upd = ra.TFMotionUpdaterHip(hm)
    for axis in (0, 1):
        p = sr.params(axis=axis, align=1, **ROOM)
        pr, ar, sref, info = sr.constrain(m, poses, attrs, p, bvh=False)
        print("cube grid axis %d:" % axis, sref, "distinct faces", len(set(info["face"].tolist())))
        assert sref["n_snapped"] >= len(xy) // 2
        pg, ag, sg, faces = gpu_constrain(ra, ctx, upd, poses, attrs, p)
        assert np.array_equal(faces, ref_faces(info))
        assert sg == sref and pg.tobytes() == pr.tobytes() and ag.tobytes() == ar.tobytes()


def test_fused_equals_separate_without_collision(ra, room):
    """check_collision == 0: motion_update with the constraint set == motion_update without it, then constrain_to_surface"""
    from rmcl_amd import types as T
    ctx, n = room.ctx, len(room.poses)
    step = T.transform_from_rpy((0.6, -0.1, 0.0), (0.0, 0.0, 0.15))
    rate = ra.combined_forget_rate(0.01, 0.001, 0.61, 0.1)
    for axis, align, on_miss in ((0, 1, 1), (1, 0, 0), (1, 1, 1)):
        p = sr.params(axis=axis, align=align, on_miss=on_miss, **ROOM)
        fused = ra.TFMotionUpdaterHip(room.hm, check_collision=False)
        fused.surface = sr.to_capi(ra, p)
        d_p, d_a = ra.DeviceArray.from_host(ctx, room.poses), ra.DeviceArray.from_host(ctx, room.attrs)
        fused.update(d_p, d_a, n, step, rate)
        plain = ra.TFMotionUpdaterHip(room.hm, check_collision=False)
        assert plain.surface is None and plain.surface_stats() == dict(n_particles=0, n_snapped=0, n_missed=0, n_steep=0)
        e_p, e_a = ra.DeviceArray.from_host(ctx, room.poses), ra.DeviceArray.from_host(ctx, room.attrs)
        plain.update(e_p, e_a, n, step, rate)
        moved = e_p.download()
        st = ra.constrain_to_surface(plain, e_p, e_a, n, sr.to_capi(ra, p))
        assert d_p.download().tobytes() == e_p.download().tobytes() and d_a.download().tobytes() == e_a.download().tobytes()
        assert fused.surface_stats() == st and st["n_snapped"] >= n // 10
        assert moved.tobytes() != e_p.download().tobytes()
        # switching the constraint off again gives the unconstrained bytes
        fused.surface = None
        g_p, g_a = ra.DeviceArray.from_host(ctx, room.poses), ra.DeviceArray.from_host(ctx, room.attrs)
        fused.update(g_p, g_a, n, step, rate)
        assert g_p.download().tobytes() == moved.tobytes()


@pytest.mark.parametrize("axis", [0, 1])
def test_fused_with_collision_matches_restatement(ra, room, axis):
    """collision on: the segment is lifted by the step height.  room30k, a 0.6 m step, 1 031 particles."""
    from rmcl_amd import types as T
    ctx, n = room.ctx, 1031
    poses, attrs = room.poses[:n], room.attrs[:n]
    step = T.transform_from_rpy((0.6, -0.1, 0.0), (0.0, 0.0, 0.15))
    rate = ra.combined_forget_rate(0.01, 0.001, 0.61, 0.1)
    p = sr.params(axis=axis, align=1, on_miss=0, **ROOM)
    pr, ar, sref, killed = sr.motion_update(room.mesh, poses, attrs, step, rate, True, p, normals=room.normals)
    print("room30k collision axis %d:" % axis, sref, "killed", int(killed.sum()))
    assert killed.any() and not killed.all() and sref["n_snapped"] >= n // 10
    upd = ra.TFMotionUpdaterHip(room.hm, check_collision=True)
    upd.surface = sr.to_capi(ra, p)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    upd.update(d_p, d_a, n, step, rate)
    assert upd.surface_stats() == sref
    assert d_p.download().tobytes() == pr.tobytes()
    assert d_a.download().tobytes() == ar.tobytes()


def test_edges_nonfinite_poses_far_particles_and_max_n_meas(ra, room):
    from rmcl_amd import types as T
    ctx, n = room.ctx, 300
    poses, attrs = room.poses[:n].copy(), room.attrs[:n].copy()
    bad = {3: ("t", "x", np.nan), 64: ("t", "z", np.inf), 65: ("R", "w", np.nan), 130: ("R", "y", -np.inf), 299: ("t", "y", -np.inf)}
    for i, (grp, k, val) in bad.items():
        poses[grp][k][i] = val
    poses["t"]["x"][200], poses["t"]["y"][200], poses["t"]["z"][200] = 5000.0, -5000.0, 0.2      # 5 km off the map
    poses["t"]["x"][201], poses["t"]["z"][201] = 3.0e9, 0.2                                      # (and where O * inv leaves float32)
    good = np.array([i for i in range(n) if i not in bad and i not in (200, 201)])
    for axis in (0, 1):
        base = sr.params(axis=axis, align=1, on_miss=0, **ROOM)
        ref_p, ref_a, ref_s, ref_i = sr.constrain(room.mesh, room.poses[:n], room.attrs[:n], base, normals=room.normals, probes=room.probes(axis)[:n])
        pg, ag, sg, faces = gpu_constrain(ra, ctx, room.upd, poses, attrs, base)
        for i in list(bad) + [200, 201]:
            assert faces[i] == NO_FACE and pg[i].tobytes() == poses[i].tobytes() and ag[i].tobytes() == attrs[i].tobytes()
        assert pg[good].tobytes() == ref_p[good].tobytes() and ag[good].tobytes() == ref_a[good].tobytes()      # neighbours unaffected
        n_bad_was_miss = int((ref_i["cls"][list(bad) + [200, 201]] == sr.MISS).sum())
        assert sg["n_missed"] == ref_s["n_missed"] + (len(bad) + 2 - n_bad_was_miss) and sg["n_particles"] == n
        assert sg["n_snapped"] + sg["n_missed"] + sg["n_steep"] == n
        # on_miss = 1 writes {0, 0, max_n_meas} with the HANDLE's max_n_meas, and leaves state_sigma
        upd = ra.TFMotionUpdaterHip(room.hm, check_collision=False)
        upd.config.max_n_meas = 777
        upd.init()
        ra._capi.check(ra._capi.lib().rmclhip_pf_set_params(upd._h, C.byref(upd.config)))
        p1 = sr.params(axis=axis, align=1, on_miss=1, **ROOM)
        pg1, ag1, sg1, _ = gpu_constrain(ra, ctx, upd, poses, attrs, p1, want_faces=False)
        assert sg1 == sg and pg1.tobytes() == pg.tobytes()
        lost = np.ones(n, bool)
        lost[good] = ref_i["cls"][good] != sr.SNAP
        assert np.all(ag1["likelihood"]["n_meas"][lost] == 777) and np.all(ag1["likelihood"]["mean"][lost] == 0) and np.all(ag1["likelihood"]["sigma"][lost] == 0)
        assert ag1[~lost].tobytes() == attrs[~lost].tobytes() and np.array_equal(ag1["state_sigma"], attrs["state_sigma"])
        # ... and through the fused launch
        upd.surface = sr.to_capi(ra, p1)
        d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        upd.update(d_p, d_a, n, T.identity(), 0.0)
        a_f = d_a.download()
        assert np.all(a_f["likelihood"]["n_meas"][lost] == 777) and upd.surface_stats() == sg


def test_invalid_arguments_leave_the_buffers_untouched(ra, room):
    ctx, n = room.ctx, 64
    L = ra._capi.lib()
    d_p, d_a = ra.DeviceArray.from_host(ctx, room.poses[:n]), ra.DeviceArray.from_host(ctx, room.attrs[:n])
    st = ra._capi.SurfaceStats()
    h = room.upd._h
    cases = [dict(height=-0.1), dict(height=np.nan), dict(height=np.inf), dict(probe_up=-1.0), dict(probe_up=np.nan), dict(probe_up=np.inf),
             dict(probe_down=-0.5), dict(probe_down=np.nan), dict(probe_down=np.inf), dict(min_up_cos=-0.01), dict(min_up_cos=1.01),
             dict(min_up_cos=np.nan), dict(axis=2), dict(align=2), dict(on_miss=7)]
    for kw in cases:
        p = ra.types.surface_params(**kw)
        assert L.rmclhip_pf_constrain_to_surface(h, d_p.ptr, d_a.ptr, n, C.byref(p), C.byref(st)) == ra._capi.ERR_INVALID, kw
        assert L.rmclhip_pf_set_surface(h, C.byref(p)) == ra._capi.ERR_INVALID, kw
    good = ra.types.surface_params(**{k: float(v) for k, v in ROOM.items()})
    assert L.rmclhip_pf_constrain_to_surface(h, None, d_a.ptr, n, C.byref(good), C.byref(st)) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_constrain_to_surface(h, d_p.ptr, None, n, C.byref(good), C.byref(st)) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_constrain_to_surface(h, d_p.ptr, d_a.ptr, n, None, C.byref(st)) == ra._capi.ERR_INVALID
    assert b"pf_constrain_to_surface" in L.rmclhip_last_error()
    assert L.rmclhip_pf_constrain_to_surface(h, None, None, 0, C.byref(good), C.byref(st)) == ra._capi.OK      # n == 0: nothing touched
    assert st.as_dict() == dict(n_particles=0, n_snapped=0, n_missed=0, n_steep=0)
    assert d_p.download().tobytes() == room.poses[:n].tobytes() and d_a.download().tobytes() == room.attrs[:n].tobytes()
    # a refused set_surface leaves the handle as it was: off
    from rmcl_amd import types as T
    room.upd.surface = None
    room.upd.update(d_p, d_a, n, T.identity(), 0.0)
    assert d_p.download()["t"].tobytes() == room.poses[:n]["t"].tobytes()


def test_sharded_equals_unsharded(ra, room):
    """a loopback communicator of 3 ranks, 4 099 particles (ragged blocks): the standalone pass, the motion update and one whole step
    with the constraint equal the single-device calls bit for bit, and the summed counts are the single device's"""
    from rmcl_amd import synthetic as syn, types as T
    ctx, n = room.ctx, len(room.poses)
    p = sr.params(axis=1, align=1, on_miss=1, **ROOM)
    cp = sr.to_capi(ra, p)
    step = T.transform_from_rpy((0.3, 0.05, 0.0), (0.0, 0.0, 0.1))
    sh = ra.ShardedParticleFilterHip(room.v, room.f, devices=(0, 0, 0), loopback=True)
    try:
        # the standalone pass
        sh.set_particles(room.poses, room.attrs)
        st_sh = sh.constrain_to_surface(cp)
        d_p, d_a = ra.DeviceArray.from_host(ctx, room.poses), ra.DeviceArray.from_host(ctx, room.attrs)
        st_1 = ra.constrain_to_surface(room.upd, d_p, d_a, n, cp)
        ps, as_ = sh.download()
        assert st_sh == st_1 and sh.surface_stats() == st_1 and st_1["n_snapped"] >= n // 10
        assert ps.tobytes() == d_p.download().tobytes() and as_.tobytes() == d_a.download().tobytes()
        # the motion update with the constraint, collision on
        upd = ra.TFMotionUpdaterHip(room.hm, check_collision=True)
        upd.surface = cp
        upd.update(d_p, d_a, n, step, 0.01)
        sh.set_surface(cp)
        sh.motion_update(step, 0.01, check_collision=True)
        ps, as_ = sh.download()
        assert sh.surface_stats() == upd.surface_stats()
        assert ps.tobytes() == d_p.download().tobytes() and as_.tobytes() == d_a.download().tobytes()
        # one whole step: motion with the constraint -> sensor update -> statistics
        beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::8] * np.float32(3.0))
        Tsb = syn.tsb_offset()
        stats = sh.step(beams, Tsb, T_bnew_bold=step, forget_rate=0.01, check_collision=True)
        upd.update(d_p, d_a, n, step, 0.01)
        sens = ra.PCDSensorUpdaterHip(room.hm)
        sens.init()
        sens.setInput(beams, Tsb)
        sens.update(d_p, d_a)
        ps, as_ = sh.download()
        assert sh.surface_stats() == upd.surface_stats()
        assert ps.tobytes() == d_p.download().tobytes() and as_.tobytes() == d_a.download().tobytes()
        rs = ra.GladiatorResamplerHip(ctx)
        ref = rs.compute_stats(d_a, n)
        assert stats["sum"] == ref["sum"] and stats["max"] == ref["max"]
        # off again: the unconstrained motion update's bytes
        sh.set_surface(None)
        sh.motion_update(step, 0.01, check_collision=True)
        upd.surface = None
        upd.update(d_p, d_a, n, step, 0.01)
        ps, as_ = sh.download()
        assert ps.tobytes() == d_p.download().tobytes() and as_.tobytes() == d_a.download().tobytes()
    finally:
        sh.close()


def test_cpp_example_dumps_the_python_paths_cloud(ra, room, tmp_path):
    """examples/surface_motion_cpp_example.cpp on room30k: init -> constrain -> three constrained motion steps through the C++ adapters;
    its counts and its dumped cloud equal the Python binding's"""
    from test_cpp_adapters import _build
    from rmcl_amd import types as T
    exe = _build(tmp_path, "surface_motion_cpp_example.cpp")
    mesh_bin, cloud_bin = tmp_path / "mesh.bin", tmp_path / "cloud.bin"
    with open(mesh_bin, "wb") as fh:
        fh.write(struct.pack("<II", len(room.v), len(room.f)))
        fh.write(np.ascontiguousarray(room.v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(room.f, np.uint32).tobytes())
    n, seed = 2500, 7
    r = subprocess.run([exe, str(mesh_bin), str(cloud_bin), str(n), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().splitlines()}
    keys = ("n_particles", "n_snapped", "n_missed", "n_steep")
    ctx = room.ctx
    d_p = ra.DeviceArray.from_host(ctx, np.zeros(n, T.TRANSFORM))
    d_a = ra.DeviceArray.from_host(ctx, np.zeros(n, T.PARTICLE_ATTRIBUTES))
    ra.init_particles_uniform(ctx, d_p, d_a, (-9.0, -9.0, -0.3, -0.1, -0.1, -3.14), (9.0, 9.0, 0.8, 0.1, 0.1, 3.14), seed, 0)
    sp = ra.types.surface_params(height=0.1, probe_up=0.5, probe_down=1.0, align=1)
    st = ra.constrain_to_surface(room.hm, d_p, d_a, n, sp)
    assert out["constrain"] == [st[k] for k in keys] and st["n_snapped"] >= n // 10
    upd = ra.TFMotionUpdaterHip(room.hm, check_collision=True)
    upd.surface = ra.types.surface_params(height=0.1, probe_up=0.5, probe_down=1.0, align=1, on_miss=1)
    step = T.transform((0.0, 0.0, 0.024997396, 0.99968752), (0.25, 0.0, 0.0))
    for k in range(3):
        upd.update(d_p, d_a, n, step, 0.01)
        assert out["step_%d" % k] == [upd.surface_stats()[kk] for kk in keys]
    pp, aa = d_p.download(), d_a.download()
    assert out["killed"] == [int((aa["likelihood"]["mean"] == 0).sum())] and 0 < out["killed"][0] < n
    blob = open(cloud_bin, "rb").read()
    assert struct.unpack("<I", blob[:4])[0] == n and len(blob) == 4 + n * 68
    assert blob[4:4 + 32 * n] == pp.tobytes() and blob[4 + 32 * n:] == aa.tobytes()
