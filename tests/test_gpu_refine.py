"""The refinement on the distance field on the device (include/rmclhip.h, REFINE ON THE FIELD): poses and result rows against the
numpy restatement (tests/refine_ref.py, fed with the device's downloaded lattice) byte for byte, the edges, monotone cost, the effect
on a cloud around the truth, the three entry points and the C++ example against each other, and the refusals."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import cpc_cases as cc
import field_ref as fr
import refine_ref as rr

pytestmark = pytest.mark.gpu
F = np.float32
PLANAR = 0b100011

# map: cell, margin
CASES = {"room30k": (0.4, 0.5), "cube": (0.25, 0.5)}
N_PARTICLES = (1, 3, 4, 5, 257)        # the boundaries of four particles per workgroup, and a ragged tail
N_BEAMS = (1, 5, 63, 64, 65, 257)      # rank-one A, fewer than six constraints, the wave's edge


@pytest.fixture(scope="module")
def world(ra, orc, ctx):
    """per map, made once: (vertices, faces, oracle mesh, device map, field, info, downloaded lattice, truth [1], Tsb, scan points)"""
    from rmcl_amd import synthetic as syn, types as T
    cache = {}

    def get(name):
        if name not in cache:
            v, f = cc.build_map(name)
            m = orc.Mesh(v, f)
            hm = ra.import_hip_map(ctx, v, f)
            cell, margin = CASES[name]
            fd = ra.DistanceFieldHip(hm, cell=cell, margin=margin)
            Tsb = syn.tsb_offset()
            truth = np.array([T.transform_from_rpy((1.0, -1.5, 1.2), (0.0, 0.0, 0.5)) if name == "room30k" else syn.pose_c2_truth()]).reshape(1)
            cloud = m.simulate_spherical(syn.model_c1(), Tsb, truth[0], bvh=True)["points"]
            cache[name] = (v, f, m, hm, fd, fd.info(), fd.download(), truth, Tsb, cloud)
        return cache[name]

    yield get
    for w in cache.values():
        w[4].close()


@pytest.fixture(scope="module")
def starts():
    cache = {}

    def get(world, name, n=257):
        if (name, n) not in cache:
            cache[name, n] = rr.perturbed_starts(world(name)[7], n, seed=17)
        return cache[name, n]

    return get


def _capi_params(ra, p):
    return ra.refine_params(iterations=p["iterations"], dof_mask=p["dof_mask"], max_dist=float(p["max_dist"]), max_step_trans=float(p["max_step_trans"]),
                            max_step_rot=float(p["max_step_rot"]), lambda0=float(p["lambda0"]))


def _device(ra, ctx, fd, poses, beams, Tsb, p, call=None):
    """one refinement on a fresh device copy: (poses', rows, stats); call(d_poses, params, d_rows): another entry point"""
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    d_rows = ra.DeviceArray.from_host(ctx, np.full(len(poses), 0xFF, np.uint8).repeat(16).view(rr.RESULT))
    cp = _capi_params(ra, p)
    st = fd.refine(d_poses, beams, Tsb, params=cp, results_dev=d_rows) if call is None else call(d_poses, cp, d_rows)
    return d_poses.download(), d_rows.download(), st


def _same_stats(a, b):
    return all(a[k] == b[k] for k in ("n_particles", "n_moved", "n_no_beams", "n_not_finite")) and \
        struct.pack("<dd", a["cost_before_sum"], a["cost_after_sum"]) == struct.pack("<dd", b["cost_before_sum"], b["cost_after_sum"])


# ---- 1. bit identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, 8])
@pytest.mark.parametrize("n_beams", N_BEAMS)
def test_poses_and_rows_are_the_restatement_byte_for_byte(ra, ctx, world, starts, n_beams, iterations):
    name = "cube" if n_beams in (5, 65) else "room30k"
    v, f, m, hm, fd, info, lat, truth, Tsb, cloud = world(name)
    beams = ra.sample_beams(cloud, n_beams, seed=7)
    assert len(beams) == n_beams
    poses = starts(world, name)
    p = rr.params(iterations=iterations)
    ref_poses, ref_rows, _ = rr.refine(info, lat, poses, beams, Tsb, p)      # particles are independent: a prefix is the smaller cloud
    if iterations == 8 and n_beams >= 63:
        assert (ref_rows["accepted"] > 0).sum() > 200
    for n in N_PARTICLES:
        got_poses, got_rows, st = _device(ra, ctx, fd, poses[:n], beams, Tsb, p)
        assert got_rows.tobytes() == ref_rows[:n].tobytes(), "rows, n = %d: %d differ" % (n, (got_rows != ref_rows[:n]).sum())
        assert got_poses.tobytes() == ref_poses[:n].tobytes(), "poses, n = %d: %d differ" % (n, (got_poses != ref_poses[:n]).sum())
        assert _same_stats(st, rr.refine(info, lat, poses[:n], beams, Tsb, p)[2]) if n <= 5 else st["n_particles"] == n
        if iterations == 0:
            assert got_poses.tobytes() == poses[:n].tobytes() and st["n_moved"] == 0


# ---- 2. edges, monotone ---------------------------------------------------------------------------------------------------------------
def test_edges(ra, ctx, world, starts):
    v, f, m, hm, fd, info, lat, truth, Tsb, cloud = world("room30k")
    beams = ra.sample_beams(cloud, 64, seed=7)
    poses = starts(world, "room30k").copy()
    poses[2]["t"]["y"] = np.nan
    poses[3]["R"]["w"] = np.inf
    poses[4]["t"]["x"] = 500.0                                     # every end point outside the lattice
    poses[256]["t"]["z"] = -np.inf
    p = rr.params()
    ref_poses, ref_rows, ref_st = rr.refine(info, lat, poses, beams, Tsb, p)
    got_poses, got_rows, st = _device(ra, ctx, fd, poses, beams, Tsb, p)
    assert got_poses.tobytes() == ref_poses.tobytes() and got_rows.tobytes() == ref_rows.tobytes() and _same_stats(st, ref_st)
    assert st["n_not_finite"] == 3 and st["n_no_beams"] == 1 and st["n_particles"] == 257 and st["n_moved"] == int((got_rows["accepted"] > 0).sum())
    for i in (2, 3, 4, 256):
        assert got_poses[i:i + 1].tobytes() == poses[i:i + 1].tobytes() and got_rows["n_used"][i] == 0 and got_rows["accepted"][i] == 0
    # monotone: on all 257 particles
    assert np.all(got_rows["cost_after"] <= got_rows["cost_before"])
    # a NaN-range beam is not used
    bad = beams.copy()
    bad["range"][11] = np.nan
    p0 = rr.params(iterations=0)
    rows_good = _device(ra, ctx, fd, truth, beams, Tsb, p0)[1]
    rows_bad = _device(ra, ctx, fd, truth, bad, Tsb, p0)[1]
    assert rows_bad["n_used"][0] == rows_good["n_used"][0] - 1 and rows_bad.tobytes() == rr.refine(info, lat, truth, bad, Tsb, p0)[1].tobytes()
    got_poses, got_rows, _ = _device(ra, ctx, fd, poses, bad, Tsb, p)
    ref = rr.refine(info, lat, poses, bad, Tsb, p)
    assert got_poses.tobytes() == ref[0].tobytes() and got_rows.tobytes() == ref[1].tobytes()
    # dof_mask 0 leaves every pose byte unchanged
    got_poses, got_rows, st = _device(ra, ctx, fd, poses, beams, Tsb, rr.params(dof_mask=0))
    assert got_poses.tobytes() == poses.tobytes() and st["n_moved"] == 0 and got_rows["cost_before"].tobytes() == got_rows["cost_after"].tobytes()
    # results and counts are optional
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    L = ra._capi.lib()
    b = np.ascontiguousarray(beams)
    assert L.rmclhip_field_refine(fd.handle, C.c_void_p(d_poses.ptr), len(poses), b.ctypes.data_as(C.c_void_p), len(b),
                                  np.ascontiguousarray(Tsb).ctypes.data_as(C.c_void_p), None, None, None) == ra._capi.OK     # params NULL: the defaults
    assert d_poses.download().tobytes() == ref_poses.tobytes()
    assert L.rmclhip_field_refine(fd.handle, None, 0, None, 0, None, None, None, None) == ra._capi.OK                     # n == 0: nothing is touched


def test_planar_mask_and_step_limits(ra, ctx, world):
    v, f, m, hm, fd, info, lat, truth, Tsb, cloud = world("room30k")
    beams = ra.sample_beams(cloud, 64, seed=7)
    poses = rr.perturbed_starts(truth, 257, seed=19, z=False)      # yaw-only poses
    p = rr.params(dof_mask=PLANAR)
    got_poses, got_rows, _ = _device(ra, ctx, fd, poses, beams, Tsb, p)
    ref = rr.refine(info, lat, poses, beams, Tsb, p)
    assert got_poses.tobytes() == ref[0].tobytes() and got_rows.tobytes() == ref[1].tobytes() and (got_rows["accepted"] > 0).sum() > 200
    assert got_poses["t"]["z"].tobytes() == poses["t"]["z"].tobytes() and np.all(got_poses["R"]["x"] == 0) and np.all(got_poses["R"]["y"] == 0)
    # the step limits bind: |delta t| <= iterations * max_step_trans plus the rounding of t + float(v) (3 axes, half an ulp of |t| < 16 each)
    p = rr.params(iterations=4, max_step_trans=1e-3, max_step_rot=1e-3)
    poses = rr.perturbed_starts(truth, 257, seed=23)
    got_poses, got_rows, _ = _device(ra, ctx, fd, poses, beams, Tsb, p)
    moved = np.sqrt(((rr.pose_arrays(got_poses)[1].astype(np.float64) - rr.pose_arrays(poses)[1]) ** 2).sum(axis=1))
    assert (got_rows["accepted"] > 0).sum() > 200 and np.all(moved <= 4 * (1e-3 * (1 + 1e-6) + 3e-6))
    assert got_poses.tobytes() == rr.refine(info, lat, poses, beams, Tsb, p)[0].tobytes()


# ---- 3. effect at test size, attributes, the filter handle's entry point ---------------------------------------------------------------
def test_effect_on_a_cloud_around_the_truth(ra, orc, ctx, world):
    from rmcl_amd import synthetic as syn, types as T
    v, f, m, hm, _, _, _, truth, Tsb, cloud = world("room30k")
    beams = ra.sample_beams(cloud, 64, seed=7)
    fine = ra.DistanceFieldHip(hm, cell=fr.RANKING_CELL, margin=0.5)
    info, lat = fine.info(), fine.download()
    poses = rr.perturbed_starts(truth, 257, seed=29)
    attrs = syn.uniform_particles(257, seed=1)[1]
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.setInput(beams, Tsb)
    with pytest.raises(ra.RmclHipError) as e:                      # no field set
        upd.refine(ra.DeviceArray.from_host(ctx, poses))
    assert e.value.status == ra._capi.ERR_INVALID
    upd.set_field(fine)

    def update(p):
        d_poses, d_attrs = ra.DeviceArray.from_host(ctx, p), ra.DeviceArray.from_host(ctx, attrs)
        upd.update(d_poses, d_attrs)
        return d_attrs.download()["likelihood"]["mean"].astype(np.float64)

    p = rr.params()
    ref_poses, ref_rows, ref_st = rr.refine(info, lat, poses, beams, Tsb, p)
    got_poses, got_rows, st = _device(ra, ctx, fine, poses, beams, Tsb, p)
    assert got_poses.tobytes() == ref_poses.tobytes() and got_rows.tobytes() == ref_rows.tobytes() and _same_stats(st, ref_st)
    # rmclhip_pf_refine equals rmclhip_field_refine, and attributes are byte-identical before and after
    d_attrs = ra.DeviceArray.from_host(ctx, attrs)
    pf_poses, pf_rows, pf_st = _device(ra, ctx, fine, poses, beams, Tsb, p, call=lambda d, cp, r: upd.refine(d, params=cp, results_dev=r))
    assert pf_poses.tobytes() == got_poses.tobytes() and pf_rows.tobytes() == got_rows.tobytes() and _same_stats(pf_st, st)
    assert d_attrs.download().tobytes() == attrs.tobytes()
    before, after = update(poses), update(got_poses)
    e0, e1 = rr.position_error(poses, truth), rr.position_error(got_poses, truth)
    print("mean likelihood %.5g -> %.5g; median position error %.4f -> %.4f m; moved %d of 257" %
          (before.mean(), after.mean(), np.median(e0), np.median(e1), st["n_moved"]))
    assert after.mean() > before.mean()
    assert np.median(e1).tobytes() == np.median(rr.position_error(ref_poses, truth)).tobytes() and np.median(e1) < np.median(e0)
    upd.close()
    fine.close()


# ---- 4. sharded, the example ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 3])
def test_sharded_refine_equals_the_unsharded_one(ra, ctx, world, starts, ranks):
    from rmcl_amd import synthetic as syn, types as T
    v, f, m, hm, fd, info, lat, truth, Tsb, cloud = world("room30k")
    beams = ra.sample_beams(cloud, 64, seed=7)
    poses = starts(world, "room30k")                               # 257 particles: a ragged split over 2 and over 3 ranks
    attrs = syn.uniform_particles(257, seed=1)[1]
    p = rr.params()
    single_poses, single_rows, single_st = _device(ra, ctx, fd, poses, beams, Tsb, p)
    spf = ra.ShardedParticleFilterHip(v, f, devices=(0,) * ranks, loopback=True)
    spf.config_ = T.pf_params(correspondence_type=1)
    spf.set_particles(poses, attrs)
    with pytest.raises(ra.RmclHipError) as e:                      # no field set
        spf.refine(beams, Tsb)
    assert e.value.status == ra._capi.ERR_INVALID
    spf.set_field(cell=CASES["room30k"][0], margin=CASES["room30k"][1])
    st = spf.refine(beams, Tsb, params=_capi_params(ra, p))
    got_poses, got_attrs = spf.download()
    assert got_poses.tobytes() == single_poses.tobytes() and got_attrs.tobytes() == attrs.tobytes()
    assert all(st[k] == single_st[k] for k in ("n_particles", "n_moved", "n_no_beams", "n_not_finite"))
    assert abs(st["cost_after_sum"] - single_st["cost_after_sum"]) <= 1e-12 * single_st["cost_after_sum"]     # rank sums added in rank order
    with pytest.raises(ra.RmclHipError):
        spf.refine(beams, Tsb, iterations=65)
    spf.close()


def test_example_matches_the_python_binding(ra, ctx, world, tmp_path):
    from rmcl_amd import pf, types as T
    exe = rr.build_example(tmp_path)
    v, f, m, hm, fd, info, lat, truth, _, _ = world("room30k")
    from rmcl_amd import synthetic as syn
    cloud = m.simulate_spherical(syn.model_c1(), T.identity(), truth[0], bvh=True)["points"]
    beams = ra.sample_beams(cloud, 64, seed=7)
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    with open(tmp_path / "guess.bin", "wb") as fh:
        fh.write(struct.pack("<I", 1) + truth.tobytes())
    with open(tmp_path / "beams.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(beams)) + beams.tobytes())
    cell, margin = CASES["room30k"]
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "guess.bin"), str(tmp_path / "beams.bin"), repr(cell), repr(margin), "65"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    n = 65
    d_poses = ra.DeviceArray(ctx, T.TRANSFORM, n)
    d_attrs = ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    cov = np.zeros((6, 6))
    cov[0, 0] = cov[1, 1] = cov[2, 2] = 0.15 * 0.15
    cov[5, 5] = 0.08 * 0.08
    pf.init_particles_pose(ctx, d_poses, d_attrs, truth[0], cov, seed=7)
    d_rows = ra.DeviceArray(ctx, rr.RESULT, n)
    st = fd.refine(d_poses, beams, T.identity(), results_dev=d_rows)
    rows = d_rows.download()
    assert [int(x) for x in out["particles"][0::2]] == [st["n_particles"], st["n_moved"], st["n_no_beams"], st["n_not_finite"]]
    assert struct.pack("<d", float(out["cost_before"][0])) == struct.pack("<d", st["cost_before_sum"])
    assert struct.pack("<d", float(out["cost_after"][0])) == struct.pack("<d", st["cost_after_sum"])
    assert st["cost_after_sum"] < st["cost_before_sum"] and st["n_moved"] > 32
    flat = [x for i in range(3) for x in (rows["cost_before"][i], rows["cost_after"][i])]
    assert np.array([float(out["rows"][4 * i + k]) for i in range(3) for k in (0, 1)], F).tobytes() == np.array(flat, F).tobytes()
    assert [int(out["rows"][4 * i + k]) for i in range(3) for k in (2, 3)] == [int(rows[c][i]) for i in range(3) for c in ("n_used", "accepted")]
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.set_field(fd)
    upd.setInput(beams, T.identity())
    upd.update(d_poses, d_attrs)
    upd.close()
    assert np.array([float(x) for x in out["means"]], F).tobytes() == d_attrs.download()["likelihood"]["mean"][:3].tobytes()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ra, ctx, world, starts):
    from rmcl_amd import types as T
    v, f, m, hm, fd, info, lat, truth, Tsb, cloud = world("room30k")
    beams = ra.sample_beams(cloud, 9, seed=7)
    poses = starts(world, "room30k")[:5]
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    E = ra._capi.ERR_INVALID
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.init()
    upd.set_field(fd)
    upd.setInput(beams, Tsb)
    for bad in rr.BAD_PARAMS:                                         # each bad parameter, mirrored by the restatement's check
        with pytest.raises(ValueError):
            rr.check(rr.params(**bad), 5, 9)
        for call in (lambda: fd.refine(d_poses, beams, Tsb, **bad), lambda: upd.refine(d_poses, **bad)):
            with pytest.raises(ra.RmclHipError) as e:
                call()
            assert e.value.status == E
    for n_beams in (0, rr.MAX_BEAMS + 1):                          # n_beams of 0 and past the bound
        many = np.zeros(n_beams, T.RANGE_MEASUREMENT)
        with pytest.raises(ra.RmclHipError) as e:
            fd.refine(d_poses, many, Tsb)
        assert e.value.status == E
    L = ra._capi.lib()
    b = np.ascontiguousarray(beams)
    tsb = np.ascontiguousarray(Tsb)
    bp, tp = b.ctypes.data_as(C.c_void_p), tsb.ctypes.data_as(C.c_void_p)
    assert L.rmclhip_field_refine(fd.handle, None, 5, bp, len(b), tp, None, None, None) == E        # null buffers with n > 0
    assert L.rmclhip_field_refine(fd.handle, C.c_void_p(d_poses.ptr), 5, None, len(b), tp, None, None, None) == E
    assert L.rmclhip_field_refine(fd.handle, C.c_void_p(d_poses.ptr), 5, bp, len(b), None, None, None, None) == E
    assert d_poses.download().tobytes() == poses.tobytes()                                          # nothing was launched
    # a field of another map is refused by the handle, which then has none to refine on
    fresh = ra.PCDSensorUpdaterHip(hm)
    fresh.init()
    fresh.setInput(beams, Tsb)
    with pytest.raises(ra.RmclHipError) as e:
        fresh.set_field(world("cube")[4])
    assert e.value.status == E
    with pytest.raises(ra.RmclHipError) as e:
        fresh.refine(d_poses)
    assert e.value.status == E
    fresh.close()
    upd.close()
