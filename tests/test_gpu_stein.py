"""The Stein variational step on the device (include/rmclhip.h, STEIN STEP ON THE FIELD): poses and result rows against the numpy
restatement (tests/stein_ref.py, fed with the device's downloaded lattice) byte for byte, independence of the particles' order, the
edges, the refusals, the effect on a cloud around the truth, and the C++ example against the Python binding."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import cpc_cases as cc
import field_ref as fr
import refine_ref as rr
import stein_ref as sr

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
PLANAR = 0b100011

# map: cell, margin (the maps of tests/test_gpu_refine.py)
CASES = {"room30k": (0.4, 0.5), "cube": (0.25, 0.5)}
N_PARTICLES = (1, 2, 4, 5, 64, 65, 257)   # the boundaries of four particles per workgroup and of a wave of records, a ragged tail


@pytest.fixture(scope="module")
def world(ra, orc, ctx):
    """per map, made once: (device map, field, info, downloaded lattice, truth [1], Tsb, scan points, updater with the field set)"""
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
            upd = ra.PCDSensorUpdaterHip(hm)
            upd.config = T.pf_params(correspondence_type=1)
            upd.init()
            upd.set_field(fd)
            cache[name] = (hm, fd, fd.info(), fd.download(), truth, Tsb, cloud, upd, m)
        return cache[name]

    yield get
    for w in cache.values():
        w[7].close()
        w[1].close()


def _capi_params(ra, p):
    return ra.stein_params(**{k: (int(v) if k in ("iterations", "dof_mask", "max_per_bin", "seed", "step") else float(v)) for k, v in p.items()})


def _device(ra, ctx, upd, poses, p):
    """one call on a fresh device copy: (poses', rows, stats)"""
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    d_rows = ra.DeviceArray.from_host(ctx, np.full(len(poses), 0xFF, np.uint8).repeat(16).view(sr.RESULT))
    st = upd.stein_step(d_poses, params=_capi_params(ra, p), results_dev=d_rows)
    return d_poses.download(), d_rows.download(), st


def _same_stats(a, b):
    return all(a[k] == b[k] for k in ("n_particles", "n_not_finite", "n_no_beams", "n_bins", "n_thinned_bins")) and \
        struct.pack("<d", a["cost_sum"]) == struct.pack("<d", b["cost_sum"])


def _assert_same(got, ref, what):
    assert got[1].tobytes() == ref[1].tobytes(), "rows, %s: %d differ" % (what, (got[1] != ref[1]).sum())
    assert got[0].tobytes() == ref[0].tobytes(), "poses, %s: %d differ" % (what, (got[0] != ref[0]).sum())
    assert _same_stats(got[2], ref[2]), "stats, %s: %r != %r" % (what, got[2], ref[2])


def _cloud(truth, kind, n=257):
    return rr.perturbed_starts(truth, n, seed=17) if kind == "dense" else sr.spread_cloud(truth, n, seed=18)


# ---- 1. byte identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "spread"])
@pytest.mark.parametrize("mask", [0x3F, PLANAR])
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("n_beams", [1, 5, 65])
def test_poses_and_rows_are_the_restatement_byte_for_byte(ra, ctx, world, n_beams, iterations, mask, kind):
    name = "cube" if n_beams == 5 else "room30k"
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world(name)
    beams = ra.sample_beams(cloud, n_beams, seed=7)
    assert len(beams) == n_beams
    upd.setInput(beams, Tsb)
    poses = _cloud(truth, kind)
    p = sr.params(iterations=iterations, dof_mask=mask)
    for n in N_PARTICLES:           # particles are NOT independent: every size is a cloud of its own
        ref = sr.step(info, lat, poses[:n], beams, Tsb, p)
        _assert_same(_device(ra, ctx, upd, poses[:n], p), ref, "n = %d" % n)
        if n == 257 and n_beams == 65:
            nb = ref[1]["n_neighbours"]
            # dense: everybody has neighbours, some more than a wave's lanes; spread: loners, and most bins hold one particle
            assert (nb.min() >= 1 and nb.max() > 64) if kind == "dense" else (nb.min() == 0 and ref[2]["n_bins"] > 100)
            assert (ref[0]["t"]["x"] != poses["t"]["x"]).sum() > 200


def _thinned(truth):
    p = sr.params(max_per_bin=sr.THINNED_MAX_PER_BIN, seed=sr.THINNED_SEED, step=sr.THINNED_STEP)      # one iteration: the premises are the start's
    poses = sr.thinned_cloud(truth, p)
    # the premises, before any device use: one bin, nobody near its edge, and the thinning lists 32 .. 128 of the 1025
    _, t = rr.pose_arrays(poses)
    assert len(poses) == 1025 and len(np.unique(sr.bins(t, p), axis=0)) == 1 and sr.bin_margin(poses, p) >= 0.05
    assert 32 <= int(sr.listed_of(poses, p).sum()) <= 128
    return poses, p


def test_thinned_bin_is_the_restatement_byte_for_byte(ra, ctx, world):
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world("room30k")
    poses, p = _thinned(truth)
    beams = ra.sample_beams(cloud, 5, seed=7)
    upd.setInput(beams, Tsb)
    ref = sr.step(info, lat, poses, beams, Tsb, p)
    listed = int(sr.listed_of(poses, p).sum())
    assert ref[2]["n_bins"] == 1 and ref[2]["n_thinned_bins"] == 1 and ref[1]["n_neighbours"].max() <= listed
    assert ref[1]["kernel_weight"].max() > listed          # a listed neighbour stands for 1025 / listed particles
    _assert_same(_device(ra, ctx, upd, poses, p), ref, "thinned")


# ---- 2. order independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "thinned"])
def test_order_independence(ra, ctx, world, case):
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world("room30k")
    upd.setInput(ra.sample_beams(cloud, 5, seed=7), Tsb)
    if case == "dense":
        poses, p = _cloud(truth, "dense"), sr.params(iterations=3)
    else:
        poses, p = _thinned(truth)
        p = dict(p, max_per_bin=2048)          # unthinned: the listed set does not follow a particle when its index changes
    a = _device(ra, ctx, upd, poses, p)
    b = _device(ra, ctx, upd, poses, p)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and _same_stats(a[2], b[2])
    perm = np.random.RandomState(5).permutation(len(poses))
    c = _device(ra, ctx, upd, poses[perm], p)
    assert c[0].tobytes() == a[0][perm].tobytes() and c[1].tobytes() == a[1][perm].tobytes()
    if case == "thinned":                      # and thinned: the same call twice
        p = _thinned(truth)[1]
        a, b = _device(ra, ctx, upd, poses, p), _device(ra, ctx, upd, poses, p)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges_not_finite_and_no_beams(ra, ctx, world):
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world("room30k")
    beams = ra.sample_beams(cloud, 64, seed=7)
    upd.setInput(beams, Tsb)
    poses = _cloud(truth, "dense").copy()
    poses[2]["t"]["y"] = np.nan
    poses[3]["R"]["w"] = np.inf
    poses[256]["t"]["z"] = -np.inf
    p = sr.params(iterations=2)
    ref = sr.step(info, lat, poses, beams, Tsb, p)
    got = _device(ra, ctx, upd, poses, p)
    _assert_same(got, ref, "not finite")
    assert got[2]["n_not_finite"] == 3
    for i in (2, 3, 256):
        assert got[0][i:i + 1].tobytes() == poses[i:i + 1].tobytes() and got[1]["n_neighbours"][i] == 0 and got[1]["kernel_weight"][i] == 0
    # nobody's neighbour: the others move as in the cloud without them
    keep = np.ones(257, bool)
    keep[[2, 3, 256]] = False
    alone = _device(ra, ctx, upd, poses[keep], p)
    assert alone[0].tobytes() == got[0][keep].tobytes() and alone[1].tobytes() == got[1][keep].tobytes()
    # n_used == 0: a quaternion of a thousand times the unit length sends every end point out of the lattice; with the rotations locked such
    # a particle is still a neighbour, and it is moved by its neighbours alone
    poses = _cloud(truth, "dense").copy()
    lost = [5, 77, 200]
    for k in "xyzw":
        poses["R"][k][lost] *= F(1000.0)
    p = sr.params(dof_mask=0x07)
    ref = sr.step(info, lat, poses, beams, Tsb, p)
    assert (ref[1]["n_used"][lost] == 0).all() and (ref[1]["n_neighbours"][lost] > 0).all() and ref[2]["n_no_beams"] >= 3
    assert all(ref[0][i:i + 1].tobytes() != poses[i:i + 1].tobytes() for i in lost)
    _assert_same(_device(ra, ctx, upd, poses, p), ref, "no beams")
    # results and counts are optional; params NULL: the defaults
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    b = np.ascontiguousarray(beams)
    L = ra._capi.lib()
    assert L.rmclhip_pf_stein_step(upd._h, C.c_void_p(d_poses.ptr), len(poses), b.ctypes.data_as(C.c_void_p), len(b),
                                   np.ascontiguousarray(Tsb).ctypes.data_as(C.c_void_p), None, None, None) == ra._capi.OK
    assert d_poses.download().tobytes() == sr.step(info, lat, poses, beams, Tsb, sr.params())[0].tobytes()
    assert L.rmclhip_pf_stein_step(upd._h, None, 0, None, 0, None, None, None, None) == ra._capi.OK        # n == 0: nothing is touched
    # iterations == 0: nothing is launched
    got = _device(ra, ctx, upd, poses, sr.params(iterations=0))
    assert got[0].tobytes() == poses.tobytes() and got[1].tobytes() == b"\xff" * (16 * len(poses)) and got[2]["n_particles"] == 257


def test_edges_beyond_the_bins_range(ra, ctx, world):
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world("room30k")
    beams = ra.sample_beams(cloud, 5, seed=7)
    upd.setInput(beams, Tsb)
    # +-8192 bins of 0.25025 m end at +-2050 m: clusters beyond them on either side share the clamped bins, as do strangers far apart
    poses = rr.perturbed_starts(truth, 40, seed=31, d_trans=0.08)
    far = np.array([(5000.0, 0.0, 0.0)] * 8 + [(-5000.0, 7000.0, -3000.0)] * 8 + [(9000.0, 0.0, 0.0)] * 4 + [(2049.9, -2049.9, 0.0)] * 8 + [(0.0, 0.0, 0.0)] * 12)
    for i, k in enumerate("xyz"):
        poses["t"][k] = (poses["t"][k].astype(D) + far[:, i]).astype(F)
    p = sr.params(iterations=2)
    ref = sr.step(info, lat, poses, beams, Tsb, p)
    assert (ref[1]["n_neighbours"][:16] > 0).sum() > 8 and ref[2]["n_no_beams"] >= 28 and (ref[1]["n_neighbours"][:28] < 8).all() and ref[2]["n_bins"] < 40
    _assert_same(_device(ra, ctx, upd, poses, p), ref, "beyond the bins")


def test_attributes_pass_through_a_following_update(ra, ctx, world):
    from rmcl_amd import synthetic as syn
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world("room30k")
    upd.setInput(ra.sample_beams(cloud, 64, seed=7), Tsb)
    poses = _cloud(truth, "dense")
    attrs = syn.uniform_particles(257, seed=1)[1]
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    upd.stein_step(d_poses, iterations=2)
    assert d_attrs.download().tobytes() == attrs.tobytes()
    moved = d_poses.download()
    upd.update(d_poses, d_attrs)
    e_poses, e_attrs = ra.DeviceArray.from_host(ctx, moved), ra.DeviceArray.from_host(ctx, attrs)
    upd.update(e_poses, e_attrs)
    assert d_attrs.download().tobytes() == e_attrs.download().tobytes() and d_poses.download().tobytes() == moved.tobytes()
    assert d_attrs.download().tobytes() != attrs.tobytes()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ra, ctx, world):
    from rmcl_amd import types as T
    hm, fd, info, lat, truth, Tsb, cloud, upd, m = world("room30k")
    beams = ra.sample_beams(cloud, 9, seed=7)
    upd.setInput(beams, Tsb)
    poses = _cloud(truth, "dense")[:5]
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    rows = np.full(5, 0xFF, np.uint8).repeat(16).view(sr.RESULT)
    d_rows = ra.DeviceArray.from_host(ctx, rows)
    E = ra._capi.ERR_INVALID

    def refused(call):
        with pytest.raises(ra.RmclHipError) as e:
            call()
        assert e.value.status == E
        assert d_poses.download().tobytes() == poses.tobytes() and d_rows.download().tobytes() == rows.tobytes()

    for bad in sr.BAD_PARAMS:                                         # each bad parameter, mirrored by the restatement's check
        with pytest.raises(ValueError):
            sr.check(sr.params(**bad), 5, 9)
        refused(lambda: upd.stein_step(d_poses, results_dev=d_rows, **bad))
    refused(lambda: upd.stein_step(d_poses, n_particles=sr.MAX_PARTICLES + 1, results_dev=d_rows))     # refused before anything is read
    for n_beams in (0, rr.MAX_BEAMS + 1):                             # n_beams of 0 and past the bound
        upd.setInput(np.zeros(n_beams, T.RANGE_MEASUREMENT), Tsb)
        refused(lambda: upd.stein_step(d_poses, results_dev=d_rows))
    upd.setInput(beams, Tsb)
    L = ra._capi.lib()
    b, tsb = np.ascontiguousarray(beams), np.ascontiguousarray(Tsb)
    bp, tp = b.ctypes.data_as(C.c_void_p), tsb.ctypes.data_as(C.c_void_p)
    assert L.rmclhip_pf_stein_step(upd._h, None, 5, bp, len(b), tp, None, None, None) == E             # null buffers with n > 0
    assert L.rmclhip_pf_stein_step(upd._h, C.c_void_p(d_poses.ptr), 5, None, len(b), tp, None, None, None) == E
    assert L.rmclhip_pf_stein_step(upd._h, C.c_void_p(d_poses.ptr), 5, bp, len(b), None, None, None, None) == E
    assert d_poses.download().tobytes() == poses.tobytes()
    fresh = ra.PCDSensorUpdaterHip(hm)                                # no field set
    fresh.init()
    fresh.setInput(beams, Tsb)
    refused(lambda: fresh.stein_step(d_poses, results_dev=d_rows))
    fresh.close()
    upd.stein_step(d_poses, results_dev=d_rows)                       # and the handle still works
    assert d_poses.download().tobytes() == sr.step(info, lat, poses, beams, Tsb)[0].tobytes()


# ---- 5. effect --------------------------------------------------------------------------------------------------------------------------
def test_effect_on_a_cloud_around_the_truth(ra, ctx, world):
    """profiles/stein_convergence.txt records the four numbers this prints"""
    from rmcl_amd import types as T
    hm, _, _, _, truth, Tsb, cloud, _, m = world("room30k")
    beams = ra.sample_beams(cloud, 64, seed=7)
    fine = ra.DistanceFieldHip(hm, cell=fr.RANKING_CELL, margin=0.5)
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.set_field(fine)
    upd.setInput(beams, Tsb)
    poses = rr.perturbed_starts(truth, 257, seed=29)                  # +-0.3 m, +-0.15 rad
    e0, tr0 = np.median(rr.position_error(poses, truth)), sr.covariance_trace(poses)
    out = {}
    for repulsion in (0.25, 0.0):
        got = _device(ra, ctx, upd, poses, sr.params(iterations=8, repulsion=repulsion))[0]
        out[repulsion] = (np.median(rr.position_error(got, truth)), sr.covariance_trace(got))
        print("repulsion %.2f: median position error %.4f -> %.4f m; covariance trace %.5f -> %.5f m^2" %
              (repulsion, e0, out[repulsion][0], tr0, out[repulsion][1]))
    upd.close()
    fine.close()
    assert out[0.25][0] < e0 and out[0.0][0] < e0
    assert out[0.25][1] > out[0.0][1]


# ---- 6. the example ---------------------------------------------------------------------------------------------------------------------
def test_example_matches_the_python_binding(ra, ctx, world, tmp_path):
    from rmcl_amd import pf, synthetic as syn, types as T
    exe = sr.build_example(tmp_path)
    hm, fd, info, lat, truth, _, _, upd, m = world("room30k")
    cloud = m.simulate_spherical(syn.model_c1(), T.identity(), truth[0], bvh=True)["points"]
    beams = ra.sample_beams(cloud, 64, seed=7)
    v, f = cc.build_map("room30k")
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    with open(tmp_path / "guess.bin", "wb") as fh:
        fh.write(struct.pack("<I", 1) + truth.tobytes())
    with open(tmp_path / "beams.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(beams)) + beams.tobytes())
    cell, margin = CASES["room30k"]
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "guess.bin"), str(tmp_path / "beams.bin"), repr(cell), repr(margin), "65", "4"],
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
    d_rows = ra.DeviceArray(ctx, sr.RESULT, n)
    upd.setInput(beams, T.identity())
    st = upd.stein_step(d_poses, iterations=4, results_dev=d_rows)
    rows = d_rows.download()
    assert [int(x) for x in out["particles"][0::2]] == [st["n_particles"], st["n_not_finite"], st["n_no_beams"], st["n_bins"], st["n_thinned_bins"]]
    assert struct.pack("<d", float(out["cost_sum"][0])) == struct.pack("<d", st["cost_sum"])
    assert st["n_particles"] == 65 and st["n_bins"] > 1 and rows["n_neighbours"].max() > 8
    flat = [x for i in range(3) for x in (rows["cost"][i], rows["kernel_weight"][i])]
    assert np.array([float(out["rows"][4 * i + k]) for i in range(3) for k in (0, 3)], F).tobytes() == np.array(flat, F).tobytes()
    assert [int(out["rows"][4 * i + k]) for i in range(3) for k in (1, 2)] == [int(rows[c][i]) for i in range(3) for c in ("n_used", "n_neighbours")]
    upd.update(d_poses, d_attrs)
    assert np.array([float(x) for x in out["means"]], F).tobytes() == d_attrs.download()["likelihood"]["mean"][:3].tobytes()
