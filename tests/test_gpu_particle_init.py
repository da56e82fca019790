"""The particle cloud's initialisations and visualisation channels on the device (rmcl_amd/csrc/particles.hip) against the numpy
restatement (tests/particle_init_ref.py): uniform and pose + covariance clouds at the sizes where the launch shape changes, slices,
the sharded filter, the visualisation pack, the refusals, and the C++ example.

Tolerances: attributes, stamps and the uniform cloud's translations are pure IEEE arithmetic -- byte-identical.  Quaternions (and the
pose form's translations, which go through Box-Muller) contain transcendentals evaluated in double and rounded to float on both sides:
atol 1e-6 and the whole 32-B record bit-equal for more than 99.9 % of the particles, the rule of tests/test_gpu_resample.py."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import particle_init_ref as pref

pytestmark = pytest.mark.gpu

COVS, RVIZ_COV = pref.COVS, pref.RVIZ_COV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 4097, 65536)
N_MAX = max(SIZES)
SEED = 0xC0FFEE1234567
BOXES = {"default": ((-50, -50, 0, 0, 0, -math.pi), (50, 50, 0, 0, 0, math.pi)),         # the reference's: z, roll, pitch degenerate
         "open": ((-9, -7, 0.2, -0.2, -0.1, -1.0), (9, 8, 3.0, 0.2, 0.3, 2.0))}
_cache = {}


def _ref(kind, key, make):
    """a reference cloud of N_MAX particles, computed once: particle i is a function of i, so a smaller cloud is its head"""
    if (kind, key) not in _cache:
        p, a = make()
        p.setflags(write=False)
        a.setflags(write=False)
        _cache[(kind, key)] = (p, a)
    return _cache[(kind, key)]


def _tlm():
    from rmcl_amd import types as T
    Tlm = T.transform_from_rpy((1.5, -2.25, 0.3), (0.1, -0.2, 0.7))
    Tlm["stamp"] = 7
    return Tlm


def _poisoned(ra, ctx, n, lead):
    """device buffers of lead + n + 3 records filled with 0xFF; the views the calls get start `lead` records in (a pose buffer that stays
    16-B aligned, an attribute buffer at every 4-B phase of a 16-B line as lead varies)"""
    from rmcl_amd import types as T
    tot = lead + n + 3
    d_p = ra.DeviceArray.from_host(ctx, np.full(tot * 32, 0xFF, np.uint8))
    d_a = ra.DeviceArray.from_host(ctx, np.full(tot * 36, 0xFF, np.uint8))
    return d_p, d_a, d_p.ptr + lead * 32, d_a.ptr + lead * 36, T


def _fetch(d_p, d_a, n, lead, T):
    rp, rawa = d_p.download(), d_a.download()
    assert np.all(rp[:lead * 32] == 0xFF) and np.all(rp[(lead + n) * 32:] == 0xFF), "poses written outside [0, count)"
    assert np.all(rawa[:lead * 36] == 0xFF) and np.all(rawa[(lead + n) * 36:] == 0xFF), "attributes written outside [0, count)"
    return rp[lead * 32:(lead + n) * 32].view(T.TRANSFORM), rawa[lead * 36:(lead + n) * 36].view(T.PARTICLE_ATTRIBUTES)


def _assert_cloud(p, a, p_ref, a_ref, exact_t, what):
    n = len(p_ref)
    assert len(p) == n and len(a) == n
    assert a.tobytes() == a_ref.tobytes(), what
    assert np.array_equal(p["stamp"], p_ref["stamp"]), what
    for k in "xyz":
        if exact_t:
            assert p["t"][k].tobytes() == p_ref["t"][k].tobytes(), (what, k)
        else:
            assert np.allclose(p["t"][k], p_ref["t"][k], rtol=0, atol=1e-6), (what, k)
    for k in "xyzw":
        assert np.allclose(p["R"][k], p_ref["R"][k], rtol=0, atol=1e-6), (what, k)
    same = (np.ascontiguousarray(p).view(np.uint8).reshape(n, 32) == np.ascontiguousarray(p_ref).view(np.uint8).reshape(n, 32)).all(1)
    print("%s: n %d, records bit-equal %.5f %%" % (what, n, 100.0 * same.mean()))
    assert same.mean() > 0.999, what


@pytest.mark.parametrize("box", ["default", "open"])
def test_uniform_init_matches_the_restatement(ra, ctx, box):
    lo, hi = BOXES[box]
    p_ref, a_ref = _ref("uniform", box, lambda: pref.init_uniform(0, N_MAX, lo, hi, SEED, 2))
    for lead, n in enumerate(SIZES):
        d_p, d_a, vp, va, T = _poisoned(ra, ctx, n, lead)
        ra.init_particles_uniform(ctx, vp, va, lo, hi, SEED, epoch=2, count=n)
        p, a = _fetch(d_p, d_a, n, lead, T)
        assert not p["stamp"].any()
        _assert_cloud(p, a, p_ref[:n], a_ref[:n], True, "uniform %s n %d" % (box, n))
        if box == "default":                       # lo == hi gives lo exactly: z = 0, roll = pitch = 0
            assert not p["t"]["z"].any() and not p["R"]["x"].any() and not p["R"]["y"].any()
        lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        for d, k in enumerate("xyz"):
            assert np.all(p["t"][k] >= lo32[d]) and np.all(p["t"][k] <= hi32[d])


def test_uniform_init_depends_on_seed_epoch_and_global_index(ra, ctx):
    from rmcl_amd import types as T
    lo, hi = BOXES["open"]
    n = 300
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)

    def run(seed, epoch, first=0):
        ra.init_particles_uniform(ctx, d_p, d_a, lo, hi, seed, epoch=epoch, first=first)
        return d_p.download()

    base = run(SEED, 2)
    assert base.tobytes() == run(SEED, 2).tobytes()
    for other in (run(SEED, 3), run(SEED + 1, 2), run(SEED ^ (1 << 40), 2)):      # epoch, low key word, high key word
        assert not np.any(other["t"]["x"] == base["t"]["x"])
    # the last particles a 32-bit counter word can name
    first = 0x100000000 - n
    hi_ref, _ = pref.init_uniform(first, n, lo, hi, SEED, 2)
    got = run(SEED, 2, first=first)
    assert got["t"].tobytes() == hi_ref["t"].tobytes()
    with pytest.raises(ra.RmclHipError, match="2\\^32"):
        run(SEED, 2, first=first + 1)
    assert d_p.download().tobytes() == got.tobytes()


@pytest.mark.parametrize("cov", ["rviz", "full", "rank3"])
def test_pose_init_matches_the_restatement(ra, ctx, cov):
    Tlm = _tlm()
    p_ref, a_ref = _ref("pose", cov, lambda: pref.init_pose(0, N_MAX, Tlm, COVS[cov], SEED, 1))
    _, err_host = ra.chol6(COVS[cov])
    for lead, n in enumerate(SIZES):
        d_p, d_a, vp, va, T = _poisoned(ra, ctx, n, lead)
        err = ra.init_particles_pose(ctx, vp, va, Tlm, COVS[cov], SEED, epoch=1, count=n)
        assert err == err_host
        p, a = _fetch(d_p, d_a, n, lead, T)
        _assert_cloud(p, a, p_ref[:n], a_ref[:n], False, "pose %s n %d" % (cov, n))
    # the cloud has the spread it was asked for (the last, largest one): x = L z rotated into the map frame keeps its trace
    d = np.stack([p["t"][k].astype(np.float64) for k in "xyz"], 1)
    want = np.trace(COVS[cov][:3, :3])
    assert abs(d.var(0).sum() - want) < 0.05 * want
    assert np.allclose(d.mean(0), [float(Tlm["t"][k]) for k in "xyz"], atol=5.0 * math.sqrt(want / N_MAX))


def test_pose_init_rviz_covariance_stays_in_the_plane(ra, ctx):
    from rmcl_amd import types as T
    n = 4097
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    ra.init_particles_pose(ctx, d_p, d_a, T.identity(), RVIZ_COV, 42)
    p = d_p.download()
    assert not p["t"]["z"].any() and not p["R"]["x"].any() and not p["R"]["y"].any()     # exactly zero
    assert p["t"]["x"].std() > 0.4 and p["R"]["z"].std() > 0.1


def test_slices_equal_the_whole(ra, ctx):
    """[0, 1001) in one call == [0, 334), [334, 668), [668, 1001) in three calls with `first` set (attribute slices start at 4-B
    phases 0, 8 and 0 of a 16-B line), byte for byte, both initialisations"""
    from rmcl_amd import types as T
    n, cuts = 1001, (0, 334, 668, 1001)
    lo, hi = BOXES["open"]
    calls = {"uniform": lambda p, a, first, count: ra.init_particles_uniform(ctx, p, a, lo, hi, SEED, epoch=5, first=first, count=count),
             "pose": lambda p, a, first, count: ra.init_particles_pose(ctx, p, a, _tlm(), COVS["full"], SEED, epoch=5, first=first, count=count)}
    for name, call in calls.items():
        whole_p, whole_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
        call(whole_p, whole_a, 0, n)
        d_p = ra.DeviceArray.from_host(ctx, np.full(n * 32, 0xFF, np.uint8))
        d_a = ra.DeviceArray.from_host(ctx, np.full(n * 36, 0xFF, np.uint8))
        for b, e in zip(cuts[:-1], cuts[1:]):
            call(d_p.ptr + b * 32, d_a.ptr + b * 36, b, e - b)
        assert d_p.download().tobytes() == whole_p.download().tobytes(), name
        assert d_a.download().tobytes() == whole_a.download().tobytes(), name


def test_sharded_init_equals_the_single_device_cloud(ra, ctx, meshes):
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cube")
    n = 1001
    lo, hi = (-4, -4, -1.5, 0, 0, -3.14), (4, 4, 1.5, 0, 0, 3.14)
    Tlm = T.transform_from_rpy((0.5, -0.3, 0.2), (0, 0, 0.4))
    beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::8] * np.float32(3.0))
    Tsb = syn.tsb_offset()
    sh = ra.ShardedParticleFilterHip(v, f, devices=(0, 0, 0), loopback=True)     # 334 + 334 + 333
    up = ra.ShardedParticleFilterHip(v, f, devices=(0, 0, 0), loopback=True)

    def single(make, m):
        d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, m), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, m)
        make(d_p, d_a)
        return d_p.download(), d_a.download()

    for m in (n, 2500, 5, n):                                                     # re-initialised larger, smaller, and again
        for name in ("uniform", "pose"):
            if name == "uniform":
                sh.init_uniform(m, lo, hi, SEED, epoch=3)
                p1, a1 = single(lambda p, a: ra.init_particles_uniform(ctx, p, a, lo, hi, SEED, epoch=3), m)
            else:
                err = sh.init_pose(m, Tlm, COVS["full"], SEED, epoch=3)
                assert err == ra.chol6(COVS["full"])[1]
                p1, a1 = single(lambda p, a: ra.init_particles_pose(ctx, p, a, Tlm, COVS["full"], SEED, epoch=3), m)
            assert sh.n_total == m
            p, a = sh.download()
            assert p.tobytes() == p1.tobytes() and a.tobytes() == a1.tobytes(), (name, m)
            # the cycle goes on as after set_particles
            up.set_particles(p1, a1)
            st, st_up = sh.step(beams, Tsb), up.step(beams, Tsb)
            assert st == st_up and st["sum"] > 0.0, (name, m, st, st_up)
            assert sh.download()[1].tobytes() == up.download()[1].tobytes()
    sh.init_uniform(0, lo, hi, SEED)                                              # an empty cloud is a cloud
    assert sh.n_total == 0 and len(sh.download()[0]) == 0
    with pytest.raises(ra.RmclHipError, match="bb_min > bb_max"):
        sh.init_uniform(10, hi, lo, SEED)
    with pytest.raises(ra.RmclHipError, match="positive semidefinite"):
        sh.init_pose(10, Tlm, -np.eye(6), SEED)
    sh.close()
    up.close()


def _viz_cloud(n, seed):
    from rmcl_amd import types as T
    rng = np.random.RandomState(seed)
    poses, attrs = pref.init_uniform(0, n, *BOXES["open"], seed, 0)
    attrs["likelihood"]["mean"] = rng.uniform(0, 1, n)
    attrs["likelihood"]["sigma"] = rng.uniform(0, 0.1, n)
    attrs["likelihood"]["n_meas"] = rng.randint(0, 10001, n)
    attrs["likelihood"]["n_meas"][0] = 10000                                       # certain: badness 0
    attrs["state_sigma"] = rng.uniform(0, 1, (n, 6))
    poses["stamp"] = rng.randint(0, 1 << 30, n)
    return poses.astype(T.TRANSFORM), attrs


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_visualization_pack_is_the_restatement(ra, ctx, n):
    poses, attrs = _viz_cloud(n, 5 + n)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    for max_n_meas in (10000, 12345):
        ref = pref.pack_visualization(poses, attrs, max_n_meas)
        got = ra.pack_visualization(ctx, d_p, d_a, n, max_n_meas)
        assert list(got) == list(ref) == list(ra.pf.VISUALIZATION_CHANNELS)
        for k in ref:
            assert got[k].dtype == np.float32 and got[k].tobytes() == ref[k].tobytes(), (k, max_n_meas)
        d_out = ra.DeviceArray.from_host(ctx, np.full(7 * n + 2, np.float32(-1.0), np.float32))
        assert ra.pack_visualization(ctx, d_p, d_a, n, max_n_meas, out_dev=d_out) is None
        dev = d_out.download()
        assert dev[:7 * n].tobytes() == np.concatenate([ref[k] for k in ref]).tobytes() and np.all(dev[7 * n:] == -1.0)
    assert got["badness"].shape == (n,) and ra.pack_visualization(ctx, d_p, d_a, n)["badness"][0] == 0.0   # n_meas == max_n_meas
    assert d_p.download().tobytes() == poses.tobytes() and d_a.download().tobytes() == attrs.tobytes()      # inputs untouched


def test_refusals_return_a_status_and_touch_nothing(ra, ctx):
    from rmcl_amd import _capi, types as T
    L = _capi.lib()
    n = 100
    raw_p, raw_a = np.full(n * 32, 0xFF, np.uint8), np.full(n * 36, 0xFF, np.uint8)
    d_p, d_a = ra.DeviceArray.from_host(ctx, raw_p), ra.DeviceArray.from_host(ctx, raw_a)
    lo, hi = BOXES["open"]
    Tlm = _tlm()
    nan_lo, inf_hi = list(lo), list(hi)
    nan_lo[4], inf_hi[0] = float("nan"), float("inf")
    bad_pose = Tlm.copy()
    bad_pose["t"]["y"] = np.nan
    not_psd = COVS["full"].copy()
    not_psd[1, 1] = -0.2
    nan_cov = COVS["full"].copy()
    nan_cov[3, 0] = np.nan
    cases = [("bb_min > bb_max", lambda: ra.init_particles_uniform(ctx, d_p, d_a, hi, lo, 1)),
             ("non-finite bound", lambda: ra.init_particles_uniform(ctx, d_p, d_a, nan_lo, hi, 1)),
             ("non-finite bound", lambda: ra.init_particles_uniform(ctx, d_p, d_a, lo, inf_hi, 1)),
             ("positive semidefinite", lambda: ra.init_particles_pose(ctx, d_p, d_a, Tlm, not_psd, 1)),
             ("non-finite", lambda: ra.init_particles_pose(ctx, d_p, d_a, Tlm, nan_cov, 1)),
             ("non-finite pose", lambda: ra.init_particles_pose(ctx, d_p, d_a, bad_pose, COVS["full"], 1)),
             ("null particle buffers", lambda: ra.init_particles_uniform(ctx, None, d_a, lo, hi, 1, count=n)),
             ("null particle buffers", lambda: ra.init_particles_uniform(ctx, d_p, None, lo, hi, 1, count=n)),
             ("null particle buffers", lambda: ra.init_particles_pose(ctx, None, None, Tlm, COVS["full"], 1, count=n)),
             ("max_n_meas", lambda: ra.pack_visualization(ctx, d_p, d_a, n, max_n_meas=0)),
             ("null buffers", lambda: ra.pack_visualization(ctx, None, d_a, n))]
    for msg, call in cases:
        with pytest.raises(ra.RmclHipError, match=msg) as e:
            call()
        assert e.value.status == _capi.ERR_INVALID, msg
        assert d_p.download().tobytes() == raw_p.tobytes() and d_a.download().tobytes() == raw_a.tobytes(), msg
    # count == 0 is fine and touches nothing, whatever else is passed
    ra.init_particles_uniform(ctx, None, None, lo, hi, 1, count=0)
    ra.init_particles_uniform(ctx, d_p, d_a, hi, lo, 1, count=0)
    assert ra.init_particles_pose(ctx, d_p, d_a, Tlm, COVS["full"], 1, count=0) == 0.0
    assert L.rmclhip_particles_pack_visualization(ctx.handle, None, None, 0, 10000, None, 0) == _capi.OK
    assert d_p.download().tobytes() == raw_p.tobytes() and d_a.download().tobytes() == raw_a.tobytes()
    assert L.rmclhip_particles_init_uniform(None, None, None, 0, 1, None, None, 1, 0) == _capi.ERR_INVALID


def test_cpp_example_prints_what_python_computes(ra, ctx, meshes, tmp_path):
    from rmcl_amd import types as T
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "particle_init_cpp_example.cpp")
    v, f = meshes("cube")
    mesh_bin = tmp_path / "mesh.bin"
    with open(mesh_bin, "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    n, seed = 1000, 42
    r = subprocess.run([exe, str(mesh_bin), str(n), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}

    lo, hi = (-4.0, -4.0, -1.5, 0.0, 0.0, -3.14), (4.0, 4.0, 1.5, 0.0, 0.0, 3.14)
    beams = np.zeros(3, dtype=T.RANGE_MEASUREMENT)
    for b, d in enumerate(((1, 0, 0), (0, 1, 0), (0.6, 0, 0.8))):
        beams["dir"]["x"][b], beams["dir"]["y"][b], beams["dir"]["z"][b] = d
        beams["range"][b] = 3.0 + b
    hm = ra.import_hip_map(ctx, v, f)
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.init()
    upd.setInput(beams, T.identity())
    rs = ra.GladiatorResamplerHip(ctx)
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    ra.init_particles_uniform(ctx, d_p, d_a, lo, hi, seed)
    upd.update(d_p, d_a)
    st = rs.compute_stats(d_a, n)
    assert [np.float32(x) for x in out["uniform_stats"]] == [np.float32(st["sum"]), np.float32(st["max"])] and st["sum"] > 0
    viz = ra.pack_visualization(ctx, d_p, d_a, n)
    sums = [float(viz[k].astype(np.float64).sum()) for k in ra.pf.VISUALIZATION_CHANNELS]
    assert np.allclose([float(x) for x in out["viz_sums"]], sums, rtol=1e-8, atol=1e-9)
    guess = T.transform((0.0, 0.0, np.float32(0.19866933), np.float32(0.98006658)), (0.5, -0.3, 0.2))
    err = ra.init_particles_pose(ctx, d_p, d_a, guess, RVIZ_COV, seed, epoch=1)
    upd.update(d_p, d_a)
    sp = rs.compute_stats(d_a, n)
    assert [np.float32(x) for x in out["pose_stats"]] == [np.float32(sp["sum"]), np.float32(sp["max"])] and sp["sum"] > 0
    assert float(out["pose_chol_err"][0]) == err and int(out["pose_off_plane"][0]) == 0
    upd.close()
    rs.close()
