"""The sampled odometry model of the motion update on the device (include/rmclhip.h, MOTION NOISE; k_pf_motion<., ., true>) against the
numpy restatement (tests/motion_noise_ref.py), device against device, and the statistics of what the device draws.

Tolerances.  Attributes and stamps are pure IEEE arithmetic: byte-identical, outside the particles tests/test_motion_noise_cpu.py's
premise (c) leaves out (a last-bit difference of the pose may flip their kill).  Poses go through Box-Muller and the Euler angles'
sines and cosines, evaluated in double and rounded to float on both sides: atol 1e-6 and the whole 32-B record bit-equal for more than
99.9 % of the particles, the rule of tests/test_gpu_resample.py.  The kill itself is exact on the DEVICE's poses.  Device against
device is byte for byte."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import motion_noise_ref as mn
from test_motion_noise_cpu import N_STAT, STAT_SIGMA, check_statistics

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
SEED = mn.SEED
RATE = 0.02


def _poisoned(ra, ctx, poses, attrs, lead):
    """device buffers of lead + n + 3 records filled with 0xFF around the cloud; the views the calls get start `lead` records in"""
    n = len(poses)
    hp = np.full((lead + n + 3) * 32, 0xFF, np.uint8)
    ha = np.full((lead + n + 3) * 36, 0xFF, np.uint8)
    hp[lead * 32:(lead + n) * 32] = np.ascontiguousarray(poses).view(np.uint8).reshape(-1)
    ha[lead * 36:(lead + n) * 36] = np.ascontiguousarray(attrs).view(np.uint8).reshape(-1)
    d_p, d_a = ra.DeviceArray.from_host(ctx, hp), ra.DeviceArray.from_host(ctx, ha)
    return d_p, d_a, d_p.ptr + lead * 32, d_a.ptr + lead * 36


def _fetch(ra, d_p, d_a, n, lead):
    T = ra.types
    rp, rawa = d_p.download(), d_a.download()
    assert np.all(rp[:lead * 32] == 0xFF) and np.all(rp[(lead + n) * 32:] == 0xFF), "poses written outside [0, n)"
    assert np.all(rawa[:lead * 36] == 0xFF) and np.all(rawa[(lead + n) * 36:] == 0xFF), "attributes written outside [0, n)"
    return rp[lead * 32:(lead + n) * 32].view(T.TRANSFORM).copy(), rawa[lead * 36:(lead + n) * 36].view(T.PARTICLE_ATTRIBUTES).copy()


def _run(ra, ctx, upd, poses, attrs, T, sigma, seed=SEED, step=1, first=0, rate=RATE, lead=0):
    """TFMotionUpdaterHip.update with noise on a copy of the cloud in poisoned buffers -> (poses, attrs)"""
    n = len(poses)
    d_p, d_a, vp, va = _poisoned(ra, ctx, poses, attrs, lead)
    upd.update(vp, va, n, T, rate, noise=sigma, seed=seed, step=step, first=first)
    return _fetch(ra, d_p, d_a, n, lead)


def _run_plain(ra, ctx, upd, poses, attrs, T, rate=RATE):
    d_p, d_a, vp, va = _poisoned(ra, ctx, poses, attrs, 0)
    upd.update(vp, va, len(poses), T, rate)
    return _fetch(ra, d_p, d_a, len(poses), 0)


def _killed(a):
    return (a["likelihood"]["n_meas"] == 10000) & (a["likelihood"]["mean"] == 0) & (a["likelihood"]["sigma"] == 0)


class Scene:
    def __init__(self, ra, orc, ctx, meshes, name, poses, attrs, T, sigma, step):
        self.v, self.f = meshes(name)
        self.mesh = orc.Mesh(self.v, self.f)
        self.hm = ra.import_hip_map(ctx, self.v, self.f)
        self.poses, self.attrs, self.T, self.sigma, self.step = poses, attrs, T, np.asarray(sigma, F), step
        for a in (self.poses, self.attrs):
            a.setflags(write=False)
        self.upd = {c: ra.TFMotionUpdaterHip(self.hm, check_collision=c) for c in (False, True)}
        self._ref = {}

    def ref(self, collision):
        """the restatement of the whole cloud, once: particle i depends on i alone, so a smaller cloud is its head"""
        if collision not in self._ref:
            p, a, k = mn.motion_update(self.mesh, self.poses, self.attrs, self.T, RATE, self.sigma, SEED, self.step, collision=collision)
            ex = mn.exclusions(self.mesh, self.poses["t"], p["t"]) if collision else np.zeros(len(p), bool)
            for x in (p, a, k, ex):
                x.setflags(write=False)
            self._ref[collision] = (p, a, k, ex)
        return self._ref[collision]


@pytest.fixture(scope="module")
def wall(ra, orc, ctx, meshes):
    poses, attrs = mn.wall_cloud(max(SIZES))
    return Scene(ra, orc, ctx, meshes, "cube", poses, attrs, mn.wall_step(), mn.WALL_SIGMA, mn.WALL_STEP)


@pytest.fixture(scope="module")
def room(ra, orc, ctx, meshes):
    from rmcl_amd import synthetic as syn
    n = max(SIZES)
    poses, _ = syn.uniform_particles(n, seed=31, bb_min=(-9.5, -9.5, 0.2, -0.1, -0.1, -math.pi), bb_max=(9.5, 9.5, 2.5, 0.1, 0.1, math.pi))
    poses["stamp"] = np.arange(n) * 3 + 1
    T = ra.types.transform_from_rpy((0.5, 0.05, 0.0), (0.0, 0.02, 0.3))
    sigma = ra.motion_noise_sigma(ra.motion_noise_params(alpha_trans_trans=(0.4, 0.2, 0.1)), T)
    assert np.all(sigma > 0)
    return Scene(ra, orc, ctx, meshes, "room30k", poses, mn.randomised_attrs(n, 32), T, sigma, 7)


def _assert_parity(ra, sc, collision, what):
    p_ref, a_ref, k_ref, ex = sc.ref(collision)
    for lead, n in enumerate(SIZES):
        p, a = _run(ra, sc.upd[collision].ctx, sc.upd[collision], sc.poses[:n], sc.attrs[:n], sc.T, sc.sigma, step=sc.step, lead=lead)
        keep = ~ex[:n]
        assert a[keep].tobytes() == a_ref[:n][keep].tobytes(), (what, n)
        assert np.array_equal(p["stamp"], sc.poses["stamp"][:n]), (what, n)
        for grp, ks in (("t", "xyz"), ("R", "xyzw")):
            for k in ks:
                assert np.allclose(p[grp][k], p_ref[grp][k][:n], rtol=0, atol=1e-6), (what, n, grp, k)
        same = (p.view(np.uint8).reshape(n, 32) == np.ascontiguousarray(p_ref[:n]).view(np.uint8).reshape(n, 32)).all(1)
        print("%s: n %d, records bit-equal %.4f %%, left out %d, killed %d" % (what, n, 100.0 * same.mean(), int(ex[:n].sum()), int(_killed(a).sum())))
        assert same.mean() > 0.999, (what, n)
        # the kill, restated on the DEVICE's poses: exact
        if collision:
            assert np.array_equal(_killed(a), mn.kill_flags(sc.mesh, sc.poses["t"][:n], p["t"])), (what, n)
        else:
            assert not _killed(a).any()
        # state_sigma is never touched
        assert a["state_sigma"].tobytes() == sc.attrs["state_sigma"][:n].tobytes()


@pytest.mark.parametrize("collision", [False, True])
def test_wall_scene_matches_the_restatement(ra, wall, collision):
    _assert_parity(ra, wall, collision, "cube wall, collision %d" % collision)
    if collision:   # premise (b) on the device: all four kinds
        p, a = _run(ra, wall.upd[True].ctx, wall.upd[True], wall.poses, wall.attrs, wall.T, wall.sigma, step=wall.step)
        _, a0 = _run_plain(ra, wall.upd[True].ctx, wall.upd[True], wall.poses, wall.attrs, wall.T)
        kn, kp = _killed(a), _killed(a0)
        assert (kn & ~kp).sum() >= 20 and (~kn & kp).sum() >= 20 and (kn & kp).sum() >= 20 and (~kn & ~kp).sum() >= 20


@pytest.mark.parametrize("collision", [False, True])
def test_room_matches_the_restatement(ra, room, collision):
    _assert_parity(ra, room, collision, "room30k, collision %d" % collision)
    if collision:
        assert 10 <= room.ref(True)[2].sum() <= len(room.poses) - 10


def test_slices_with_first_index_equal_the_whole_call(ra, ctx, wall):
    upd = wall.upd[True]
    n = len(wall.poses)
    p, a = _run(ra, ctx, upd, wall.poses, wall.attrs, wall.T, wall.sigma, step=wall.step)
    for cuts in ((0, 1, 64, 65, 700, n), (0, 333, n)):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ps, as_ = _run(ra, ctx, upd, wall.poses[lo:hi], wall.attrs[lo:hi], wall.T, wall.sigma, step=wall.step, first=lo, lead=lo % 5)
            assert ps.tobytes() == p[lo:hi].tobytes() and as_.tobytes() == a[lo:hi].tobytes(), (lo, hi)
    # the last particles a 32-bit counter word can name, against the restatement
    first = 0x100000000 - 64
    ps, _ = _run(ra, ctx, wall.upd[False], wall.poses[:64], wall.attrs[:64], wall.T, wall.sigma, step=wall.step, first=first)
    ref = mn.xmul(mn.xmul(wall.poses[:64], wall.T), mn.noise_transforms(first, 64, wall.sigma, SEED, wall.step))
    assert np.allclose(mn._t64(ps), mn._t64(ref), rtol=0, atol=1e-6) and (ps.tobytes() != p[:64].tobytes())


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_filter_equals_the_single_device(ra, ctx, wall, world):
    n = 1001
    poses, attrs = mn.wall_cloud(n, seed=19)
    upd = wall.upd[True]
    p, a = _run(ra, ctx, upd, poses, attrs, wall.T, wall.sigma, step=4)
    sh = ra.ShardedParticleFilterHip(wall.v, wall.f, devices=(0,) * world, loopback=True)
    try:
        sh.set_particles(poses, attrs)
        sh.motion_update(wall.T, RATE, check_collision=True, noise=wall.sigma, seed=SEED, step=4)
        ps, as_ = sh.download()
        assert ps.tobytes() == p.tobytes() and as_.tobytes() == a.tobytes()
        # a params struct gives the sigma of this step
        params = ra.motion_noise_params(alpha_trans_rot=0.0, alpha_rot_rot=0.0)
        sh.set_particles(poses, attrs)
        sh.motion_update(wall.T, RATE, check_collision=True, noise=params, seed=SEED, step=4)
        p2, a2 = _run(ra, ctx, upd, poses, attrs, wall.T, ra.motion_noise_sigma(params, wall.T), step=4)
        ps, as_ = sh.download()
        assert ps.tobytes() == p2.tobytes() and as_.tobytes() == a2.tobytes() and p2.tobytes() != p.tobytes()
    finally:
        sh.close()


@pytest.mark.parametrize("world", [1, 3])
def test_sharded_step_with_motion_noise_equals_the_calls_one_by_one(ra, ctx, wall, world):
    from rmcl_amd import synthetic as syn, types as T
    n = 1001
    poses, attrs = mn.wall_cloud(n, seed=23)
    beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::8] * F(3.0))
    Tsb = syn.tsb_offset()
    params = ra.motion_noise_params(alpha_trans_trans=(0.5, 0.3, 0.0))
    Tm = T.transform_from_rpy((0.3, 0.0, 0.0), (0.0, 0.0, 0.1))
    mot, sens, rs = wall.upd[True], ra.PCDSensorUpdaterHip(wall.hm), ra.GladiatorResamplerHip(ctx, seed=77)
    sens.init()
    sens.setInput(beams, Tsb)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    sh = ra.ShardedParticleFilterHip(wall.v, wall.f, devices=(0,) * world, loopback=True)
    try:
        sh.set_particles(poses, attrs)
        plain = sh.step(beams, Tsb, T_bnew_bold=Tm, forget_rate=RATE, resample=None, seed=77, step=0)     # a fresh handle: today's bytes
        p_plain, a_plain = sh.download()
        sh.set_motion_noise(params)
        for k in (0, 1):
            if k == 0:
                sh.set_particles(poses, attrs)
            mot.update(d_p, d_a, n, Tm, RATE, noise=params, seed=77, step=k)
            sens.update(d_p, d_a)
            st_ref = rs.compute_stats(d_a, n)
            rs.step = k
            rs.update(d_p, d_a, d_pn, d_an, n)
            d_p, d_pn, d_a, d_an = d_pn, d_p, d_an, d_a
            st = sh.step(beams, Tsb, T_bnew_bold=Tm, forget_rate=RATE, resample="gladiator", seed=77, step=k)
            ps, as_ = sh.download()
            assert st["sum"] == st_ref["sum"] and st["max"] == st_ref["max"], k
            assert ps.tobytes() == d_p.download().tobytes() and as_.tobytes() == d_a.download().tobytes(), k
        # NULL switches it off again: the bytes of the fresh handle
        sh.set_motion_noise(None)
        sh.set_particles(poses, attrs)
        again = sh.step(beams, Tsb, T_bnew_bold=Tm, forget_rate=RATE, resample=None, seed=77, step=0)
        pa, aa = sh.download()
        assert again == plain and pa.tobytes() == p_plain.tobytes() and aa.tobytes() == a_plain.tobytes()
        d0p, d0a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        mot.update(d0p, d0a, n, Tm, RATE)
        assert d0p.download().tobytes() == p_plain.tobytes()
        # refusals of the setting and of a step it cannot take a sigma of
        bad = ra.motion_noise_params()
        bad.alpha_rot_rot[1] = -1.0
        with pytest.raises(ra.RmclHipError, match="alpha"):
            sh.set_motion_noise(bad)
        sh.set_motion_noise(params)
        Tbad = Tm.copy()
        Tbad["t"]["y"] = np.nan
        with pytest.raises(ra.RmclHipError, match="non-finite"):
            sh.step(beams, Tsb, T_bnew_bold=Tbad, forget_rate=RATE, resample=None, seed=77, step=0)
        pb, ab = sh.download()
        assert pb.tobytes() == pa.tobytes() and ab.tobytes() == aa.tobytes()
    finally:
        sh.close()
        sens.close()
        rs.close()


def test_all_sigmas_zero_is_the_deterministic_update(ra, ctx, wall):
    """... also for a cloud with -0.0f components, which a product with an exact identity would turn into +0.0f"""
    n = 300
    poses, attrs = (x.copy() for x in mn.wall_cloud(n, seed=29))
    poses["R"]["x"] = F(-0.0)
    poses["R"]["y"][::2] = F(-0.0)
    poses["t"]["z"][::3] = F(-0.0)
    poses["t"]["y"][::5] = F(-0.0)
    ident = ra.types.identity()
    Tneg = wall.T.copy()             # the wall step with negative zeros of its own: the deterministic update then KEEPS some of the cloud's
    for k in "xyz":
        Tneg["R"][k] = F(-0.0)
    Tneg["t"]["y"] = Tneg["t"]["z"] = F(-0.0)
    moved = mn.xmul(poses, Tneg)
    flipped = (mn.xmul(moved, ident).view(np.uint32) != moved.view(np.uint32)).sum()
    assert flipped >= 100, "a product with an exact identity changes nothing here: the cloud tests nothing"
    for T in (Tneg, wall.T, ident):
        for collision in (False, True):
            upd = wall.upd[collision]
            p0, a0 = _run_plain(ra, ctx, upd, poses, attrs, T)
            if T is Tneg:
                assert p0.tobytes() == moved.tobytes()
            for zero in (np.zeros(6, F), np.full(6, -0.0, F)):
                p, a = _run(ra, ctx, upd, poses, attrs, T, zero, step=9)
                assert p.tobytes() == p0.tobytes() and a.tobytes() == a0.tobytes()
    # an identity step has sigma zero whatever the alphas
    for collision in (False, True):
        p, a = _run(ra, ctx, wall.upd[collision], poses, attrs, ident, ra.motion_noise_params(), step=9)
        pi, ai = _run_plain(ra, ctx, wall.upd[collision], poses, attrs, ident)
        assert p.tobytes() == pi.tobytes() and a.tobytes() == ai.tobytes()


@pytest.mark.parametrize("collision", [False, True])
def test_fused_surface_constraint_equals_the_two_calls(ra, ctx, room, collision):
    """with the surface constraint set, the call equals motion_update_noisy without it followed by rmclhip_pf_constrain_to_surface, on
    the particles whose collision flag agrees (the fused launch lifts the collision segment by the step height)"""
    n = len(room.poses)
    sp = ra.types.surface_params(height=0.1, probe_up=0.5, probe_down=1.0, align=1)
    fused = ra.TFMotionUpdaterHip(room.hm, check_collision=collision)
    fused.surface = sp
    try:
        pf, af = _run(ra, ctx, fused, room.poses, room.attrs, room.T, room.sigma, step=room.step)
        st = fused.surface_stats()
        d_p, d_a, vp, va = _poisoned(ra, ctx, room.poses, room.attrs, 0)
        room.upd[collision].update(vp, va, n, room.T, RATE, noise=room.sigma, seed=SEED, step=room.step)
        _, a_mid = _fetch(ra, d_p, d_a, n, 0)
        st2 = ra.constrain_to_surface(room.upd[collision], vp, va, n, sp)
        p2, a2 = _fetch(ra, d_p, d_a, n, 0)
        assert st == st2 and st["n_snapped"] >= n // 10
        assert pf.tobytes() == p2.tobytes()                       # the pose does not depend on the kill
        agree = _killed(af) == _killed(a_mid)
        print("fused surface, collision %d: %d of %d kill flags agree, snapped %d" % (collision, int(agree.sum()), n, st["n_snapped"]))
        assert agree.sum() >= n // 2
        assert af[agree].tobytes() == a2[agree].tobytes()
        # ... and the constraint did probe the noisy pose: without noise other particles snap elsewhere
        p_plain, _ = _run_plain(ra, ctx, fused, room.poses, room.attrs, room.T)
        assert p_plain.tobytes() != pf.tobytes()
    finally:
        fused.close()


def test_only_nonzero_sigmas_move_their_components(ra, ctx, wall):
    """inv(moved) * pose_new per group: translation sigmas all zero leave the position bit for bit, rotation sigmas all zero the
    quaternion.  One nonzero sigma moves its own component and leaves the others at the rounding of the float32 product moved * N:
    the rotation of N.t (|N.t| < 1 m) is two quaternion products of 7 operations each, 14 * 2^-24 = 8.4e-7 m, and the sum with a
    position of up to 8 m adds half an ulp, 2.4e-7 m: bound 2e-6 m.  A component of the quaternion product is 7 operations on values
    below 1, 4.2e-7, and a small Euler angle is twice a component: bound 1e-6 rad."""
    upd = wall.upd[False]
    n = 500
    poses, attrs = wall.poses[:n], wall.attrs[:n]
    moved, _ = _run_plain(ra, ctx, upd, poses, attrs, wall.T)
    for k in range(6):
        sigma = np.zeros(6, F)
        sigma[k] = 0.2
        p, _ = _run(ra, ctx, upd, poses, attrs, wall.T, sigma, step=2)
        if k < 3:
            for c in "xyzw":
                assert np.array_equal(p["R"][c], moved["R"][c]), (k, c)       # an identity rotation, exactly
        else:
            for c in "xyz":
                assert np.array_equal(p["t"][c], moved["t"][c]), (k, c)       # exact zeros
        comp = mn.relative_components_f64(moved, p)
        want = mn.noise_components(0, n, sigma, SEED, 2)[:, k].astype(np.float64)
        assert np.allclose(comp[:, k], want, rtol=0, atol=2e-6), k
        assert comp[:, k].std() > 0.15
        others = np.delete(comp, k, axis=1)
        tol = np.delete(np.array([2e-6] * 3 + [1e-6] * 3), k)
        assert np.all(np.abs(others) <= tol), (k, np.abs(others).max(0))


def test_step_and_seed_change_the_draws_and_the_resamplers_stream_is_untouched(ra, ctx, wall):
    from rmcl_amd import types as T
    upd = wall.upd[False]
    n = 600
    poses, attrs = wall.poses[:n], wall.attrs[:n]
    sigma = np.full(6, 0.1, F)
    base, _ = _run(ra, ctx, upd, poses, attrs, wall.T, sigma, seed=SEED, step=3)
    again, _ = _run(ra, ctx, upd, poses, attrs, wall.T, sigma, seed=SEED, step=3)
    assert base.tobytes() == again.tobytes()
    for seed, step in ((SEED, 4), (SEED + 1, 3), (SEED ^ (1 << 40), 3)):          # step, low key word, high key word
        other, _ = _run(ra, ctx, upd, poses, attrs, wall.T, sigma, seed=seed, step=step)
        assert not np.any(other["t"]["x"] == base["t"]["x"]), (seed, step)
    # the systematic resampler with the same (seed, step): its bytes do not depend on whether, or with what, the motion noise drew --
    # and its draws are not the noise's (stream 0 against stream 2: tests/test_motion_noise_cpu.py)
    rs = ra.AdaptiveResamplerHip(ctx, seed=SEED)
    try:
        out = []
        for noise in (None, sigma):
            d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
            d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
            before = (d_p.download(), d_a.download())
            if noise is not None:
                d_q, d_b = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
                upd.update(d_q, d_b, n, wall.T, RATE, noise=noise, seed=SEED, step=3)
            rs.step = 3
            rs.update_systematic(d_p, d_a, d_pn, d_an, n)
            assert d_p.download().tobytes() == before[0].tobytes() and d_a.download().tobytes() == before[1].tobytes()
            out.append((d_pn.download(), d_an.download()))
        assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    finally:
        rs.close()


def test_statistics_of_the_devices_draws(ra, ctx, wall):
    """premise (a) on the device's output: inv(moved) * pose_new of 65 536 particles has the standard deviations it was asked for, and
    no correlation between its components"""
    upd = wall.upd[False]
    rng = np.random.RandomState(41)
    poses = np.zeros(N_STAT, ra.types.TRANSFORM)
    q = rng.normal(size=(N_STAT, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for i, k in enumerate("xyzw"):
        poses["R"][k] = q[:, i]
    for i, k in enumerate("xyz"):
        poses["t"][k] = rng.uniform(-1, 1, N_STAT)
    attrs = np.zeros(N_STAT, ra.types.PARTICLE_ATTRIBUTES)
    moved, _ = _run_plain(ra, ctx, upd, poses, attrs, wall.T)
    p, _ = _run(ra, ctx, upd, poses, attrs, wall.T, STAT_SIGMA, seed=SEED, step=1)
    comp = mn.relative_components_f64(moved, p)
    check_statistics(comp, STAT_SIGMA, "device")
    want = mn.noise_components(0, N_STAT, STAT_SIGMA, SEED, 1).astype(np.float64)
    assert np.allclose(comp, want, rtol=0, atol=2e-6)


def test_refusals_leave_the_buffers_untouched(ra, ctx, wall):
    L = ra._capi.lib()
    upd = wall.upd[True]
    upd.init()
    n = 70
    d_p, d_a, vp, va = _poisoned(ra, ctx, wall.poses[:n], wall.attrs[:n], 2)
    before = (d_p.download(), d_a.download())
    T = np.ascontiguousarray(wall.T, ra.types.TRANSFORM).reshape(1)
    tp = T.ctypes.data_as(C.c_void_p)
    good = np.full(6, 0.1, F)
    sp = lambda s: s.ctypes.data_as(C.c_void_p)

    def call(poses=vp, attrs=va, count=n, Tp=tp, rate=RATE, sigma=good, first=0, h=None):
        return L.rmclhip_pf_motion_update_noisy(upd._h if h is None else h, poses, attrs, count, Tp, rate, 1, None if sigma is None else sp(sigma), SEED, 1, first)

    for k in range(6):
        for bad in (-1e-3, float("nan"), float("inf")):
            s = good.copy()
            s[k] = bad
            assert call(sigma=s) == ra._capi.ERR_INVALID, (k, bad)
            assert b"sigma" in L.rmclhip_last_error()
    assert call(sigma=None) == ra._capi.ERR_INVALID
    for rate in (-0.01, 1.01, float("nan")):
        assert call(rate=rate) == ra._capi.ERR_INVALID
        assert b"forget_rate" in L.rmclhip_last_error()
    assert call(poses=None) == ra._capi.ERR_INVALID and call(attrs=None) == ra._capi.ERR_INVALID
    assert call(Tp=None) == ra._capi.ERR_INVALID
    assert call(first=0x100000000 - n + 1) == ra._capi.ERR_INVALID and b"2^32" in L.rmclhip_last_error()
    # the refusals come before n == 0 is looked at; n == 0 itself is OK, also without buffers
    assert call(count=0, sigma=np.full(6, -1.0, F)) == ra._capi.ERR_INVALID
    assert call(count=0, poses=None, attrs=None) == ra._capi.OK
    assert d_p.download().tobytes() == before[0].tobytes() and d_a.download().tobytes() == before[1].tobytes()
    # the sharded calls refuse the same, before any device is touched
    sh = ra.ShardedParticleFilterHip(wall.v, wall.f, devices=(0, 0), loopback=True)
    try:
        sh.set_particles(wall.poses[:n], wall.attrs[:n])
        for bad in (np.array([0.1, 0.1, -0.1, 0, 0, 0], F), np.array([0, 0, 0, np.nan, 0, 0], F)):
            with pytest.raises(ra.RmclHipError, match="sigma"):
                sh.motion_update(wall.T, RATE, noise=bad, seed=SEED, step=1)
        with pytest.raises(ra.RmclHipError, match="forget_rate"):
            sh.motion_update(wall.T, 1.5, noise=good, seed=SEED, step=1)
        ps, as_ = sh.download()
        assert ps.tobytes() == wall.poses[:n].tobytes() and as_.tobytes() == wall.attrs[:n].tobytes()
    finally:
        sh.close()
    # ... and a call that is accepted does write (the refusals above are not the only thing this buffer can show)
    assert call() == ra._capi.OK
    assert d_p.download().tobytes() != before[0].tobytes()


def test_cpp_example_prints_what_the_python_binding_computes(ra, ctx, wall, tmp_path):
    """examples/motion_noise_cpp_example.cpp on the cube room: TFMotionUpdaterHip::setNoise through the C++ adapters -- a standing step,
    three driving steps with the adapter's own step count, the sharded updater, reset"""
    from test_cpp_adapters import _build
    from rmcl_amd import types as T
    exe = _build(tmp_path, "motion_noise_cpp_example.cpp")
    mesh_bin, cloud_bin = tmp_path / "mesh.bin", tmp_path / "cloud.bin"
    with open(mesh_bin, "wb") as fh:
        fh.write(struct.pack("<II", len(wall.v), len(wall.f)))
        fh.write(np.ascontiguousarray(wall.v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(wall.f, np.uint32).tobytes())
    n, seed = 1500, 11
    r = subprocess.run([exe, str(mesh_bin), str(cloud_bin), str(n), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    d_p = ra.DeviceArray.from_host(ctx, np.zeros(n, T.TRANSFORM))
    d_a = ra.DeviceArray.from_host(ctx, np.zeros(n, T.PARTICLE_ATTRIBUTES))
    ra.init_particles_uniform(ctx, d_p, d_a, (3.4, -2.0, -0.5, 0.0, 0.0, -0.3), (4.0, 2.0, 0.5, 0.0, 0.0, 0.3), seed, 0)
    p0 = d_p.download()
    params = ra.motion_noise_params(alpha_trans_trans=(0.2, 0.05, 0.0), alpha_trans_rot=(0.2, 0.2, 0.0))
    stand = T.identity()
    drive = T.transform((0.0, 0.0, 0.024997396, 0.99968752), (0.3, 0.0, 0.0))
    assert [float(x) for x in out["sigma_stand"]] == [0.0] * 6
    assert np.array_equal(np.array([float(x) for x in out["sigma_drive"]], F), ra.motion_noise_sigma(params, drive))
    upd = wall.upd[True]
    upd.update(d_p, d_a, n, stand, 0.0, noise=params, seed=seed, step=0)
    assert d_p.download().tobytes() == p0.tobytes() and out["stand_unchanged"] == ["1"]
    for k in (1, 2, 3):
        upd.update(d_p, d_a, n, drive, 0.01, noise=params, seed=seed, step=k)
    pp, aa = d_p.download(), d_a.download()
    assert out["steps"] == ["4"] and out["steps_after_reset"] == ["0", "0"] and out["sharded_equal"] == ["1"]
    killed = int((aa["likelihood"]["mean"] == 0).sum())
    assert out["killed"] == [str(killed)] and 0 < killed < n
    s0, s3 = float(out["spread_x_0"][0]), float(out["spread_x_3"][0])
    assert abs(s0 - p0["t"]["x"].astype(np.float64).std()) < 1e-6 and abs(s3 - pp["t"]["x"].astype(np.float64).std()) < 1e-6 and s3 > s0
    blob = open(cloud_bin, "rb").read()
    assert struct.unpack("<I", blob[:4])[0] == n and len(blob) == 4 + n * 68
    assert blob[4:4 + 32 * n] == pp.tobytes() and blob[4 + 32 * n:] == aa.tobytes()
