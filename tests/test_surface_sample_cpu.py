"""CPU tests of the surface sampler and the recovery rule: the premises of tests/surface_sample_cases.py on the host build,
rmclhip_recovery_update_host (a host function: no device) against the restatement exactly in double, the restated sampler's
distribution, and its cross-check with the surface constraint's restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_ref as sref
import surface_sample_cases as sc
import surface_sample_ref as ssr

F = np.float32


# ---- premises of the maps ----------------------------------------------------------------------------------------------------
def test_twofloor_premises(ra):
    tris, nf, info = sc.records("twofloor")
    assert nf == 14 and info["n_tri_records"] == 14
    nz = {int(r[15]): float(r.view(F)[14]) for r in tris}
    assert nz[0] == 1.0 and nz[1] == 1.0 and nz[2] == 1.0 and nz[3] == -1.0           # one face of the upper floor is wound downwards
    assert all(nz[k] == 0.0 for k in range(4, 12))                                     # walls
    c = sc.ramp_cos()
    assert abs(float(c) - 0.8) < 1e-6
    on, off = sc.ref_sampler("twofloor_ramp_on"), sc.ref_sampler("twofloor_ramp_off")
    assert float(off.p["min_up_cos"]) > float(on.p["min_up_cos"]) and np.nextafter(on.p["min_up_cos"], F(2)) == off.p["min_up_cos"]
    assert on.tab["eligible"][list(sc.TWOFLOOR_RAMP)].all() and not off.tab["eligible"][list(sc.TWOFLOOR_RAMP)].any()
    assert on.tab["eligible"][[0, 1, 2, 3]].all() and not on.tab["eligible"][4:12].any()
    # areas: four floor faces of 50 m^2, two ramp faces of 5 m^2 (true area, not the projected 4 m^2)
    assert np.allclose(on.tab["area"][[0, 1, 2, 3]], 50.0, rtol=1e-6, atol=0) and np.allclose(on.tab["area"][[12, 13]], 5.0, rtol=1e-6, atol=0)
    assert on.info()["n_eligible"] == 6 and off.info()["n_eligible"] == 4
    assert int(on.tab["w"].max()) == 2 ** 32


def test_spatial_splits_weigh_every_face_once(ra):
    tris, nf, info = sc.records("cadmix20k")
    assert info["n_tri_records"] > info["n_faces"] == nf and info["spatial_splits"] > 0
    fid = tris[:, 15]
    assert np.array_equal(np.unique(fid), np.arange(nf))
    # the records of a face are identical: the table does not depend on which one is read
    order = np.argsort(fid, kind="stable")
    same = fid[order][1:] == fid[order][:-1]
    assert same.any() and np.array_equal(tris[order][1:][same], tris[order][:-1][same])
    s = sc.ref_sampler("cadmix20k")
    highest = np.zeros(nf, np.int64)
    np.maximum.at(highest, fid.astype(np.int64), np.arange(len(tris)))
    assert (highest != s.tab["rec"]).any() and np.array_equal(tris[highest], tris[s.tab["rec"]])
    assert s.info()["n_weighted"] <= s.info()["n_eligible"] <= nf


def test_face_table_does_not_depend_on_the_builders_spatial_splits(ra, tmp_path):
    """the restated table of cadmix20k from the record array built without spatial splits (RMCLHIP_SBVH_ALPHA=0, read once per process:
    a child process builds it) equals the one from this process's array, which has them"""
    assert "RMCLHIP_SBVH_ALPHA" not in os.environ
    tris, nf, info = sc.records("cadmix20k")
    out = str(tmp_path / "tris.npy")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r]; import surface_sample_cases as sc; t, nf, i = sc.records('cadmix20k'); "
            "assert i['spatial_splits'] == 0 and len(t) == nf; np.save(%r, t)" % (root, os.path.join(root, "tests"), out))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, RMCLHIP_SBVH_ALPHA="0"))
    plain = np.load(out)
    assert len(plain) == nf < len(tris)
    name, kw = sc.parametrisations()["cadmix20k"]
    a, b = ssr.face_table(plain, nf, ssr.params(**kw)), sc.ref_sampler("cadmix20k").tab
    assert a["T"] == b["T"] and np.array_equal(a["w"], b["w"]) and np.array_equal(a["C"], b["C"]) and np.array_equal(a["eligible"], b["eligible"])
    assert a["area"].tobytes() == b["area"].tobytes() and not np.array_equal(a["rec"], b["rec"])
    assert np.array_equal(plain[a["rec"]], tris[b["rec"]])           # the record that stands for a face: the same 64 bytes


def test_duplicate_and_degenerate_faces(ra):
    s = sc.ref_sampler("dupsoup")
    v, f = sc.build_map("dupsoup")
    tri = np.sort(np.asarray(f).reshape(-1, 3), axis=1)
    _, inverse, counts = np.unique(tri, axis=0, return_inverse=True, return_counts=True)
    assert (counts == 2).all()                                   # every face twice, as distinct ids
    w = s.tab["w"]
    pairs = np.argsort(inverse.reshape(-1), kind="stable").reshape(-1, 2)
    assert np.array_equal(w[pairs[:, 0]], w[pairs[:, 1]]) and (w[pairs[:, 0]] > 0).any()   # both weigh, and the same
    d = sc.ref_sampler("degcube")
    zero = d.tab["area"] == 0.0
    assert zero.any() and (d.tab["w"][zero] == 0).all()
    _, _, faces = ssr.init_surface(d, 0, 4096, sc.SEED, with_faces=True)
    assert not zero[faces].any() and (d.tab["w"][faces] > 0).all()          # never drawn


def test_scene_and_strip_premises(ra):
    s = sc.ref_sampler("scene")
    assert s.n_faces == 28 and s.tab["eligible"][[0, 1, 2, 3, 12, 13, 14, 15, 16, 17, 26, 27]].all() and s.info()["n_eligible"] == 12
    _, _, faces = ssr.init_surface(s, 0, 2000, sc.SEED, with_faces=True)
    assert (faces >= 14).any() and (faces < 14).any()                      # both instances are drawn, by global face id
    for name in ("strip1025", "strip4097"):
        t = sc.ref_sampler(name)
        w = t.tab["w"]
        big = (t.n_faces - 1) // 2
        assert t.n_faces in (1026, 4098) and int(w[big]) == 2 ** 32 and (np.delete(w, big) == 2 ** 12).all()    # 2^20 times smaller
        assert t.tab["T"] == 2 ** 32 + (t.n_faces - 1) * 2 ** 12 and t.n_faces > 1024                           # more than one scan block
    small = sc.ref_sampler("strip4097_small")
    assert small.info()["n_eligible"] == 4097 and (small.tab["w"][small.tab["eligible"]] == 2 ** 32).all()
    _, _, faces = ssr.init_surface(small, 0, 4097, sc.SEED, with_faces=True)
    assert len(set(faces // 1024)) == 5                                    # draws on every block of the scan
    name, kw = sc.OUTSIDE
    tris, nf, _ = sc.records(name)
    with pytest.raises(ValueError):
        ssr.Sampler(tris, nf, ssr.params(**kw))
    one = sc.ref_sampler("single")
    assert one.info()["n_eligible"] == 1 and one.info()["weight_total"] == 2 ** 32
    for bad in sc.BAD_PARAMS:
        with pytest.raises(ValueError):
            ssr.check_params(ssr.params(**bad))


def test_alignment_branches_of_the_restatement(ra):
    """the quarter turn of the vertical wall is the largest arc a draw can ask for; the half-turn branch is out of a draw's reach and is
    held against the surface constraint's restatement directly"""
    s = sc.ref_sampler("vertical")
    poses, _, _ = ssr.init_surface(s, 0, 257, sc.SEED, with_faces=True)
    assert not s.last_half_turn.any()
    q = np.stack([poses["R"][k] for k in "xyzw"], 1).astype(np.float64)
    zb = np.stack([2 * (q[:, 0] * q[:, 2] + q[:, 3] * q[:, 1]), 2 * (q[:, 1] * q[:, 2] - q[:, 3] * q[:, 0]),
                   1 - 2 * (q[:, 0] ** 2 + q[:, 1] ** 2)], 1)
    assert np.abs(zb - np.array([0.0, 1.0, 0.0])).max() < 1e-6 or np.abs(zb - np.array([0.0, -1.0, 0.0])).max() < 1e-6
    assert np.abs(poses["t"]["y"] - np.sign(zb[0, 1]) * 0.25).max() < 1e-6          # height along the flipped normal
    # align() on arrays == surface_ref.snap_one's step 5, including w < 1e-6
    rs = np.random.RandomState(5)
    R = rs.normal(size=(40, 4)).astype(F)
    R = (R / np.linalg.norm(R, axis=1, keepdims=True)).astype(F)
    n = np.zeros((40, 3), F)
    for k in range(40):
        zb_k = sref.qrot(R[k], (0, 0, 1))
        n[k] = -zb_k if k % 2 else sref.qrot(R[(k + 1) % 40], (0, 0, 1))
    got, half = ssr.align(tuple(R[:, k].copy() for k in range(4)), tuple(n[:, k].copy() for k in range(3)))
    assert half[1::2].all() and not half[0::2].any()
    for k in range(40):
        probe = (sref.SNAP, np.array([0, 0, 1], F), np.zeros(3, F), F(0), n[k], 0, False)
        want, _ = sref.snap_one(R[k], np.zeros(3, F), probe, sref.params(align=1))
        assert np.array([got[c][k] for c in range(4)], F).tobytes() == want.tobytes(), k


# ---- the recovery rule ---------------------------------------------------------------------------------------------------------
def _update(ra, state, prm, total, n):
    p = C.c_double(-1.0)
    st = ra._capi.lib().rmclhip_recovery_update_host(C.byref(state), C.byref(prm), float(total), int(n), C.byref(p))
    return st, p.value


def test_recovery_update_host_matches_the_restatement_exactly(ra):
    for kw in (dict(), dict(alpha_slow=0.05, alpha_fast=0.5, p_max=0.25)):
        prm_ref = ssr.recovery_params(**kw)
        prm = ra._capi.RecoveryParams(prm_ref["alpha_slow"], prm_ref["alpha_fast"], prm_ref["p_max"])
        state, ref = ra._capi.RecoveryState(0.0, 0.0), [0.0, 0.0]
        ps = []
        for k, total in enumerate(sc.RECOVERY_SUMS):
            st, p = _update(ra, state, prm, total, sc.RECOVERY_N)
            want = ssr.recovery_update(ref, prm_ref, total, sc.RECOVERY_N)
            assert st == 0 and p == want and state.w_slow == ref[0] and state.w_fast == ref[1], k
            ps.append(p)
            if k == sc.RECOVERY_RESET_AFTER:
                assert ra._capi.lib().rmclhip_recovery_reset_host(C.byref(state)) == 0
                ssr.recovery_reset(ref)
                assert state.w_slow == 0.0 and state.w_fast == 0.0
        assert all(p == 0.0 for p in ps[:6])                     # steady: nothing to inject
        assert 0.0 < ps[6] < ps[7] < ps[8] or ps[6] == ps[7] == ps[8] == prm_ref["p_max"]      # the drop
        assert ps[8] <= prm_ref["p_max"] and ps[9] == 0.0        # after the reset the averages adopt the next mean
        assert all(p == 0.0 for p in ps[9:])                     # the likelihood recovers: the fast average leads
    d = ra._capi.RecoveryParams()
    ra._capi.lib().rmclhip_recovery_params_default(C.byref(d))
    assert (d.alpha_slow, d.alpha_fast, d.p_max) == (0.001, 0.1, 1.0)
    r = ra.RecoveryHip()
    assert r.update({"sum": 800.0, "max": 1.0}, 1000) == 0.0 and r.update(80.0, 1000) == ssr.recovery_update([0.8, 0.8], ssr.recovery_params(), 80.0, 1000)
    r.reset()
    assert (r.state.w_slow, r.state.w_fast) == (0.0, 0.0)


def test_recovery_update_host_refusals_leave_the_state(ra):
    lib = ra._capi.lib()
    good = ra._capi.RecoveryParams(0.001, 0.1, 1.0)

    def refused(prm, total, n):
        state = ra._capi.RecoveryState(0.25, 0.125)
        st, p = _update(ra, state, prm, total, n)
        return st == ra._capi.ERR_INVALID and p == 0.0 and (state.w_slow, state.w_fast) == (0.25, 0.125)

    for bad in sc.BAD_RECOVERY:
        k = ssr.recovery_params(**bad)
        assert refused(ra._capi.RecoveryParams(k["alpha_slow"], k["alpha_fast"], k["p_max"]), 10.0, 10), bad
        with pytest.raises(ValueError):
            ssr.recovery_update([0.25, 0.125], k, 10.0, 10)
    for total, n in ((10.0, 0), (-1.0, 10), (float("inf"), 10), (float("nan"), 10)):
        assert refused(good, total, n), (total, n)
        with pytest.raises(ValueError):
            ssr.recovery_update([0.25, 0.125], ssr.recovery_params(), total, n)
    state = ra._capi.RecoveryState(0.25, 0.125)
    assert lib.rmclhip_recovery_update_host(None, C.byref(good), 1.0, 1, None) == ra._capi.ERR_INVALID
    assert lib.rmclhip_recovery_update_host(C.byref(state), None, 1.0, 1, None) == ra._capi.ERR_INVALID
    assert lib.rmclhip_recovery_reset_host(None) == ra._capi.ERR_INVALID
    assert lib.rmclhip_recovery_update_host(C.byref(state), C.byref(good), 0.0, 7, None) == 0          # a nullable output, a zero sum
    # alpha 1: the averages are the last mean; a slow average of 0 gives p = 0
    one = ra._capi.RecoveryParams(1.0, 1.0, 1.0)
    st, p = _update(ra, state, one, 0.0, 7)
    assert st == 0 and p == 0.0 and state.w_slow == 0.0


# ---- the restated sampler's distribution and its cross-check with the constraint -------------------------------------------------------
N_DRAWS = 40000
DIST_SEED = 20240611


@pytest.fixture(scope="module")
def twofloor_draws(ra):
    s = sc.ref_sampler("twofloor")
    poses, attrs, faces = ssr.init_surface(s, 0, N_DRAWS, DIST_SEED, epoch=1, with_faces=True)
    return s, poses, attrs, faces


def test_restated_sampler_is_uniform_by_area(twofloor_draws):
    s, poses, attrs, faces = twofloor_draws
    T, w = s.tab["T"], s.tab["w"].astype(np.float64)
    counts = np.bincount(faces, minlength=s.n_faces)
    pf = w / T
    sd = np.sqrt(N_DRAWS * pf * (1.0 - pf))
    assert (counts[w == 0] == 0).all()
    assert (np.abs(counts - N_DRAWS * pf)[w > 0] <= 5.0 * sd[w > 0]).all(), (counts, N_DRAWS * pf)
    # the ramp's share follows its true area 10 / 210, not its projected area 8 / 208
    ramp = counts[list(sc.TWOFLOOR_RAMP)].sum()
    p_true, p_proj = 10.0 / 210.0, 8.0 / 208.0
    assert abs(ramp - N_DRAWS * p_true) <= 5.0 * np.sqrt(N_DRAWS * p_true * (1 - p_true))
    assert abs(ramp - N_DRAWS * p_proj) > 3.0 * np.sqrt(N_DRAWS * p_proj * (1 - p_proj))      # (the two shares lie 8.6 deviations apart)
    # every pose stands `height` above its face: the floors at z = 0.2 / 3.2, the ramp in between; yaw-only rotations
    z = poses["t"]["z"]
    on0, on1 = np.isin(faces, sc.TWOFLOOR_FLOOR0), np.isin(faces, sc.TWOFLOOR_FLOOR1)
    assert (z[on0] == F(0.2)).all() and (z[on1] == F(3.0) + F(0.2)).all()
    x, y = poses["t"]["x"], poses["t"]["y"]
    assert (x[on0 | on1] >= 0).all() and (x[on0 | on1] <= 10).all() and (y >= 0).all() and (y <= 10).all()
    onr = np.isin(faces, sc.TWOFLOOR_RAMP)
    assert np.abs(z[onr] - (0.2 + 0.75 * (x[onr] - 10.0))).max() < 1e-5 and (x[onr] >= 10).all() and (x[onr] <= 14).all() and (y[onr] <= 2).all()
    assert (poses["R"]["x"] == 0).all() and (poses["R"]["y"] == 0).all() and (poses["stamp"] == 0).all()
    yaw = 2.0 * np.arctan2(poses["R"]["z"].astype(np.float64), poses["R"]["w"].astype(np.float64))
    assert abs(yaw.mean()) < 5.0 * (2 * np.pi / np.sqrt(12.0)) / np.sqrt(N_DRAWS) and yaw.min() < -3.1 and yaw.max() > 3.1
    # both halves of every square are filled: the reflection keeps the barycentric point inside the triangle
    assert (counts[[0, 1, 2, 3]] > 0.2 * N_DRAWS).all()
    assert attrs["likelihood"]["mean"].min() == 1.0 and attrs["likelihood"]["n_meas"].max() == 0


def test_restated_draws_stand_where_the_constraint_puts_them(orc, twofloor_draws):
    """every draw (height 0.2) fed to the surface constraint's restatement with probe_up 0.3 and the same min_up_cos is classed snap
    and moves by no more than 1e-5 m, for all but at most 0.5 % of the draws (points on the outline of a floor, where the probe may
    meet a wall)."""
    s, poses, attrs, faces = twofloor_draws
    n = len(poses)
    v, f = sc.build_map("twofloor")
    mesh = orc.Mesh(v, f)
    p = sref.params(axis=0, height=0.2, probe_up=0.3, probe_down=1.0, min_up_cos=float(s.p["min_up_cos"]), align=0)
    out, _, stats, info = sref.constrain(mesh, poses[:n], attrs[:n], p)
    moved = np.sqrt(sum((out["t"][k].astype(np.float64) - poses[:n]["t"][k].astype(np.float64)) ** 2 for k in "xyz"))
    bad = (info["cls"] != sref.SNAP) | (moved > 1e-5)
    print("constraint cross-check: %d of %d draws are exceptions, largest move of the rest %.3g m" % (bad.sum(), n, moved[~bad].max()))
    assert bad.sum() <= 0.005 * n
    assert np.array_equal(info["face"][~bad] // 2, faces[:n][~bad] // 2)       # the probe meets the quad the draw stands on
