"""CPU tests of the motion-compensated PointCloud2 input (include/rmclhip.h, MOTION-COMPENSATED INPUT): the numpy restatement
(tests/deskew_ref.py) against an independent float64 slerp, the two host helpers of the library, the premise on the oracle -- a scan
taken in motion misleads MICP by decimetres, rays cast from their own poses restore it -- and the fixture that pins the
restatement's bytes.  No device is needed; tests/test_gpu_deskew.py holds the kernel to the restatement byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import deskew_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def ulp32(x):
    return float(np.spacing(F(abs(x))))


def test_restatement_matches_an_independent_float64_slerp():
    """0.3 rad about a tilted axis and 0.5 m during the scan, 16-fold subdivided knots: every compensated point within
    1e-5 |expected| + 2 ulp32 of the largest coordinate or knot translation entering it (the tolerance form of DESIGN.md 7) of
    R(t) p + tr(t) with R, tr by TRUE slerp / lerp between the scan's two end poses, in float64."""
    rng = np.random.RandomState(5)
    n = 600
    p = (rng.normal(size=(n, 3)) / 1.0)
    p = (p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(0.5, 30.0, n)[:, None]).astype(F)
    t_raw = rng.uniform(0.0, 0.1, n).astype(F)
    t_raw[:3] = (0.0, 0.1, 0.05)
    axis = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    S0 = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    S1 = (np.r_[axis * np.sin(0.15), np.cos(0.15)], np.array([0.4, 0.3, 0.0]))    # 0.3 rad, 0.5 m
    t0, t1 = 20.0, 20.1
    kq, kt, ktimes = dr.motion_knots64(S0, S1, (t0, t1), t0, 16)
    assert len(ktimes) == 17
    buf, lay, tf = dr.make_cloud(p, t_raw)
    res = dr.deskew(buf, lay, tf + (1.0, t0), kq, kt, ktimes)
    ktmax = float(np.abs(kt).max())
    worst = 0.0
    for i in range(n):
        t = t0 + float(t_raw[i])                              # the restatement's own time: float32 raw, double sum
        u = min(1.0, (t - t0) / (t1 - t0))
        q, tr = dr.slerp64_pose(S0[0], S0[1], S1[0], S1[1], u)
        exp = dr.rot64(q, p[i].astype(np.float64)) + tr
        tol = 1e-5 * np.abs(exp) + 2 * ulp32(max(float(np.abs(p[i]).max()), ktmax))
        err = np.abs(res["points"][i].astype(np.float64) - exp)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (i, err, tol)
    print("worst error / tolerance: %.3f" % worst)
    assert res["stats"]["n_time_clamped"] <= 1 and res["stats"]["n_valid"] == n   # (20.0 + float32(0.1) lies 1.5e-9 s past the last knot)


def test_restatement_edges():
    """times on knots take the knot itself; before / after the motion clamp to the end knots and are counted; a NaN time takes
    knots[0], is masked and counted apart; q and -q interpolate as one rotation; non-finite coordinates give range 0, dir 0"""
    kq = np.array([[0, 0, 0, 1], [0, 0, np.sin(0.1), np.cos(0.1)], [0, 0, -np.sin(0.2), -np.cos(0.2)]], F)   # knot 2 = -(yaw 0.4)
    kt = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    ktimes = np.array([0.0, 1.0, 2.0])
    t = np.array([0.0, 1.0, 2.0, -0.5, 2.5, np.nan, np.inf, 1.5])
    q, tr, clamped, bad = dr.poses(t, kq, kt, ktimes)
    assert q[0].tobytes() == kq[0].tobytes() and tr[0].tobytes() == kt[0].tobytes()
    assert np.array_equal(tr[1], kt[1]) and np.allclose(q[1], kq[1], atol=1e-7)
    assert np.allclose(q[2], -kq[2], atol=1e-7) and np.array_equal(tr[2], kt[2])                              # flipped onto the shorter arc
    assert np.array_equal(tr[3], kt[0]) and np.array_equal(tr[4], kt[2])
    assert clamped.tolist() == [False, False, False, True, True, False, False, False]
    assert bad.tolist() == [False, False, False, False, False, True, True, False]
    assert np.array_equal(tr[5], kt[0]) and np.array_equal(tr[6], kt[0])
    yaw = 2 * np.arctan2(float(q[7][2]), float(q[7][3]))
    assert abs(yaw - 0.3) < 1e-4 and np.array_equal(tr[7], F([1.5, 0, 0]))                                     # half way between yaw 0.2 and 0.4
    xyz = np.array([[1, 2, 2], [np.nan, 1, 1], [1, np.inf, 1], [0, 0, 200]], F)
    buf, lay, tf = dr.make_cloud(xyz, np.array([0.5, 0.5, 0.5, np.nan], F))
    r = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.5, 100.0)
    assert r["ranges"].tolist() == [3.0, 0.0, 0.0, 200.0] and r["mask"].tolist() == [1, 0, 0, 0]
    assert not r["dirs"][1].any() and not r["dirs"][2].any() and np.array_equal(r["points"][1], r["origs"][1])
    assert r["stats"] == dict(n_points=4, n_finite=2, n_valid=1, n_time_clamped=0, n_time_nonfinite=1)
    assert np.isnan(r["cloud"][1:]).all() and np.array_equal(r["cloud"][0], r["points"][0])


def test_nlerp_error_bound_of_the_header():
    """rmclhip.h: over a segment of angle theta nlerp is off slerp by at most theta^3 / (144 sqrt 3) along the arc to leading order
    (the next term: theta^2 / 80 of that), attained near s = 0.21; 16 segments take a 0.3 rad scan below 2^-24"""
    for theta in (0.3, 0.3 / 16):
        s = np.linspace(0, 1, 4001)
        om = theta / 2
        nl = 2 * np.arctan2(s * np.sin(om), (1 - s) + s * np.cos(om))
        err = np.abs(nl - s * theta)
        bound = theta ** 3 / (144 * np.sqrt(3))
        assert bound * 0.999 <= err.max() <= bound * (1 + theta * theta / 80) * 1.0005
        assert abs(s[err.argmax()] - 0.2113) < 2e-3 or abs(s[err.argmax()] - 0.7887) < 2e-3
    assert 1.0e-4 < 0.3 ** 3 / (144 * np.sqrt(3)) < 1.2e-4 and (0.3 / 16) ** 3 / (144 * np.sqrt(3)) < 2.0 ** -24


# ---- the host helpers of the library -------------------------------------------------------------------------------------------------
def _yaw(ra, yaw, t):
    return ra.types.transform((0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)), t)


def test_scan_motion_helper_frames_and_subdivision(ra):
    """rmclhip_scan_motion_from_base_poses_host: t_ref on a knot gives the identity there; (n - 1) * subdivide + 1 knots at evenly
    spaced times; the knots are ~Tsb ~T(t_ref) T(t_k) Tsb -- checked against the float64 slerp of tests/deskew_ref.py"""
    T = ra.types
    Tsb = ra.synthetic.tsb_offset()
    P = np.array([_yaw(ra, 0.2, (1.0, 2.0, 0.0)), _yaw(ra, 0.5, (1.4, 2.1, 0.0)), _yaw(ra, 0.6, (1.5, 2.5, 0.1))], T.TRANSFORM)
    times = [10.0, 10.1, 10.25]
    for sub in (1, 4, 16):
        for ref_idx in (0, 1, 2):
            knots, kt = ra.wire.scan_motion(Tsb, P, times, times[ref_idx], sub)
            assert len(knots) == 2 * sub + 1 and len(kt) == 2 * sub + 1
            assert np.allclose(kt[:sub + 1], np.linspace(10.0, 10.1, sub + 1), atol=1e-12) and kt[sub] == 10.1 and kt[-1] == 10.25
            k = knots[ref_idx * sub]
            assert np.allclose([k["R"][c] for c in "xyzw"], [0, 0, 0, 1], atol=1e-7) and np.allclose([k["t"][c] for c in "xyz"], 0, atol=1e-7)
    # two poses against the independent implementation, Tsb included, t_ref inside the segment
    sb = (np.array([float(Tsb["R"][c]) for c in "xyzw"]), np.array([float(Tsb["t"][c]) for c in "xyz"]))
    S = [(np.array([float(P[i]["R"][c]) for c in "xyzw"]), np.array([float(P[i]["t"][c]) for c in "xyz"])) for i in (0, 1)]
    kq, ktr, ktimes = dr.motion_knots64(S[0], S[1], (10.0, 10.1), 10.03, 8, Tsb=sb)
    knots, kt = ra.wire.scan_motion(Tsb, P[:2], times[:2], 10.03, 8)
    got_q = np.array([[k["R"][c] for c in "xyzw"] for k in knots], F)
    got_t = np.array([[k["t"][c] for c in "xyz"] for k in knots], F)
    assert np.allclose(got_q, kq, atol=2e-7) and np.allclose(got_t, ktr, atol=1e-6) and np.allclose(kt, ktimes, atol=1e-12)


def test_scan_motion_helper_refusals(ra):
    T = ra.types
    I = T.identity()
    P = np.array([_yaw(ra, 0.0, (0, 0, 0)), _yaw(ra, 0.1, (0.1, 0, 0))], T.TRANSFORM)
    ok = lambda **kw: ra.wire.scan_motion(kw.get("Tsb", I), kw.get("P", P), kw.get("times", [0.0, 0.1]), kw.get("t_ref", 0.05),
                                          kw.get("sub", 4), kw.get("cap", 64))
    assert len(ok()[0]) == 5 and len(ok(sub=63)[0]) == 64
    bad_pose = P.copy()
    bad_pose[1]["t"]["x"] = np.nan
    zero_q = P.copy()
    for c in "xyzw":
        zero_q[0]["R"][c] = 0.0
    for kw in (dict(sub=64), dict(sub=0), dict(cap=4), dict(times=[0.1, 0.1]), dict(times=[0.0, np.inf]), dict(t_ref=0.2),
               dict(t_ref=-0.01), dict(t_ref=np.nan), dict(P=bad_pose), dict(P=zero_q), dict(P=P[:1], times=[0.0])):
        with pytest.raises(ra.RmclHipError) as e:
            ok(**kw)
        assert e.value.status == ra._capi.ERR_INVALID, kw
    n = C.c_uint32(7)
    assert ra._capi.lib().rmclhip_scan_motion_from_base_poses_host(None, None, None, 2, 0.0, 1, None, None, 64, C.byref(n)) == ra._capi.ERR_INVALID
    assert n.value == 0


def _cloud_for_sampler():
    rng = np.random.RandomState(3)
    n = 500
    p = rng.uniform(-6, 6, (n, 3)).astype(F)
    p[rng.randint(0, n, 40), rng.randint(0, 3, 40)] = np.nan
    t = rng.uniform(0, 0.1, n).astype(F)
    return dr.make_cloud(p, t, gap=6, width=50) + (p, t)


def test_deskewed_beam_sampler(ra):
    """identity motion: the bytes of rmclhip_pf_sample_beams_pointcloud2; a real motion: the same points (same ranges, same draws),
    each with the origin and rotated direction the restatement gives its point"""
    buf, lay, tf, p, t = _cloud_for_sampler()
    T = ra.types
    ident = (np.array([T.identity()] * 3, T.TRANSFORM), [0.0, 0.05, 0.1])
    args = [lay[k] for k in ("width", "height", "point_step", "row_step", "offset_x", "offset_y", "offset_z")]
    for seed in (1, 77):
        plain = ra.pf.sample_beams_pointcloud2(buf, *args, 64, seed)
        desk = ra.wire.sample_beams_pointcloud2_deskewed(buf, *args, tf, ident, 64, seed)
        assert len(plain) == 64 and desk.tobytes() == plain.tobytes()
    kq, kt, ktimes = dr.motion_knots64((np.array([0, 0, 0, 1.0]), np.zeros(3)), (np.array([0, 0, np.sin(0.1), np.cos(0.1)]), np.array([0.3, 0.1, 0.0])),
                                       (0.0, 0.1), 0.1, 8)
    knots = np.zeros(len(kq), T.TRANSFORM)
    for i in range(len(kq)):
        knots[i] = T.transform(tuple(kq[i]), tuple(kt[i]))
    plain = ra.pf.sample_beams_pointcloud2(buf, *args, 64, 5)
    desk = ra.wire.sample_beams_pointcloud2_deskewed(buf, *args, tf, (knots, ktimes), 64, 5)
    ref = dr.deskew(buf, lay, tf, kq, kt, ktimes)
    assert np.array_equal(desk["range"], plain["range"]) and np.array_equal(desk["cov"], plain["cov"])
    finite = np.isfinite(p).all(axis=1)
    for b in desk:
        i = np.nonzero(finite & (ref["ranges"] == b["range"]))[0]
        assert len(i) >= 1
        i = i[0]
        assert np.array([b["orig"][c] for c in "xyz"], F).tobytes() == ref["origs"][i].tobytes()
        assert np.array([b["dir"][c] for c in "xyz"], F).tobytes() == ref["dirs"][i].tobytes()
    # refusals: a time datatype that is none of 6 / 7 / 8, one knot, data too short for the time field
    with pytest.raises(ra.RmclHipError) as e:
        ra.wire.sample_beams_pointcloud2_deskewed(buf, *args, (tf[0], 2), ident, 4, 1)
    assert e.value.status == ra._capi.ERR_UNSUPPORTED
    with pytest.raises(ra.RmclHipError):
        ra.wire.sample_beams_pointcloud2_deskewed(buf, *args, tf, (ident[0][:1], ident[1][:1]), 4, 1)
    with pytest.raises(ra.RmclHipError):
        ra.wire.sample_beams_pointcloud2_deskewed(buf[:-1], *args, tf, ident, 4, 1)


# ---- the premise ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def premise(orc):
    from rmcl_amd import synthetic as syn
    v, f = syn.cube_room()
    mesh = orc.Mesh(v, f)
    return mesh, dr.premise_scene(mesh)


def _refind(orc, mesh, model, pts, mask, start, n_iter):
    import oracle_micp as om
    ident = orc.transform()
    T = start
    for _ in range(n_iter):
        sim = om.simulate_model(mesh, model, ident, T)
        s = orc.statistics_p2l_exact(ident, pts, mask, sim["points"], sim["normals"], sim["hits"], 1.0)
        T = orc.tmult(T, orc.umeyama(s))
    return T


def test_premise_raw_scan_misleads_micp_compensated_scan_does_not(orc, premise):
    """cube room, 8 x 64 full-circle scanner, 0.4 m and 0.15 rad during the scan, 40 re-finding iterations from a (0.1, 0.1, 0) m /
    0.05 rad yaw offset.  Oracle figures: raw 0.25 m / 0.092 rad; compensated (OnDn rays from their own poses + moved points)
    2e-6 m / 4e-6 rad.  Every ray hits in this scene."""
    mesh, sc = premise
    W, H = sc["W"], sc["H"]
    start = dr.premise_start(sc["truth"])
    e0 = dr.pose_error(start, sc["truth"])
    assert abs(e0[0] - 0.1414) < 1e-3 and abs(e0[1] - 0.05) < 1e-4
    raw = dict(kind="o1dn", width=W, height=H, range_min=0.1, range_max=100.0, orig=(0, 0, 0), dirs=sc["d_local"])
    e_raw = dr.pose_error(_refind(orc, mesh, raw, sc["xyz"], np.ones(W * H, np.uint8), start, dr.PREMISE_ITERATIONS), sc["truth"])
    c = sc["comp"]
    assert c["mask"].all() and c["stats"]["n_time_clamped"] == 0
    ondn = dict(kind="ondn", width=W, height=H, range_min=0.1, range_max=100.0, origs=c["origs"], dirs=c["dirs"])
    e_comp = dr.pose_error(_refind(orc, mesh, ondn, c["points"], c["mask"], start, dr.PREMISE_ITERATIONS), sc["truth"])
    print("raw %.4f m %.4f rad | compensated %.2e m %.2e rad" % (e_raw + e_comp))
    assert e_raw[0] > 0.1
    assert e_comp[0] < 1e-3 and e_comp[1] < 1e-3


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_pins_the_restatement():
    from conftest import golden_path
    g = np.load(golden_path("g12_deskew.npz"))
    lay = dict(zip(("width", "height", "point_step", "row_step", "offset_x", "offset_y", "offset_z", "datatype"), (int(v) for v in g["layout"])))
    assert lay["point_step"] == 22 and lay["width"] == 300
    tf = (int(g["time_field"][0]), int(g["time_field"][1]), float(g["time_field"][2]), float(g["time_field"][3]))
    r = dr.deskew(g["data"], lay, tf, g["knot_q"], g["knot_t"], g["knot_times"], float(g["range"][0]), float(g["range"][1]))
    for k in ("origs", "dirs", "points", "mask"):
        assert r[k].tobytes() == g[k].tobytes(), k
    assert [r["stats"][k] for k in ("n_points", "n_finite", "n_valid", "n_time_clamped", "n_time_nonfinite")] == g["stats"].tolist()
    assert g["stats"][3] >= 2 and g["stats"][4] == 1 and g["stats"][1] < 300
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_g12_deskew", os.path.join(ROOT, "tests", "golden", "make_g12_deskew.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    again = mod.build()
    assert all(np.asarray(again[k]).tobytes() == g[k].tobytes() for k in again)
