"""The pose information on the device (pose_information.hip; include/rmclhip.h, POSE COVARIANCE) against tests/pose_information_ref.py:
the free function on caller-owned views, the operator form after a find, the batch form, determinism, and what the result says about
a tube and a room.

The bound everywhere: n_meas exact, every entry e of A, g, rss within n_meas * 2^-52 * sum |terms of e| of the reference -- the worst
case of any summation order in double (pose_information_ref.assert_matches).  Two device results of the same sums in different orders
differ by at most the same figure ((n - 1) additions of half an ulp each, twice)."""
import numpy as np
import pytest

import pose_information_ref as pir

pytestmark = pytest.mark.gpu

F = np.float32
MAX_DIST = F(0.3)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _free_case(n, seed):
    """n random correspondences within +-10 m, about half of them inside the gate, with the first elements' residuals exactly at
    max_dist, one ulp inside and one ulp outside (both signs) -- exact under the identity pre-transform: N = z, D_z = 0, I_z = the
    residual.  Model points and normals are NaN wherever the model mask is 0."""
    rng = np.random.RandomState(seed)
    D = rng.uniform(-10.0, 10.0, (n, 3)).astype(F)
    N = _unit(rng.normal(size=(n, 3))).astype(F)
    r = rng.uniform(-0.6, 0.6, n)
    tang = np.cross(N.astype(np.float64), rng.normal(size=(n, 3))) * 0.2
    I = (D.astype(np.float64) + N.astype(np.float64) * r[:, None] + tang).astype(F)
    edges = [MAX_DIST, np.nextafter(MAX_DIST, F(0)), np.nextafter(MAX_DIST, F(1)), -MAX_DIST, -np.nextafter(MAX_DIST, F(0)),
             -np.nextafter(MAX_DIST, F(1))]
    if n == 1:
        edges = edges[1:2]          # the lone element: one ulp inside
    n_edge = min(n, len(edges))
    for k in range(n_edge):
        N[k] = (0.0, 0.0, 1.0)
        D[k, 2] = 0.0
        I[k] = (D[k, 0] + F(0.25), D[k, 1] - F(0.5), edges[k])
    dmask = (rng.uniform(size=n) < 0.9).astype(np.uint8)
    mmask = (rng.uniform(size=n) < 0.85).astype(np.uint8)
    dmask[:n_edge] = 1
    mmask[:n_edge] = 1
    I_nan, N_nan = I.copy(), N.copy()
    I_nan[mmask == 0] = np.nan
    N_nan[mmask == 0] = np.nan
    return dict(D=D, I=I, N=N, I_nan=I_nan, N_nan=N_nan, dmask=dmask, mmask=mmask, n_edge=n_edge)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_free_function_matches_the_reference(ra, ctx, n):
    T = ra.types
    c = _free_case(n, 100 + n)
    up = (lambda a: ra.DeviceArray.from_host(ctx, a)) if n else (lambda a: None)
    dev = {k: up(c[k]) for k in ("D", "I", "N", "I_nan", "N_nan", "dmask", "mmask")}
    Tgen = T.transform_from_rpy((0.03, -0.02, 0.04), (0.01, -0.02, 0.015))
    kept_seen = 0
    for Tpre in (T.identity(), Tgen):
        for use_d, use_m in ((True, True), (False, True), (True, False)):
            pts, nrm = ("I_nan", "N_nan") if use_m else ("I", "N")
            args = (dev["D"], dev["dmask"] if use_d else None, dev[pts], dev[nrm], dev["mmask"] if use_m else None, n, float(MAX_DIST))
            got = ra.pose_information_p2l(ctx, Tpre, *args)
            ref = pir.pose_information(Tpre, c["D"], c["dmask"] if use_d else None, c[pts], c[nrm], c["mmask"] if use_m else None, MAX_DIST)
            what = "n=%d masks=(%s, %s)" % (n, use_d, use_m)
            pir.assert_matches(got, ref, what)
            assert int(got["n_meas"]) == int(ra.statistics_p2l(ctx, Tpre, *args)["n_meas"]), what
            kept_seen += ref["n_meas"]
            if Tpre is not Tgen and n >= 6:
                # exactly at max_dist: rejected (strict); one ulp inside: kept; one ulp outside: rejected
                assert list(ref["kept"][:6]) == [False, True, False, False, True, False]
            if n == 1 and Tpre is not Tgen:
                assert ref["n_meas"] == 1          # (the lone element sits one ulp inside the gate)
            if ref["n_meas"]:
                assert abs(np.trace(got["A"][:3, :3]) / ref["n_meas"] - 1.0) < 1e-6
    if n == 0:
        assert got.tobytes() == T.pose_information_identity().tobytes()
    if n >= 63:
        assert kept_seen > n      # the gate keeps and rejects: both sides are exercised


def test_all_rejected_and_all_masked_give_zeros(ra, ctx):
    T = ra.types
    c = _free_case(257, 7)
    d = {k: ra.DeviceArray.from_host(ctx, c[k]) for k in ("D", "I", "N", "I_nan", "N_nan")}
    zeros = ra.DeviceArray.from_host(ctx, np.zeros(257, np.uint8))
    got = ra.pose_information_p2l(ctx, T.identity(), d["D"], None, d["I"], d["N"], None, 257, 1e-30)
    assert got.tobytes() == T.pose_information_identity().tobytes()
    got = ra.pose_information_p2l(ctx, T.identity(), d["D"], None, d["I_nan"], d["N_nan"], zeros, 257, 10.0)
    assert got.tobytes() == T.pose_information_identity().tobytes()


def _adaptive(max_dist, amin, p):
    return float(F(np.float64(F(max_dist)) * (1.0 - p) + np.float64(F(amin)) * p))


@pytest.fixture(scope="module")
def room(ra, orc, ctx, meshes):
    """smoke()'s scene: cube room, model_c1, tsb_offset, the perturbed pose; the dataset is the scan from the true pose"""
    from rmcl_amd import synthetic as syn
    T = ra.types
    v, f = meshes("cube")
    hm = ra.import_hip_map(ctx, v, f)
    m = orc.Mesh(v, f)
    model, Tsb, truth = syn.model_c1(), syn.tsb_offset(), syn.pose_c2_truth()
    est = T.mult(truth, syn.pose_c2_perturbation())
    meas = m.simulate_spherical(model, Tsb, truth, bvh=False)
    dirs = orc.spherical_directions(model)
    ds = (dirs * meas["ranges"][:, None]).astype(F)

    def make(tsb=Tsb, points=ds, mask=meas["hits"]):
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(tsb)
        rcc.setModel(model)
        rcc.set_dataset(points, mask)
        rcc.params.max_dist = 1.0
        rcc.adaptive_max_dist_min = 0.15
        return rcc
    return dict(hm=hm, mesh=m, model=model, dirs=dirs, Tsb=Tsb, truth=truth, est=est, ds=ds, dmask=meas["hits"], make=make)


def test_operator_form_matches_the_reference_and_leaves_the_statistics_alone(ra, room):
    T = ra.types
    rcc = room["make"]()
    rcc.find(room["est"])
    mv = rcc.modelView()
    Tpre = T.transform_from_rpy((0.02, -0.01, 0.015), (0.002, -0.003, 0.004))
    for p in (0.0, 0.5, 1.0):
        for Tp in (T.identity(), Tpre):
            before = rcc.computeCrossStatistics(Tp, p)
            got = rcc.computePoseInformation(Tp, p)
            ref = pir.pose_information(Tp, room["ds"], room["dmask"], mv["points"], mv["normals"], mv["hits"], _adaptive(1.0, 0.15, p))
            pir.assert_matches(got, ref, "p=%g" % p)
            assert ref["n_meas"] > 300 and int(before["n_meas"]) == ref["n_meas"]
            assert rcc.computeCrossStatistics(Tp, p).tobytes() == before.tobytes()
    assert ref["n_meas"] < pir.pose_information(T.identity(), room["ds"], room["dmask"], mv["points"], mv["normals"], mv["hits"], 1.0)["n_meas"]


def test_operator_form_refusals(ra, room):
    T = ra.types
    rcc = room["make"]()
    with pytest.raises(ra.RmclHipError):            # no find has run
        rcc.computePoseInformation(T.identity())
    with pytest.raises(ra.RmclHipError):
        rcc.computePoseInformationBatch(1)
    rcc.find(room["est"])
    assert int(rcc.computePoseInformation(T.identity())["n_meas"]) > 300
    rcc.set_outputs(["hits", "ranges", "points"])   # normals dropped
    with pytest.raises(ra.RmclHipError):
        rcc.computePoseInformation(T.identity())
    with pytest.raises(ra.RmclHipError):
        rcc.computePoseInformationBatch(1)
    rcc.close()


def test_batch_form_matches_the_single_form(ra, room):
    T = ra.types
    rcc = room["make"]()
    poses = np.array([room["est"], room["truth"], T.mult(room["truth"], T.transform_from_rpy((-0.1, 0.2, 0.0), (0.0, 0.01, -0.03)))],
                     dtype=T.TRANSFORM)
    rcc.find_batch(poses)
    batch = rcc.computePoseInformationBatch(3, 1.0)
    again = rcc.computePoseInformationBatch(3, 1.0)
    assert batch.tobytes() == again.tobytes()
    mvb = rcc.modelView()
    n = len(room["ds"])
    maxd = _adaptive(1.0, 0.15, 1.0)
    for bad in (2, 4, 0):
        with pytest.raises(ra.RmclHipError):
            rcc.computePoseInformationBatch(bad, 1.0)
    for i in range(3):
        sl = slice(i * n, (i + 1) * n)
        ref_b = pir.pose_information(T.identity(), room["ds"], room["dmask"], mvb["points"][sl], mvb["normals"][sl], mvb["hits"][sl], maxd)
        pir.assert_matches(batch[i], ref_b, "batch pose %d" % i)
        rcc.find(poses[i])
        single = rcc.computePoseInformation(T.identity(), 1.0)
        mv = rcc.modelView()
        ref = pir.pose_information(T.identity(), room["ds"], room["dmask"], mv["points"], mv["normals"], mv["hits"], maxd)
        pir.assert_matches(single, ref, "single pose %d" % i)
        pir.assert_matches(batch[i], dict(ref, A=single["A"], g=single["g"], rss=float(single["rss"])), "batch against single, pose %d" % i)
        with pytest.raises(ra.RmclHipError):        # the last find held one pose
            rcc.computePoseInformationBatch(3, 1.0)
    assert len({int(b["n_meas"]) for b in batch}) > 1


def test_same_call_twice_gives_the_same_bytes(ra, ctx, room):
    """fixed summation order: a kernel that adds with floating-point atomics fails here"""
    T = ra.types
    c = _free_case(4099, 5)
    d = {k: ra.DeviceArray.from_host(ctx, c[k]) for k in ("D", "I_nan", "N_nan", "dmask", "mmask")}
    runs = [ra.pose_information_p2l(ctx, T.identity(), d["D"], d["dmask"], d["I_nan"], d["N_nan"], d["mmask"], 4099, float(MAX_DIST)).tobytes()
            for _ in range(4)]
    assert len(set(runs)) == 1
    rcc = room["make"]()
    rcc.find(room["est"])
    runs = [rcc.computePoseInformation(T.identity(), 0.0).tobytes() for _ in range(4)]
    assert len(set(runs)) == 1


def _tube(half_width=2.0, half_length=150.0):
    """an open square tube along x: four walls of two triangles each"""
    w, L = half_width, half_length
    v = np.array([[x, y, z] for x in (-L, L) for y in (-w, w) for z in (-w, w)], np.float32)   # index = 4 ix + 2 iy + iz
    quads = [(0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]                           # y = -w, y = +w, z = -w, z = +w
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return v, f


def test_a_tube_does_not_constrain_the_pose_along_its_axis(ra, orc, ctx):
    from rmcl_amd import synthetic as syn
    T = ra.types
    v, f = _tube()
    assert len(f) == 8 and np.abs(v[:, 0]).min() > syn.model_c1().range.max
    model = syn.model_c1()
    m = orc.Mesh(v, f)
    meas = m.simulate_spherical(model, T.identity(), T.transform_from_rpy((0.3, 0.05, -0.03), (0.0, 0.0, 0.0)), bvh=False)
    ds = (orc.spherical_directions(model) * meas["ranges"][:, None]).astype(F)
    rcc = ra.RCCHipSpherical(ra.import_hip_map(ctx, v, f))
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    rcc.set_dataset(ds, meas["hits"])
    rcc.params.max_dist = 1.0
    rcc.find(T.identity())                      # on the axis, identity rotation
    mv = rcc.modelView()
    assert mv["hits"].sum() > 900 and np.all(mv["normals"][mv["hits"] > 0][:, 0] == 0.0)
    info = rcc.computePoseInformation(T.identity(), 0.0)
    pir.assert_matches(info, pir.pose_information(T.identity(), ds, meas["hits"], mv["points"], mv["normals"], mv["hits"], 1.0), "tube")
    assert int(info["n_meas"]) > 900 and float(info["A"][0, 0]) == 0.0 and np.all(info["A"][0] == 0.0)
    cov = T.pose_covariance(info, sigma=0.02, degenerate_variance=50.0, min_eig_trans=1e-3, min_eig_rot=1e-3)
    assert int(cov["n_degenerate_trans"]) == 1
    assert np.array_equal(np.abs(cov["eigvec_trans"][0]), [1.0, 0.0, 0.0]) and float(cov["eig_trans"][0]) == 0.0
    assert float(cov["covariance"][0, 0]) == 50.0
    # across the tube the scan does constrain the pose: centimetres, not the 7 m of the degenerate variance
    assert 0.0 < float(cov["covariance"][1, 1]) < 1e-4 and 0.0 < float(cov["covariance"][2, 2]) < 1e-4
    # the correction the scan asks for is the offset it was taken at, across the tube only
    xi = T.pose_information_solve(info)
    assert xi[0] == 0.0 and abs(xi[1] - 0.05) < 2e-3 and abs(xi[2] + 0.03) < 2e-3


def test_a_room_constrains_every_direction(ra, room):
    T = ra.types
    rcc = room["make"]()
    rcc.find(room["est"])
    info = rcc.computePoseInformation(T.identity(), 0.0)
    cov = T.pose_covariance(info, min_eig_trans=1e-3, min_eig_rot=1e-3)
    assert int(cov["n_degenerate_trans"]) == 0 and int(cov["n_degenerate_rot"]) == 0
    assert float(cov["eig_trans"][0]) > 0.01 and abs(cov["eig_trans"].sum() - 1.0) < 1e-6
    np.linalg.cholesky(cov["covariance"])
    assert np.array_equal(cov["covariance"], cov["covariance"].T)
    assert abs(float(cov["s2"]) - float(info["rss"]) / (int(info["n_meas"]) - 6)) <= 1e-15 * float(cov["s2"])


def test_two_sensors_merge_in_the_base_frame(ra, room):
    """MICPLocalization.poseInformation: per sensor Tsb, then Tbo, then the weighted merge == the reference on the two sensors'
    correspondences expressed in the base frame and concatenated (relative 1e-10 of the largest entry)"""
    T = ra.types
    Tsb2 = T.transform_from_rpy((-0.2, 0.15, 0.5), (0.02, -0.01, -0.6))
    meas2 = room["mesh"].simulate_spherical(room["model"], Tsb2, room["truth"], bvh=False)
    ds2 = (room["dirs"] * meas2["ranges"][:, None]).astype(F)
    data = {"front": (room["ds"], room["dmask"]), "rear": (ds2, meas2["hits"])}
    sensors = []
    for name, tsb, w in (("front", room["Tsb"], 1.0), ("rear", Tsb2, 0.5)):
        rcc = room["make"](tsb, *data[name])
        sensors.append(ra.MICPSensor(name, rcc, Tsb=tsb, merge_weight_multiplier=w))
    loc = ra.MICPLocalization(sensors)
    loc.Tom_ = room["est"]
    for s in sensors:
        s.setTom(loc.Tom_)
        s.findCorrespondences()
    merged, cov = loc.poseInformation()
    S = np.zeros((7, 7))
    n_total = 0
    for s in sensors:
        mv = s.correspondences_.modelView()
        kept, D, r = pir.gate(T.identity(), *data[s.name], mv["points"], mv["normals"], mv["hits"], 1.0)
        assert kept.sum() > 300, s.name
        R, t = pir.rotation_f64(s.Tsb), np.array([float(s.Tsb["t"][k]) for k in "xyz"])
        Db, Nb = D[kept].astype(np.float64) @ R.T + t, mv["normals"][kept].astype(np.float64) @ R.T
        U = np.concatenate([Nb, np.cross(Db, Nb), r[kept].astype(np.float64)[:, None]], axis=1)
        S += s.merge_weight_multiplier * pir.sums_of(U)[0]
        n_total += int(kept.sum())
    assert int(merged["n_meas"]) == n_total > 600
    norm = "relative to the LARGEST entry (the frame change mixes the entries), not per entry"
    assert np.max(np.abs(merged["A"] - S[:6, :6])) <= 1e-10 * np.max(np.abs(S[:6, :6])), "A: " + norm
    assert np.max(np.abs(merged["g"] - S[:6, 6])) <= 1e-10 * np.max(np.abs(S[:6, 6])), "g: " + norm
    assert abs(float(merged["rss"]) - S[6, 6]) <= 1e-10 * S[6, 6]
    assert np.linalg.norm(cov["covariance"] - float(cov["s2"]) * np.linalg.inv(S[:6, :6])) <= 1e-9 * np.linalg.norm(cov["covariance"])
