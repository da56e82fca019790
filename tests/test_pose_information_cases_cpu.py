"""The case generator of the pose information's edge tests (tests/pose_information_cases.py) without a device: the conditions
tests/test_gpu_pose_information_edges.py relies on, shown on the reference (tests/pose_information_ref.py), the CPU oracle and the
host algebra before any kernel runs.

* rows() gives the row counts the sizes are named for;
* every free case keeps between 30 % and 70 % of its rows, none of the poisoned ones and all of the zero-normal ones, which add
  nothing; the far cases cancel where they say they do;
* the batch poses are what batch_empty says;
* every scene's block eigenvalues lie at least a factor of ten from the thresholds it is reported with, `plane` has its exact zeros;
* the covariance and the Gauss-Newton step of the three scenes' reference records equal the construction from numpy's eigh."""
import numpy as np
import pytest

import pose_information_cases as cs
import pose_information_ref as pir


def test_rows_restates_the_sizes():
    assert [cs.rows(n) for n in cs.FREE_SIZES] == list(cs.FREE_ROWS) == [1, 2, 14, 15, 16, 17, 31, 32, 33]
    assert all(n % 512 not in (0, 256) and n % 256 for n in cs.FREE_SIZES)          # ragged in the last row, and in its last 256 lanes
    assert set(cs.FAR_ROWS) <= set(cs.FREE_ROWS)
    assert cs.CAP_SIZE == 524545 and cs.rows(cs.CAP_SIZE) == cs.CAP_ROWS == 1024 and cs.rows(1024 * 512) == 1024 and cs.rows(1023 * 512 + 1) == 1024
    assert cs.CAP_SIZE - 2 * 1024 * 256 == 257                                        # a third trip for 257 lanes
    assert cs.rows(0) == 1 and cs.rows(1) == 1 and cs.rows(512) == 1 and cs.rows(4096, 4) == 1 and cs.rows(4097, 4) == 2
    assert cs.BATCH_RAYS == 8777 and cs.BATCH_COUNTS == (1, 3, 4, 5, 9)
    assert [cs.rows(cs.BATCH_RAYS, k) for k in cs.BATCH_COUNTS] == [18, 18, 3, 3, 3]
    assert cs.rows(cs.SHORT_DATASET) == 10 and cs.SHORT_DATASET % 512
    m = cs.batch_model()
    assert (int(m.phi.size), int(m.theta.size)) == (67, 131)
    # the finalize loop's trips and tails, from its text: b = g, g + 16, ... while b + 14 < rows, then the rest two by two
    def trips(r, g):
        b, t = g, 0
        while b + 14 < r:
            b, t = b + 16, t + 1
        return t, len(range(b, r, 2))
    assert trips(14, 0) == (0, 7) and trips(15, 0) == (1, 0) and trips(15, 1) == (0, 7) and trips(16, 1) == (1, 0)
    assert trips(17, 0) == (1, 1) and trips(31, 0) == (2, 0) and trips(31, 1) == (1, 7) and trips(32, 1) == (2, 0)
    assert trips(33, 0) == (2, 1) and trips(33, 1) == (2, 0) and trips(1024, 0) == trips(1024, 1) == (64, 0) and trips(18, 1) == (1, 1)
    assert trips(3, 0) == (0, 2) and trips(3, 1) == (0, 1)


FREE = [(n, False) for n in cs.FREE_SIZES] + [(n, True) for n, r in zip(cs.FREE_SIZES, cs.FREE_ROWS) if r in cs.FAR_ROWS]


@pytest.mark.parametrize("n,far", FREE + [(cs.CAP_SIZE, False)])
def test_free_cases_keep_and_reject_what_they_say(ra, n, far):
    T = ra.types
    c = cs.free_case(n, cs.free_seed(n, far), far)
    again = cs.free_case(n, cs.free_seed(n, far), far)
    assert all(c[k].tobytes() == again[k].tobytes() for k in ("D", "I", "N", "I_nan", "N_nan", "dmask", "mmask"))
    poison, zero = c["poison"], c["zero"]
    assert sorted(poison) == [0, 63, 64, 255, 256, n - 1] and sorted(poison.values()) == sorted(2 * cs.POISON_KINDS)
    assert zero == [1, 62, 65, 254, 257]
    assert {i >> 6 for i in poison} >= {0, 1, 3, 4, (n - 1) >> 6}                     # different waves, different workgroups
    assert np.isnan(c["D"][[i for i, k in poison.items() if k == "nan_dataset"]]).any(axis=1).all()
    assert np.isinf(c["I_nan"][[i for i, k in poison.items() if k == "inf_model"]]).any(axis=1).all()
    assert np.isnan(c["N_nan"][[i for i, k in poison.items() if k == "nan_normal"]]).any(axis=1).all()
    assert all(c["dmask"][i] == 1 and c["mmask"][i] == 1 for i in list(poison) + zero)
    assert not c["N"][zero].any() and np.isfinite(c["D"][zero]).all() and np.isfinite(c["I_nan"][zero]).all()
    assert np.isnan(c["I_nan"][c["mmask"] == 0]).all() and np.isnan(c["N_nan"][c["mmask"] == 0]).all()
    assert 0.05 < (c["dmask"] == 0).mean() < 0.15 and 0.1 < (c["mmask"] == 0).mean() < 0.2
    settings = cs.MASK_SETTINGS if n != cs.CAP_SIZE else cs.MASK_SETTINGS[:1]
    for which, Tpre in (("identity", T.identity()), ("general", cs.tpre_general(far)))[:2 if n != cs.CAP_SIZE else 1]:
        for use_d, use_m in settings:
            ref = cs.reference(c, Tpre, use_d, use_m)
            what = "n=%d far=%s Tpre=%s masks=(%s, %s)" % (n, far, which, use_d, use_m)
            assert 0.3 * n <= ref["n_meas"] <= 0.7 * n, what
            assert not ref["kept"][sorted(poison)].any(), what
            assert ref["kept"][zero].all(), what
            at = np.cumsum(ref["kept"])[zero] - 1                                     # where the zero-normal rows sit among the kept ones
            assert not ref["U"][at].any(), what
            assert abs(np.trace(ref["A"][:3, :3]) / (ref["n_meas"] - len(zero)) - 1.0) < 1e-6, what
            if far and which == "identity":
                a, b = cs.FAR_CANCELLING
                ratio = abs(ref["A"][a, b]) / ref["A_abs"][a, b]
                print("%s: |A[%d, %d]| = %.3g of the sum of its terms' magnitudes %.3g" % (what, a, b, ratio, ref["A_abs"][a, b]))
                assert 0.0 < ratio < 1e-3, what
                assert ref["A_abs"][a, b] > 1e3 * ref["n_meas"] * 0.1                 # the terms are some thousand metres each


def test_batch_poses():
    import pose_batch_cases as pc
    full = pc.truth_and_estimates(9)[1]
    for k in cs.BATCH_COUNTS:
        P = cs.batch_poses(k)
        far, nan = cs.batch_empty(k)
        assert len(P) == k and P.tobytes() == cs.batch_poses(k).tobytes()
        if k < 4:
            assert (far, nan) == (None, None) and P.tobytes() == full[:k].tobytes()
            continue
        assert 0 < far < nan < k and P[far].tobytes() == pc.far_pose().tobytes() and np.isnan(P[nan]["t"]["x"])
        interior = [i for i in range(k) if i not in (far, nan)]
        assert len(interior) == k - 2 and all(P[i].tobytes() == full[i].tobytes() for i in interior)
    for p in full:                                                                    # inside the cube room (side 10 m)
        assert all(abs(float(p["t"][a])) < 4.0 for a in "xyz")


def test_batch_scans_hit_and_the_empty_poses_see_nothing(orc):
    import pose_batch_cases as pc
    mesh = orc.Mesh(*pc.map_arrays("cube"))
    m = {"kind": "spherical", "model": cs.batch_model()}
    r, pts, mask = pc.measure(mesh, m, cs.batch_truth())
    assert mask.all() and len(pts) == cs.BATCH_RAYS                                   # a closed room: the unmasked dataset holds no miss
    P = cs.batch_poses(9)
    far, nan = cs.batch_empty(9)
    sim = pc.simulate(mesh, m, P, bvh=False)
    hits = sim["hits"].reshape(9, cs.BATCH_RAYS)
    assert not hits[far].any() and not hits[nan].any()
    from rmcl_amd import types as T
    for i in range(9):
        if i in (far, nan):
            continue
        sl = slice(i * cs.BATCH_RAYS, (i + 1) * cs.BATCH_RAYS)
        for p in (0.0, 1.0):
            ref = pir.pose_information(T.identity(), pts, mask, sim["points"][sl], sim["normals"][sl], sim["hits"][sl],
                                       cs.adaptive(cs.BATCH_MAX_DIST, cs.BATCH_MAX_DIST_MIN, p))
            per_row = [int(ref["kept"][a:a + 4096].sum()) for a in range(0, cs.BATCH_RAYS, 4096)]
            print("pose %d, p = %g: kept %s of the rows of 4096" % (i, p, per_row))
            assert len(per_row) == 3 and min(per_row) > 64, (i, p)                    # every row of the batch form holds kept elements
        assert ref["n_meas"] < cs.BATCH_RAYS - 64                                     # and the narrow gate rejects some


@pytest.fixture(scope="module")
def scene_refs(orc):
    """per scene: (scene, reference of the oracle's correspondences)"""
    from rmcl_amd import types as T
    out = {}
    for name in cs.SCENES:
        s = cs.scene(name)
        mesh = orc.Mesh(*s["map"])
        ds, dmask = cs.scene_dataset(orc, mesh, s)
        mod = mesh.simulate_spherical(s["model"], T.identity(), s["estimate"], bvh=False)
        out[name] = (s, pir.pose_information(T.identity(), ds, dmask, mod["points"], mod["normals"], mod["hits"], s["max_dist"]), mod)
    return out


@pytest.mark.parametrize("name", cs.SCENES)
def test_scene_eigenvalues_stand_clear_of_the_thresholds(scene_refs, name):
    s, ref, mod = scene_refs[name]
    n = ref["n_meas"]
    assert 2000 < n <= int(mod["hits"].sum())
    et, er = np.linalg.eigvalsh(ref["A"][:3, :3] / n), np.linalg.eigvalsh(ref["A"][3:, 3:] / n)
    print("%s: n_meas %d, eigenvalues of A / n_meas: translation block %s, rotation block %s" % (name, n, et.tolist(), er.tolist()))
    p = s["params"]
    for ev, thr in ((et, p["min_eig_trans"]), (er, p["min_eig_rot"])):
        assert all(e <= thr / 10.0 or e >= thr * 10.0 for e in ev), (name, ev, thr)
    assert (int((et < p["min_eig_trans"]).sum()), int((er < p["min_eig_rot"]).sum())) == s["n_degenerate"]
    lam = np.linalg.eigvalsh(ref["A"])
    cut = p["rcond"] * lam.max()
    assert all(e <= cut / 10.0 or e >= cut * 10.0 for e in lam) and int((lam <= cut).sum()) == s["n_deficient"]
    nrm = mod["normals"][mod["hits"] > 0]
    if name == "plane":
        assert np.all(nrm == np.array([0.0, 0.0, 1.0], np.float32))
        for k in s["zero_rows"]:
            assert not ref["A"][k].any() and not ref["A"][:, k].any() and ref["g"][k] == 0.0 and ref["A_abs"][k, k] == 0.0
        assert sorted(set(range(6)) - set(s["zero_rows"])) == [2, 3, 4] and np.all(np.diag(ref["A"])[[2, 3, 4]] > 0)
    elif name == "sphere_centre":
        assert er.min() > 1e-4 and er.max() < 0.1 * et.min()                          # small beside the translations, and not zero
    else:
        a = nrm[0]
        assert np.all((nrm == a) | (nrm == -a)) and (nrm == a).all(axis=1).any() and (nrm == -a).all(axis=1).any()
        assert np.abs(a).min() > 0.05                                                 # no coordinate axis
        assert not s["zero_rows"] and np.abs(ref["A"]).min() > 0.0


@pytest.mark.parametrize("name", cs.SCENES)
def test_host_algebra_on_the_scenes_reference_records(ra, scene_refs, name):
    T = ra.types
    s, ref, _ = scene_refs[name]
    rec = pir.as_record(T, ref)
    cov, xi, V, kept = cs.check_host_algebra(T, rec, s, name)
    p = s["params"]
    assert np.linalg.norm(xi) > 0.01                                                  # the estimate is off: there is a step to compare
    if name == "plane":
        z = list(s["zero_rows"])
        assert np.array_equal(cov["eigvec_trans"][:2], np.eye(3)[:2]) and np.all(cov["eig_trans"][:2] == 0.0)
        assert np.array_equal(cov["eigvec_rot"][0], [0.0, 0.0, 1.0]) and float(cov["eig_rot"][0]) == 0.0
        assert np.all(np.diag(cov["covariance"])[z] == p["degenerate_variance"]) and np.all(xi[z] == 0.0)
        off = cov["covariance"][z].copy()
        off[np.arange(3), z] = 0.0
        assert not off.any()
        assert abs(xi[2] + 0.04) < 2e-3                                               # the estimate stands 4 cm too high
    if name == "sphere_centre":
        want = p["sigma"] ** 2 * np.linalg.inv(ref["A"])
        assert np.linalg.norm(cov["covariance"] - want) <= cs.COV_TOL * np.linalg.norm(want)
        np.linalg.cholesky(cov["covariance"])
