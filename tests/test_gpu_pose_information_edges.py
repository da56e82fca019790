"""The pose information's reduction (pose_information.hip) at every row count and batch shape, and the degeneracy
report on what a find returns -- on the cases of tests/pose_information_cases.py, whose premises
tests/test_pose_information_cases_cpu.py asserts without a device.

k_pose_information_partials writes rows(n, nposes) rows per pose and k_pose_information_finalize folds them: the free function runs at
1, 2, 14, 15, 16, 17, 31, 32 and 33 rows (below, at and after the finalize's unrolled loop of eight loads per half-wave, with every
tail) and at the cap of 1024; the batch form at 18 rows of 512 correspondences (one and three poses) and at 3 rows of 4096 (four, five
and nine poses); the operator form with a dataset shorter than the model and without a mask.  Every test prints the row count it
reaches.

The bound is the one of tests/test_gpu_pose_information.py: n_meas exact, every entry of A, g, rss within n_meas * 2^-52 * sum |terms|
of the math.fsum reference (pose_information_ref.assert_matches), which holds for any summation order in double."""
import numpy as np
import pytest

import pose_batch_cases as pc
import pose_information_cases as cs
import pose_information_ref as pir

pytestmark = pytest.mark.gpu

F = np.float32
ARRAYS = ("D", "I", "N", "I_nan", "N_nan", "dmask", "mmask")


class _Free:
    """a free case, its device copies (made on first use, on the session's context) and its references, computed once"""

    def __init__(self, ra, ctx, n, far):
        self.ra, self.ctx, self.n, self.far = ra, ctx, n, far
        self.case = cs.free_case(n, cs.free_seed(n, far), far)
        self.dev = {k: ra.DeviceArray.from_host(ctx, self.case[k]) for k in ARRAYS}
        self._refs = {}

    def args(self, use_d, use_m):
        pts, nrm = ("I_nan", "N_nan") if use_m else ("I", "N")
        d = self.dev
        return (d["D"], d["dmask"] if use_d else None, d[pts], d[nrm], d["mmask"] if use_m else None, self.n, float(cs.MAX_DIST))

    def ref(self, which, use_d, use_m):
        key = (which, use_d, use_m)
        if key not in self._refs:
            self._refs[key] = cs.reference(self.case, self.tpre(which), use_d, use_m)
        return self._refs[key]

    def tpre(self, which):
        return self.ra.types.identity() if which == "identity" else cs.tpre_general(self.far)

    def free(self):
        for d in self.dev.values():
            d.free()


@pytest.fixture(scope="module")
def free(ra, ctx):
    cache = {}

    def get(n, far=False):
        if (n, far) not in cache:
            cache[(n, far)] = _Free(ra, ctx, n, far)
        return cache[(n, far)]
    yield get
    for c in cache.values():
        c.free()


FREE = [(n, False) for n in cs.FREE_SIZES] + [(n, True) for n, r in zip(cs.FREE_SIZES, cs.FREE_ROWS) if r in cs.FAR_ROWS]


@pytest.mark.parametrize("n,far", FREE)
def test_every_row_count_of_the_free_function(ra, ctx, free, n, far):
    c = free(n, far)
    print("n = %d, far = %s: rows(n, 1) = %d" % (n, far, cs.rows(n, 1)))
    assert cs.rows(n, 1) in cs.FREE_ROWS
    for which in ("identity", "general"):
        Tpre = c.tpre(which)
        for use_d, use_m in cs.MASK_SETTINGS:
            what = "n=%d far=%s Tpre=%s masks=(%s, %s)" % (n, far, which, use_d, use_m)
            got = ra.pose_information_p2l(ctx, Tpre, *c.args(use_d, use_m))
            ref = c.ref(which, use_d, use_m)
            pir.assert_matches(got, ref, what)
            assert 0.3 * n <= ref["n_meas"] <= 0.7 * n, what
            assert int(got["n_meas"]) == int(ra.statistics_p2l(ctx, Tpre, *c.args(use_d, use_m))["n_meas"]), what
            assert ra.pose_information_p2l(ctx, Tpre, *c.args(use_d, use_m)).tobytes() == got.tobytes(), what


def test_row_cap(ra, ctx):
    T = ra.types
    n = cs.CAP_SIZE
    print("n = %d: rows(n, 1) = %d" % (n, cs.rows(n, 1)))
    assert cs.rows(n, 1) == cs.CAP_ROWS == 1024
    c = _Free(ra, ctx, n, False)
    try:
        got = ra.pose_information_p2l(ctx, T.identity(), *c.args(True, True))
        again = ra.pose_information_p2l(ctx, T.identity(), *c.args(True, True))
        ref = c.ref("identity", True, True)
        pir.assert_matches(got, ref, "cap")
        assert 0.3 * n <= ref["n_meas"] <= 0.7 * n
        assert again.tobytes() == got.tobytes()
        assert int(got["n_meas"]) == int(ra.statistics_p2l(ctx, T.identity(), *c.args(True, True))["n_meas"])
    finally:
        c.free()


def test_row_count_changes_on_one_context(ra, free):
    """the partials buffer only grows: after 33 rows, a call of 1 row and a call of 17 rows must read their own rows alone"""
    T = ra.types
    sizes = [cs.FREE_SIZES[cs.FREE_ROWS.index(r)] for r in (33, 1, 17)]
    own, fresh = ra.Context(0), ra.Context(0)
    try:
        got = {}
        for n in sizes:
            c = free(n)
            print("n = %d: rows(n, 1) = %d" % (n, cs.rows(n, 1)))
            got[n] = ra.pose_information_p2l(own, T.identity(), *c.args(True, True))
            pir.assert_matches(got[n], c.ref("identity", True, True), "n=%d after the others" % n)
        one = sizes[1]
        assert cs.rows(one, 1) == 1
        alone = ra.pose_information_p2l(fresh, T.identity(), *free(one).args(True, True))
        assert alone.tobytes() == got[one].tobytes()
    finally:
        own.close()
        fresh.close()


@pytest.fixture(scope="module")
def room(ra, orc, ctx):
    """the cube room, batch_model() on the mount of pose_batch_cases, the dataset the truth measures (a closed room: no miss)"""
    v, f = pc.map_arrays("cube")
    hm = ra.import_hip_map(ctx, v, f)
    m = {"kind": "spherical", "model": cs.batch_model()}
    ranges, pts, mask = pc.measure(orc.Mesh(v, f), m, cs.batch_truth())
    assert len(pts) == cs.BATCH_RAYS and mask.all()

    def make(points=pts, mask=mask):
        rcc = pc.operator(ra, hm, m)
        if points is not None:
            rcc.set_dataset(points, mask)
        rcc.params.max_dist = cs.BATCH_MAX_DIST
        rcc.adaptive_max_dist_min = cs.BATCH_MAX_DIST_MIN
        return rcc
    return dict(make=make, ranges=ranges, pts=pts, mask=mask)


def _as_ref(ref, record):
    """a reference's bounds around another device result: what the existing batch test compares the batch form to the single form with"""
    return dict(ref, A=record["A"], g=record["g"], rss=float(record["rss"]))


def test_batch_form_on_both_sides_of_the_switch(ra, room):
    T = ra.types
    n = cs.BATCH_RAYS
    rcc, rcc1 = room["make"](), room["make"]()
    identity_bytes = T.pose_information_identity().tobytes()
    singles = {}                                # (pose bytes, p) -> (record, reference) of the single form
    rows_seen = set()
    for k in cs.BATCH_COUNTS:
        poses = cs.batch_poses(k)
        far, nan = cs.batch_empty(k)
        print("%d poses of %d rays: rows(n, nposes) = %d per pose" % (k, n, cs.rows(n, k)))
        rows_seen.add(cs.rows(n, k))
        rcc.find_batch(poses)
        mvb = rcc.modelView()
        for p in (0.0, 1.0):
            maxd = cs.adaptive(cs.BATCH_MAX_DIST, cs.BATCH_MAX_DIST_MIN, p)
            batch = rcc.computePoseInformationBatch(k, p)
            assert rcc.computePoseInformationBatch(k, p).tobytes() == batch.tobytes()
            for i in range(k):
                what = "%d poses, p = %g, pose %d" % (k, p, i)
                sl = slice(i * n, (i + 1) * n)
                ref_b = pir.pose_information(T.identity(), room["pts"], room["mask"], mvb["points"][sl], mvb["normals"][sl], mvb["hits"][sl], maxd)
                pir.assert_matches(batch[i], ref_b, what)
                if i in (far, nan):
                    assert not mvb["hits"][sl].any() and batch[i].tobytes() == identity_bytes, what
                    continue
                assert ref_b["n_meas"] > 64 and (p == 0.0 or ref_b["n_meas"] < n), what
                key = (poses[i].tobytes(), p)
                if key not in singles:
                    rcc1.find(poses[i])
                    single = rcc1.computePoseInformation(T.identity(), p)
                    mv = rcc1.modelView()
                    ref = pir.pose_information(T.identity(), room["pts"], room["mask"], mv["points"], mv["normals"], mv["hits"], maxd)
                    pir.assert_matches(single, ref, "single form, " + what)
                    singles[key] = (single, ref)
                single, ref = singles[key]
                pir.assert_matches(batch[i], _as_ref(ref, single), "batch against single, " + what)
    assert rows_seen == {18, 3}
    rcc.close()
    rcc1.close()


def test_operator_form_with_a_shorter_and_an_unmasked_dataset(ra, room):
    T = ra.types
    n, short = cs.BATCH_RAYS, cs.SHORT_DATASET
    est = cs.batch_poses(3)
    Tgen = cs.tpre_general()
    rcc = room["make"](room["pts"][:short], None)
    print("dataset of %d points, model of %d rays: rows(n, 1) = %d" % (short, n, cs.rows(short, 1)))

    def single_against_reference(pts, mask, n_used, what):
        mv = rcc.modelView()
        assert len(mv["hits"]) == n
        for p in (0.0, 1.0):
            maxd = cs.adaptive(cs.BATCH_MAX_DIST, cs.BATCH_MAX_DIST_MIN, p)
            for Tp in (T.identity(), Tgen):
                got = rcc.computePoseInformation(Tp, p)
                ref = pir.pose_information(Tp, pts[:n_used], None if mask is None else mask[:n_used], mv["points"][:n_used],
                                           mv["normals"][:n_used], mv["hits"][:n_used], maxd)
                pir.assert_matches(got, ref, "%s, p = %g" % (what, p))
                assert ref["n_meas"] > 64 and int(rcc.computeCrossStatistics(Tp, p)["n_meas"]) == ref["n_meas"]
                assert rcc.computePoseInformation(Tp, p).tobytes() == got.tobytes()
        return ref

    rcc.find(est[0])
    ref = single_against_reference(room["pts"], None, short, "short unmasked dataset")
    assert ref["n_meas"] < short
    # the batch form: refused for more than one pose, since pose i's model rows start at i * n_model; one pose is the single form
    rcc.find_batch(est)
    with pytest.raises(ra.RmclHipError, match="dataset size != model size"):
        rcc.computePoseInformationBatch(3, 1.0)
    rcc.find_batch(est[:1])
    one = rcc.computePoseInformationBatch(1, 1.0)
    assert len(one) == 1
    rcc.find(est[0])
    assert one[0].tobytes() == rcc.computePoseInformation(T.identity(), 1.0).tobytes()
    # the dataset made on the device from ranges: as long as the model, with the mask the range interval gives
    assert rcc.set_dataset_from_ranges(room["ranges"]) == int(room["mask"].sum())
    made = rcc.inputView()
    assert len(made["points"]) == n and made["mask"] is not None and np.array_equal(made["mask"], room["mask"])
    print("dataset from %d ranges: rows(n, 1) = %d" % (n, cs.rows(n, 1)))
    rcc.find(est[1])
    single_against_reference(made["points"], made["mask"], n, "dataset from ranges")
    rcc.find_batch(est)
    batch = rcc.computePoseInformationBatch(3, 0.0)
    mvb = rcc.modelView()
    for i in range(3):
        sl = slice(i * n, (i + 1) * n)
        pir.assert_matches(batch[i], pir.pose_information(T.identity(), made["points"], made["mask"], mvb["points"][sl], mvb["normals"][sl],
                                                          mvb["hits"][sl], cs.BATCH_MAX_DIST), "dataset from ranges, batch pose %d" % i)
    rcc.close()


@pytest.mark.parametrize("name", cs.SCENES)
def test_degeneracy_report_on_device_results(ra, orc, ctx, name):
    T = ra.types
    s = cs.scene(name)
    v, f = s["map"]
    ds, dmask = cs.scene_dataset(orc, orc.Mesh(v, f), s)
    rcc = ra.RCCHipSpherical(ra.import_hip_map(ctx, v, f))
    rcc.setTsb(T.identity())
    rcc.setModel(s["model"])
    rcc.set_dataset(ds, dmask)
    rcc.params.max_dist = s["max_dist"]
    rcc.find(s["estimate"])
    mv = rcc.modelView()
    info = rcc.computePoseInformation(T.identity(), 0.0)
    print("%s: %d rays: rows(n, 1) = %d" % (name, len(ds), cs.rows(len(ds), 1)))
    pir.assert_matches(info, pir.pose_information(T.identity(), ds, dmask, mv["points"], mv["normals"], mv["hits"], s["max_dist"]), name)
    assert int(info["n_meas"]) > 2000
    cov, xi, V, kept = cs.check_host_algebra(T, info, s, name)
    p = s["params"]
    if name == "plane":
        nrm = mv["normals"][mv["hits"] > 0]
        assert np.all(nrm[:, :2] == 0.0) and np.all(np.abs(nrm[:, 2]) == 1.0)
        z = list(s["zero_rows"])
        for k in z:
            assert not info["A"][k].any() and not info["A"][:, k].any() and float(info["g"][k]) == 0.0
        assert np.array_equal(cov["eigvec_trans"][:2], np.eye(3)[:2]) and np.all(cov["eig_trans"][:2] == 0.0)
        assert np.array_equal(cov["eigvec_rot"][0], [0.0, 0.0, 1.0]) and float(cov["eig_rot"][0]) == 0.0
        assert np.all(np.diag(cov["covariance"])[z] == p["degenerate_variance"])
        off = cov["covariance"][z].copy()
        off[np.arange(3), z] = 0.0
        assert not off.any()
        assert np.all(xi[z] == 0.0) and abs(xi[2] + 0.04) < 2e-3                      # the estimate stands 4 cm too high
        assert np.all(np.diag(cov["covariance"])[[2, 3, 4]] < 1e-5)                   # millimetres where the plane does hold the pose
    elif name == "sphere_centre":
        assert float(cov["eig_rot"][2]) < 0.1 * float(cov["eig_trans"][0]) and float(cov["eig_rot"][0]) > 1e-4
        np.linalg.cholesky(cov["covariance"])
    else:
        nrm = mv["normals"][mv["hits"] > 0].astype(np.float64)
        a = nrm[0]
        assert np.abs(np.abs(nrm @ a) - 1.0).max() < 1e-6 and np.abs(a).min() > 0.05   # every normal +-a, a no coordinate axis
        free_dirs = V[:, ~kept]                                                        # translation across a, rotation about a
        along = np.concatenate([a, np.zeros(3)]), np.concatenate([np.zeros(3), a])
        assert np.linalg.norm(free_dirs.T @ along[0]) < 1e-5 and abs(np.linalg.norm(free_dirs.T @ along[1]) - 1.0) < 1e-5
    rcc.close()
