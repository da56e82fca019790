"""GPU tests of the pose hypotheses (rmcl_amd/csrc/hypotheses.hip, capi_hypotheses.cpp) against the numpy restatement
tests/hypotheses_ref.py: the clusters of the cloud's occupied bins -- count, ids, integer weights, bins, particles, order and labels
exact; every hypothesis's estimate within the tolerances tests/test_gpu_pf_cycle.py derives for the sharded estimate -- and of the
single-device pose estimate against the sharded filter's, bit for bit."""
import numpy as np
import pytest

import adaptive_ref as ar
import hypotheses_ref as hr
import pf_cycle_cases as pc

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 257, 1025)
NONE = hr.NONE
_refs = {}


@pytest.fixture(scope="module")
def est(ra, ctx):
    e = ra.PoseEstimatorHip(ctx)
    yield e
    e.close()


def _kld_params(ra, p):
    return ra.kld_params(bin_xyz=p.bin_xyz, bin_rpy=p.bin_rpy, min_likelihood_rel=p.min_likelihood_rel)


def _ref(key, poses, attrs, p, max_h):
    """the reference of a cloud, computed once (key names the cloud)"""
    if key not in _refs:
        _refs[key] = hr.hypotheses(poses, attrs, p, max_h)
    return _refs[key]


def _run(ra, ctx, est, poses, attrs, p, max_h=8):
    n = len(poses)
    est.kld = _kld_params(ra, p)
    d_p = ra.DeviceArray.from_host(ctx, poses if n else np.zeros(1, poses.dtype))
    d_a = ra.DeviceArray.from_host(ctx, attrs if n else np.zeros(1, attrs.dtype))
    d_l = ra.DeviceArray.from_host(ctx, np.zeros(max(n, 1), np.uint32))
    got = est.hypotheses(d_p, d_a, n, max_h, labels=d_l)
    return got, d_l.download()[:n]


def _check_estimate(poses, attrs, got, ref, concentrated, what):
    """tests/test_gpu_pf_cycle.py::_check_estimate on the members of one cluster: its tolerances and its two covariance floors"""
    for k in ("mean", "sigma", "min", "max"):
        print(what, "likelihood", k, got["likelihood"][k], ref["likelihood"][k])
        assert abs(got["likelihood"][k] - ref["likelihood"][k]) <= 1e-9 + 1e-9 * abs(ref["likelihood"][k]), (what, k)
    for k in ("trans_bb_min", "trans_bb_max"):
        assert np.array_equal(got[k], ref[k].astype(np.float32)), (what, k, got[k], ref[k])
    q = np.array([got["pose"]["R"][k] for k in "xyzw"], np.float64)
    t = np.array([got["pose"]["t"][k] for k in "xyz"], np.float64)
    print(what, "q", q, ref["q"], "t", t, ref["t"])
    assert min(np.linalg.norm(q - ref["q"]), np.linalg.norm(q + ref["q"])) < 1e-6, (what, q, ref["q"])
    assert q[3] >= 0 and abs(np.linalg.norm(q) - 1.0) <= 1e-6, (what, q)
    assert np.allclose(t, ref["t"], rtol=1e-6, atol=1e-6), (what, t, ref["t"])
    cov = pc.estimate_ref(poses, attrs, mean_pose=got["pose"])["covariance"]     # judged around the returned mean, in float64
    if concentrated:
        t_max = float(np.sqrt(poses["t"]["x"].astype(np.float64) ** 2 + poses["t"]["y"].astype(np.float64) ** 2 + poses["t"]["z"].astype(np.float64) ** 2).max())
        eps = 2.0 ** -23 * (t_max + np.pi)
        atol = 2.0 * np.sqrt(np.diag(cov).max()) * eps + eps * eps
    else:
        atol = 1e-6 * np.abs(cov).max()
    err = np.abs(got["covariance"] - cov)
    print(what, "covariance: largest error %.3g, floor %.3g, largest entry %.3g" % (err.max(), atol, np.abs(cov).max()))
    assert not (err > atol + 1e-4 * np.abs(cov)).any(), (what, err.max(), atol)
    assert np.array_equal(got["covariance"], got["covariance"].T), what


def _check(ra, ctx, est, key, poses, attrs, p, max_h=8, estimates=True):
    """run on the device, compare with the reference; returns (got, labels, ref)"""
    ref = _ref(key, poses, attrs, p, max_h)
    got, labels = _run(ra, ctx, est, poses, attrs, p, max_h)
    what = str(key)
    assert got["n_clusters"] == ref["n_clusters"], what
    assert len(got["hypotheses"]) == len(ref["hypotheses"]) == min(max_h, ref["n_clusters"]), what
    assert np.array_equal(labels, ref["labels"]), what
    for r, (g, w) in enumerate(zip(got["hypotheses"], ref["hypotheses"])):
        for k in ("key_min", "weight", "n_bins", "nparticles"):
            assert g[k] == w[k], (what, r, k, g[k], w[k])
        assert g["weight_share"] == float(w["weight"]) / float(ref["total"]), (what, r)
        if estimates:
            m = w["members"]
            _check_estimate(poses[m], attrs[m], g, w, w["n_bins"] == 1 or len(m) == 1, "%s, hypothesis %d" % (what, r))
    return got, labels, ref


# ---- 1, 2: what the feature is for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_one_bin_is_the_global_estimate(ra, ctx, est, n):
    poses, attrs = hr.at_bins(hr.rep(n, [hr.BASE]), 1)
    attrs["likelihood"]["mean"] = np.random.RandomState(n).uniform(0.2, 1.0, n)
    p = hr.kld()
    hr.assert_margin(poses, attrs, p)
    got, labels, ref = _check(ra, ctx, est, ("one_bin", n), poses, attrs, p)
    assert got["n_clusters"] == 1 and got["hypotheses"][0]["n_bins"] == 1 and (labels == 0).all()
    whole = est.estimate(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), n)
    _check_estimate(poses, attrs, whole, ref["hypotheses"][0], True, "one_bin %d, the global estimate" % n)


def _inside(t, box):
    return all(lo <= v < hi for v, lo, hi in zip(t, box[0], box[1]))


@pytest.mark.parametrize("n", NS)
def test_two_blobs_with_a_gap(ra, ctx, est, n):
    poses, attrs, p, (light, heavy) = hr.two_blobs(n)
    hr.assert_margin(poses, attrs, p)
    got, labels, ref = _check(ra, ctx, est, ("two_blobs", n), poses, attrs, p)
    if n == 1:
        assert got["n_clusters"] == 1
        return
    assert got["n_clusters"] == 2 and got["hypotheses"][0]["nparticles"] == n - (n + 2) // 3 and got["hypotheses"][0]["n_bins"] == 9
    whole = est.estimate(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), n)
    t_all = [float(whole["pose"]["t"][k]) for k in "xyz"]
    t_0 = [float(got["hypotheses"][0]["pose"]["t"][k]) for k in "xyz"]
    assert not _inside(t_all, light) and not _inside(t_all, heavy), t_all      # the one mean lies between the modes ...
    assert _inside(t_0, heavy), t_0                                            # ... hypothesis 0 inside the heavier one


# ---- 3, 4, 5: adjacency -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_diagonal_touch(ra, ctx, est, n):
    b = np.array(hr.BASE)
    for name, other, want in (("touch", b + 1, 1), ("apart_x", b + (2, 1, 1, 1, 1, 1), 2), ("apart_yaw", b + (1, 1, 1, 1, 1, 2), 2)):
        poses, attrs = hr.at_bins(hr.rep(n, [b, other]), 3)
        hr.assert_margin(poses, attrs, hr.kld())
        got, _, _ = _check(ra, ctx, est, ("diagonal", name, n), poses, attrs, hr.kld())
        assert got["n_clusters"] == min(want, n), name


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kill", ["zero", "nan", "below_floor"])
def test_killed_bridge(ra, ctx, est, n, kill):
    left, bridge, right = hr.blob((0, -2, 1, 18, 17, 5), (1, -1, 1, 18, 17, 5)), np.array([[2, -2, 1, 18, 17, 5]]), hr.blob((3, -2, 1, 18, 17, 5), (4, -1, 1, 18, 17, 5))
    rows = hr.rep(n, np.concatenate([left, bridge, right]))
    poses, attrs = hr.at_bins(rows, 4)
    on_bridge = rows[:, 0] == 2
    attrs["likelihood"]["mean"][on_bridge] = {"zero": 0.0, "nan": np.nan, "below_floor": 0.005}[kill]
    p = hr.kld()
    hr.assert_margin(poses, attrs, p)
    got, labels, _ = _check(ra, ctx, est, ("bridge", kill, n), poses, attrs, p)
    assert (labels[on_bridge] == NONE).all() and (labels[~on_bridge] != NONE).all()
    if n >= 63:
        assert got["n_clusters"] == 2 and on_bridge.any()
        alive = attrs.copy()
        alive["likelihood"]["mean"] = 1.0                   # the bridge alive: one cluster
        assert _check(ra, ctx, est, ("bridge", "alive", n), poses, alive, p)[0]["n_clusters"] == 1


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("width", [0.17453292, 1.0])
@pytest.mark.parametrize("field", [3, 5], ids=["roll_wrap", "yaw_wrap"])
def test_wrap(ra, ctx, est, field, width, n):
    last = hr.last_index(width)
    assert last == (36 if width < 1.0 else 6)
    for name, indices, with_pi in (("across", (last - 2, last - 1, 0, 1), False), ("across_pi", (last - 2, last - 1, 0, 1), True),
                                   ("short", (last - 3, last - 2, 1, 2), False)):
        poses, attrs, p, exact = hr.wrap_case(n, field, width, indices, with_pi)
        hr.assert_margin(poses, attrs, p, exact)
        got, _, ref = _check(ra, ctx, est, ("wrap", field, width, name, n), poses, attrs, p)
        if n < 4:                                           # fewer particles than bins: the reference alone says what is right
            continue
        if name != "short":
            assert got["n_clusters"] == 1 and got["hypotheses"][0]["n_bins"] == 4 + (1 if with_pi else 0)
        elif width < 1.0:
            assert got["n_clusters"] == min(n, 2)           # {33, 34} and {1, 2}: neither |i - j| <= 1 nor the wrap joins them
        else:
            # last = 6: {3, 4} and {1, 2} are plain neighbours (|3 - 2| = 1) -- one cluster by the adjacency rule itself
            assert got["n_clusters"] == 1


# ---- 6, 7, 11: sizes of their own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["line", "snake"])
def test_chain_of_2000_bins(ra, ctx, est, shape):
    poses, attrs = hr.at_bins(hr.chain_rows(shape), 70)
    hr.assert_margin(poses, attrs, hr.kld())
    got, labels, _ = _check(ra, ctx, est, ("chain", shape), poses, attrs, hr.kld())
    assert got["n_clusters"] == 1 and got["hypotheses"][0]["n_bins"] == 2000 and (labels == 0).all()


def test_isolated_grid(ra, ctx, est):
    poses, attrs = hr.at_bins(hr.isolated_grid_rows(), 71)
    attrs["likelihood"]["mean"] = np.random.RandomState(72).randint(1, 40, len(poses)).astype(np.float32) / np.float32(64.0)   # many ties
    hr.assert_margin(poses, attrs, hr.kld())
    got, labels, ref = _check(ra, ctx, est, "isolated_grid", poses, attrs, hr.kld())
    assert got["n_clusters"] == 4096 and len(got["hypotheses"]) == 8 and (labels != NONE).sum() == 8
    w = [h["weight"] for h in got["hypotheses"]]
    assert len(set(w)) < 8, "the case was meant to hold ties among its top eight"


def test_hot_root(ra, ctx, est):
    n = 65536
    rows = np.concatenate([hr.rep(n, [hr.BASE]), [np.array(hr.BASE) + (10, 0, 0, 0, 0, 0)]])
    poses, attrs = hr.at_bins(rows, 73)
    attrs["likelihood"]["mean"] = np.random.RandomState(74).uniform(0.3, 1.0, n + 1)
    hr.assert_margin(poses, attrs, hr.kld())
    got, labels, _ = _check(ra, ctx, est, "hot_root", poses, attrs, hr.kld())
    assert got["n_clusters"] == 2 and [h["nparticles"] for h in got["hypotheses"]] == [n, 1] and labels[-1] == 1


# ---- 8, 10: order and the cut -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_ties(ra, ctx, est, n):
    rows = hr.rep(4 * n, [hr.BASE])
    rows[:, 1] += 3 * (np.arange(4 * n) % 4)                # four clusters, n particles each, along y
    poses, attrs = hr.at_bins(rows, 8)
    p = hr.kld()
    hr.assert_margin(poses, attrs, p)
    got, _, _ = _check(ra, ctx, est, ("ties", n), poses, attrs, p)
    keys = [h["key_min"] for h in got["hypotheses"]]
    assert len(keys) == 4 and keys == sorted(keys) and len({h["weight"] for h in got["hypotheses"]}) == 1
    for name, v in (("ulp_down", np.nextafter(np.float32(1.0), np.float32(0.0))), ("ulp_up", np.nextafter(np.float32(1.0), np.float32(2.0)))):
        a2 = attrs.copy()
        a2["likelihood"]["mean"][1] = v                     # a particle of the second cluster
        g2, _, _ = _check(ra, ctx, est, ("ties", name, n), poses, a2, p)
        k2 = [h["key_min"] for h in g2["hypotheses"]]
        assert sorted(k2) == keys and (k2[-1] == keys[1] if name == "ulp_down" else k2[0] == keys[1]), (name, k2, keys)


@pytest.mark.parametrize("n", NS)
def test_max_hypotheses(ra, ctx, est, n):
    poses, attrs, p = hr.five_clusters(n)
    hr.assert_margin(poses, attrs, p)
    n_c = min(n, 5)                                         # (one particle is one cluster)
    for max_h in (1, 2, 64):
        got, labels, ref = _check(ra, ctx, est, ("five", n, max_h), poses, attrs, p, max_h)
        assert got["n_clusters"] == n_c and len(got["hypotheses"]) == min(max_h, n_c)
        assert set(labels.tolist()) == set(range(min(max_h, n_c))) | ({NONE} if max_h < n_c else set())
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    for bad in (0, 65):
        with pytest.raises(ra.RmclHipError, match="max_hypotheses") as e:
            est.hypotheses(d_p, d_a, n, bad)
        assert e.value.status == ra._capi.ERR_INVALID


# ---- 9: ignored dimensions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_ignored_dimensions(ra, ctx, est, n):
    cases = hr.rnd_cases(n)
    assert len(cases) == 7
    for name, (poses, attrs, p) in cases.items():
        hr.assert_margin(poses, attrs, p)
        _check(ra, ctx, est, ("rnd", name, n), poses, attrs, p)


# ---- 12: order independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_order_independence(ra, ctx, est, n):
    poses, attrs, p, _ = hr.two_blobs(n)
    attrs["likelihood"]["mean"] = np.random.RandomState(n).uniform(0.2, 1.0, n)
    got, labels, _ = _check(ra, ctx, est, ("two_blobs_weighted", n), poses, attrs, p)
    for seed in (1, 2, 3):
        perm = np.random.RandomState(seed).permutation(n)
        g2, l2 = _run(ra, ctx, est, poses[perm], attrs[perm], p)
        assert g2["n_clusters"] == got["n_clusters"] and np.array_equal(l2, labels[perm])
        for a, b in zip(g2["hypotheses"], got["hypotheses"]):
            assert all(a[k] == b[k] for k in ("key_min", "weight", "weight_share", "n_bins", "nparticles")), (seed, n)


# ---- 13: nothing to cluster -------------------------------------------------------------------------------------------------------
def test_empty(ra, ctx, est):
    poses, attrs = hr.at_bins(hr.rep(257, [hr.BASE]), 13)
    dead = attrs.copy()
    dead["likelihood"]["mean"] = 0.0
    nan = poses.copy()
    for k in "xyzw":
        nan["R"][k] = np.nan
    for k in "xyz":
        nan["t"][k] = np.nan
    inf = attrs.copy()
    inf["likelihood"]["mean"][5] = np.inf
    for what, P, A in (("n = 0", poses[:0], attrs[:0]), ("all zero", poses, dead), ("all NaN", nan, attrs), ("infinite maximum", poses, inf)):
        got, labels = _run(ra, ctx, est, P, A, hr.kld())
        assert got == {"n_clusters": 0, "hypotheses": []} and (labels == NONE).all(), what
        assert hr.hypotheses(P, A, hr.kld())["n_clusters"] == 0, what


# ---- 14: the handle -----------------------------------------------------------------------------------------------------------------
def _count_bins(ra, est, d_p, d_a, n):
    import ctypes as C
    k, c = C.c_uint32(0), C.c_uint32(0)
    ra._capi.check(ra._capi.lib().rmclhip_particles_count_bins(est._h, C.c_void_p(d_p.ptr), C.c_void_p(d_a.ptr), n, C.byref(est.kld), C.byref(k), C.byref(c)))
    return k.value, c.value


def test_handle_reuse(ra, ctx, est):
    big, small = hr.rnd_cases(1025)["zero_bin_dim_2"], hr.rnd_cases(63)["zero_bin_dim_2"]
    p = big[2]
    est.kld = _kld_params(ra, p)
    est.init()
    d_p, d_a = ra.DeviceArray.from_host(ctx, big[0]), ra.DeviceArray.from_host(ctx, big[1])
    before = _count_bins(ra, est, d_p, d_a, 1025)
    assert before == ar.count_bins(big[0], big[1], p)
    first = _check(ra, ctx, est, ("rnd", "zero_bin_dim_2", 1025), *big)
    assert _count_bins(ra, est, d_p, d_a, 1025) == before
    _check(ra, ctx, est, ("rnd", "zero_bin_dim_2", 63), *small)
    again = _run(ra, ctx, est, *big)
    assert np.array_equal(again[1], first[1]) and _same(again[0], first[0])


def _same(a, b):
    """two results of the binding, byte for byte"""
    if a["n_clusters"] != b["n_clusters"] or len(a["hypotheses"]) != len(b["hypotheses"]):
        return False
    return all(_same_estimate(x, y) and all(x[k] == y[k] for k in ("key_min", "weight", "weight_share", "n_bins"))
               for x, y in zip(a["hypotheses"], b["hypotheses"]))


def _same_estimate(x, y):
    return (x["pose"].tobytes() == y["pose"].tobytes() and x["covariance"].tobytes() == y["covariance"].tobytes() and
            x["likelihood"] == y["likelihood"] and x["trans_bb_min"].tobytes() == y["trans_bb_min"].tobytes() and
            x["trans_bb_max"].tobytes() == y["trans_bb_max"].tobytes() and x["nparticles"] == y["nparticles"])


# ---- 15: the single-device estimate ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank(ra, meshes):
    v, f = meshes("cube")
    sh = ra.ShardedParticleFilterHip(v, f, devices=(0,))
    yield sh
    sh.close()


@pytest.mark.parametrize("name", pc.ESTIMATE_CASES)
def test_single_device_estimate_is_the_one_rank_estimate(ra, ctx, est, one_rank, name):
    c = pc.estimate_case(name)
    n = len(c["poses"])
    one_rank.set_particles(c["poses"], c["attrs"])
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
    for n_ind in c["n_inductions"]:
        assert _same_estimate(est.estimate(d_p, d_a, n, n_ind), one_rank.pose_estimate(n_ind)), (name, n_ind)


def test_single_device_estimate_refusals(ra, ctx, est, one_rank):
    c = pc.estimate_case("single_weight")
    n = len(c["poses"])
    one_rank.set_particles(c["poses"], c["attrs"])
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
    for n_ind, msg in ((0, "no particles"), (1000, "sum to zero")):    # (the one particle with weight is the 1001st)
        for call in (lambda: est.estimate(d_p, d_a, n, n_ind), lambda: one_rank.pose_estimate(n_ind)):
            with pytest.raises(ra.RmclHipError, match=msg) as e:
                call()
            assert e.value.status == ra._capi.ERR_INVALID
    with pytest.raises(ra.RmclHipError, match="no particles"):
        est.estimate(d_p, d_a, 0)
    assert _same_estimate(est.estimate(d_p, d_a, n, 1001), one_rank.pose_estimate(1001))


# ---- 16: the sharded form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_hypotheses_are_the_single_device_bytes(ra, ctx, est, meshes, world):
    v, f = meshes("cube")
    sh = ra.ShardedParticleFilterHip(v, f, devices=(0,) * world, loopback=True)
    blobs = hr.two_blobs(1025)[:3]
    blobs[1]["likelihood"]["mean"] = np.random.RandomState(16).uniform(0.2, 1.0, 1025)
    for poses, attrs, p in (blobs, hr.rnd_cases(1025)["amcl_x_y_yaw"]):
        assert len(poses) % world != 0                      # a ragged partition
        sh.set_particles(poses, attrs)
        single, _ = _run(ra, ctx, est, poses, attrs, p)
        got = sh.pose_hypotheses(_kld_params(ra, p), 8)
        assert single["n_clusters"] >= 2 and _same(got, single)
        back = sh.download()
        assert back[0].tobytes() == poses.tobytes() and back[1].tobytes() == attrs.tobytes()
    assert sh.pose_hypotheses(_kld_params(ra, p), 1)["hypotheses"][0]["key_min"] == single["hypotheses"][0]["key_min"]
    with pytest.raises(ra.RmclHipError, match="max_hypotheses"):
        sh.pose_hypotheses(_kld_params(ra, p), 0)
    sh.close()


# ---- the C++ adapters -----------------------------------------------------------------------------------------------------------------
def test_cpp_example_prints_the_python_paths_results(ra, ctx, tmp_path):
    """examples/pose_hypotheses_cpp_example.cpp: a cloud with two modes through the C++ adapters; the global estimate and the two
    hypotheses it prints are the Python binding's"""
    import subprocess
    from test_cpp_adapters import _build
    from rmcl_amd import types as T
    exe = _build(tmp_path, "pose_hypotheses_cpp_example.cpp")
    n, seed = 3001, 7
    r = subprocess.run([exe, str(n), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: [float(x) for x in ln.split()[1:]] for ln in r.stdout.strip().splitlines()}
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    cov = np.zeros(36)
    cov[0], cov[7], cov[35] = 0.04, 0.04, 0.01
    n_a = n - n // 3
    ra.init_particles_pose(ctx, d_p, d_a, T.transform((0.0, 0.0, 0.19866933, 0.98006658), (1.5, -2.0, 0.0)), cov, seed, 0, 0, n_a)
    ra.init_particles_pose(ctx, d_p.ptr + 32 * n_a, d_a.ptr + 36 * n_a, T.transform((0.0, 0.0, -0.97572336, 0.21900669), (7.5, -2.0, 0.0)), cov,
                           seed, 0, n_a, n - n_a)
    e = ra.PoseEstimatorHip(ctx)

    def line(d):
        return [float(d["nparticles"])] + [float("%.9g" % d["pose"]["t"][k]) for k in "xyz"] + [float("%.9g" % d["pose"]["R"][k]) for k in "xyzw"]
    assert out["global"] == line(e.estimate(d_p, d_a, n))
    h = e.hypotheses(d_p, d_a, n, 2)
    assert out["clusters"] == [float(h["n_clusters"])] and len(h["hypotheses"]) == 2
    for r_, d in enumerate(h["hypotheses"]):
        assert out["hypothesis%d" % r_] == line(d)
        assert out["share%d" % r_] == [float("%.9g" % d["weight_share"]), float(d["n_bins"])]
    # what the example is about: the one mean lies between the rooms, the hypotheses inside them
    assert 2.5 < out["global"][1] < 6.5 and abs(out["hypothesis0"][1] - 1.5) < 0.1 and abs(out["hypothesis1"][1] - 7.5) < 0.1
    assert h["hypotheses"][0]["nparticles"] + h["hypotheses"][1]["nparticles"] <= n
    e.close()
