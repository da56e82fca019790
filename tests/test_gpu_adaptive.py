"""GPU tests of the adaptive particle count (rmcl_amd/csrc/adaptive.hip, resample.hip) against the numpy restatement tests/adaptive_ref.py:
occupied bins (k and the counted particles exact), systematic resampling to any size (sources and attributes byte-identical,
perturbed poses within the 1e-6 the other resamplers' tests allow), and the one call a Resampler plugin makes."""
import math

import numpy as np
import pytest

import adaptive_ref as ar
from particle_init_ref import euler_to_quat

pytestmark = pytest.mark.gpu

f32 = np.float32
BASE = (3, -2, 1, 18, 17, 5)          # a bin well inside every range (pitch index 17: -0.09 rad)
SEED = 0xC0FFEE1234567


@pytest.fixture(scope="module")
def rs(ra, ctx):
    r = ra.AdaptiveResamplerHip(ctx, seed=SEED)
    yield r
    r.close()


# ---- bins -------------------------------------------------------------------------------------------------
def _at_bins(idx, seed, widths=(0.5, 0.5, 0.5, 0.17453292, 0.17453292, 0.17453292)):
    """particles at the centres of the bins idx [n, 6] plus a jitter of at most 0.3 bin per dimension; likelihoods 1"""
    from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM
    idx = np.asarray(idx, dtype=np.float64).reshape(-1, 6)
    n = len(idx)
    jit = np.random.RandomState(seed).uniform(-0.3, 0.3, size=(n, 6))
    c = (idx + 0.5 + jit) * np.asarray(widths, dtype=np.float64)[None, :]
    c[:, 3:] -= math.pi
    assert np.abs(c[:, 4]).max() <= 1.2                    # pitch stays away from the poles
    c = c.astype(f32)
    p = np.zeros(n, dtype=TRANSFORM)
    for k, q in zip("xyzw", euler_to_quat(c[:, 3], c[:, 4], c[:, 5])):
        p["R"][k] = q
    for d, k in enumerate("xyz"):
        p["t"][k] = c[:, d]
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = 1.0
    return p, a


def _rep(n, rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    return rows[np.arange(n) % len(rows)]


def _bin_cases(n):
    """name -> (poses, attrs, params, expected k or None)"""
    i = np.arange(n)
    rs_ = np.random.RandomState(100 + n)
    out = {}
    out["one_bin"] = _at_bins(_rep(n, [BASE]), 1) + (ar.Kld(), 1)
    distinct = _rep(n, [BASE]).copy()
    distinct[:, 0], distinct[:, 1] = i % 500 - 250, i // 500 - 100
    out["all_distinct"] = _at_bins(distinct, 2) + (ar.Kld(), n)
    for d in range(6):                                      # tuples that differ in exactly one dimension
        rows = _rep(n, [BASE]).copy()
        rows[:, d] += i % 7 - 3
        out["differ_in_dim_%d" % d] = _at_bins(rows, 3 + d) + (ar.Kld(), min(n, 7))
    clamp = _rep(n, [BASE]).copy()                          # indices beyond the clamp on both sides, in x, y and z
    beyond = np.array([-9000, -8193, -8192, -8191, 8190, 8191, 8192, 9000])
    for d in range(3):
        clamp[:, d] = beyond[(i // 8 ** d) % 8]
    out["beyond_clamp"] = _at_bins(clamp, 10) + (ar.Kld(), min(n, 4) if n <= 8 else None)
    rnd = np.stack([rs_.randint(-6, 6, n), rs_.randint(-6, 6, n), rs_.randint(-2, 2, n), rs_.randint(14, 22, n), rs_.randint(14, 22, n),
                    rs_.randint(0, 36, n)], axis=1)
    out["amcl_x_y_yaw"] = _at_bins(rnd, 11) + (ar.Kld(bin_xyz=(0.5, 0.5, 0.0), bin_rpy=(0.0, 0.0, 0.17453292)), None)
    for d in range(6):                                      # a zero bin size per dimension
        bx, br = [0.5] * 3, [0.17453292] * 3
        (bx if d < 3 else br)[d % 3] = 0.0
        out["zero_bin_dim_%d" % d] = _at_bins(rnd, 12) + (ar.Kld(bin_xyz=bx, bin_rpy=br), None)
    oth = np.stack([rs_.randint(-6, 6, n), rs_.randint(-6, 6, n), rs_.randint(-2, 2, n), rs_.randint(0, 125, n), rs_.randint(7, 14, n),
                    rs_.randint(0, 6, n)], axis=1)
    out["other_bin_sizes"] = _at_bins(oth, 13, (0.25, 1.0, 2.0, 0.05, 0.3, 1.0)) + (ar.Kld(bin_xyz=(0.25, 1.0, 2.0), bin_rpy=(0.05, 0.3, 1.0)), None)
    p, a = _at_bins(rnd, 14)                                # the likelihood floor cuts a known subset: 0.01f * 1.0f is 0.01f exactly
    a["likelihood"]["mean"] = np.array([1.0, 0.5, 0.02, f32(0.01), np.nextafter(f32(0.01), f32(0)), 0.005, 1e-30], dtype=f32)[i % 7]
    out["likelihood_floor"] = (p, a, ar.Kld(), None)
    p, a = _at_bins(rnd, 15)
    a["likelihood"]["mean"][i % 3 == 1] = 0.0               # what the collision test killed
    a["likelihood"]["mean"][i % 5 == 2] = -1.0
    out["zero_likelihood"] = (p, a, ar.Kld(min_likelihood_rel=0.0), None)
    a0 = a.copy()
    a0["likelihood"]["mean"] = 0.0
    out["all_zero_likelihood"] = (p, a0, ar.Kld(min_likelihood_rel=0.0), 0)
    p, a = _at_bins(rnd, 16)
    p = p.copy()
    bad = [("R", "x", np.nan), ("R", "w", np.inf), ("t", "x", np.nan), ("t", "y", -np.inf), ("t", "z", np.inf), ("R", "z", np.nan)]
    for m, (grp, k, v) in enumerate(bad):
        p[grp][k][i % 11 == m] = v
    a["likelihood"]["mean"][i % 11 == 7] = np.nan
    a["likelihood"]["mean"][i % 11 == 8] = -np.inf
    out["nan_inf"] = (p, a, ar.Kld(), None)
    a1 = a.copy()
    a1["likelihood"]["mean"][i % 11 == 9] = np.inf          # an infinite maximum: the floor is infinite, nothing is counted
    out["inf_likelihood"] = (p, a1, ar.Kld(), 0 if n > 9 else None)
    return out


def _kld_params(ra, p):
    return ra.kld_params(bin_xyz=p.bin_xyz, bin_rpy=p.bin_rpy, min_likelihood_rel=p.min_likelihood_rel, epsilon=p.epsilon, z=p.z, n_min=p.n_min,
                         n_max=p.n_max)


def _check_bins(ra, ctx, rs, poses, attrs, p, expect_k, what):
    # the margin, from the restatement, before the device is used: an ulp between the device's and numpy's atan2 cannot change a bin
    assert ar.bin_margin(poses, attrs, p) >= 0.19, what
    k_ref, counted_ref = ar.count_bins(poses, attrs, p)
    if expect_k is not None:
        assert k_ref == expect_k, what
    rs.kld = _kld_params(ra, p)
    n = len(poses)
    got = rs.count_bins(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), n)
    assert got == {"bins": k_ref, "counted": counted_ref}, what
    return k_ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_count_bins_matches_restatement(ra, ctx, rs, n):
    cases = _bin_cases(n)
    assert len(cases) == 22
    for name, (poses, attrs, p, expect_k) in cases.items():
        k = _check_bins(ra, ctx, rs, poses, attrs, p, expect_k, (name, n))
        perm = np.random.RandomState(n).permutation(n)      # the same cloud permuted: the same k
        assert _check_bins(ra, ctx, rs, poses[perm], attrs[perm], p, expect_k, (name, n, "permuted")) == k
    if n >= 1000:                                           # the cases do what their names say
        assert ar.count_bins(*cases["likelihood_floor"][:3])[1] == int(np.isin(np.arange(n) % 7, (0, 1, 2, 3)).sum())
        assert 0 < ar.count_bins(*cases["zero_likelihood"][:3])[1] < n and 0 < ar.count_bins(*cases["nan_inf"][:3])[1] < n
        assert ar.count_bins(*cases["beyond_clamp"][:3])[0] == 4 ** 3


def test_count_bins_100k(ra, ctx, rs):
    n = 100000
    cases = _bin_cases(n)
    for name, (poses, attrs, p, expect_k) in cases.items():
        _check_bins(ra, ctx, rs, poses, attrs, p, expect_k, name)


def test_count_bins_arguments(ra, ctx, rs):
    poses, attrs = _at_bins(_rep(10, [BASE]), 1)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    rs.kld = ra.kld_params()
    assert rs.count_bins(d_p, d_a, 0) == {"bins": 0, "counted": 0}
    for bad in (dict(bin_xyz=(0.5, -1.0, 0.5)), dict(bin_xyz=(float("nan"), 0.5, 0.5)), dict(bin_rpy=(0.01, 0.2, 0.2)), dict(bin_rpy=(0.2, float("inf"), 0.2)),
                dict(min_likelihood_rel=1.5), dict(min_likelihood_rel=float("nan"))):
        rs.kld = ra.kld_params(**bad)
        with pytest.raises(ra.RmclHipError, match="particles_count_bins"):
            rs.count_bins(d_p, d_a, 10)
    rs.kld = ra.kld_params()
    with pytest.raises(ra.RmclHipError, match="null particle buffers"):
        rs.count_bins(None, d_a, 10)


# ---- systematic resampling --------------------------------------------------------------------------------
NOISE = dict(min_noise_tz=0.01, min_noise_roll=0.005, min_noise_pitch=0.005)


def _run_systematic(ra, ctx, rs, d_p, d_a, n, n_new, step, first=0, count=None):
    from rmcl_amd import types as T
    count = n_new - first if count is None else count
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, count), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, count)
    rs.step = step
    assert rs.update_systematic(d_p, d_a, d_pn, d_an, n, n_new, first, count) == {"n_particles": count}
    return d_pn.download(), d_an.download()


def _assert_cloud(pn, an, ref, what):
    pn_ref, an_ref, src = ref
    assert np.array_equal(pn["stamp"], src), what                              # the source of every slot (stamp = index)
    assert an.tobytes() == an_ref.tobytes(), what                              # likelihoods, n_meas, state_sigma: bit-exact
    for grp, keys in (("t", "xyz"), ("R", "xyzw")):
        for k in keys:
            assert np.allclose(pn[grp][k], pn_ref[grp][k], rtol=0, atol=1e-6), what


@pytest.mark.parametrize("n", ar.SYS_N)
def test_systematic_matches_restatement(ra, ctx, rs, n):
    from rmcl_amd import types as T
    poses, attrs = ar.cloud(n, 21)
    d_p = ra.DeviceArray.from_host(ctx, poses)
    rs.config = T.gladiator_config(**NOISE)
    cfg = ar.gladiator_cfg(**NOISE)
    for name, L in ar.weight_cases(n).items():
        attrs["likelihood"]["mean"] = L
        d_a = ra.DeviceArray.from_host(ctx, attrs)
        for n_new in ar.sys_n_new(n):
            got = {}
            for step in (0, 1):
                ref = ar.systematic(poses, attrs, n_new, cfg, SEED, step)
                pn, an = _run_systematic(ra, ctx, rs, d_p, d_a, n, n_new, step)
                _assert_cloud(pn, an, ref, (name, n, n_new, step))
                first_of_run = np.ones(n_new, bool)
                first_of_run[1:] = ref[2][1:] != ref[2][:-1]
                assert pn[first_of_run].tobytes() == poses[ref[2][first_of_run]].tobytes()      # first copies: the source's bytes
                got[step] = (pn, first_of_run)
            if name == "even" and n_new == n:
                assert got[0][0].tobytes() == poses.tobytes() and got[1][0].tobytes() == poses.tobytes()
            if name == "one_holds_all":
                assert np.all(got[0][0]["stamp"] == n // 2)
            both = ~got[0][1] & ~got[1][1]                  # slots perturbed in both steps: other Gaussians
            if both.sum() > 3:
                assert (got[0][0]["t"]["x"][both] != got[1][0]["t"]["x"][both]).mean() > 0.9
    # metric 1 (|t|^2) is honoured
    attrs["likelihood"]["mean"] = ar.weight_cases(n)["span_1e-6_1"]
    d_a = ra.DeviceArray.from_host(ctx, attrs)
    rs.config = T.gladiator_config(trans_dist_metric=1, **NOISE)
    pn, an = _run_systematic(ra, ctx, rs, d_p, d_a, n, 3 * n, 4)
    _assert_cloud(pn, an, ar.systematic(poses, attrs, 3 * n, ar.gladiator_cfg(trans_dist_metric=1, **NOISE), SEED, 4), ("metric 1", n))


@pytest.mark.parametrize("n", [64, 65, 1025, 4097])
def test_systematic_shrinks_an_even_cloud_where_residual_cannot(ra, ctx, rs, n):
    """the gap this resampler closes: an evenly weighted (converged) cloud resampled to a twentieth of its size"""
    from rmcl_amd import types as T
    poses, attrs = ar.cloud(n, 22)
    attrs["likelihood"]["mean"] = 0.37
    n_new = n // 20
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    rs.config = T.gladiator_config(**NOISE)
    pn, an = _run_systematic(ra, ctx, rs, d_p, d_a, n, n_new, 0)
    _assert_cloud(pn, an, ar.systematic(poses, attrs, n_new, ar.gladiator_cfg(**NOISE), SEED, 0), n)
    assert len(set(pn["stamp"].tolist())) == n_new and pn.tobytes() == poses[pn["stamp"]].tobytes()   # n_new distinct particles, copied
    assert np.all(np.diff(pn["stamp"].astype(np.int64)) >= 19)                                     # spread evenly over the cloud
    res = ra.ResidualResamplerHip(ctx, seed=SEED)
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n_new), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n_new)
    with pytest.raises(ra.RmclHipError, match="truncates to 0"):
        res.update(d_p, d_a, d_pn, d_an, n, n_new)
    res.close()


@pytest.mark.parametrize("n,n_new", [(1025, 3075), (4097, 585), (65, 65)])
def test_systematic_slices_equal_one_call(ra, ctx, rs, n, n_new):
    from rmcl_amd import types as T
    poses, attrs = ar.cloud(n, 23)
    attrs["likelihood"]["mean"] = ar.weight_cases(n)["span_1e-6_1"]
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    rs.config = T.gladiator_config(**NOISE)
    whole = _run_systematic(ra, ctx, rs, d_p, d_a, n, n_new, 3)
    cuts = [0, n_new // 3, n_new // 3 + 1, n_new]           # (a slice of one slot; slices that start inside a run)
    parts = [_run_systematic(ra, ctx, rs, d_p, d_a, n, n_new, 3, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in range(2):
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes()
    ref = ar.systematic(poses, attrs, n_new, ar.gladiator_cfg(**NOISE), SEED, 3, first=cuts[1], count=cuts[3] - cuts[1])
    _assert_cloud(np.concatenate([parts[1][0], parts[2][0]]), np.concatenate([parts[1][1], parts[2][1]]), ref, (n, n_new))


def test_systematic_error_cases(ra, ctx, rs):
    from rmcl_amd import types as T
    n = 100
    poses, attrs = ar.cloud(n, 24)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_pn, d_an = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    rs.config = T.gladiator_config()
    for L in (0.0, -1.0, float("inf"), float("nan")):       # max <= 0 or not finite (NaN is never the maximum: it stays 0)
        bad = attrs.copy()
        bad["likelihood"]["mean"] = L
        with pytest.raises(ra.RmclHipError, match="nothing to resample from"):
            rs.update_systematic(d_p, ra.DeviceArray.from_host(ctx, bad), d_pn, d_an, n, n)
    with pytest.raises(ra.RmclHipError, match="0 particles"):
        rs.update_systematic(d_p, d_a, d_pn, d_an, n, 0, 0, 0)
    with pytest.raises(ra.RmclHipError, match="slot range"):
        rs.update_systematic(d_p, d_a, d_pn, d_an, n, 50, 40, 11)
    with pytest.raises(ra.RmclHipError, match="null particle buffers"):
        rs.update_systematic(d_p, d_a, None, d_an, n, 50)
    with pytest.raises(ra.RmclHipError, match="out of place"):
        rs.update_systematic(d_p, d_a, d_p, d_a, n, n)
    # count == 0: OK and nothing touched, null buffers included
    before = d_pn.download().tobytes()
    assert rs.update_systematic(d_p, d_a, d_pn, d_an, n, 50, 50, 0) == {"n_particles": 0}
    assert rs.update_systematic(None, None, None, None, n, 50, 7, 0) == {"n_particles": 0}
    assert d_pn.download().tobytes() == before


# ---- the one call of a Resampler plugin -------------------------------------------------------------------
def _uniform_cloud(n, seed):
    from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM
    r = np.random.RandomState(seed)
    v = r.uniform((-50, -50, -50, -math.pi, -1.2, -math.pi), (50, 50, 50, math.pi, 1.2, math.pi), size=(n, 6)).astype(f32)
    p = np.zeros(n, dtype=TRANSFORM)
    for k, q in zip("xyzw", euler_to_quat(v[:, 3], v[:, 4], v[:, 5])):
        p["R"][k] = q
    for d, k in enumerate("xyz"):
        p["t"][k] = v[:, d]
    p["stamp"] = np.arange(n, dtype=np.uint32)
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = r.uniform(0.2, 1.0, n)
    a["likelihood"]["n_meas"] = r.randint(0, 10001, n)
    return p, a


def test_adaptive_follows_the_posterior(ra, ctx, rs):
    from rmcl_amd import types as T
    n, cap = 20000, 30000
    rs.config = T.gladiator_config(**NOISE)
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, cap), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, cap)

    # a global localisation: uniform in a 100 m box -- nearly every particle has a bin of its own
    poses, attrs = _uniform_cloud(n, 31)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    for kw, clamped in ((dict(), True), (dict(epsilon=0.5, z=1.6448536), False)):
        p = ar.Kld(**kw)
        rs.kld = _kld_params(ra, p)
        k_ref, _ = ar.count_bins(poses, attrs, p)
        assert k_ref > 0.99 * n
        free = ar.kld_bound(k_ref, p.epsilon, p.z, p.n_min, p.n_max)
        n_ref = ar.kld_bound(k_ref, p.epsilon, p.z, p.n_min, min(p.n_max, cap))
        assert (free > cap and n_ref == cap) if clamped else (n < free == n_ref < cap)
        rs.step = 5
        res = rs.update(d_p, d_a, d_pn, d_an, n, cap)
        assert res == {"n_particles": n_ref, "bins": k_ref}
        got = d_pn.download()[:n_ref], d_an.download()[:n_ref]
        # ... and equals the three calls made one after the other
        assert rs.count_bins(d_p, d_a, n)["bins"] == k_ref and rs.kld_bound(k_ref, cap) == n_ref
        sep = _run_systematic(ra, ctx, rs, d_p, d_a, n, n_ref, 5)
        assert got[0].tobytes() == sep[0].tobytes() and got[1].tobytes() == sep[1].tobytes()
        _assert_cloud(got[0], got[1], ar.systematic(poses, attrs, n_ref, ar.gladiator_cfg(**NOISE), SEED, 5), kw)

    # the same cloud collapsed to three bins: n_min
    idx = _rep(n, [BASE, (4, -2, 1, 18, 17, 5), (3, -2, 1, 18, 17, 6)])
    cp, _ = _at_bins(idx, 32)
    cp["stamp"] = poses["stamp"]
    p = ar.Kld()
    assert ar.bin_margin(cp, attrs, p) >= 0.19 and ar.count_bins(cp, attrs, p)[0] == 3
    rs.kld = _kld_params(ra, p)
    d_p = ra.DeviceArray.from_host(ctx, cp)
    rs.step = 6
    assert rs.update(d_p, d_a, d_pn, d_an, n, cap) == {"n_particles": 500, "bins": 3}
    _assert_cloud(d_pn.download()[:500], d_an.download()[:500], ar.systematic(cp, attrs, 500, ar.gladiator_cfg(**NOISE), SEED, 6), "collapsed")
    # room for fewer than n_min: the room wins
    assert rs.update(d_p, d_a, d_pn, d_an, n, 100) == {"n_particles": 100, "bins": 3}
    with pytest.raises(ra.RmclHipError, match="0 particles"):
        rs.update(d_p, d_a, d_pn, d_an, n, 0)
    rs.kld = ra.kld_params(n_min=0)
    with pytest.raises(ra.RmclHipError, match="n_min"):
        rs.update(d_p, d_a, d_pn, d_an, n, cap)
    rs.kld = ra.kld_params(epsilon=0.0)
    with pytest.raises(ra.RmclHipError, match="epsilon"):
        rs.update(d_p, d_a, d_pn, d_an, n, cap)
    rs.kld = ra.kld_params()


def test_cpp_example_adopts_the_python_paths_counts(ra, ctx, tmp_path):
    """examples/adaptive_resample_cpp_example.cpp: the node's resample step with the count adopted, through the C++ adapters; its
    counts and its dumped cloud equal the Python binding's"""
    import subprocess
    from test_cpp_adapters import _build
    from rmcl_amd import types as T
    exe = _build(tmp_path, "adaptive_resample_cpp_example.cpp")
    cloud_bin = tmp_path / "cloud.bin"
    cap, seed = 20000, 7
    r = subprocess.run([exe, str(cloud_bin), str(cap), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.strip().splitlines()}
    res = ra.AdaptiveResamplerHip(ctx, seed=seed)
    bufs = [(ra.DeviceArray(ctx, T.TRANSFORM, cap), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, cap)) for _ in range(2)]
    ra.init_particles_uniform(ctx, bufs[0][0], bufs[0][1], (-50.0, -50.0, 0.0, 0.0, 0.0, -3.14), (50.0, 50.0, 0.0, 0.0, 0.0, 3.14), seed, 0)
    g = res.update(bufs[0][0], bufs[0][1], bufs[1][0], bufs[1][1], cap, cap)
    assert out["global"] == [g["n_particles"], g["bins"]] and g["n_particles"] == cap and g["bins"] > cap // 2
    bufs.reverse()
    cov = np.zeros(36)
    cov[0], cov[7], cov[35] = 0.04, 0.04, 0.01
    ra.init_particles_pose(ctx, bufs[0][0], bufs[0][1], T.transform((0.0, 0.0, 0.19866933, 0.98006658), (0.5, -0.3, 0.2)), cov, seed, 1)
    c = res.update(bufs[0][0], bufs[0][1], bufs[1][0], bufs[1][1], cap, cap)
    assert out["converged"] == [c["n_particles"], c["bins"]] and 500 <= c["n_particles"] < cap // 2 and 3 < c["bins"] < 500
    bufs.reverse()
    a = res.update(bufs[0][0], bufs[0][1], bufs[1][0], bufs[1][1], c["n_particles"], cap)
    assert out["again"] == [a["n_particles"], a["bins"]] and 500 <= a["n_particles"] < cap // 2
    n = a["n_particles"]
    raw = cloud_bin.read_bytes()
    assert int(np.frombuffer(raw[:4], np.uint32)[0]) == n and len(raw) == 4 + 68 * n
    assert raw[4:4 + 32 * n] == bufs[1][0].download()[:n].tobytes() and raw[4 + 32 * n:] == bufs[1][1].download()[:n].tobytes()
    res.close()
