"""GPU parity of the particle-filter cycle around the sensor update, at its edges (cases: tests/pf_cycle_cases.py, proved non-vacuous
on the CPU by tests/test_pf_cycle_cases_cpu.py):

  k_pf_motion          against the oracle's BRUTE-FORCE collision test byte for byte: deep maps (the private-memory rows of
                       trace_lane_bf<16, true>), one wall of two triangles, the length gate, roll / pitch, NaN, forgetting; particle
                       counts around the block size with the records past n untouched; the sharded path; forget rates outside [0, 1]
  k_pose_moments*      and the host's eigenvector against a float64 restatement of RmclNode::estimateStats: mixed-sign quaternions, a
                       cloud across yaw = +-pi, one particle with all the weight, induction counts that end inside a rank, more than
                       262144 particles on one rank (the grid-stride second trip, the unrolled fold), a cloud without weight
  k_scan_*             of the residual resampler with more draws than one trip of the block-total scan covers

Every comparison is against the oracle or the float64 reference; the sign-flip property alone compares the product with itself."""
import numpy as np
import pytest

import pf_cycle_cases as pc

pytestmark = pytest.mark.gpu

_maps = {}


def _hip_map(ra, ctx, case):
    if case["map"] not in _maps:
        _maps[case["map"]] = ra.import_hip_map(ctx, case["v"], case["f"])
    return _maps[case["map"]]


def _padded(arr, n, pad=64):
    """the first n records and `pad` more filled with a byte pattern"""
    out = np.zeros(n + pad, arr.dtype)
    out.view(np.uint8)[:] = 0xA5
    out[:n] = arr[:n]
    return out


def _assert_same(name, what, got, want, n=None):
    msg = pc.first_difference(name, what, got, want, n)
    assert msg is None, msg


# ---- motion update ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collision", [False, True])
@pytest.mark.parametrize("name", pc.MOTION_CASES)
def test_motion_update_matches_brute_force(ra, orc, ctx, meshes, name, collision):
    c = pc.motion_case(name, meshes)
    n = len(c["poses"])
    upd = ra.TFMotionUpdaterHip(_hip_map(ra, ctx, c), check_collision=collision)
    h_p, h_a = _padded(c["poses"], n), _padded(c["attrs"], n)
    d_p, d_a = ra.DeviceArray.from_host(ctx, h_p), ra.DeviceArray.from_host(ctx, h_a)
    upd.update(d_p, d_a, n, c["T_delta"], c["rate"])
    p_ref, a_ref = pc.motion_reference(c, orc, collision)
    p, a = d_p.download(), d_a.download()
    what = "with the collision test" if collision else "without the collision test"
    _assert_same(name, "poses %s (device, brute-force oracle)" % what, p, p_ref, n)
    _assert_same(name, "attributes %s (device, brute-force oracle)" % what, a, a_ref, n)
    assert p[n:].tobytes() == h_p[n:].tobytes() and a[n:].tobytes() == h_a[n:].tobytes(), "%s: records past n were written" % name
    upd.close()


@pytest.mark.parametrize("n", (0,) + pc.BLOCK_EDGE_COUNTS)
def test_motion_update_around_the_block_size_leaves_the_tail_alone(ra, orc, ctx, meshes, n):
    """n below, at and above the 64-lane wave and the 256-thread block: lanes past n read particle 0 and trace nothing; what lies behind
    the n-th record stays as it was, byte for byte"""
    for name in ("chain200_long", "nested200_short"):
        c = pc.motion_case(name, meshes)
        upd = ra.TFMotionUpdaterHip(_hip_map(ra, ctx, c), check_collision=True)
        off = 0 if name == "chain200_long" else 3       # (another alignment of the aimed cloud's cycle of eight step fractions)
        h_p, h_a = _padded(c["poses"][off:], n), _padded(c["attrs"][off:], n)
        d_p, d_a = ra.DeviceArray.from_host(ctx, h_p), ra.DeviceArray.from_host(ctx, h_a)
        assert upd.update(d_p, d_a, n, c["T_delta"], c["rate"]) == {}
        p_ref, a_ref = pc.motion_reference(c, orc, True)
        p, a = d_p.download(), d_a.download()
        _assert_same("%s n %d" % (name, n), "poses", p, p_ref[off:], n)
        _assert_same("%s n %d" % (name, n), "attributes", a, a_ref[off:], n)
        _assert_same("%s n %d" % (name, n), "poses past n", p[n:], h_p[n:])
        _assert_same("%s n %d" % (name, n), "attributes past n", a[n:], h_a[n:])
        if n >= 63:
            k = pc.killed(a_ref[off:off + n])
            assert k.any() and not k.all()
        upd.close()


def test_motion_update_sharded_ragged_on_a_deep_map(ra, orc, ctx, meshes):
    """three loopback ranks, 1999 particles (667 + 666 + 666): the sharded update == the unsharded one == the brute-force oracle"""
    c = pc.motion_case("nested200_long", meshes)
    n = 1999
    sh = ra.ShardedParticleFilterHip(c["v"], c["f"], devices=(0, 0, 0), loopback=True)
    sh.set_particles(c["poses"][:n], c["attrs"][:n])
    sh.motion_update(c["T_delta"], c["rate"], check_collision=True)
    p, a = sh.download()
    sh.close()
    upd = ra.TFMotionUpdaterHip(_hip_map(ra, ctx, c), check_collision=True)
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"][:n]), ra.DeviceArray.from_host(ctx, c["attrs"][:n])
    upd.update(d_p, d_a, n, c["T_delta"], c["rate"])
    upd.close()
    p_ref, a_ref = pc.motion_reference(c, orc, True)
    _assert_same("nested200_long sharded", "poses (sharded, brute-force oracle)", p, p_ref, n)
    _assert_same("nested200_long sharded", "attributes (sharded, brute-force oracle)", a, a_ref, n)
    _assert_same("nested200_long sharded", "poses (sharded, unsharded)", p, d_p.download(), n)
    _assert_same("nested200_long sharded", "attributes (sharded, unsharded)", a, d_a.download(), n)


def test_forget_rate_outside_the_unit_interval_is_refused(ra, ctx, meshes):
    """uint32(n_meas - rate * n_meas) of a negative double (or one past 2^32) is undefined: the three entry points refuse the rate with
    RMCLHIP_ERR_INVALID and touch nothing; the ends of the interval are accepted"""
    from rmcl_amd import _capi, synthetic as syn, types as T
    c = pc.motion_case("forget_3", meshes)
    n = len(c["poses"])
    upd = ra.TFMotionUpdaterHip(_hip_map(ra, ctx, c), check_collision=True)
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
    sh = ra.ShardedParticleFilterHip(c["v"], c["f"], devices=(0, 0, 0), loopback=True)
    sh.set_particles(c["poses"], c["attrs"])
    beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::32] * np.float32(3.0))
    for rate in pc.BAD_FORGET_RATES:
        calls = {"rmclhip_pf_motion_update": lambda: upd.update(d_p, d_a, n, c["T_delta"], rate),
                 "rmclhip_pf_sharded_motion_update": lambda: sh.motion_update(c["T_delta"], rate),
                 "rmclhip_pf_sharded_step": lambda: sh.step(beams, T.identity(), T_bnew_bold=c["T_delta"], forget_rate=rate)}
        for fn, call in calls.items():
            with pytest.raises(ra.RmclHipError, match="forget_rate") as e:
                call()
            assert e.value.status == _capi.ERR_INVALID, "%s(forget_rate = %r): status %d" % (fn, rate, e.value.status)
        assert d_p.download().tobytes() == c["poses"].tobytes() and d_a.download().tobytes() == c["attrs"].tobytes(), rate
        p, a = sh.download()
        assert p.tobytes() == c["poses"].tobytes() and a.tobytes() == c["attrs"].tobytes(), rate
    for rate in (0.0, 1.0):
        upd.update(d_p, d_a, n, T.identity(), rate)
        sh.motion_update(T.identity(), rate)
    assert (d_a.download()["likelihood"]["n_meas"] == 0).all() and (sh.download()[1]["likelihood"]["n_meas"] == 0).all()
    sh.close()
    upd.close()


# ---- pose estimate ----------------------------------------------------------------------------------------------------------------
_sharded = {}
_refs = {}


def _filter(ra, meshes, world):
    if world not in _sharded:
        v, f = meshes("cube")
        _sharded[world] = ra.ShardedParticleFilterHip(v, f, devices=(0,) * world, loopback=world > 1)
    return _sharded[world]


def _ref(c, n_ind):
    key = (c["name"], min(n_ind, len(c["poses"])))
    if key not in _refs:
        _refs[key] = pc.estimate_ref(c["poses"], c["attrs"], n_ind)
    return _refs[key]


def _check_estimate(c, n_ind, est, what):
    name, n = c["name"], len(c["poses"])
    n_use = min(n, n_ind)
    ref = _ref(c, n_ind)
    assert est["nparticles"] == ref["nparticles"] == n_use, what
    for k in ("mean", "sigma", "min", "max"):
        assert abs(est["likelihood"][k] - ref["likelihood"][k]) <= 1e-9 + 1e-9 * abs(ref["likelihood"][k]), \
            "%s: likelihood %s %r, reference %r" % (what, k, est["likelihood"][k], ref["likelihood"][k])
    for k in ("trans_bb_min", "trans_bb_max"):
        assert np.array_equal(est[k], ref[k].astype(np.float32)), "%s: %s %s, reference %s" % (what, k, est[k], ref[k])
    q = np.array([est["pose"]["R"][k] for k in "xyzw"], np.float64)
    t = np.array([est["pose"]["t"][k] for k in "xyz"], np.float64)
    assert min(np.linalg.norm(q - ref["q"]), np.linalg.norm(q + ref["q"])) < 1e-6, "%s: mean quaternion %s, reference %s" % (what, q, ref["q"])
    assert q[3] >= 0 and abs(np.linalg.norm(q) - 1.0) <= 1e-6, "%s: mean quaternion %s: w < 0 or not of unit length" % (what, q)
    assert np.allclose(t, ref["t"], rtol=1e-6, atol=1e-6), "%s: mean translation %s, reference %s" % (what, t, ref["t"])
    # the covariance pass is judged around the mean the device returned (a float32 record), in float64
    cov = pc.estimate_ref(c["poses"], c["attrs"], n_ind, mean_pose=est["pose"])["covariance"]
    if name in pc.CONCENTRATED or n_use == 1:
        # derived, not tuned: the device forms d = (translation, angles) of ~Tbm * T_i in float32; a float32 component of magnitude m
        # carries at most 2^-23 m, so a component of d is off by at most eps = 2^-23 (|t|max + pi) and an entry sum w d_a d_b by at
        # most 2 sigma_max eps + eps^2, sigma_max the largest standard deviation of the reference covariance
        P = c["poses"][:n_use]
        t_max = float(np.sqrt(P["t"]["x"].astype(np.float64) ** 2 + P["t"]["y"].astype(np.float64) ** 2 + P["t"]["z"].astype(np.float64) ** 2).max())
        eps = 2.0 ** -23 * (t_max + np.pi)
        atol = 2.0 * np.sqrt(np.diag(cov).max()) * eps + eps * eps
    else:
        atol = 1e-6 * np.abs(cov).max()
    err = np.abs(est["covariance"] - cov)
    bad = err > atol + 1e-4 * np.abs(cov)
    ij = np.unravel_index(np.argmax(err - (atol + 1e-4 * np.abs(cov))), cov.shape)
    assert not bad.any(), "%s: covariance entry %s is %r, reference around the returned mean %r (absolute floor %.3g); %d entries off" % (
        what, ij, est["covariance"][ij], cov[ij], atol, bad.sum())
    assert np.array_equal(est["covariance"], est["covariance"].T), what


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name", pc.ESTIMATE_CASES)
def test_pose_estimate_matches_float64(ra, meshes, name, world):
    c = pc.estimate_case(name)
    sh = _filter(ra, meshes, world)
    sh.set_particles(c["poses"], c["attrs"])
    for n_ind in c["n_inductions"]:
        _check_estimate(c, n_ind, sh.pose_estimate(n_ind), "%s, %d rank(s), n_induction %d of %d" % (name, world, n_ind, len(c["poses"])))


@pytest.mark.parametrize("world", [1, 3])
def test_pose_estimate_does_not_see_the_sign_of_a_quaternion(ra, meshes, world):
    """q and -q are one rotation: q q^T is even in q, ~Tbm * T_i turns the sign of the whole product and the ZYX extraction reads
    products of two components -- the estimate of the flipped cloud is the estimate of the cloud, bit for bit"""
    a, b = pc.estimate_case("converged_pi"), pc.estimate_case("converged_pi_flipped")
    sh = _filter(ra, meshes, world)
    for n_ind in a["n_inductions"]:
        sh.set_particles(a["poses"], a["attrs"])
        ea = sh.pose_estimate(n_ind)
        sh.set_particles(b["poses"], b["attrs"])
        eb = sh.pose_estimate(n_ind)
        what = "%d rank(s), n_induction %d" % (world, n_ind)
        assert ea["pose"].tobytes() == eb["pose"].tobytes(), "%s: mean pose %s, of the flipped cloud %s" % (what, ea["pose"], eb["pose"])
        assert np.array_equal(ea["covariance"], eb["covariance"]), "%s: covariance differs by %.3g" % (
            what, np.abs(ea["covariance"] - eb["covariance"]).max())
        assert ea["likelihood"] == eb["likelihood"]


@pytest.mark.parametrize("world", [1, 3])
def test_pose_estimate_refuses_a_cloud_without_weight(ra, meshes, world):
    """every particle killed by the collision test: likelihoods {0, 0, MAX}; L / 0 has no mean.  Refused as the residual resampler
    refuses it -- and the next estimate on a cloud with weight is right"""
    from rmcl_amd import _capi
    c = pc.estimate_case("single_weight")
    dead = c["attrs"].copy()
    dead["likelihood"]["mean"] = 0.0
    dead["likelihood"]["sigma"] = 0.0
    dead["likelihood"]["n_meas"] = pc.MAX_N_MEAS
    sh = _filter(ra, meshes, world)
    sh.set_particles(c["poses"], dead)
    for n_ind in (len(dead), 1, 1000):
        with pytest.raises(ra.RmclHipError, match="sum to zero") as e:
            sh.pose_estimate(n_ind)
        assert e.value.status == _capi.ERR_INVALID
    sh.set_particles(c["poses"], c["attrs"])
    with pytest.raises(ra.RmclHipError, match="sum to zero"):
        sh.pose_estimate(1000)                  # the one particle with weight is the 1001st
    _check_estimate(c, 1001, sh.pose_estimate(1001), "single_weight after a refusal, %d rank(s), n_induction 1001" % world)


# ---- residual resampler: the carry of the block-total scan ---------------------------------------------------------------------------
def test_residual_scan_carries_across_trips(ra, orc, ctx):
    """n = n_new = 300007 with nearly flat weights: ~599 000 draws, 586 block totals of 1024 draws, three trips of 256 in k_scan_totals.
    The bars of test_residual_matches_oracle: sources, likelihoods, n_meas and the number of draws bit-exact, poses within 1e-6; a
    shard from the far end of the slots (filled by draws past the 256th scan block) == the slice of the whole"""
    from rmcl_amd import types as T
    poses, attrs = pc.residual_case()
    n = pc.RESIDUAL_N
    pn_ref, an_ref, filled, draws = orc.residual_resample(poses, attrs, orc.gladiator_config(**pc.RESIDUAL_NOISE), seed=pc.RESIDUAL_SEED, step=0)
    assert filled == n and draws > 2 * pc.SCAN_TRIP
    rs = ra.ResidualResamplerHip(ctx, seed=pc.RESIDUAL_SEED)
    rs.config = T.gladiator_config(**pc.RESIDUAL_NOISE)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    assert rs.update(d_p, d_a, d_pn, d_an, n, n) == {"n_particles": n}
    assert rs.last_draws == draws, "residual: %d draws, the oracle's sequential loop %d" % (rs.last_draws, draws)
    pn, an = d_pn.download(), d_an.download()
    _assert_same("residual n = n_new = %d" % n, "attributes (source likelihoods, n_meas) of the slots", an, an_ref)
    bad = np.flatnonzero(pn["stamp"] != pn_ref["stamp"])
    assert bad.size == 0, "residual: the source of %d slots differs, first slots %s" % (bad.size, bad[:8].tolist())
    for grp, keys in (("t", "xyz"), ("R", "xyzw")):
        for k in keys:
            err = np.abs(pn[grp][k].astype(np.float64) - pn_ref[grp][k])
            assert err.max() <= 1e-6, "residual: slot %d %s.%s %r, the oracle %r" % (err.argmax(), grp, k, pn[grp][k][err.argmax()], pn_ref[grp][k][err.argmax()])
    same = (pn.view(np.uint8).reshape(n, 32) == pn_ref.view(np.uint8).reshape(n, 32)).all(1)
    assert same.mean() > 0.99
    first = n - 700
    rs.step = 0
    d_ps, d_as = ra.DeviceArray(ctx, T.TRANSFORM, 500), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, 500)
    rs.update(d_p, d_a, d_ps, d_as, n, n, first=first, count=500)
    _assert_same("residual shard [%d, %d)" % (first, first + 500), "attributes (shard, slice of the oracle's whole)", d_as.download(), an_ref[first:first + 500])
    _assert_same("residual shard [%d, %d)" % (first, first + 500), "poses (shard, slice of the device's whole)", d_ps.download(), pn[first:first + 500])
    rs.close()
