"""The two shipped resamplers and the statistics kernel they share at their edges: k_gladiator_resample, k_likelihood_stats_* and the
k_residual_* passes against the oracle on the cases of tests/resample_cases.py (tests/test_resample_cases_cpu.py shows on the CPU
that every case reaches what it claims).  attrs bit for bit (who won, likelihood bits with NaN payloads, n_meas with the pinned
conversion), stamps equal, perturbed poses within 1e-6 of the oracle; nothing behind `count` is written, inputs stay as they were,
shards cut off the wave boundary reassemble the whole call byte for byte; {sum, max} within the bound double accumulation gives;
configurations outside the documented range are refused by every resampler before anything is written."""
import math

import numpy as np
import pytest

import resample_cases as rc

pytestmark = pytest.mark.gpu

PAD = 5                                     # records behind `count`, pre-filled with 0xA5
ERR_INVALID = 1


def _guarded(ra, ctx, dtype, count):
    d = ra.DeviceArray(ctx, dtype, count + PAD)
    d.upload(np.frombuffer(b"\xA5" * d.nbytes, dtype=dtype))
    return d


def _take(d, count):
    """(the first `count` records, True when every byte behind them is still 0xA5)"""
    h = d.download()
    return h[:count], bool((h[count:].view(np.uint8) == 0xA5).all())


def _assert_poses(pn, ref, what):
    assert np.array_equal(pn["stamp"], ref["stamp"]), what
    for k in "xyz":
        assert np.allclose(pn["t"][k], ref["t"][k], rtol=0, atol=1e-6), "%s: t.%s" % (what, k)
    for k in "xyzw":
        assert np.allclose(pn["R"][k], ref["R"][k], rtol=0, atol=1e-6), "%s: R.%s" % (what, k)
    n = len(pn)
    return float((pn.view(np.uint8).reshape(n, 32) == ref.view(np.uint8).reshape(n, 32)).all(1).mean()) if n else 1.0


@pytest.mark.parametrize("name", rc.TOURNAMENT)
def test_tournament_matches_oracle(ra, orc, ctx, name):
    from rmcl_amd import types as T
    c = rc.tournament_case(name)
    poses, attrs = c["poses"], c["attrs"]
    n = len(poses)
    rs = ra.GladiatorResamplerHip(ctx, seed=rc.SEED)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    by_enemy = {}
    for kw in c["configs"]:
        for step in rc.STEPS:
            d_pn, d_an = _guarded(ra, ctx, T.TRANSFORM, n), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, n)
            rs.config, rs.step = T.gladiator_config(**kw), step
            assert rs.update(d_p, d_a, d_pn, d_an, n) == {"n_particles": n}
            (pn, ok_p), (an, ok_a) = _take(d_pn, n), _take(d_an, n)
            assert ok_p and ok_a, "%s: the tournament wrote behind its %d champions" % (name, n)
            pn_ref, an_ref = rc.tournament_reference(c, kw, step)
            what = "%s %s step %d" % (name, kw, step)
            bad = np.flatnonzero((an.view(np.uint32).reshape(n, 9) != an_ref.view(np.uint32).reshape(n, 9)).any(1))
            assert bad.size == 0, "%s: %d records differ, first champion %d: device %s, oracle %s" % (what, bad.size, bad[0], an[bad[0]], an_ref[bad[0]])
            share = _assert_poses(pn, pn_ref, what)
            print("[resample-edges] tournament %s: %.4f of the poses bit-identical" % (what, share))
            rep = rc.replaced_mask(c, an)
            assert pn[~rep].tobytes() == poses[~rep].tobytes() and an[~rep].tobytes() == attrs[~rep].tobytes(), "%s: a champion that stays is a byte copy" % what
            if name == "ties":
                assert not rep.any()
            if name == "gimbal" and kw == rc.ZERO_NOISE:
                # without noise a winner's pose is a function of the enemy's pose alone: whatever the champion, the step, the draw
                e = rc.enemies(n, step)
                for k in np.flatnonzero(rep):
                    rec = pn[k].tobytes()
                    assert by_enemy.setdefault(int(e[k]), rec) == rec, "%s: enemy %d gives two different poses" % (what, e[k])
                    assert pn[k]["t"] == poses[e[k]]["t"]
    if name == "gimbal":
        assert len(by_enemy) > 1000
    assert d_p.download().tobytes() == poses.tobytes() and d_a.download().tobytes() == attrs.tobytes(), "the inputs changed"
    rs.close()


@pytest.mark.parametrize("name", ["gimbal", "nan_inf", "n_meas_edges", "n65", "n1023"])
def test_tournament_shards_reassemble_the_whole(ra, ctx, name):
    """device against device, poses included"""
    from rmcl_amd import types as T
    c = rc.tournament_case(name)
    n = len(c["poses"])
    rs = ra.GladiatorResamplerHip(ctx, seed=rc.SEED)
    rs.config = T.gladiator_config(**c["configs"][-1])
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
    d_pn, d_an = _guarded(ra, ctx, T.TRANSFORM, n), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, n)
    rs.step = rc.STEPS[1]
    rs.update(d_p, d_a, d_pn, d_an, n)
    whole_p, whole_a = _take(d_pn, n)[0], _take(d_an, n)[0]
    parts_p, parts_a = [], []
    for lo, hi in rc.shard_cuts(n):
        d_ps, d_as = _guarded(ra, ctx, T.TRANSFORM, hi - lo), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, hi - lo)
        rs.step = rc.STEPS[1]
        rs.update(d_p, d_a, d_ps, d_as, n, first=lo, count=hi - lo)
        (p, ok_p), (a, ok_a) = _take(d_ps, hi - lo), _take(d_as, hi - lo)
        assert ok_p and ok_a, "shard [%d, %d) wrote behind its count" % (lo, hi)
        parts_p.append(p)
        parts_a.append(a)
    assert np.concatenate(parts_a).tobytes() == whole_a.tobytes()
    assert np.concatenate(parts_p).tobytes() == whole_p.tobytes()
    rs.close()


@pytest.mark.parametrize("fill", rc.STATS_FILLS)
def test_statistics_on_every_size(ra, orc, ctx, meshes, fill):
    """max bit-equal to the oracle (0 for an all-negative vector, NaN ignored); sum NaN exactly when a NaN is in; otherwise
    |sum - fsum| <= 1/2 ulp32(fsum) + n 2^-53 sum|L|: what ANY order of double accumulation followed by one rounding to float32 gives
    (a float accumulator misses it: one_big).  The stride-9 and the stride-1 form give the same bits."""
    from rmcl_amd import types as T
    v_, f_ = meshes("cube")
    upd = ra.PCDSensorUpdaterHip(ra.import_hip_map(ctx, v_, f_))
    upd.init()
    rs = ra.GladiatorResamplerHip(ctx)
    for n in [m for m, f in rc.STATS_CASES if f == fill]:
        v = rc.stats_vector(n, fill)
        attrs = rc.stats_attrs(v)
        r = orc.likelihood_stats(attrs)
        if n == 0:
            s = rs.compute_stats(None, 0)
            w = rs.compute_stats_weights(None, 0)
            assert s == {"sum": 0.0, "max": 0.0} and w == s
            continue
        d_a = ra.DeviceArray.from_host(ctx, attrs)
        d_w = _guarded(ra, ctx, np.float32, n)
        upd.extract_weights(d_a, n, d_w)
        w_host, ok = _take(d_w, n)
        assert ok and w_host.tobytes() == v.tobytes(), "extract_weights: n %d" % n
        s, w = rs.compute_stats(d_a, n), rs.compute_stats_weights(d_w, n)
        for k in ("sum", "max"):
            assert np.float32(s[k]).tobytes() == np.float32(w[k]).tobytes(), "n %d %s: attributes give %r, the dense weights %r" % (n, k, s[k], w[k])
        assert np.float32(s["max"]).tobytes() == np.float32(r["max"]).tobytes(), "n %d %s: max %r, oracle %r" % (n, fill, s["max"], r["max"])
        if np.isnan(v).any():
            assert math.isnan(s["sum"]), "n %d %s: sum %r with a NaN in the vector" % (n, fill, s["sum"])
            continue
        exact, bound = rc.stats_sum_bound(v)
        print("[resample-edges] stats %-13s n %6d: sum %.9g, fsum %.17g, error %.3g, bound %.3g" % (fill, n, s["sum"], exact, abs(s["sum"] - exact) if math.isfinite(exact) else 0.0, bound))
        assert not math.isnan(s["sum"])
        if math.isinf(exact):
            assert s["sum"] == exact
        else:
            assert abs(s["sum"] - exact) <= bound, "n %d %s: sum %r, fsum %r, bound %g" % (n, fill, s["sum"], exact, bound)
        if fill == "negative":
            assert s["max"] == 0.0 and math.copysign(1.0, s["max"]) == 1.0
    rs.close()
    upd.close()


def _residual_run(ra, ctx, c, kw, step, d_p, d_a, rs, first=0, count=None):
    from rmcl_amd import types as T
    n, n_new = len(c["poses"]), c["n_new"]
    count = n_new - first if count is None else count
    d_pn, d_an = _guarded(ra, ctx, T.TRANSFORM, count), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, count)
    rs.config, rs.step = T.gladiator_config(**kw), step
    assert rs.update(d_p, d_a, d_pn, d_an, n, n_new, first=first, count=count) == {"n_particles": count}
    (pn, ok_p), (an, ok_a) = _take(d_pn, count), _take(d_an, count)
    assert ok_p and ok_a, "residual %s: wrote behind its %d slots" % (c["name"], count)
    return pn, an


@pytest.mark.parametrize("name", rc.RESIDUAL)
def test_residual_matches_oracle(ra, orc, ctx, name):
    c = rc.residual_case(name)
    poses, attrs, n_new = c["poses"], c["attrs"], c["n_new"]
    rs = ra.ResidualResamplerHip(ctx, seed=rc.RESIDUAL_SEED)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    for kw, step in c["runs"]:
        pn, an = _residual_run(ra, ctx, c, kw, step, d_p, d_a, rs)
        pn_ref, an_ref, filled, draws = rc.residual_reference(c, kw, step)
        what = "residual %s %s step %d" % (name, kw, step)
        assert filled == n_new and rs.last_draws == draws, "%s: %d draws, oracle %d" % (what, rs.last_draws, draws)
        bad = np.flatnonzero((an.view(np.uint32).reshape(n_new, 9) != an_ref.view(np.uint32).reshape(n_new, 9)).any(1))
        assert bad.size == 0, "%s: %d slots differ, first %d: device %s, oracle %s" % (what, bad.size, bad[0], an[bad[0]], an_ref[bad[0]])
        share = _assert_poses(pn, pn_ref, what)
        print("[resample-edges] %s: %d draws, %.4f of the poses bit-identical" % (what, draws, share))
        if name == "retry_twice":
            assert rs.last_draws == 17793
        # the last slots as a shard of their own (it reports the draws too), and a shard off the wave boundary from the middle
        for lo, hi in {(max(0, n_new - 67), n_new), (min(1, n_new - 1), min(n_new, 258))}:
            ps, as_ = _residual_run(ra, ctx, c, kw, step, d_p, d_a, rs, first=lo, count=hi - lo)
            assert as_.tobytes() == an[lo:hi].tobytes() and ps.tobytes() == pn[lo:hi].tobytes(), "%s: shard [%d, %d)" % (what, lo, hi)
            if hi == n_new:
                assert rs.last_draws == draws
    assert d_p.download().tobytes() == poses.tobytes() and d_a.download().tobytes() == attrs.tobytes(), "the inputs changed"
    rs.close()


@pytest.mark.parametrize("name", ["gimbal", "n_meas_edges", "single_5"])
def test_residual_shards_reassemble_the_whole(ra, ctx, name):
    """device against device, poses included: every shard repeats the draws and fills its own slots"""
    c = rc.residual_case(name)
    kw, step = c["runs"][-1]
    rs = ra.ResidualResamplerHip(ctx, seed=rc.RESIDUAL_SEED)
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
    whole_p, whole_a = _residual_run(ra, ctx, c, kw, step, d_p, d_a, rs)
    parts = [_residual_run(ra, ctx, c, kw, step, d_p, d_a, rs, first=lo, count=hi - lo) for lo, hi in rc.shard_cuts(c["n_new"])]
    assert np.concatenate([a for _, a in parts]).tobytes() == whole_a.tobytes()
    assert np.concatenate([p for p, _ in parts]).tobytes() == whole_p.tobytes()
    rs.close()


def test_residual_negatives_and_nan(ra, orc, ctx):
    """rmclhip.h: a sum that is zero, negative or NaN is refused (one NaN is enough); a negative likelihood under a positive sum is
    never inserted -- the oracle's `share > 0`"""
    from rmcl_amd import types as T
    for label, L, n_new, refused in rc.residual_refused_clouds():
        poses, attrs = rc.cloud(len(L), 69)
        attrs["likelihood"]["mean"] = L
        c = {"name": label, "poses": poses, "attrs": attrs, "n_new": n_new}
        rs = ra.ResidualResamplerHip(ctx, seed=rc.RESIDUAL_SEED)
        d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        if refused is None:
            pn, an = _residual_run(ra, ctx, c, rc.NOISY, 0, d_p, d_a, rs)
            pn_ref, an_ref, filled, draws = rc.residual_reference(c, rc.NOISY, 0)
            assert filled == n_new and rs.last_draws == draws and an.tobytes() == an_ref.tobytes()
            _assert_poses(pn, pn_ref, label)
            assert (an["likelihood"]["mean"] > 0).all()
        else:
            d_pn, d_an = _guarded(ra, ctx, T.TRANSFORM, n_new), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, n_new)
            with pytest.raises(ra.RmclHipError, match=refused) as ei:
                rs.update(d_p, d_a, d_pn, d_an, len(L), n_new)
            assert ei.value.status == ERR_INVALID
            assert _take(d_pn, 0)[1] and _take(d_an, 0)[1], "%s: a refused call wrote" % label
        rs.close()


def _entry_points(ra, ctx, rss, d_p, d_a, n, cfg):
    """the four single-device resamplers at step 0, each on fresh guarded outputs; yields (label, call, outputs)"""
    from rmcl_amd import types as T
    g, r, a = rss
    calls = (("gladiator", lambda o: g.update(d_p, d_a, o[0], o[1], n)),
             ("gladiator count 0", lambda o: g.update(d_p, d_a, o[0], o[1], n, first=0, count=0)),
             ("residual", lambda o: r.update(d_p, d_a, o[0], o[1], n, n)),
             ("systematic", lambda o: a.update_systematic(d_p, d_a, o[0], o[1], n, n)),
             ("adaptive", lambda o: a.update(d_p, d_a, o[0], o[1], n, n)))
    for label, fn in calls:
        for rs in rss:
            rs.config, rs.step = cfg, 0
        o = (_guarded(ra, ctx, T.TRANSFORM, n), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, n))
        yield label, (lambda fn=fn, o=o: fn(o)), o


def test_bad_configs_are_refused_by_every_resampler(ra, orc, ctx, meshes):
    from rmcl_amd import types as T
    n = 700
    poses, attrs = rc.cloud(n, 90)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    v, f = meshes("cube")
    sh = ra.ShardedParticleFilterHip(v, f, devices=(0, 0), loopback=True)
    sh.set_particles(poses, attrs)
    rss = (ra.GladiatorResamplerHip(ctx, seed=rc.SEED), ra.ResidualResamplerHip(ctx, seed=rc.SEED), ra.AdaptiveResamplerHip(ctx, seed=rc.SEED))
    for kw in rc.BAD_CONFIGS:
        cfg = T.gladiator_config(**kw)
        for label, call, (o_p, o_a) in _entry_points(ra, ctx, rss, d_p, d_a, n, cfg):
            with pytest.raises(ra.RmclHipError) as ei:
                call()
            assert ei.value.status == ERR_INVALID, "%s with %s: status %d" % (label, kw, ei.value.status)
            assert _take(o_p, 0)[1] and _take(o_a, 0)[1], "%s with %s: a refused call wrote its outputs" % (label, kw)
        for residual in (False, True):
            with pytest.raises(ra.RmclHipError) as ei:
                sh.resample(cfg=cfg, seed=rc.SEED, step=0, residual=residual)
            assert ei.value.status == ERR_INVALID, "sharded (residual %s) with %s" % (residual, kw)
    p_sh, a_sh = sh.download()
    assert p_sh.tobytes() == poses.tobytes() and a_sh.tobytes() == attrs.tobytes(), "a refused sharded resampling changed the cloud"
    assert d_p.download().tobytes() == poses.tobytes() and d_a.download().tobytes() == attrs.tobytes()
    # a valid call afterwards is right, the ends 0 and 1 included
    for kw in [dict(rc.NOISY)] + [dict(rc.NOISY, **e) for e in rc.GOOD_END_CONFIGS]:
        cfg = T.gladiator_config(**kw)
        c = {"name": "valid", "poses": poses, "attrs": attrs, "n_new": n}
        for label, call, (o_p, o_a) in _entry_points(ra, ctx, rss, d_p, d_a, n, cfg):
            res = call()
            if label == "gladiator":
                pn_ref, an_ref = orc.gladiator_resample(poses, attrs, orc.gladiator_config(**kw), rc.SEED, 0)
            elif label == "residual":
                pn_ref, an_ref, _, _ = orc.residual_resample(poses, attrs, orc.gladiator_config(**kw), rc.SEED, 0, n_new=n)
            else:
                assert label == "gladiator count 0" or res["n_particles"] >= 1
                continue
            (pn, ok_p), (an, ok_a) = _take(o_p, n), _take(o_a, n)
            assert ok_p and ok_a and an.tobytes() == an_ref.tobytes(), "%s with %s" % (label, kw)
            _assert_poses(pn, pn_ref, label)
    sh.resample(cfg=T.gladiator_config(**rc.NOISY), seed=rc.SEED, step=0)
    pn_ref, an_ref = orc.gladiator_resample(poses, attrs, orc.gladiator_config(**rc.NOISY), rc.SEED, 0)
    p_sh, a_sh = sh.download()
    assert a_sh.tobytes() == an_ref.tobytes()
    _assert_poses(p_sh, pn_ref, "sharded after the refusals")
    sh.close()
    for rs in rss:
        rs.close()


def test_systematic_fill_uses_the_pinned_conversion(ra, ctx):
    """the third site of the conversion (resample.hip: k_sys_fill) on the n_meas edges, against tests/adaptive_ref.py"""
    import adaptive_ref as ar
    from rmcl_amd import types as T
    c = rc.tournament_case("n_meas_edges")
    poses, attrs = c["poses"], c["attrs"]
    n, n_new = len(poses), 3 * len(poses) + 1
    rs = ra.AdaptiveResamplerHip(ctx, seed=rc.SEED)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    for fm, fr in ((0.0, 0.0), (1.0, 0.0), (0.3, 0.2)):
        kw = dict(ar.gladiator_cfg(), likelihood_forget_per_meter=fm, likelihood_forget_per_radian=fr)
        d_pn, d_an = _guarded(ra, ctx, T.TRANSFORM, n_new), _guarded(ra, ctx, T.PARTICLE_ATTRIBUTES, n_new)
        rs.config, rs.step = T.gladiator_config(**kw), 0
        rs.update_systematic(d_p, d_a, d_pn, d_an, n, n_new)
        (pn, ok_p), (an, ok_a) = _take(d_pn, n_new), _take(d_an, n_new)
        pn_ref, an_ref, src = ar.systematic(poses, attrs, n_new, kw, rc.SEED, 0)
        assert ok_p and ok_a
        assert np.array_equal(an["likelihood"]["n_meas"], an_ref["likelihood"]["n_meas"]), "forget (%g, %g)" % (fm, fr)
        if (fm, fr) == (0.0, 0.0):
            assert (an["likelihood"]["n_meas"] == 0xFFFFFFFF).sum() > 1000
    rs.close()
