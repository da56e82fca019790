"""The cases of tests/resample_cases.py are what they claim to be -- checked on the CPU oracle alone, so that the GPU test
(tests/test_gpu_resample_edges.py) cannot pass vacuously: the gimbal cloud has particles (and winners) on both sides of |sinp| >= 1, the
two-level cloud's winners are the closed form, zeros of either sign never beat each other, denormals and infinities are ordered as IEEE
orders them and NaN records survive bit for bit, every n_meas edge is forgotten from under every pair of rates, the retry case needs the
draw block doubled twice, the exact shares fill in exactly n_new / share draws, the one_big vector sums differently in float and in
double; the oracle's pinned conversion equals its three-line restatement and its statistics equal math.fsum."""
import math

import numpy as np
import pytest

import resample_cases as rc

f32 = np.float32


def _runs(case):
    for kw in case["configs"]:
        for step in rc.STEPS:
            yield kw, step


@pytest.mark.parametrize("name", rc.TOURNAMENT)
def test_tournament_case_reaches_what_it_claims(orc, name):
    c = rc.tournament_case(name)
    poses, attrs = c["poses"], c["attrs"]
    n = len(poses)
    L = attrs["likelihood"]["mean"]
    Lb = L.view(np.uint32)
    assert np.abs(np.stack([poses["t"][k] for k in "xyz"])).max() <= 9.0
    for kw, step in _runs(c):
        pn, an = rc.tournament_reference(c, kw, step)
        e = rc.enemies(n, step)
        rep = rc.replaced_mask(c, an)
        with np.errstate(invalid="ignore"):
            ieee = L[e] > L
        assert np.array_equal(rep, ieee & (e != np.arange(n))), "%s: the oracle's winners are not IEEE's" % name
        # wherever the champion stays, its record is a byte copy
        assert an[~rep].tobytes() == attrs[~rep].tobytes() and pn[~rep].tobytes() == poses[~rep].tobytes()
        # a winner keeps the enemy's likelihood bits and everything but n_meas and the pose
        assert np.array_equal(an["likelihood"]["mean"].view(np.uint32)[rep], Lb[e][rep])
        assert np.array_equal(pn["stamp"][rep], poses["stamp"][e][rep])
        print("[resample] %-12s step %10d %s: %d of %d champions replaced" % (name, step, kw, rep.sum(), n))
        if name == "ties":
            assert not rep.any()
        elif name == "two_level":
            assert np.array_equal(rep, (L == f32(0.25)) & (L[e] == f32(0.75)))
            assert rep.sum() > n // 8 and (~rep).sum() > n // 2
        elif name == "signed_zero":
            zc, ze = (Lb << 1) == 0, (Lb[e] << 1) == 0
            assert not rep[zc & ze].any()
            for sc, se in ((0, 0x80000000), (0x80000000, 0)):                         # +0 against -0 and -0 against +0 both occur
                assert ((Lb == sc) & (Lb[e] == se)).sum() > n // 10
            assert rep[zc & ~ze].all() and rep[zc].sum() > 20                          # the 1e-3 enemies do win
        elif name == "denormal":
            sub = lambda v: (v > 0) & (v < f32(2.0 ** -126))
            assert sub(L).sum() > n // 2 and (L == 0).sum() > n // 10
            assert (rep & (L == 0) & sub(L[e])).sum() > 50, "a denormal beating 0"
            assert (rep & sub(L) & sub(L[e])).sum() > 50, "a denormal beating a smaller one"
            assert (~rep & sub(L) & (L[e] == 0)).sum() > 50
        elif name == "nan_inf":
            nan_c, nan_e = np.isnan(L), np.isnan(L[e])
            assert not rep[nan_c | nan_e].any() and (nan_c & ~nan_e).sum() > 50 and (~nan_c & nan_e).sum() > 50
            for bits in rc.NAN_PAYLOADS:                                               # every payload is kept, bit for bit
                at = Lb == bits
                assert at.sum() > 50 and (an["likelihood"]["mean"].view(np.uint32)[at] == bits).all()
            assert (rep & np.isposinf(L[e])).sum() > 50 and (rep & np.isneginf(L)).sum() > 50
            assert (~rep & np.isposinf(L) & np.isposinf(L[e])).sum() > 5 and (~rep & np.isneginf(L[e])).sum() > 50
            assert (rep & np.isfinite(L) & np.isfinite(L[e])).sum() > 50
        elif name == "gimbal":
            sp = rc.sinp_of(poses)
            assert 1200 < (np.abs(sp) >= 1).sum() < n - 400, "both sides of the branch"
            for sign in (1.0, -1.0):
                for side in (np.abs(sp) >= 1, np.abs(sp) < 1):
                    assert (rep & (side & (np.sign(sp) == sign))[e]).sum() > 30, "winners from both sides, both signs"
            assert (poses["R"]["w"] < 0).sum() > n // 4 and (poses["R"]["w"] > 0).sum() > n // 4
            if kw == rc.ZERO_NOISE:
                for k in "xyz":
                    assert np.array_equal(pn["t"][k][rep], poses["t"][k][e][rep])
        elif name == "unnormalised":
            nrm = np.sqrt(sum(poses["R"][k].astype(np.float64) ** 2 for k in "xyzw"))
            assert (np.abs(nrm - 0.5) < 1e-6).sum() > n // 3 and (np.abs(nrm - 2.0) < 1e-6).sum() > n // 3
            assert (rep & (np.abs(nrm - 0.5) < 1e-6)[e]).sum() > 50 and (rep & (np.abs(nrm - 2.0) < 1e-6)[e]).sum() > 50
            qn = np.sqrt(sum(pn["R"][k].astype(np.float64) ** 2 for k in "xyzw"))
            assert np.allclose(qn[rep], 1.0, atol=1e-6)                                # a winner leaves as a unit quaternion
        elif name == "n_meas_edges":
            src = attrs["likelihood"]["n_meas"][e]
            out = an["likelihood"]["n_meas"]
            for v in rc.N_MEAS_EDGES:
                assert (rep & (src == v)).sum() >= 20, "n_meas %d: too few winners carry it" % v
            fm, fr = kw["likelihood_forget_per_meter"], kw["likelihood_forget_per_radian"]
            if (fm, fr) in ((0.0, 0.0), (1e-12, 0.0)) or kw.get("min_noise_tx") == 0.0:   # remember_rate rounds to 1
                want = np.array([rc.n_meas_scaled(int(v), 1.0) for v in src], dtype=np.uint32)
                assert np.array_equal(out[rep], want[rep])
                assert (out[rep & (src >= 2 ** 32 - 128)] == 0xFFFFFFFF).all() and (out[rep & (src == 2 ** 32 - 129)] == 2 ** 32 - 256).all()
            elif 1.0 in (fm, fr):                                                      # 1 - pow(0, d > 0) = 1: everything forgotten
                assert (out[rep] == 0).all()
            else:
                assert (out[rep & (src > 3)] < src[rep & (src > 3)]).all() and (out[rep & (src >= 9999)] > 0).all()
        else:
            if n >= 63:
                assert rep.any() and (~rep).any()
            if n == 1:
                assert not rep.any()
            if n > 300000:
                assert (rep & (np.arange(n) >= 262144)).sum() > 1000 and (rep & (e >= 262144)).sum() > 1000


def test_shards_partition_the_cloud_off_the_wave_boundary():
    for n in (rc.N, 300007):
        cuts = rc.shard_cuts(n)
        assert cuts[0][0] == 0 and cuts[-1][1] == n and all(a[1] == b[0] for a, b in zip(cuts[:-1], cuts[1:]))
        assert {1, 63, 65, 257, n - 1} <= {c[0] for c in cuts} and any(c[1] - c[0] == 1 for c in cuts)


def test_oracle_conversion_is_the_pinned_rule(orc):
    """saturate, NaN -> 0 -- on the n_meas_edges set and every rate a resampler can produce, plus the ones a refused config would"""
    rates = [0.0, 1.0, 0.5, 0.7, 0.8, 1e-12, float(f32(1.0) - f32(2.0 ** -24)), float(np.nextafter(f32(1.0), f32(2.0))), 2.0, -0.0, -1.0, -1e-30,
             1e-45, math.inf, -math.inf, math.nan]
    for nm in rc.N_MEAS_EDGES:
        for r in rates:
            assert orc.n_meas_scaled(nm, r) == rc.n_meas_scaled(nm, r), (nm, r)
    assert rc.n_meas_scaled(2 ** 32 - 128, 1.0) == 0xFFFFFFFF and rc.n_meas_scaled(2 ** 32 - 129, 1.0) == 2 ** 32 - 256
    assert rc.n_meas_scaled(10000, math.nan) == 0 and rc.n_meas_scaled(0, math.inf) == 0 and rc.n_meas_scaled(1, math.inf) == 0xFFFFFFFF
    assert float(f32(2 ** 32 - 128)) == 2.0 ** 32 and float(f32(2 ** 32 - 129)) == 2.0 ** 32 - 256


def test_adaptive_ref_conversion_is_the_pinned_rule():
    import adaptive_ref as ar
    nm = np.array(rc.N_MEAS_EDGES * 4, dtype=np.uint32)
    rate = np.repeat(np.array([1.0, 0.5, 0.0, np.nan], dtype=f32), len(rc.N_MEAS_EDGES))
    want = [rc.n_meas_scaled(int(a), float(b)) for a, b in zip(nm, rate)]
    assert ar.n_meas_scaled(nm, rate).tolist() == want


@pytest.mark.parametrize("fill", rc.STATS_FILLS)
def test_stats_vectors_and_the_oracle_against_fsum(orc, fill):
    sizes = [n for n, f in rc.STATS_CASES if f == fill]
    assert sizes, fill
    for n in sizes:
        v = rc.stats_vector(n, fill)
        assert v.dtype == f32 and len(v) == n and rc.stats_vector(n, fill).tobytes() == v.tobytes()
        r = orc.likelihood_stats(rc.stats_attrs(v))
        has_nan = bool(np.isnan(v).any())
        assert has_nan == fill.startswith("nan_")
        want_max = f32(max([0.0] + [float(x) for x in v[~np.isnan(v)]]))
        assert f32(r["max"]).tobytes() == want_max.tobytes(), (n, fill)
        if has_nan:
            assert math.isnan(r["sum"])
        else:
            s, bound = rc.stats_sum_bound(v)
            assert r["sum"] == s if math.isinf(s) else abs(r["sum"] - s) <= bound, (n, fill, r["sum"], s, bound)
        if fill == "negative":
            assert (v < 0).all() and r["max"] == 0.0 and r["sum"] < 0
        elif fill == "denormal":
            assert ((v > 0) & (v < f32(2.0 ** -126))).all() and 0 < r["max"] < 2.0 ** -126
        elif fill == "zero":
            assert r == {"sum": 0.0, "max": 0.0}
        elif fill.startswith("max_"):
            at = int(np.argmax(v))
            stride = rc.stats_stride(n)
            assert v[at] == f32(1.5) and at == {"max_last": n - 1, "max_255": 255, "max_256": 256, "max_last_trip": ((n - 1) // stride) * stride}[fill]
            if fill == "max_last_trip":
                assert n > stride and at + stride >= n > at
        elif fill == "one_big":
            s = math.fsum(float(x) for x in v)
            in_float = float(np.add.accumulate(v, dtype=f32)[-1])                      # a float accumulator, in order
            assert s == 16842751.0 and in_float == 16777216.0
            assert abs(in_float - s) > rc.stats_sum_bound(v)[1] and r["sum"] in (16842750.0, 16842752.0)
    if fill == "uniform":
        assert sizes == list(rc.STATS_SIZES) + [rc.ONE_BIG_N]
        assert orc.likelihood_stats(rc.stats_attrs(rc.stats_vector(0, fill))) == {"sum": 0.0, "max": 0.0}
    if fill == "max_last_trip":
        assert sizes == [n for n in rc.STATS_SIZES + (rc.ONE_BIG_N,) if n > rc.stats_stride(n)] and {257, 1025, 262145, 300007} <= set(sizes)


def test_retry_twice_needs_the_block_doubled_twice(orc):
    c = rc.residual_case("retry_twice")
    L, n, n_new = c["attrs"]["likelihood"]["mean"], rc.RETRY_N, rc.RETRY_N_NEW
    (kw, step), = c["runs"]
    pn, an, filled, draws = rc.residual_reference(c, kw, step)
    expect = rc.residual_expect(L, n_new)
    block = rc.first_block(n, n_new, expect)
    print("[resample] retry_twice: heavy particle %d, second appearance at draw %d, %d draws, expect %d, first block %d" % (c["heavy"], c["second"], draws, expect, block))
    assert filled == n_new and draws == c["second"] + 1
    assert draws > 4.0 * n_new / (expect / n), "the condition: more draws than four times n_new / (expect / n)"
    assert 2 * block < draws <= 4 * block, "the block of %d draws doubles exactly twice" % block
    assert (c["heavy"], draws, expect, block) == (1699, 17793, 999, 6598)
    # the clamp: the first draw of the heavy particle inserts 999 copies, the second the one that is left
    assert (an["state_sigma"] == c["attrs"]["state_sigma"][c["heavy"]]).all() and (an["likelihood"]["mean"] == 1.0).all()


@pytest.mark.parametrize("name", [r for r in rc.RESIDUAL if r != "retry_twice"])
def test_residual_case_reaches_what_it_claims(orc, name):
    c = rc.residual_case(name)
    poses, attrs, n_new = c["poses"], c["attrs"], c["n_new"]
    n = len(poses)
    for kw, step in c["runs"]:
        pn, an, filled, draws = rc.residual_reference(c, kw, step)
        assert filled == n_new
        stream = (orc.philox_word0(0, max(draws, 1), step, 2, rc.RESIDUAL_SEED).astype(np.uint64) % np.uint64(n)).astype(np.int64)
        print("[resample] residual %-14s step %10d: n %d -> %d in %d draws" % (name, step, n, n_new, draws))
        if name.startswith("single"):
            assert draws == 1 and (an["state_sigma"] == attrs["state_sigma"][0]).all()
        elif name.startswith("exact_shares"):
            share = float(attrs["likelihood"]["mean"][0]) / math.fsum(float(x) for x in attrs["likelihood"]["mean"]) * n_new
            assert share == float(n_new // 1024) and draws == n_new / share, "every draw inserts exactly `share` copies"
            src = np.repeat(stream[:draws], int(share))
            assert np.array_equal(an["state_sigma"], attrs["state_sigma"][src])
        elif name == "one_slot":
            assert n_new == 1 and stream[draws - 1] == 17 and (stream[:draws - 1] != 17).all() and draws > 1
            assert (an["state_sigma"] == attrs["state_sigma"][17]).all()
        elif name == "n_meas_edges":
            out = an["likelihood"]["n_meas"]
            by_sigma = {attrs["state_sigma"][i].tobytes(): i for i in range(n)}
            src = attrs["likelihood"]["n_meas"][[by_sigma[r.tobytes()] for r in an["state_sigma"]]]
            for v in rc.N_MEAS_EDGES:
                assert (src == v).sum() >= 50
            fm, fr = kw["likelihood_forget_per_meter"], kw["likelihood_forget_per_radian"]
            if (fm, fr) == (1.0, 1.0) or kw.get("min_noise_tx") == 0.0:                    # a factor of exactly 1
                assert out.tolist() == [rc.n_meas_scaled(int(v), 1.0) for v in src] and (out == 0xFFFFFFFF).sum() >= 100
            elif fm == 0.0:
                assert (out == 0).all()
            else:
                assert (out[src > 3] < src[src > 3]).all() and (out[src >= 9999] > 0).all()
        elif name == "gimbal":
            sp = rc.sinp_of(poses)
            by_sigma = {attrs["state_sigma"][i].tobytes(): i for i in range(n)}
            s = sp[[by_sigma[r.tobytes()] for r in an["state_sigma"]]]
            assert (np.abs(s) >= 1).sum() > 1000 and (np.abs(s) < 1).sum() > 500 and (s > 0).sum() > 1000 and (s < 0).sum() > 1000


def test_residual_negatives_are_never_inserted_and_the_rest_has_no_reference(orc):
    for label, L, n_new, refused in rc.residual_refused_clouds():
        poses, attrs = rc.cloud(len(L), 69)
        attrs["likelihood"]["mean"] = L
        s = math.fsum(float(x) for x in L)
        if refused is None:
            pn, an, filled, draws = orc.residual_resample(poses, attrs, orc.gladiator_config(**rc.NOISY), rc.RESIDUAL_SEED, 0, n_new=n_new)
            assert s > 0 and (L < 0).sum() > 300 and filled == n_new and (an["likelihood"]["mean"] > 0).all()
        else:
            assert not s > 0.0, label                       # the library refuses a sum that is not positive
            pn, an, filled, draws = orc.residual_resample(poses, attrs, orc.gladiator_config(**rc.NOISY), rc.RESIDUAL_SEED, 0, n_new=n_new, max_draws=5000)
            if math.isnan(s):
                assert filled == 0 and draws == 5000        # every share is NaN: the reference's loop never inserts and would not end
            else:
                assert s < 0 and filled == n_new            # negative over negative: the reference resamples by |L|; the library refuses (rmclhip.h)


def test_config_cases_are_outside_the_rule_and_the_ends_inside():
    def ok(kw):
        c = dict(likelihood_forget_per_meter=0.3, likelihood_forget_per_radian=0.2, **{f: 0.01 for f in rc.NOISE_FIELDS})
        c.update(kw)
        rates = all(0.0 <= float(f32(c[f])) <= 1.0 for f in ("likelihood_forget_per_meter", "likelihood_forget_per_radian"))
        return rates and all(math.isfinite(float(f32(c[f]))) for f in rc.NOISE_FIELDS)
    assert len(rc.BAD_CONFIGS) == 2 * 7 + 6 * 2 and not any(ok(kw) for kw in rc.BAD_CONFIGS)
    assert len(rc.GOOD_END_CONFIGS) == 4 and all(ok(kw) for kw in rc.GOOD_END_CONFIGS)
    assert float(f32(-1e-9)) < 0.0 and float(f32(1.0 + 1e-6)) > 1.0               # the near misses survive the rounding to float32
