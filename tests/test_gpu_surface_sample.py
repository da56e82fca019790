"""The surface sampler on the device (rmcl_amd/csrc/surface_sample.hip, surface_sample.hip.h, particles.hip, the scan of resample.hip)
against the numpy restatement (tests/surface_sample_ref.py) on the maps and shapes of tests/surface_sample_cases.py: the sampler's info,
the initialisation on the surface, slices and shards, the recovery injection alone, behind every resampler and sharded, the adaptive
resampler's recovery= path, and the refusals.

Everything is compared byte for byte: face choice, weights and the mask are integers; the point and the translation are IEEE double and
float arithmetic; the yaw's half-angle cosine and sine are evaluated in double and rounded to float on both sides.
Independence of the tree: the builder's spatial splits are switched off by RMCLHIP_SBVH_ALPHA=0, which it reads once per process, so a
child process builds cadmix20k without them and this process compares its info and clouds with its own, whose tree has them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_cases as rc
import surface_sample_cases as sc
import surface_sample_ref as ssr

pytestmark = pytest.mark.gpu

N_MAX = max(sc.COUNTS)
SEED = sc.SEED
EPOCH = 5
_cache = {}


def _map_of(ra, ctx, name):
    if ("map", name) not in _cache:
        if name == "scene":
            _cache[("map", name)] = ra.import_hip_scene(ctx, *sc.scene_parts())
        else:
            _cache[("map", name)] = ra.import_hip_map(ctx, *sc.build_map(name))
    return _cache[("map", name)]


def _kw(key):
    name, kw = sc.parametrisations()[key]
    p = ssr.params(**kw)
    return name, {k: (float(v) if np.ndim(v) == 0 else [float(x) for x in v]) for k, v in p.items()}


def _sampler(ra, ctx, key):
    if ("sampler", key) not in _cache:
        name, kw = _kw(key)
        _cache[("sampler", key)] = ra.SurfaceSamplerHip(_map_of(ra, ctx, name), **kw)
    return _cache[("sampler", key)]


def _ref_cloud(key):
    """the restated cloud of N_MAX particles, computed once: particle i is a function of i, so a smaller cloud is its head"""
    if ("ref", key) not in _cache:
        p, a = ssr.init_surface(sc.ref_sampler(key), 0, N_MAX, SEED, EPOCH)
        p.setflags(write=False)
        a.setflags(write=False)
        _cache[("ref", key)] = (p, a)
    return _cache[("ref", key)]


def _poisoned(ra, ctx, n, lead):
    from rmcl_amd import types as T
    tot = lead + n + 3
    d_p = ra.DeviceArray.from_host(ctx, np.full(tot * 32, 0xFF, np.uint8))
    d_a = ra.DeviceArray.from_host(ctx, np.full(tot * 36, 0xFF, np.uint8))
    return d_p, d_a, d_p.ptr + lead * 32, d_a.ptr + lead * 36, T


def _fetch(d_p, d_a, n, lead, T):
    rp, rawa = d_p.download(), d_a.download()
    assert np.all(rp[:lead * 32] == 0xFF) and np.all(rp[(lead + n) * 32:] == 0xFF), "poses written outside [0, count)"
    assert np.all(rawa[:lead * 36] == 0xFF) and np.all(rawa[(lead + n) * 36:] == 0xFF), "attributes written outside [0, count)"
    return rp[lead * 32:(lead + n) * 32].view(T.TRANSFORM), rawa[lead * 36:(lead + n) * 36].view(T.PARTICLE_ATTRIBUTES)


def _same(p, a, p_ref, a_ref, what):
    assert len(p) == len(p_ref) and len(a) == len(a_ref), what
    rows = (ssr.pose_bytes(p) == ssr.pose_bytes(p_ref)).all(1)
    assert rows.all(), (what, "first differing pose", int(np.argmin(rows)), p[np.argmin(rows)], p_ref[np.argmin(rows)])
    assert a.tobytes() == np.ascontiguousarray(a_ref).tobytes(), what


@pytest.mark.parametrize("key", sorted(sc.parametrisations()))
def test_info_and_init_match_the_restatement(ra, ctx, key):
    s = _sampler(ra, ctx, key)
    ref = sc.ref_sampler(key)
    got, want = s.info(), ref.info()
    assert got == want, (got, want)           # area_eligible: the same double
    assert got["weight_total"] >= 2 ** 32 and got["n_weighted"] >= 1
    p_ref, a_ref = _ref_cloud(key)
    for lead, n in enumerate(sc.counts_of(key)):
        d_p, d_a, vp, va, T = _poisoned(ra, ctx, n, lead)
        s.init(vp, va, SEED, epoch=EPOCH, count=n)
        p, a = _fetch(d_p, d_a, n, lead, T)
        _same(p, a, p_ref[:n], a_ref[:n], "%s n %d" % (key, n))
        assert not p["stamp"].any()
    if key == "cadmix20k":
        mi = _map_of(ra, ctx, "cadmix20k").info()
        assert mi["n_tri_records"] > mi["n_faces"]


@pytest.mark.parametrize("key", ["twofloor_align", "cadmix20k"])
def test_slices_and_shards_equal_the_whole(ra, ctx, key):
    from rmcl_amd import types as T
    s = _sampler(ra, ctx, key)
    p_ref, a_ref = _ref_cloud(key)
    for lead, (first, count) in enumerate(sc.SLICES):
        d_p, d_a, vp, va, T_ = _poisoned(ra, ctx, count, lead + 1)
        ra.init_particles_surface(s, vp, va, SEED, epoch=EPOCH, first=first, count=count)
        p, a = _fetch(d_p, d_a, count, lead + 1, T_)
        _same(p, a, p_ref[first:first + count], a_ref[first:first + count], "%s slice %d+%d" % (key, first, count))
    # a three-rank ragged loopback shard: 1000 = 334 + 333 + 333
    name, kw = _kw(key)
    v, f = sc.build_map(name)
    pf = ra.ShardedParticleFilterHip(v, f, devices=(0, 0, 0), loopback=True)
    try:
        with pytest.raises(ra.RmclHipError, match="no surface sampler"):
            pf.init_surface(1000, SEED, EPOCH)
        pf.set_surface_sampler(**kw)
        pf.init_surface(1000, SEED, EPOCH)
        p, a = pf.download()
        _same(p, a, p_ref[:1000], a_ref[:1000], "%s sharded" % key)
        # the injection on the shards
        for prob, step in ((0.25, 3), (1.0, 4), (0.0, 5)):
            want_p, want_a, mask = ssr.inject(sc.ref_sampler(key), p, a, 0, prob, SEED, step)
            assert pf.inject_surface(prob, SEED, step) == int(mask.sum())
            p, a = pf.download()
            _same(p, a, want_p, want_a, "%s sharded inject p %g" % (key, prob))
        # behind the sharded tournament
        cp, ca = rc.cloud(1000, 17)
        pf.set_particles(cp, ca)
        pf.resample(seed=SEED, step=9)
        p, a = pf.download()
        want_p, want_a, mask = ssr.inject(sc.ref_sampler(key), p, a, 0, 0.25, SEED, 9)
        assert pf.inject_surface(0.25, SEED, 9) == int(mask.sum()) and 150 < mask.sum() < 350
        _same(*pf.download(), want_p, want_a, "%s sharded resample + inject" % key)
        pf.drop_surface_sampler()
        with pytest.raises(ra.RmclHipError, match="no surface sampler"):
            pf.inject_surface(0.25, SEED, 9)
    finally:
        pf.close()


@pytest.mark.parametrize("first,n", [(0, 1), (0, 257), (3, 4097), (1021, 256)])
def test_inject_replaces_the_masked_slots_and_no_other_byte(ra, ctx, first, n):
    s = _sampler(ra, ctx, "twofloor_align")
    ref = sc.ref_sampler("twofloor_align")
    cp, ca = rc.cloud(n, 23 + n)
    for lead, prob in enumerate((0.0, 2.0 ** -32, 0.25, 1.0)):
        d_p, d_a, vp, va, T = _poisoned(ra, ctx, n, lead)
        raw_p, raw_a = d_p.download(), d_a.download()
        raw_p[lead * 32:(lead + n) * 32] = cp.view(np.uint8)
        raw_a[lead * 36:(lead + n) * 36] = ca.view(np.uint8)
        d_p.upload(raw_p)
        d_a.upload(raw_a)
        want_p, want_a, mask = ssr.inject(ref, cp, ca, first, prob, SEED, 11)
        got_n = s.inject(vp, va, prob, SEED, 11, first=first, count=n)
        assert got_n == int(mask.sum()), (prob, got_n, int(mask.sum()))
        p, a = _fetch(d_p, d_a, n, lead, T)
        _same(p, a, want_p, want_a, "inject first %d n %d p %g" % (first, n, prob))
        if prob == 0.0:
            assert d_p.download().tobytes() == raw_p.tobytes() and d_a.download().tobytes() == raw_a.tobytes()
        if prob == 1.0:
            assert mask.all()
            # a replaced slot is the initialisation's function of another counter: never the initialisation's own draw
            init_p, _ = ssr.init_surface(ref, first, n, SEED, 11)
            assert not (ssr.pose_bytes(p) == ssr.pose_bytes(init_p)).all(1).any()
        if prob == 0.25 and n >= 256:
            assert 0.1 * n < mask.sum() < 0.4 * n
            assert (ssr.pose_bytes(p)[~mask] == ssr.pose_bytes(cp)[~mask]).all() and a[~mask].tobytes() == ca[~mask].tobytes()


@pytest.mark.parametrize("which", ["gladiator", "gladiator_shard", "residual", "systematic", "adaptive"])
def test_inject_behind_each_resampler(ra, ctx, which):
    from rmcl_amd import types as T
    s = _sampler(ra, ctx, "cadmix20k")
    ref = sc.ref_sampler("cadmix20k")
    n = 1500
    cp, ca = rc.cloud(n, 31)
    d_p, d_a = ra.DeviceArray.from_host(ctx, cp), ra.DeviceArray.from_host(ctx, ca)
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    first, step = 0, 6
    if which.startswith("gladiator"):
        rs = ra.GladiatorResamplerHip(ctx, seed=SEED)
        rs.step = step
        first = 100 if which.endswith("shard") else 0
        count = rs.update(d_p, d_a, d_pn, d_an, n, first=first, count=300 if first else None)["n_particles"]
    elif which == "residual":
        rs = ra.ResidualResamplerHip(ctx, seed=SEED)
        rs.step = step
        count = rs.update(d_p, d_a, d_pn, d_an, n)["n_particles"]
    else:
        rs = ra.AdaptiveResamplerHip(ctx, seed=SEED)
        rs.step = step
        count = (rs.update_systematic(d_p, d_a, d_pn, d_an, n, 1200) if which == "systematic" else rs.update(d_p, d_a, d_pn, d_an, n))["n_particles"]
    try:
        before_p, before_a = d_pn.download()[:count], d_an.download()[:count]
        want_p, want_a, mask = ssr.inject(ref, before_p, before_a, first, 0.25, SEED, step)
        assert s.inject(d_pn, d_an, 0.25, SEED, step, first=first, count=count) == int(mask.sum()) and mask.any() and not mask.all()
        _same(d_pn.download()[:count], d_an.download()[:count], want_p, want_a, which)
        assert d_p.download().tobytes() == cp.tobytes() and d_a.download().tobytes() == ca.tobytes()      # the old cloud is not touched
    finally:
        rs.close()


def test_adaptive_update_with_recovery_equals_the_five_calls(ra, ctx):
    from rmcl_amd import types as T
    s = _sampler(ra, ctx, "twofloor")
    n = 2000
    cp, ca = rc.cloud(n, 41)
    ca["likelihood"]["mean"] *= np.float32(0.25)           # the cloud's likelihood has dropped ...
    d_p, d_a = ra.DeviceArray.from_host(ctx, cp), ra.DeviceArray.from_host(ctx, ca)
    outs = []
    for fused in (True, False):
        rs = ra.AdaptiveResamplerHip(ctx, seed=SEED)
        rs.step = 2
        rec = ra.RecoveryHip()
        assert rec.update(0.5 * n, n) == 0.0               # ... from a mean of 0.5
        d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
        if fused:
            out = rs.update(d_p, d_a, d_pn, d_an, n, recovery=rec, sampler=s)
        else:
            p_inject = rec.update(rs.compute_stats(d_a, n), n)
            out = rs.update(d_p, d_a, d_pn, d_an, n)
            out["injected"] = s.inject(d_pn, d_an, p_inject, SEED, 2, count=out["n_particles"])
            out["p_inject"] = p_inject
            rec.reset()
        assert rs.step == 3 and (rec.state.w_slow, rec.state.w_fast) == (0.0, 0.0)
        outs.append((out, d_pn.download()[:out["n_particles"]].tobytes(), d_an.download()[:out["n_particles"]].tobytes()))
        plain = rs.update(d_p, d_a, d_pn, d_an, n)
        assert sorted(plain) == ["bins", "n_particles"]    # without the pair: the dict it always returned
        with pytest.raises(ValueError):
            rs.update(d_p, d_a, d_pn, d_an, n, recovery=rec)
        rs.close()
    assert outs[0] == outs[1]
    out = outs[0][0]
    assert 0.0 < out["p_inject"] < 1.0 and 0 < out["injected"] < out["n_particles"]
    # nothing to inject: the averages stay, the bytes are the plain resampler's
    rs = ra.AdaptiveResamplerHip(ctx, seed=SEED)
    rs.step = 2
    rec = ra.RecoveryHip()
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    out = rs.update(d_p, d_a, d_pn, d_an, n, recovery=rec, sampler=s)
    assert out["injected"] == 0 and out["p_inject"] == 0.0 and rec.state.w_slow > 0.0
    with_pair = (d_pn.download()[:out["n_particles"]].tobytes(), d_an.download()[:out["n_particles"]].tobytes())
    rs.step = 2
    plain = rs.update(d_p, d_a, d_pn, d_an, n)
    assert plain["n_particles"] == out["n_particles"]
    assert with_pair == (d_pn.download()[:out["n_particles"]].tobytes(), d_an.download()[:out["n_particles"]].tobytes())
    rs.close()


def test_refusals_leave_the_buffers_untouched(ra, ctx):
    m = _map_of(ra, ctx, "single")
    for bad in sc.BAD_PARAMS:
        with pytest.raises(ra.RmclHipError) as e:
            ra.SurfaceSamplerHip(m, **bad)
        assert e.value.status == ra._capi.ERR_INVALID, bad
    with pytest.raises(ra.RmclHipError, match="eligible") as e:
        ra.SurfaceSamplerHip(m, **sc.OUTSIDE[1])
    assert e.value.status == ra._capi.ERR_INVALID
    s = _sampler(ra, ctx, "single")
    n = 300
    d_p, d_a, vp, va, T = _poisoned(ra, ctx, n, 1)
    raw_p, raw_a = d_p.download(), d_a.download()

    def untouched():
        return d_p.download().tobytes() == raw_p.tobytes() and d_a.download().tobytes() == raw_a.tobytes()

    for prob in (-0.1, 1.5, float("nan")):
        with pytest.raises(ra.RmclHipError, match="p_inject"):
            s.inject(vp, va, prob, SEED, 0, count=n)
    with pytest.raises(ra.RmclHipError, match="2\\^32"):
        s.init(vp, va, SEED, first=0x100000000 - n + 1, count=n)
    with pytest.raises(ra.RmclHipError, match="2\\^32"):
        s.inject(vp, va, 1.0, SEED, 0, first=0x100000000 - n + 1, count=n)
    for pp, aa in ((None, va), (vp, None)):
        with pytest.raises(ra.RmclHipError, match="null"):
            s.init(pp, aa, SEED, count=n)
        with pytest.raises(ra.RmclHipError, match="null"):
            s.inject(pp, aa, 1.0, SEED, 0, count=n)
    lib = ra._capi.lib()
    assert lib.rmclhip_particles_init_surface(None, vp, va, 0, n, SEED, 0) == ra._capi.ERR_INVALID
    assert lib.rmclhip_particles_inject_surface(None, vp, va, 0, n, 1.0, SEED, 0, None) == ra._capi.ERR_INVALID
    assert lib.rmclhip_surface_sampler_create(None, None, None) == ra._capi.ERR_INVALID
    # count == 0: RMCLHIP_OK with nothing touched, null buffers included
    s.init(vp, va, SEED, count=0)
    s.init(None, None, SEED, count=0)
    assert s.inject(vp, va, 1.0, SEED, 0, count=0) == 0 and s.inject(None, None, 1.0, SEED, 0, count=0) == 0
    assert untouched()
    # the last particles a 32-bit counter word can name; a nullable count
    first = 0x100000000 - n
    s.init(vp, va, SEED, epoch=EPOCH, first=first, count=n)
    p, a = _fetch(d_p, d_a, n, 1, T)
    _same(p, a, *ssr.init_surface(sc.ref_sampler("single"), first, n, SEED, EPOCH), "last indices")
    assert lib.rmclhip_particles_inject_surface(s._h, vp, va, first, n, 1.0, SEED, 0, None) == 0
    # the sampler keeps its map alive
    v, f = sc.build_map("single")
    m2 = ra.import_hip_map(ctx, v, f)
    s2 = ra.SurfaceSamplerHip(m2, height=0.5)
    m2.release()
    s2.init(vp, va, SEED, epoch=EPOCH, count=n)
    p, a = _fetch(d_p, d_a, n, 1, T)
    _same(p, a, *ssr.init_surface(sc.ref_sampler("single"), 0, n, SEED, EPOCH), "after the map's owner let go")
    s2.close()


_NO_SPLITS_CHILD = r'''
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import rmcl_amd as ra
from rmcl_amd import types as T
import surface_sample_cases as sc
name, kw = sc.parametrisations()["cadmix20k"]
ctx = ra.Context(0)
m = ra.import_hip_map(ctx, *sc.build_map(name))
mi = m.info()
assert mi["spatial_splits"] == 0 and mi["n_tri_records"] == mi["n_faces"], mi
s = ra.SurfaceSamplerHip(m, **kw)
n = %(n)d
d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
s.init(d_p, d_a, %(seed)d, epoch=%(epoch)d)
p0, a0 = d_p.download(), d_a.download()
injected = s.inject(d_p, d_a, 0.25, %(seed)d, 7)
i = s.info()
np.savez(%(out)r, p0=p0.view(np.uint8), a0=a0.view(np.uint8), p1=d_p.download().view(np.uint8), a1=d_a.download().view(np.uint8),
         injected=injected, info=np.array([i["n_faces"], i["n_eligible"], i["n_weighted"], i["weight_total"]], np.uint64),
         area=np.array([i["area_eligible"]]), records=mi["n_tri_records"])
'''


def test_the_cloud_does_not_depend_on_the_builders_spatial_splits(ra, ctx, tmp_path):
    """the same info, the same initialised cloud and the same injection from cadmix20k built with spatial splits (this process) and
    without (a child process: the builder reads RMCLHIP_SBVH_ALPHA once)"""
    from rmcl_amd import types as T
    assert "RMCLHIP_SBVH_ALPHA" not in os.environ
    key, n = "cadmix20k", N_MAX
    m = _map_of(ra, ctx, key)
    mi = m.info()
    assert mi["spatial_splits"] > 0 and mi["n_tri_records"] > mi["n_faces"]
    out = str(tmp_path / "no_splits.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _NO_SPLITS_CHILD % dict(root=root, tests=os.path.join(root, "tests"), n=n, seed=SEED, epoch=EPOCH, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RMCLHIP_SBVH_ALPHA="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    other = np.load(out)
    assert int(other["records"]) == mi["n_faces"] < mi["n_tri_records"]
    s = _sampler(ra, ctx, key)
    i = s.info()
    assert [i["n_faces"], i["n_eligible"], i["n_weighted"], i["weight_total"]] == [int(x) for x in other["info"]]
    assert i["area_eligible"] == float(other["area"][0])
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    s.init(d_p, d_a, SEED, epoch=EPOCH)
    assert d_p.download().tobytes() == other["p0"].tobytes() and d_a.download().tobytes() == other["a0"].tobytes()
    assert s.inject(d_p, d_a, 0.25, SEED, 7) == int(other["injected"]) > 0
    assert d_p.download().tobytes() == other["p1"].tobytes() and d_a.download().tobytes() == other["a1"].tobytes()
