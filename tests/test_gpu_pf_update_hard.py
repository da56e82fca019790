"""GPU parity of the particle filter's sensor update with ray-casting correspondences (k_pf_update_v3, correspondence_type 0, 2, 3) on
the hard maps and at the edges of its beams, poses, launch shapes and accumulators.  Cases: tests/pf_update_cases.py, proved non-vacuous
on the CPU by tests/test_pf_update_cases_cpu.py.  Product variants only (none needs the experiments library).

Every comparison is against the oracle's BRUTE FORCE (Mesh.pf_update(..., bvh=False)): the class of every beam (the three penalties are
negative and compared bit for bit), the NaN pattern, the geometric errors, n_meas bit for bit, mean and sigma within the bar of
tests/test_gpu_pf.py, state_sigma untouched; the variants among themselves bit for bit."""
import time

import numpy as np
import pytest

import pf_update_cases as uc
from test_gpu_pf import _check_all_particles, _run

pytestmark = pytest.mark.gpu

_maps = {}
_T0 = [None]
_BIT_DIFFERENCES = {}       # what -> number of beams whose error bits differ from the oracle's (printed by the last test)


def _hip_map(ra, ctx, case):
    if _T0[0] is None:
        _T0[0] = time.time()
    key = id(case["v"])                 # (the case modules keep every map alive)
    if key not in _maps:
        _maps[key] = ra.import_hip_map(ctx, case["v"], case["f"])
    return _maps[key]


def _device(ra, ctx, case, mode, variant, **over):
    from rmcl_amd import types as T
    return _run(ra, ctx, _hip_map(ra, ctx, case), case["poses"], case["attrs"].copy(), case["beams"], uc.identity(),
                params=uc.params(T, case, mode, **over), variant=variant)


def _check_errors(case, mode, e_gpu, e_ref, what):
    """classes and NaN pattern equal, the three penalties bit for bit (a class IS its value); geometric errors within 1e-5 relative plus
    2 ulp32(M) absolute, M the largest coordinate magnitude entering that beam (|O|, |pint|, |preal|, from the reference): up to 10 m the
    bar of test_gpu_pf._check stated in float32 resolution, on the maps 5 km out what float32 can hold.  Beams whose bits equal the
    oracle's need no bar; M is worked out for the others alone."""
    cg, cr = uc.beam_class(e_gpu), uc.beam_class(e_ref)
    bad = np.argwhere(cg != cr)
    assert len(bad) == 0, "%s: the class of %d of %d beams differs, first (particle, beam) %s: device %s, oracle %s" % (
        what, len(bad), cg.size, bad[:5].tolist(), [uc.CLASS_NAMES[cg[i, j]] for i, j in bad[:5]], [uc.CLASS_NAMES[cr[i, j]] for i, j in bad[:5]])
    g, r = np.asarray(e_gpu, np.float32), np.asarray(e_ref, np.float32)
    differ = np.argwhere(g.view(np.uint32) != r.view(np.uint32))
    _BIT_DIFFERENCES[what] = len(differ)
    if len(differ) == 0:
        return
    g64, r64 = g[differ[:, 0], differ[:, 1]].astype(np.float64), r[differ[:, 0], differ[:, 1]].astype(np.float64)
    assert np.isfinite(g64).all() and np.isfinite(r64).all(), "%s: %s" % (what, uc.first_beam_difference("errors", g, r))
    tol = 1e-5 * np.abs(r64) + 2.0 * uc.ulp32(uc.magnitude(case, mode, differ))
    out = np.abs(g64 - r64) > tol
    assert not out.any(), "%s: %d of %d beam errors outside 1e-5 relative + 2 ulp32(M), first (particle, beam) %s: device %r, oracle %r, bar %.3g" % (
        what, out.sum(), g.size, differ[out][0].tolist(), g64[out][0], r64[out][0], tol[out][0])


def _check_attrs(a_gpu, a_ref, what):
    g, r = a_gpu["likelihood"]["sigma"], a_ref["likelihood"]["sigma"]
    assert np.array_equal(np.isnan(g), np.isnan(r)), "%s: NaN pattern of sigma differs at particles %s" % (what, np.flatnonzero(np.isnan(g) != np.isnan(r))[:8].tolist())
    _check_all_particles(a_gpu, a_ref, what)


def _compare_variants(case, mode, results, what):
    """errors bit-identical across ALL variants; attributes across the accumulating ones, and across the stored ones"""
    v0, (a0, e0) = next(iter(results.items()))
    for v, (a, e) in results.items():
        msg = uc.first_beam_difference("%s: variant %s against variant %s" % (what, v, v0), e, e0)
        assert msg is None, msg
    for stored in (False, True):
        grp = [(v, a) for v, (a, e) in results.items() if uc.is_stored(v) == stored]
        for v, a in grp[1:]:
            msg = uc.pc.first_difference(what, "attributes of variant %s and variant %s" % (v, grp[0][0]), a, grp[0][1])
            assert msg is None, msg


# ---- the hard maps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", uc.MODES)
@pytest.mark.parametrize("name", uc.MAPS)
def test_hard_map_matches_brute_force_in_every_variant(ra, orc, ctx, name, mode):
    c = uc.update_case(name, orc)
    a_ref, e_ref = uc.reference(c, orc, mode)
    results = {}
    for variant in uc.VARIANTS:
        what = "%s mode %d variant %s" % (name, mode, variant)
        a, e = _device(ra, ctx, c, mode, variant)
        _check_errors(c, mode, e, e_ref, what)
        _check_attrs(a, a_ref, what)
        results[variant] = (a, e)
    _compare_variants(c, mode, results, "%s mode %d" % (name, mode))


# ---- beam and pose edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, 64 | uc.STORED])
@pytest.mark.parametrize("mode", uc.MODES)
def test_edge_table(ra, orc, ctx, mode, variant):
    """range at, just below and just above both ends of the sensor interval; a wall exactly range_min away; NaN, infinite, zero and
    negative ranges; NaN, zero, short and long directions; an origin 1 km off; NaN, zero and non-unit quaternions, a NaN translation;
    particles on a face and on a vertex; particles 10, 100 and 1000 box diagonals out.  The whole particle x beam matrix against the
    oracle; the rows of the table carry the class (held against the oracle by the CPU test, against the device here)"""
    c = uc.with_mesh(uc.edge_case(), orc)
    a_ref, e_ref = uc.reference(c, orc, mode)
    a, e = _device(ra, ctx, c, mode, variant)
    what = "edge table mode %d variant %s" % (mode, variant)
    cls = uc.beam_class(e)
    for label, pi, bi, expect in c["rows"]:
        assert cls[pi, bi] == expect[mode], "%s, row `%s`: device %s (%r), table %s" % (what, label, uc.CLASS_NAMES[cls[pi, bi]], float(e[pi, bi]), uc.CLASS_NAMES[expect[mode]])
    _check_errors(c, mode, e, e_ref, what)
    _check_attrs(a, a_ref, what)


@pytest.mark.parametrize("variant", [None, 64 | uc.STORED])
@pytest.mark.parametrize("offset", uc.TFAR_OFFSETS)
def test_mode_3_ends_its_rays_at_1e4(ra, orc, ctx, offset, variant):
    c = uc.with_mesh(uc.tfar_case(offset), orc)
    for mode in uc.MODES:
        a_ref, e_ref = uc.reference(c, orc, mode)
        a, e = _device(ra, ctx, c, mode, variant)
        what = "tri1 %g m ahead, mode %d variant %s" % (offset, mode, variant)
        _check_errors(c, mode, e, e_ref, what)
        _check_attrs(a, a_ref, what)
        want = uc.GEO if (mode != 3 or offset < 1.0e4) else uc.C_RHSM
        assert (uc.beam_class(e)[:, :2] == want).all(), what


# ---- launch shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, 64 | uc.STORED])
@pytest.mark.parametrize("n_particles,n_beams", uc.SHAPES)
def test_launch_shapes(ra, orc, ctx, n_particles, n_beams, variant):
    """the three rules that choose the particles of a workgroup (2048 / n_beams, at most 16 in the accumulating form, halving for small
    clouds), partial last workgroups, one beam, one particle, 8192 beams; the records behind the cloud stay as they were"""
    from rmcl_amd import types as T
    c = uc.with_mesh(uc.shape_case(n_particles, n_beams), orc)
    mode = (0, 2, 3)[(n_particles + n_beams) % 3]
    a_ref, e_ref = uc.reference(c, orc, mode)
    pad = 8
    attrs = np.zeros(n_particles + pad, c["attrs"].dtype)
    attrs.view(np.uint8)[:] = 0xA5
    attrs[:n_particles] = c["attrs"]
    upd = ra.PCDSensorUpdaterHip(_hip_map(ra, ctx, c))
    upd.config = uc.params(T, c, mode)
    upd.init()
    if variant is not None:
        upd.set_variant(variant)
    upd.setInput(c["beams"], uc.identity())
    d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, attrs)
    d_e = ra.DeviceArray(ctx, np.float32, n_particles * n_beams + pad)
    sentinel = np.full(n_particles * n_beams + pad, -7.0, np.float32)
    d_e.upload(sentinel)
    upd.set_error_output(d_e)
    upd.update(d_p, d_a, n_particles=n_particles)
    a, e = d_a.download(), d_e.download()
    upd.close()
    what = "%d particles x %d beams, mode %d variant %s" % (n_particles, n_beams, mode, variant)
    assert a[n_particles:].tobytes() == attrs[n_particles:].tobytes(), what + ": attributes behind the cloud were written"
    assert np.array_equal(e[n_particles * n_beams:], sentinel[n_particles * n_beams:]), what + ": errors behind the cloud were written"
    _check_errors(c, mode, e[:n_particles * n_beams].reshape(n_particles, n_beams), e_ref, what)
    _check_attrs(a[:n_particles], a_ref, what)


def test_more_than_8192_beams_is_refused(ra, ctx):
    from rmcl_amd import _capi, types as T
    c = uc.shape_case(3, uc.MAX_BEAMS)
    beams = np.concatenate([c["beams"], c["beams"][:1]])
    assert len(beams) == uc.MAX_BEAMS + 1
    for variant in (None, 64 | uc.STORED):
        upd = ra.PCDSensorUpdaterHip(_hip_map(ra, ctx, c))
        upd.config = uc.params(T, c, 0)
        upd.init()
        if variant is not None:
            upd.set_variant(variant)
        upd.setInput(beams, uc.identity())
        d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
        with pytest.raises(ra.RmclHipError, match="more than 8192 beams") as err:
            upd.update(d_p, d_a)
        assert err.value.status == _capi.ERR_UNSUPPORTED
        assert d_a.download().tobytes() == c["attrs"].tobytes()
        upd.close()


# ---- accumulator range ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, 64 | uc.STORED])
def test_smallest_dist_sigma_sits_below_the_top_of_the_accumulators(ra, orc, ctx, variant):
    """dist_sigma = 1e-10f: the peak eval 3.99e9 lies below the 2^32 top of the first fixed-point row; particles AT the truth (errors
    exactly 0) come back with that mean, not with NaN"""
    c = uc.sigma_case(orc)
    a_ref, e_ref = uc.reference(c, orc, 0)
    a, e = _device(ra, ctx, c, 0, variant)
    what = "dist_sigma 1e-10 variant %s" % variant
    _check_errors(c, 0, e, e_ref, what)
    _check_attrs(a, a_ref, what)
    assert np.isfinite(a["likelihood"]["mean"]).all() and a["likelihood"]["mean"][:c["n_truth"]].max() > 3.9e9


def test_dist_sigma_below_1e_10_is_refused(ra, ctx):
    from rmcl_amd import _capi, types as T
    c = uc.edge_case()
    upd = ra.PCDSensorUpdaterHip(_hip_map(ra, ctx, c))
    upd.init()
    for sigma in (uc.SIGMA_BELOW, 1e-11, 1e-20, 1e-38):
        upd.config = uc.params(T, c, 0, dist_sigma=sigma)
        with pytest.raises(ra.RmclHipError, match="1e-10") as err:
            upd.init()
        assert err.value.status == _capi.ERR_INVALID, sigma
    upd.config = uc.params(T, c, 0, dist_sigma=uc.SIGMA_MIN)
    upd.init()
    sh = ra.ShardedParticleFilterHip(c["v"], c["f"], devices=(0, 0), loopback=True)
    sh.set_particles(c["poses"], c["attrs"])
    sh.config_ = uc.params(T, c, 0, dist_sigma=uc.SIGMA_BELOW)
    with pytest.raises(ra.RmclHipError, match="1e-10"):
        sh.update(c["beams"], uc.identity())
    assert sh.download()[1].tobytes() == c["attrs"].tobytes()
    sh.close()
    upd.close()


# ---- other dealings of the same rays -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain200", "fan20k"])
def test_particle_minor_dealing_with_an_order_array_keeps_the_bits(ra, orc, ctx, name):
    from rmcl_amd import types as T
    c = uc.update_case(name, orc)
    n = len(c["poses"])
    order = np.random.RandomState(17000).permutation(n).astype(np.uint32)
    for mode in uc.MODES:
        a0, e0 = _device(ra, ctx, c, mode, None)
        upd = ra.PCDSensorUpdaterHip(_hip_map(ra, ctx, c))
        upd.config = uc.params(T, c, mode)
        upd.init()
        upd.set_mapping(1, 16, ra.DeviceArray.from_host(ctx, order))
        upd.setInput(c["beams"], uc.identity())
        d_p, d_a = ra.DeviceArray.from_host(ctx, c["poses"]), ra.DeviceArray.from_host(ctx, c["attrs"])
        d_e = ra.DeviceArray(ctx, np.float32, n * len(c["beams"]))
        upd.set_error_output(d_e)
        upd.update(d_p, d_a)
        a, e = d_a.download(), d_e.download().reshape(n, -1)
        upd.close()
        msg = uc.first_beam_difference("%s mode %d: particle-minor with an order array against the default" % (name, mode), e, e0)
        assert msg is None, msg
        msg = uc.pc.first_difference("%s mode %d" % (name, mode), "attributes (particle-minor with an order array, default)", a, a0)
        assert msg is None, msg
        _check_errors(c, mode, e, uc.reference(c, orc, mode)[1], "%s mode %d particle-minor" % (name, mode))


def test_sharded_update_on_a_deep_map_keeps_the_bits(ra, orc, ctx):
    """three loopback ranks (50 particles each) over chain200: the sharded update == the unsharded one, bit for bit"""
    from rmcl_amd import types as T
    c = uc.update_case("chain200", orc)
    sh = ra.ShardedParticleFilterHip(c["v"], c["f"], devices=(0, 0, 0), loopback=True)
    for mode in uc.MODES:
        sh.set_particles(c["poses"], c["attrs"])
        sh.config_ = uc.params(T, c, mode)
        w = sh.update(c["beams"], uc.identity())
        p, a = sh.download()
        a0, _ = _device(ra, ctx, c, mode, None)
        msg = uc.pc.first_difference("chain200 mode %d" % mode, "attributes (sharded over three ranks, unsharded)", a, a0)
        assert msg is None, msg
        assert p.tobytes() == c["poses"].tobytes()
        assert np.array_equal(np.asarray(w).view(np.uint32), a0["likelihood"]["mean"].view(np.uint32))
        _check_attrs(a, uc.reference(c, orc, mode)[0], "chain200 mode %d sharded" % mode)
    sh.close()


def test_zz_wall_time_of_this_module():
    """printed for profiles/pf_update_hard_cases.txt"""
    if _T0[0] is not None:
        print("[pf-update] wall time of tests/test_gpu_pf_update_hard.py: %.1f s" % (time.time() - _T0[0]))
    off = {k: v for k, v in _BIT_DIFFERENCES.items() if v}
    print("[pf-update] beam errors: %d comparisons with the oracle's brute force, %d of them with beams that are not bit-equal%s" % (
        len(_BIT_DIFFERENCES), len(off), "".join("\n[pf-update]   %s: %d beams" % kv for kv in sorted(off.items())[:40])))
