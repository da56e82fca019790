"""The distance field's build, lookup, sensor update and refinement (k_field_level, k_field_query, k_pf_update_field, k_field_refine)
on deep, sliver, degenerate, duplicated, tiny, far-away and overflowing maps -- the inputs of tests/field_cases.py, which
tests/test_field_cases_cpu.py proves non-vacuous without a device.

Node values three ways: the bytes the exact correspondence_type 1 update reports for beams that end on the nodes, the brute-force
oracle at every node with the comparison of tests/test_gpu_cpc_hard.py (1e-5 relative + 1e-7, the NaN pattern identical; against
float64 within cpc_cases.f64_bound, two-sided on the well-scaled maps and from below on slivers and the CAD mix), and the layout.  The
lookup, the update's errors and attributes and the refinement's poses, rows and counts against their numpy restatements
(tests/field_ref.py, tests/refine_ref.py) fed with the device's own lattice: the same NaN pattern and the same bytes everywhere else
(field_cases.same_bits says why a NaN's payload is not compared).  The banded build (k_field_level at strides 16 and 8, k_band_fill)
on every one of these maps against the restatement's cut of the device's own dense lattice (tests/band_field_ref.py).

The last test prints the module's wall time and one line per map (recorded in profiles/field_hard_cases.txt)."""
import time

import numpy as np
import pytest

import band_field_ref as bfr
import cpc_cases as cc
import field_cases as fc
import field_ref as fr
import refine_ref as rr
from conftest import assert_close_rel
from test_gpu_refine import _capi_params, _device, _same_stats

pytestmark = pytest.mark.gpu
F = np.float32
_T0 = [None]
_LINES = {}         # map -> what the last test prints


class _World:
    def __init__(self, ra, orc, ctx, name):
        self.name = name
        self.v, self.f = fc.build_map(name)
        self.hm = ra.import_hip_map(ctx, self.v, self.f)
        cell, margin = fc.cell_margin(name)
        self.fd = ra.DistanceFieldHip(self.hm, cell=cell, margin=margin)
        self.info, self.lat = self.fd.info(), self.fd.download()
        self.oracle = fc.oracle_lattice(orc, name)          # (info, lattice, face ids), brute force, once per process


@pytest.fixture(scope="module")
def world(ra, orc, ctx):
    """per map, made once: the device map, its field, the downloaded lattice and the oracle's"""
    if _T0[0] is None:
        _T0[0] = time.time()
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _World(ra, orc, ctx, name)
        return cache[name]

    yield get
    for w in cache.values():
        w.fd.close()


def _updater(ra, hm, field=None):
    from rmcl_amd import types as T
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    if field is not None:
        upd.set_field(field)
    return upd


def _run(ra, ctx, upd, poses, attrs, beams, Tsb):
    """one update on fresh device copies: (attrs, errors [n_particles, n_beams])"""
    upd.setInput(beams, Tsb)
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_err = ra.DeviceArray(ctx, np.float32, len(poses) * len(beams))
    upd.set_error_output(d_err)
    upd.update(d_poses, d_attrs)
    upd.set_error_output(None)
    return d_attrs.download(), d_err.download().reshape(len(poses), len(beams))


# ---- 1. node values, three ways ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.MAPS)
def test_node_values(ra, orc, ctx, world, name):
    from rmcl_amd import synthetic as syn, types as T
    w = world(name)
    info, lat = w.info, w.lat
    # (c) the layout
    assert fr.same_layout(fc.layout(name), info) and tuple(info["n"]) == fc.expected_n(name)
    assert lat.shape == (info["n"][2], info["n"][1], info["n"][0])
    tree = w.hm.info()
    if name == "cadmix20k":
        assert tree["n_tri_records"] > tree["n_faces"]
    if name in cc.DEEP_MAPS:
        assert 16 < tree["stack_need"] <= 64
    # (b) the brute-force oracle at every node
    _, ref, faces = w.oracle
    n_nan = int(np.isnan(lat).sum())
    both = ~np.isnan(lat) & ~np.isnan(ref)
    worst = float(np.abs(lat[both].astype(np.float64) - ref[both]).max())
    differ = (lat.view(np.uint32) != ref.view(np.uint32)) & both
    _LINES[name] = "%-9s %5d nodes, %d level(s), %3d NaN nodes, max |device - oracle| = %.3g m (%d nodes differ in bits)" % (
        name, lat.size, len(fc.schedule(info["n"])), n_nan, worst, differ.sum())
    print("[field-hard] " + _LINES[name])
    assert np.array_equal(np.isnan(lat), np.isnan(ref)), "%s: %d NaN nodes on the device, %d in the oracle" % (name, n_nan, np.isnan(ref).sum())
    assert (n_nan > 0) == (name == "chain2000") and n_nan < lat.size
    assert_close_rel(lat, ref, 1e-5, 1e-7, "node values " + name)
    pos = fr.node_positions(info).reshape(-1, 3)
    if name in cc.WELL_SCALED + cc.ONE_SIDED:
        # float64 at the nodes whose bits differ from the oracle's (the farthest apart first, at most 1200) and at 800 seeded ones: a
        # node with the oracle's bits has the oracle's float64 deviation, which tests/test_field_cases_cpu.py holds to the same bound
        gap = np.where(differ, np.abs(lat.astype(np.float64) - ref), -1.0).reshape(-1)
        sel = np.argsort(-gap)[:min(1200, int(differ.sum()))]
        sel = np.unique(np.concatenate([sel, np.random.RandomState(78).permutation(lat.size)[:800]]))
        d64, _, _ = cc.ref64(w.v, w.f, pos[sel], hint=faces[sel])
        dev, bound = lat.reshape(-1)[sel].astype(np.float64) - d64, cc.f64_bound(w.v, pos[sel])
        print("[field-hard] %-9s device - float64 at %d nodes in [%.3g, %.3g] of the bound" % (name, len(sel), (dev / bound).min(), (dev / bound).max()))
        assert (dev >= -bound).all(), name
        if name in cc.WELL_SCALED:
            assert (dev <= bound).all(), name
    # (a) what the exact correspondence_type 1 update reports for beams that end on the nodes
    poses, attrs = syn.uniform_particles(1, seed=1)
    poses[0] = T.identity()
    upd = _updater(ra, w.hm)
    got = np.empty(len(pos), F)
    for lo in range(0, len(pos), fc.MAX_BEAMS):
        got[lo:lo + fc.MAX_BEAMS] = _run(ra, ctx, upd, poses, attrs, fc.node_beams(pos[lo:lo + fc.MAX_BEAMS]), T.identity())[1][0]
    upd.close()
    assert np.array_equal(np.isnan(got), np.isnan(lat.reshape(-1))), name + ": the exact update and the field disagree on which nodes find nothing"
    assert fc.same_bits(got, lat) is None, "%s: %s" % (name, fc.same_bits(got, lat))
    # the lookup at node (0, 0, 0) is that node's value -- where its cell has no NaN corner (chain2000: the restatement says NaN)
    at_node = fr.lookup(info, lat, pos[:1])
    assert fc.same_bits(w.fd.query(pos[:1]), at_node) is None and (name == "chain2000" or at_node.tobytes() == lat.reshape(-1)[:1].tobytes())


# ---- 2. the lookup ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.LOOKUP_MAPS)
def test_lookup_is_the_numpy_restatement_bit_for_bit(ra, world, name):
    w = world(name)
    pts, kinds = fc.lookup_points(w.info)
    assert len(pts) == fc.N_LOOKUP_POINTS and len(set(kinds)) == 26 + 6
    ref = fr.lookup(w.info, w.lat, pts)
    special = kinds == "special"
    assert np.isnan(ref[special]).sum() >= 6
    if name == "chain2000":
        assert np.isnan(ref[~special]).all()                   # every cell has a NaN corner
    else:
        assert np.isnan(ref[special]).sum() == 6 and not np.isnan(ref[~special]).any()
        assert np.isfinite(ref[np.char.startswith(kinds, "outside")]).all() and np.isfinite(ref[kinds == "inside"]).all()
    for n in fc.LOOKUP_PREFIXES + (len(pts),):
        got = w.fd.query(pts[:n])
        assert np.array_equal(np.isnan(got), np.isnan(ref[:n])), "%s, n = %d" % (name, n)
        assert fc.same_bits(got, ref[:n]) is None, "%s, n = %d: %s" % (name, n, fc.same_bits(got, ref[:n]))
    # device memory in, device memory out: the same bytes as through the host
    d_pts = ra.DeviceArray.from_host(w.fd.ctx, pts)
    d_out = ra.DeviceArray(w.fd.ctx, np.float32, len(pts))
    w.fd.query(d_pts, out_dev=d_out, n=len(pts))
    assert d_out.download().tobytes() == w.fd.query(pts).tobytes()


# ---- 3. the update from the field -------------------------------------------------------------------------------------------------------------
def _check_update(poses, attrs, beams, Tsb, info, lat, a_gpu, e_gpu, what):
    from rmcl_amd import types as T
    ends = fc.end_points(poses, Tsb, beams)
    k = min(len(poses), 2)
    assert fc.same_bits(ends[:k], fr.end_points(poses[:k], Tsb, beams)) is None, what     # field_ref's own loop, on two particles
    e_ref = fr.lookup(info, lat, ends.reshape(-1, 3)).reshape(len(poses), len(beams))
    assert fc.same_bits(e_gpu, e_ref) is None, "%s errors: %s" % (what, fc.same_bits(e_gpu, e_ref))
    p = T.pf_params(correspondence_type=1)
    mean, sigma, n_meas = fr.chain(attrs, e_gpu, p.dist_sigma, p.max_n_meas)
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], n_meas), what
    for key, ref in (("mean", mean), ("sigma", sigma)):
        msg = fc.same_bits(a_gpu["likelihood"][key], ref)
        assert msg is None, "%s %s: %s" % (what, key, msg)
    assert a_gpu["state_sigma"].tobytes() == attrs["state_sigma"].tobytes(), what
    return e_ref


@pytest.mark.parametrize("n_particles,n_beams", fc.UPDATE_SHAPES)
def test_update_from_the_field(ra, orc, ctx, world, n_particles, n_beams):
    w = world("cadmix20k")
    poses, attrs, beams, Tsb = fc.update_case(ra, orc, n_particles, n_beams)
    upd = _updater(ra, w.hm, w.fd)
    a_gpu, e_gpu = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    upd.close()
    e_ref = _check_update(poses, attrs, beams, Tsb, w.info, w.lat, a_gpu, e_gpu, "cadmix20k %d x %d" % (n_particles, n_beams))
    assert np.isfinite(e_ref).all()


def test_update_refuses_more_than_8192_beams(ra, orc, ctx, world):
    w = world("cadmix20k")
    poses, attrs, beams, Tsb = fc.update_case(ra, orc, 5, fc.MAX_BEAMS)
    beams = np.concatenate([beams, beams[:1]])
    assert len(beams) == fc.MAX_BEAMS + 1
    upd = _updater(ra, w.hm, w.fd)
    upd.setInput(beams, Tsb)
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    sentinel = np.full(5 * len(beams), -7.0, F)
    d_err = ra.DeviceArray.from_host(ctx, sentinel)
    upd.set_error_output(d_err)
    with pytest.raises(ra.RmclHipError, match="more than 8192 beams") as e:
        upd.update(d_poses, d_attrs)
    assert e.value.status == ra._capi.ERR_UNSUPPORTED
    upd.sync()
    assert d_attrs.download().tobytes() == attrs.tobytes() and d_err.download().tobytes() == sentinel.tobytes()
    assert d_poses.download().tobytes() == poses.tobytes()
    upd.set_error_output(None)
    upd.close()


def test_update_on_nan_cells(ra, orc, ctx, world):
    """chain2000: every cell has a NaN corner, so every error is NaN and poisons its particle -- as the restatement's chain says, and as
    a beam without a closest point does in the exact mode"""
    w = world("chain2000")
    poses, attrs, beams, Tsb = fc.chain2000_update_case(ra, orc)
    upd = _updater(ra, w.hm, w.fd)
    a_gpu, e_gpu = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    upd.close()
    e_ref = _check_update(poses, attrs, beams, Tsb, w.info, w.lat, a_gpu, e_gpu, "chain2000")
    assert np.isnan(e_ref).all() and np.isnan(a_gpu["likelihood"]["mean"]).all()
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], attrs["likelihood"]["n_meas"] + len(beams))


# ---- 4. the refinement at known poses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.REFINE_MAPS)
def test_refinement_is_the_restatement_byte_for_byte(ra, orc, ctx, world, name):
    w = world(name)
    truth, Tsb, beams, starts, p = fc.refine_case(ra, orc, name)
    ref_poses, ref_rows, ref_st = rr.refine(w.info, w.lat, starts, beams, Tsb, p)
    got_poses, got_rows, st = _device(ra, ctx, w.fd, starts, beams, Tsb, p)
    assert got_rows.tobytes() == ref_rows.tobytes(), "%s rows: %d differ" % (name, (got_rows != ref_rows).sum())
    assert got_poses.tobytes() == ref_poses.tobytes(), "%s poses: %d differ" % (name, (got_poses != ref_poses).sum())
    assert _same_stats(st, ref_st), (st, ref_st)
    assert np.all(got_rows["cost_after"] <= got_rows["cost_before"])
    e0, e1 = rr.position_error(starts, truth), rr.position_error(got_poses, truth)
    print("[field-hard] %-9s refinement: median position error %.4f -> %.4f m, moved %d of %d, n_used %d..%d" % (
        name, np.median(e0), np.median(e1), st["n_moved"], len(starts), got_rows["n_used"].min(), got_rows["n_used"].max()))
    if name in ("cadmix20k", "degcube"):
        assert np.median(e1) < np.median(e0) and st["n_moved"] == len(starts)
    if name == "floor":
        _, t0 = rr.pose_arrays(starts)
        _, t1 = rr.pose_arrays(got_poses)
        tz = rr.pose_arrays(truth)[1][0, 2]
        assert st["n_moved"] == len(starts) and np.median(np.abs(t1[:, 2] - tz)) < 0.1 * np.median(np.abs(t0[:, 2] - tz))
    if name == "chain2000":
        assert np.isnan(w.lat).any() and (got_rows["n_used"] == 0).all() and st["n_no_beams"] == len(starts) and st["n_moved"] == 0
        assert got_poses.tobytes() == starts.tobytes()
    # one pass at the truth: the count of used beams is the restatement's
    p0 = dict(p, iterations=0)
    assert _device(ra, ctx, w.fd, truth, beams, Tsb, p0)[1].tobytes() == rr.refine(w.info, w.lat, truth, beams, Tsb, p0)[1].tobytes()


def test_refinement_at_its_limits(ra, orc, ctx, world):
    """8192 beams x 64 iterations on 1, 4 and 5 particles: every lane takes 128 beams, particles are independent"""
    w = world("cadmix20k")
    truth, Tsb, cloud = fc.scan(orc, "cadmix20k")
    beams = ra.sample_beams(cloud, rr.MAX_BEAMS, seed=51)
    assert len(beams) == rr.MAX_BEAMS == fc.MAX_BEAMS
    starts = rr.perturbed_starts(truth, max(fc.LIMIT_PARTICLES), seed=151, d_trans=0.3, d_yaw=0.1)
    p = rr.params(iterations=rr.MAX_ITERATIONS, max_dist=1.5)
    ref_poses, ref_rows, _ = rr.refine(w.info, w.lat, starts, beams, Tsb, p)
    assert (ref_rows["accepted"] > 8).all() and (ref_rows["n_used"] > 8000).all()
    for n in fc.LIMIT_PARTICLES:
        got_poses, got_rows, st = _device(ra, ctx, w.fd, starts[:n], beams, Tsb, p)
        assert got_rows.tobytes() == ref_rows[:n].tobytes(), "rows, n = %d" % n
        assert got_poses.tobytes() == ref_poses[:n].tobytes(), "poses, n = %d" % n
        assert _same_stats(st, rr.refine(w.info, w.lat, starts[:n], beams, Tsb, p)[2]) if n == 1 else st["n_moved"] == n


# ---- 5. sharded ---------------------------------------------------------------------------------------------------------------------------------
def test_sharded_field_update_and_refine_equal_the_unsharded_calls(ra, orc, ctx, world):
    """three loopback ranks over cadmix20k: every replica builds its own field from its own copy of the map"""
    from rmcl_amd import types as T
    w = world("cadmix20k")
    poses, attrs, beams, Tsb = fc.update_case(ra, orc, 257, 257)             # a ragged split over three ranks
    upd = _updater(ra, w.hm, w.fd)
    single_attrs, _ = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    upd.close()
    truth, Tsb_r, rbeams, starts, p = fc.refine_case(ra, orc, "cadmix20k")
    single_poses, _, single_st = _device(ra, ctx, w.fd, starts, rbeams, Tsb_r, p)
    cell, margin = fc.cell_margin("cadmix20k")
    spf = ra.ShardedParticleFilterHip(w.v, w.f, devices=(0, 0, 0), loopback=True)
    spf.config_ = T.pf_params(correspondence_type=1)
    spf.set_particles(poses, attrs)
    spf.set_field(cell=cell, margin=margin)
    weights = spf.update(beams, Tsb)
    got_poses, got_attrs = spf.download()
    assert got_attrs.tobytes() == single_attrs.tobytes() and got_poses.tobytes() == poses.tobytes()
    assert np.asarray(weights).tobytes() == single_attrs["likelihood"]["mean"].tobytes()
    r_attrs = attrs[:len(starts)].copy()
    spf.set_particles(starts, r_attrs)
    st = spf.refine(rbeams, Tsb_r, params=_capi_params(ra, p))
    got_poses, got_attrs = spf.download()
    assert got_poses.tobytes() == single_poses.tobytes() and got_attrs.tobytes() == r_attrs.tobytes()
    assert all(st[k] == single_st[k] for k in ("n_particles", "n_moved", "n_no_beams", "n_not_finite"))
    assert abs(st["cost_after_sum"] - single_st["cost_after_sum"]) <= 1e-12 * single_st["cost_after_sum"]     # rank sums added in rank order
    spf.close()


# ---- 6. the banded build on the same maps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.MAPS)
def test_banded_build_is_the_cut_of_the_dense_lattice(ra, world, name):
    """both layouts' node values come from one kernel and one query: at band = half a cell every brick is stored
    (tests/test_field_cases_cpu.py), so every node of the dense lattice is held a second time, by k_band_fill or the coarse level"""
    w = world(name)
    cell, margin = fc.cell_margin(name)
    bf = ra.DistanceFieldHip.banded(w.hm, cell=cell, margin=margin, band=0.5 * cell)
    info, band = bf.info(), bf.band_info()
    table, coarse, bricks = bf.download_banded()
    bf.close()
    assert fr.same_layout(dict(w.info, bytes=info["bytes"]), info), (w.info, info)
    logical, ref_b = fc.band_layout(name)
    ref = bfr.build(logical, ref_b, w.lat)
    print("[field-hard] %-9s banded: %d of %d bricks stored, %d bytes, %d NaN nodes in the bricks" % (
        name, band["n_stored"], band["n_bricks"], band["bytes"], np.isnan(bricks).sum()))
    assert bfr.same_layout((dict(logical, bytes=ref["bytes"]), dict(ref_b, n_stored=ref["n_stored"], bytes=ref["bytes"])), (info, band)), (info, band)
    assert band["n_stored"] == ref["n_stored"] == band["n_bricks"] and band["bytes"] == info["bytes"] == ref["bytes"]
    assert np.array_equal(table, ref["table"])
    for key, got in (("coarse", coarse), ("bricks", bricks)):
        assert got.shape == ref[key].shape, key
        msg = fc.same_bits(got, ref[key])
        assert msg is None, "%s %s: %s" % (name, key, msg)


def test_zz_wall_time_of_this_module():
    """printed for the record: one line per map and the module's wall time"""
    for name in fc.MAPS:
        if name in _LINES:
            print("[field-hard] " + _LINES[name])
    if _T0[0] is not None:
        print("[field-hard] wall time of tests/test_gpu_field_hard.py: %.1f s" % (time.time() - _T0[0]))
