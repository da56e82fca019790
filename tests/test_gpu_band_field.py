"""The banded distance field on the device (include/rmclhip.h, BANDED DISTANCE FIELD; k_field_level, k_band_classify, k_band_table,
k_band_fill and the banded instantiations of k_field_query, k_pf_update_field, k_field_refine and k_stein_drive) on the smallest maps
that have FAR, STORED and ragged bricks (tests/band_field_ref.py, CASES; tests/test_band_field_cpu.py proves them non-vacuous).

The three downloaded arrays against the restatement's cut of the device's own dense lattice, the lookup against the restatement and
against the dense field, the sensor update's errors and attributes, refine and the Stein step against the same calls on the dense
field, the sharded entry point, a map the dense field refuses, the refusals and the lifetime."""
import ctypes as C
import math
import subprocess
import time

import numpy as np
import pytest

import band_field_ref as bfr
import field_ref as fr
import refine_ref as rr
import stein_ref as sr

pytestmark = pytest.mark.gpu
F = np.float32
# the field the refinement and the Stein step run on (CASES' band of 0.05 leaves them few beams): 81^3 logical nodes, 216 of its 1000
# bricks FAR
REFINE_CELL, REFINE_BAND = 0.05, 0.3


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, ref):
    """equal to the bit, a NaN matching any NaN"""
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(ref)[~nan])


class _World:
    def __init__(self, ra, orc, ctx, name):
        mesh, cell, margin, band = bfr.CASES[name]
        self.v, self.f, self.logical, self.bricks = bfr.case(name)
        self.cell, self.margin, self.band = cell, margin, band
        self.mesh = orc.Mesh(self.v, self.f)
        self.hm = ra.import_hip_map(ctx, self.v, self.f)
        self.dense = ra.DistanceFieldHip(self.hm, cell=cell, margin=margin)
        self.lat = self.dense.download()
        self.bf = ra.DistanceFieldHip.banded(self.hm, cell=cell, margin=margin, band=band)
        self.ref = bfr.build(self.logical, self.bricks, self.lat)      # the restatement's cut of the device's dense lattice

    def close(self):
        self.bf.close()
        self.dense.close()


@pytest.fixture(scope="module")
def world(ra, orc, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _World(ra, orc, ctx, name)
        return cache[name]

    yield get
    for w in cache.values():
        w.close()


def _updater(ra, hm, field):
    from rmcl_amd import types as T
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.set_field(field)
    return upd


@pytest.fixture(scope="module")
def scan(ra, world):
    """(truth [1], Tsb, beams of a scan of the cube taken at the truth)"""
    from rmcl_amd import synthetic as syn, types as T
    w = world("cube")
    Tsb = syn.tsb_offset()
    truth = np.array([T.transform_from_rpy((0.3, -0.5, 0.2), (0.0, 0.0, 0.5))]).reshape(1)
    cloud = w.mesh.simulate_spherical(syn.model_c1(), Tsb, truth[0], bvh=True)["points"]
    return truth, Tsb, cloud


# ---- 1. the three arrays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bfr.CASES))
def test_download_is_the_restatement(ra, world, name):
    w = world(name)
    info, band = w.bf.info(), w.bf.band_info()
    ref_l, ref_b = dict(w.logical), dict(w.bricks)
    ref_b["n_stored"], ref_b["bytes"] = w.ref["n_stored"], w.ref["bytes"]
    ref_l["bytes"] = w.ref["bytes"]
    assert bfr.same_layout((ref_l, ref_b), (info, band)), (info, band)
    assert fr.same_layout(dict(w.dense.info(), bytes=info["bytes"]), info)                  # the logical lattice is the dense field's
    table, coarse, bricks = w.bf.download_banded()
    n_far = int((w.ref["table"] == bfr.FAR).sum())
    assert 0 < n_far < table.size and bfr.is_ragged(w.logical) == (name in bfr.RAGGED)     # FAR, STORED and (where meant) ragged bricks
    assert np.array_equal(table, w.ref["table"])
    assert coarse.tobytes() == w.ref["coarse"].tobytes() and not np.isnan(coarse).any()
    assert _same(bricks, w.ref["bricks"])
    assert np.isnan(bricks).any() == (name in bfr.RAGGED)                                   # NaN in the ragged padding, nowhere else
    # a dense field has no bricks, a banded one no dense lattice
    with pytest.raises(ra.RmclHipError, match="dense"):
        w.dense.band_info()
    with pytest.raises(ra.RmclHipError, match="banded") as e:
        w.bf.download()
    assert e.value.status == ra._capi.ERR_INVALID
    view = C.c_void_p(1)
    assert ra._capi.lib().rmclhip_field_device_view(w.bf.handle, C.byref(view)) == ra._capi.ERR_INVALID


# ---- 2. the lookup -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bfr.CASES))
def test_query_is_the_restatement_and_the_dense_field_where_stored(ra, world, name):
    w = world(name)
    pts, kinds = bfr.query_points(w.logical)
    ref = bfr.lookup(w.logical, w.bricks, w.ref, pts)
    got = w.bf.query(pts)
    assert np.isnan(ref[kinds == "special"]).all() and not np.isnan(ref[kinds != "special"]).any()
    assert _same(got, ref), "%d differ" % (_bits(got) != _bits(ref)).sum()
    stored = bfr.stored_mask(w.logical, w.bricks, w.ref["table"], pts)
    far = ~stored & (kinds != "special")
    assert stored[kinds == "inside"].any() and far[kinds == "inside"].any() and far[np.char.startswith(kinds, "face")].any()
    assert stored[np.char.startswith(kinds, "outside")].any() and stored[kinds == "top"].any()
    dense = w.dense.query(pts)
    assert got[stored].tobytes() == dense[stored].tobytes()
    assert (got[far] > w.band).all() and (dense[far] > w.band).all()
    # device memory in and out: the same bytes; and one point at a time
    d_pts, d_out = ra.DeviceArray.from_host(w.bf.ctx, pts), ra.DeviceArray(w.bf.ctx, np.float32, len(pts))
    w.bf.query(d_pts, out_dev=d_out, n=len(pts))
    assert _same(d_out.download(), got) and _same(w.bf.query(pts[:1]), got[:1])


# ---- 3. the sensor update ---------------------------------------------------------------------------------------------------------------------
def test_update_is_the_restatements_chain(ra, ctx, world, scan):
    from rmcl_amd import synthetic as syn, types as T
    w = world("cube")
    truth, Tsb, cloud = scan
    beams = ra.sample_beams(cloud, 32, seed=7)
    poses, attrs = syn.uniform_particles(64, seed=16, bb_min=(-1.8, -1.8, -1.8, 0, 0, -math.pi), bb_max=(1.8, 1.8, 1.8, 0, 0, math.pi))
    poses[5] = truth[0]
    upd = _updater(ra, w.hm, w.bf)
    upd.setInput(beams, Tsb)
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_err = ra.DeviceArray(ctx, np.float32, 64 * 32)
    upd.set_error_output(d_err)
    upd.update(d_poses, d_attrs)
    upd.set_error_output(None)
    a_gpu, e_gpu = d_attrs.download(), d_err.download().reshape(64, 32)
    upd.close()
    ends = fr.end_points(poses, Tsb, beams).reshape(-1, 3)
    stored = bfr.stored_mask(w.logical, w.bricks, w.ref["table"], ends)
    assert 100 < stored.sum() < len(ends) - 100                      # both kinds of brick answer
    e_ref = bfr.lookup(w.logical, w.bricks, w.ref, ends).reshape(64, 32)
    assert _same(e_gpu, e_ref) and _same(e_gpu, w.bf.query(ends).reshape(64, 32))
    p = T.pf_params(correspondence_type=1)
    mean, sigma, n_meas = fr.chain(attrs, e_ref, p.dist_sigma, p.max_n_meas)
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], n_meas)
    assert _same(a_gpu["likelihood"]["mean"], mean) and _same(a_gpu["likelihood"]["sigma"], sigma)
    assert d_poses.download().tobytes() == poses.tobytes()


# ---- 4. refine and the Stein step ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refine_world(ra, ctx, world, scan):
    """the cube at REFINE_CELL with a band of REFINE_BAND: (banded field, updaters on the dense and on the banded field, starts, beams,
    Tsb)"""
    w = world("cube")
    truth, Tsb, cloud = scan
    dense = ra.DistanceFieldHip(w.hm, cell=REFINE_CELL)
    bf = ra.DistanceFieldHip.banded(w.hm, cell=REFINE_CELL, band=REFINE_BAND)
    table = bf.download_banded()[0]
    assert (table == bfr.FAR).sum() == 216 and table.size == 1000
    beams = ra.sample_beams(cloud, 65, seed=9)
    # near the truth, where beams are used, and far from it, where end points fall into FAR bricks
    starts = np.concatenate([rr.perturbed_starts(truth, 49, seed=17, d_trans=0.15, d_yaw=0.05),
                             rr.perturbed_starts(truth, 16, seed=18, d_trans=1.2, d_yaw=0.5)])
    ends = fr.end_points(starts, Tsb, beams).reshape(-1, 3)
    logical, bricks = bfr.layout(w.v.min(axis=0), w.v.max(axis=0), REFINE_CELL, 0.0, REFINE_BAND)
    stored = bfr.stored_mask(logical, bricks, table, ends)
    assert 500 < stored.sum() < len(ends) - 20                       # both kinds of brick are met
    ud, ub = _updater(ra, w.hm, dense), _updater(ra, w.hm, bf)
    ud.setInput(beams, Tsb)
    ub.setInput(beams, Tsb)
    yield bf, ud, ub, starts, beams, Tsb
    ud.close()
    ub.close()
    bf.close()
    dense.close()


def _refine(ra, ctx, call, starts, **kw):
    d_poses = ra.DeviceArray.from_host(ctx, starts)
    d_rows = ra.DeviceArray.from_host(ctx, np.full(len(starts), 0xFF, np.uint8).repeat(16).view(rr.RESULT))
    st = call(d_poses, results_dev=d_rows, **kw)
    return d_poses.download(), d_rows.download(), st


@pytest.mark.parametrize("max_dist", [0.2, REFINE_BAND])
def test_refine_is_the_dense_fields_bytes(ra, ctx, refine_world, max_dist):
    bf, ud, ub, starts, beams, Tsb = refine_world
    ref = _refine(ra, ctx, ud.refine, starts, iterations=4, max_dist=max_dist)
    got = _refine(ra, ctx, ub.refine, starts, iterations=4, max_dist=max_dist)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]
    assert ref[2]["n_moved"] >= 40 and (ref[1]["n_used"][:49] > 0).all() and (ref[1]["n_used"] < len(beams)).any()
    # rmclhip_field_refine, on the field's own stream
    own = _refine(ra, ctx, lambda d, **kw: bf.refine(d, beams, Tsb, **kw), starts, iterations=4, max_dist=max_dist)
    assert own[0].tobytes() == ref[0].tobytes() and own[1].tobytes() == ref[1].tobytes()


def test_stein_step_is_the_dense_fields_bytes(ra, ctx, refine_world):
    bf, ud, ub, starts, beams, Tsb = refine_world
    out = []
    for upd in (ud, ub):
        d_poses = ra.DeviceArray.from_host(ctx, starts)
        d_rows = ra.DeviceArray.from_host(ctx, np.full(len(starts), 0xFF, np.uint8).repeat(16).view(sr.RESULT))
        st = upd.stein_step(d_poses, results_dev=d_rows, iterations=2, max_dist=REFINE_BAND)
        out.append((d_poses.download(), d_rows.download(), st))
    ref, got = out
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]
    assert ref[0].tobytes() != starts.tobytes() and (ref[1]["n_used"] > 0).any()


def test_max_dist_beyond_the_band_is_refused(ra, ctx, refine_world):
    bf, ud, ub, starts, beams, Tsb = refine_world
    too_far = float(np.nextafter(F(REFINE_BAND), F(1)))
    calls = (lambda d: ub.refine(d, max_dist=too_far), lambda d: bf.refine(d, beams, Tsb, max_dist=too_far),
             lambda d: ub.stein_step(d, max_dist=too_far), lambda d: ub.refine(d))          # (the default max_dist is 0.5)
    for call in calls:
        d_poses = ra.DeviceArray.from_host(ctx, starts)
        with pytest.raises(ra.RmclHipError, match="band") as e:
            call(d_poses)
        assert e.value.status == ra._capi.ERR_INVALID
        assert d_poses.download().tobytes() == starts.tobytes()
    # the dense field takes it
    assert ud.refine(ra.DeviceArray.from_host(ctx, starts), max_dist=too_far)["n_particles"] == len(starts)


# ---- 5. sharded ---------------------------------------------------------------------------------------------------------------------------------
def test_sharded_banded_field_equals_the_unsharded_bytes(ra, ctx, world, refine_world, scan):
    from rmcl_amd import synthetic as syn, types as T
    w = world("cube")
    bf, ud, ub, starts, beams, Tsb = refine_world
    poses, attrs = syn.uniform_particles(len(starts), seed=21, bb_min=(-1.8, -1.8, -1.8, 0, 0, -math.pi), bb_max=(1.8, 1.8, 1.8, 0, 0, math.pi))
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    ub.update(d_poses, d_attrs)
    single_attrs = d_attrs.download()
    single = _refine(ra, ctx, ub.refine, starts, iterations=4, max_dist=REFINE_BAND)
    spf = ra.ShardedParticleFilterHip(w.v, w.f, devices=(0, 0), loopback=True)
    spf.config_ = T.pf_params(correspondence_type=1)
    spf.set_particles(poses, attrs)
    spf.set_field_banded(cell=REFINE_CELL, band=REFINE_BAND)
    spf.update(beams, Tsb)
    got_poses, got_attrs = spf.download()
    assert got_attrs.tobytes() == single_attrs.tobytes() and got_poses.tobytes() == poses.tobytes()
    spf.set_particles(starts, attrs)
    st = spf.refine(beams, Tsb, iterations=4, max_dist=REFINE_BAND)
    got_poses, _ = spf.download()
    assert got_poses.tobytes() == single[0].tobytes()
    assert all(st[k] == single[2][k] for k in ("n_particles", "n_moved", "n_no_beams", "n_not_finite"))
    with pytest.raises(ra.RmclHipError, match="band"):
        spf.refine(beams, Tsb, max_dist=0.5)
    with pytest.raises(ra.RmclHipError, match="band must be finite"):
        spf.set_field_banded(cell=REFINE_CELL, band=0.0)
    spf.close()


# ---- 6. the capability itself -----------------------------------------------------------------------------------------------------------------
def test_a_map_the_dense_field_refuses(ra, orc, ctx):
    """four walls of 100 m x 100 m x 3 m at 0.05 m: 2.4e8 logical nodes"""
    v, f = bfr.walls_mesh()
    hm = ra.import_hip_map(ctx, v, f)
    before = hm.info()["device_bytes"]
    with pytest.raises(ra.RmclHipError, match="max_nodes") as e:
        ra.DistanceFieldHip(hm, cell=0.05)
    assert e.value.status == ra._capi.ERR_INVALID
    t0 = time.time()
    bf = ra.DistanceFieldHip.banded(hm, cell=0.05)                 # the default band and max_nodes
    dt = time.time() - t0
    info, band = bf.info(), bf.band_info()
    print("[band-field] walls 100 x 100 x 3 m at 0.05 m: %d logical nodes (%.0f MB dense), %d of %d bricks stored, %.1f MB, built in %.2f s" % (
        info["n_nodes"], 4e-6 * info["n_nodes"], band["n_stored"], band["n_bricks"], 1e-6 * band["bytes"], dt))
    assert info["n_nodes"] > (1 << 26) and 729 * band["n_stored"] + band["n_coarse"] <= (1 << 26)
    assert 0 < band["n_stored"] < band["n_bricks"] // 4
    assert hm.info()["device_bytes"] == before + band["bytes"] == before + info["bytes"]
    # a few hundred points within the band of a wall
    rng = np.random.RandomState(3)
    along, depth, height = rng.uniform(1, 99, 400), rng.uniform(0.0, 0.45, 400), rng.uniform(0.05, 2.95, 400)
    side = rng.randint(0, 4, 400)
    x = np.where(side == 0, along, np.where(side == 1, 100 - depth, np.where(side == 2, along, depth)))
    y = np.where(side == 0, depth, np.where(side == 1, along, np.where(side == 2, 100 - depth, along)))
    pts = np.stack([x, y, height], -1).astype(F)
    truth = fr.oracle_distances(orc.Mesh(v, f), pts)
    assert (truth <= 0.5).all()
    got = bf.query(pts)
    err = np.abs(got.astype(np.float64) - truth)
    print("[band-field] walls: max |lookup - oracle| within the band = %.3g m of %.3g allowed" % (err.max(), fr.SQRT3_2 * info["cell"]))
    assert (err <= fr.SQRT3_2 * info["cell"]).all()
    # far from every wall the coarse lattice answers, beyond the band
    assert (bf.query(np.array([[50, 50, 1.5], [20, 70, 0.2]], F)) > 0.5).all()
    bf.close()
    assert hm.info()["device_bytes"] == before


# ---- 7. refusals and lifetime ---------------------------------------------------------------------------------------------------------------
def test_refusals_leak_nothing(ra, ctx, world):
    w = world("cube")
    before = w.hm.info()["device_bytes"]
    need = 729 * w.ref["n_stored"] + w.bricks["n_coarse"]
    with pytest.raises(ra.RmclHipError, match="max_nodes") as e:
        ra.DistanceFieldHip.banded(w.hm, cell=w.cell, margin=w.margin, band=w.band, max_nodes=need - 1)
    assert e.value.status == ra._capi.ERR_INVALID and w.hm.info()["device_bytes"] == before
    ok = ra.DistanceFieldHip.banded(w.hm, cell=w.cell, margin=w.margin, band=w.band, max_nodes=need)
    assert w.hm.info()["device_bytes"] == before + ok.band_info()["bytes"] and ok.band_info()["bytes"] == w.ref["bytes"]
    ok.close()
    assert w.hm.info()["device_bytes"] == before
    for kw, match in ((dict(band=0.0), "band must be finite"), (dict(band=math.nan), "band must be finite"), (dict(cell=-1.0), "cell must be finite"),
                      (dict(cell=1e-6), "2\\^20 cells")):
        with pytest.raises(ra.RmclHipError, match=match):
            ra.DistanceFieldHip.banded(w.hm, **kw)
    assert w.hm.info()["device_bytes"] == before


def test_field_of_another_map_and_lifetime(ra, ctx, world, scan):
    from rmcl_amd import synthetic as syn
    w, other = world("cube"), world("quad")
    truth, Tsb, cloud = scan
    beams = ra.sample_beams(cloud, 32, seed=7)
    upd = _updater(ra, w.hm, None)
    with pytest.raises(ra.RmclHipError, match="another map") as e:
        upd.set_field(other.bf)
    assert e.value.status == ra._capi.ERR_INVALID
    # the creator's reference goes while the filter handle holds the field
    before = w.hm.info()["device_bytes"]
    bf = ra.DistanceFieldHip.banded(w.hm, cell=w.cell, margin=w.margin, band=w.band)
    held = w.hm.info()["device_bytes"]
    upd.set_field(bf)
    bf.close()
    assert w.hm.info()["device_bytes"] == held > before
    poses, attrs = syn.uniform_particles(64, seed=16, bb_min=(-1.8, -1.8, -1.8, 0, 0, -math.pi), bb_max=(1.8, 1.8, 1.8, 0, 0, math.pi))
    upd.setInput(beams, Tsb)
    out = []
    for u in (upd, _updater(ra, w.hm, w.bf)):
        if u is not upd:
            u.setInput(beams, Tsb)
        d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        u.update(d_poses, d_attrs)
        out.append(d_attrs.download())
        u.close()
    assert out[0].tobytes() == out[1].tobytes()
    assert w.hm.info()["device_bytes"] == before


# ---- 8. the C++ example ---------------------------------------------------------------------------------------------------------------------------
def test_example_runs(ra, tmp_path):
    exe = bfr.build_example(tmp_path)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "dense field refused" in out.stdout and "banded field built" in out.stdout and "OK" in out.stdout
