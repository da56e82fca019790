"""The cases of the distance-field tests on hard maps (tests/field_cases.py) without a device: each map has the property it was chosen
for (on the host tree build and the brute-force oracle alone), rmclhip_field_layout_host against its restatement on every map with the
automatic cell and the default max_nodes, the restated lookup and refinement at NaN nodes, and the premise of every known-pose case of
tests/test_gpu_field_hard.py on a lattice of oracle distances.  These are conditions, not measurements."""
import time

import numpy as np
import pytest

import band_field_ref as bfr
import cpc_cases as cc
import field_cases as fc
import field_ref as fr
import refine_ref as rr

F = np.float32


# ---- 1. the maps are what the table says ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.MAPS + ("floor",))
def test_lattice_and_levels(ra, name):
    from rmcl_amd import registration as reg
    v, f = fc.build_map(name)
    info = fc.layout(name)
    n = info["n"]
    assert n == fc.expected_n(name) and info["n_nodes"] < 25000
    cell, margin = fc.cell_margin(name)
    assert fr.same_layout(info, ra.field_layout(v.min(0), v.max(0), cell=cell, margin=margin))
    tree = reg.build_bvh_host(v, f)[0]
    strides = fc.schedule(n)
    print("[field-hard] %-9s %dx%dx%d = %d nodes, %d level(s) %s, n_faces %d n_tri_records %d max_depth %d stack_need %d" % (
        name, n[0], n[1], n[2], info["n_nodes"], len(strides), strides, tree["n_faces"], tree["n_tri_records"], tree["max_depth"], tree["stack_need"]))
    assert tree["stack_need"] <= 64
    if name == "floor":
        assert n[2] > 2                                          # margin 1.0: the lattice has volume
        return
    # the three brackets of the level schedule
    n_max = max(n)
    assert len(strides) == fc.TABLE[name][3] == (1 if n_max <= 8 else 2 if n_max <= 32 else 3)
    if name == "cadmix20k":
        assert tree["n_tri_records"] > tree["n_faces"] == len(f)  # spatial splits: the seeds index records, not faces
    if name == "dupsoup":
        ff = np.sort(np.asarray(f, np.int64), axis=1)
        assert len(np.unique(ff, axis=0)) * 2 == len(f)           # every face twice
    if name == "degcube":
        assert cc.degenerate_cube()[2].sum() == 72
    if name in cc.DEEP_MAPS:
        assert tree["stack_need"] > 16                            # the private spill of nearest_lane_ww<16>
    if name == "farsoup":
        assert min(abs(float(x)) for x in info["origin"][:2]) > 2900.0
    if name == "tri1":
        assert len(f) == 1 and n[2] == 2 and tree["n_nodes"] == 1  # a root with one child: three empty slots
    if name == "tri3":
        assert all((k - 1) % 4 != 0 and (k - 1) % 16 != 0 for k in n)     # the last node of every axis lies off the coarse level
    if name == "chain200":
        assert [fc.level_nodes(n, s) for s in strides] == [(3, 1, 1), (11, 1, 1), (42, 4, 4)]
        assert float(info["inv_cell"]) == float(F(1.0) / F(1e16)) and 0 < float(info["origin"][0]) < 1e-17
    if name == "nested200":
        v64 = np.asarray(v, np.float64)
        assert np.ptp(v64[:, 0]) > 1e13 and np.ptp(v64[:, 2]) < 2.0
    # every seed index the build reads lies inside the previous level, and the last node of an axis that is no multiple of the stride
    # is seeded from the previous level's last node
    for prev, s in zip(strides, strides[1:]):
        for k in range(3):
            pn = fc.level_nodes(n, prev)[k]
            idx = [fc.seed_index(i, prev, pn) for i in range(0, n[k], s)]
            assert min(idx) == 0 and max(idx) == pn - 1 and idx == sorted(idx)


def test_chain2000_has_nan_nodes_and_finite_ones(orc):
    """squared distances beyond 3.4e38 are no distance in float32: the brute-force oracle finds nothing at most nodes, and something
    at the few on the x axis that lie within 1.8e19 of a vertex"""
    info, lat, faces = fc.oracle_lattice(orc, "chain2000")
    n_nan, n_fin = int(np.isnan(lat).sum()), int(np.isfinite(lat).sum())
    print("[field-hard] chain2000 oracle: %d nodes without a distance, %d with one (largest %.4g)" % (n_nan, n_fin, np.nanmax(lat)))
    assert n_nan > 0 and n_fin > 0 and n_nan + n_fin == lat.size
    assert np.array_equal(np.isnan(lat).reshape(-1), faces == cc.INVALID_FACE)
    # the device starts at 3e38 where the oracle starts at INFINITY: no node's squared distance lies between the two
    d2 = lat[np.isfinite(lat)].astype(np.float64) ** 2
    assert (d2 < 2.9e38).all()
    # every cell of this lattice has a NaN corner: a lookup anywhere in it is NaN
    pts, kinds = fc.lookup_points(info)
    assert fc.cell_has_nan_corner(info, lat, pts)[kinds != "special"].all()
    for name in fc.MAPS:
        if name != "chain2000":
            assert not np.isnan(fc.oracle_lattice(orc, name)[1]).any(), name


@pytest.mark.parametrize("name", fc.MAPS)
def test_banded_cut_of_the_oracle_lattice(orc, name):
    """what tests/test_gpu_field_hard.py's banded test takes for granted, on the oracle's lattice: at band = half a cell every brick
    is stored (so that test says nothing about FAR bricks), every lattice is ragged (NaN padding in the last bricks), three maps run
    the banded build's stride-16 level, and chain2000's bricks hold NaN nodes"""
    info, lat, _ = fc.oracle_lattice(orc, name)
    logical, bricks = fc.band_layout(name)
    assert fr.same_layout(dict(info, bytes=0), logical)
    cut = bfr.build(logical, bricks, lat)
    n_nan = int(np.isnan(lat).sum())
    print("[field-hard] %-9s banded at half a cell: %d of %d bricks stored, %d NaN nodes, n_max %d" % (
        name, cut["n_stored"], bricks["n_bricks"], n_nan, max(logical["n"])))
    assert cut["n_stored"] == bricks["n_bricks"] >= 1 and not (cut["table"] == bfr.FAR).any()
    assert bfr.is_ragged(logical) and np.isnan(cut["bricks"]).any()
    assert (max(logical["n"]) > 32) == (name in fc.BAND_N_MAX_OVER_32)
    assert (n_nan > 0) == (name == "chain2000")
    if name == "chain2000":
        assert np.isnan(cut["coarse"]).any() and np.isfinite(cut["coarse"]).any()


@pytest.mark.parametrize("name", [m for m in fc.MAPS if m in cc.WELL_SCALED + cc.ONE_SIDED])
def test_oracle_lattice_against_float64(orc, name):
    """the bound tests/test_gpu_field_hard.py holds the device's nodes to, on the oracle's: 600 seeded nodes per map"""
    v, f = fc.build_map(name)
    info, lat, faces = fc.oracle_lattice(orc, name)
    pos = fr.node_positions(info).reshape(-1, 3)
    sel = np.random.RandomState(77).permutation(len(pos))[:600]
    d64, _, _ = cc.ref64(v, f, pos[sel], hint=faces[sel])
    dev, bound = lat.reshape(-1)[sel].astype(np.float64) - d64, cc.f64_bound(v, pos[sel])
    print("[field-hard] %-9s oracle - float64 in [%.3g, %.3g] of the bound" % (name, (dev / bound).min(), (dev / bound).max()))
    assert (dev >= -bound).all()
    if name in cc.WELL_SCALED:
        assert (dev <= bound).all()


# ---- 2. the layout ----------------------------------------------------------------------------------------------------------------------------
def _layout_or_refusal(lo, hi, max_nodes):
    """field_ref.layout with the refusals of rmclhip_field_layout_host restated: None for a lattice of more than max_nodes nodes or of
    2^31 steps along an axis"""
    with np.errstate(all="ignore"):
        ext = np.asarray(hi, F) - np.asarray(lo, F)
        vol = max(float(ext[0]), 1e-3) * max(float(ext[1]), 1e-3) * max(float(ext[2]), 1e-3)
        cell = F(np.cbrt(np.float64(vol / 2.0e6)))
        if any(not float(np.ceil(ext[k] / cell)) < 2147483648.0 for k in range(3)):
            return None
    ref = fr.layout(lo, hi)
    return ref if ref["n_nodes"] <= max_nodes else None


@pytest.mark.parametrize("name", [m for m in cc.MAPS if m != "fan200k"])
def test_layout_with_the_automatic_cell_and_default_max_nodes(ra, name):
    v, _ = fc.build_map(name)
    lo, hi = np.asarray(v, F).reshape(-1, 3).min(0), np.asarray(v, F).reshape(-1, 3).max(0)
    ref = _layout_or_refusal(lo, hi, 1 << 26)
    if ref is None:
        with pytest.raises(ra.RmclHipError) as e:
            ra.field_layout(lo, hi)
        assert e.value.status == ra._capi.ERR_INVALID and "max_nodes" in str(e.value)
        print("[field-hard] %-9s automatic lattice refused" % name)
    else:
        got = ra.field_layout(lo, hi)
        assert fr.same_layout(ref, got), (ref, got)
        print("[field-hard] %-9s automatic lattice %s" % (name, got["n"]))
    if name == "nested200":
        assert ref is None and fr.layout(lo, hi)["n"] == (2256448, 2256448, 2)
    if name == "floor":
        assert ref is not None and ref["n"] == (2886, 2886, 2)
    if name not in ("nested200",):
        assert ref is not None, name


# ---- 3. NaN corners -------------------------------------------------------------------------------------------------------------------------------
def test_lookup_is_nan_exactly_where_a_corner_is(orc):
    """lerp(a, b, f) = a + f * (b - a) carries a NaN of either end whatever f is (0 * NaN is NaN): the weight path of the blend reaches
    all eight corners of the cell at every point, on a node and on a face too.  So the restated lookup is NaN exactly where the point is
    not finite or one of the eight corners of its cell -- the clamped cell for a point outside -- is NaN."""
    info, lat, _ = fc.oracle_lattice(orc, "tri3")
    holed = fc.nan_holes(lat, seed=5)
    pts, kinds = fc.lookup_points(info)
    assert len(pts) == fc.N_LOOKUP_POINTS and len(set(kinds)) == 26 + 6
    full, got = fr.lookup(info, lat, pts), fr.lookup(info, holed, pts)
    bad = fc.cell_has_nan_corner(info, holed, pts)
    fin = (np.abs(pts) <= fr.FLT_MAX).all(axis=1)
    assert np.array_equal(np.isnan(got), bad | ~fin) and np.array_equal(np.isnan(full), ~fin)
    assert got[~bad & fin].tobytes() == full[~bad & fin].tobytes()
    print("[field-hard] tri3 with 12 NaN nodes: %d of %d lookups are NaN, %d of them outside the lattice" % (
        bad.sum(), fin.sum(), (bad & np.char.startswith(kinds, "outside")).sum()))
    assert 20 < bad.sum() < 0.5 * fin.sum() and (bad & np.char.startswith(kinds, "outside")).any() and (bad & (kinds == "node")).any()
    # a point ON a node whose neighbour is NaN: weight one on the node, zero on the hole, NaN all the same
    pos = fr.node_positions(info)
    k, j, i = np.argwhere(np.isnan(holed))[0]
    i2 = i - 1 if i > 0 else i + 1
    assert np.isnan(fr.lookup(info, holed, pos[k, j, i2][None]))[0] and not np.isnan(holed[k, j, i2])
    # the gradient restatement reads the same corners
    d, g, valid = rr.lookup_grad(info, holed, pts)
    assert not valid[bad].any() and valid[(kinds == "inside") & ~bad].all()


def test_a_beam_in_a_nan_cell_is_not_used(ra, orc):
    info, lat, _ = fc.oracle_lattice(orc, "degcube")
    truth, Tsb, beams, starts, p = fc.refine_case(ra, orc, "degcube")
    holed = fc.nan_holes(lat, seed=6, n_holes=500)
    R, t = rr.pose_arrays(truth)
    ends = rr.end_points(R, t, Tsb, beams).reshape(-1, 3)
    bad = fc.cell_has_nan_corner(info, holed, ends)
    d, g, valid = rr.lookup_grad(info, lat, ends)
    used = valid & (d < p["max_dist"])
    assert (bad & used).sum() >= 10 and (~bad & used).sum() >= 10
    C0, _, _, n0 = rr.evaluate(info, lat, R, t, Tsb, beams, p)
    C1, _, _, n1 = rr.evaluate(info, holed, R, t, Tsb, beams, p)
    assert int(n1[0]) == int(n0[0]) - int((bad & used).sum()) and C1[0] > C0[0]        # each costs max_dist^2 instead of d^2
    out, rows, st = rr.refine(info, holed, starts, beams, Tsb, p)
    assert np.all(rows["cost_after"] <= rows["cost_before"]) and np.isfinite(rows["cost_after"]).all() and not np.isnan(rr.pose_arrays(out)[1]).any()


# ---- 4. the premises of the known-pose cases ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refined(ra, orc):
    """per map, made once: (info, lattice, truth, Tsb, beams, starts, params, poses', rows, stats, counts)"""
    cache = {}

    def get(name):
        if name not in cache:
            info, lat, _ = fc.oracle_lattice(orc, name)
            truth, Tsb, beams, starts, p = fc.refine_case(ra, orc, name)
            out, rows, st = rr.refine(info, lat, starts, beams, Tsb, p)
            traced = fc.refine_trace(info, lat, starts, beams, Tsb, p)
            assert traced[0].tobytes() == out.tobytes() and traced[1].tobytes() == rows.tobytes()      # the trace IS the restatement
            cache[name] = (info, lat, truth, Tsb, beams, starts, p, out, rows, st, traced[2])
        return cache[name]

    return get


@pytest.mark.parametrize("name", ["cadmix20k", "degcube"])
def test_premise_six_degrees_of_freedom(refined, name):
    """all six degrees of freedom are constrained: the restatement's median position error falls on the oracle's lattice"""
    info, lat, truth, Tsb, beams, starts, p, out, rows, st, count = refined(name)
    e0, e1 = rr.position_error(starts, truth), rr.position_error(out, truth)
    print("[field-hard] %-9s restatement on the oracle lattice: median position error %.4f -> %.4f m, yaw %.4f -> %.4f rad, moved %d of %d, %s" % (
        name, np.median(e0), np.median(e1), np.median(fc.yaw_error(starts, truth)), np.median(fc.yaw_error(out, truth)), st["n_moved"], len(starts), count))
    assert np.median(e1) < np.median(e0) and np.median(fc.yaw_error(out, truth)) < np.median(fc.yaw_error(starts, truth))
    assert np.all(rows["cost_after"] <= rows["cost_before"]) and st["n_moved"] == len(starts) and (rows["n_used"] >= 6).all()
    # rank six at the truth: the smallest eigenvalue of A is far from rounding
    R, t = rr.pose_arrays(truth)
    A = rr.evaluate(info, lat, R, t, Tsb, beams, p)[1][0]
    H = np.zeros((6, 6))
    for k, (a, c) in enumerate(rr.TRI):
        H[a, c] = H[c, a] = A[k]
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 1e-6 * ev[-1], ev


def test_premise_floor_is_rank_three(refined):
    """a plane constrains z, roll and pitch alone: A has rank three (the rows of x, y and yaw are zero to rounding), the damping's 1e-9
    carries the Cholesky through them, the cost never rises and x, y and yaw stay where they started.

    Counts, printed: with max_step_trans = 0.05 against z errors of up to 0.45 m most early steps are step-limited.  NO step is
    rejected at a pivot, here or for any other start: with finite A (a sum of outer products, positive semidefinite to 1e-16
    relative) every pivot of A + lambda diag(A) + 1e-9 I is at least lambda A_jj + 1e-9 - rounding with lambda >= 1e-6, which is
    positive.  A pivot fails only on an A that is not finite (a J beyond float32), which a plane 0.85 m below the sensor does not
    produce; the count is printed and left free."""
    info, lat, truth, Tsb, beams, starts, p, out, rows, st, count = refined("floor")
    print("[field-hard] floor     restatement on the oracle lattice: %d particle-iterations, %d rejected at a pivot, %d step-limited, moved %d of %d" % (
        count["tried"], count["rejected"], count["limited"], st["n_moved"], len(starts)))
    assert count["limited"] > 0 and count["tried"] == len(starts) * p["iterations"]
    assert np.all(rows["cost_after"] <= rows["cost_before"]) and st["n_moved"] == len(starts)
    R, t = rr.pose_arrays(truth)
    A = rr.evaluate(info, lat, R, t, Tsb, beams, p)[1][0]
    H = np.zeros((6, 6))
    for k, (a, c) in enumerate(rr.TRI):
        H[a, c] = H[c, a] = A[k]
    ev = np.linalg.eigvalsh(H)
    assert ev[2] < 1e-9 * ev[-1] and ev[3] > 1e-3 * ev[-1], ev
    _, t0 = rr.pose_arrays(starts)
    _, t1 = rr.pose_arrays(out)
    assert np.abs(t1[:, :2].astype(np.float64) - t0[:, :2]).max() < 1e-4          # x and y: unobservable, not moved
    assert np.abs(fc.yaw_error(out, truth) - fc.yaw_error(starts, truth)).max() < 1e-4
    z_err0, z_err1 = np.abs(t0[:, 2] - rr.pose_arrays(truth)[1][0, 2]), np.abs(t1[:, 2] - rr.pose_arrays(truth)[1][0, 2])
    assert np.median(z_err1) < 0.1 * np.median(z_err0)


def test_premise_chain2000_uses_no_beam(refined):
    info, lat, truth, Tsb, beams, starts, p, out, rows, st, count = refined("chain2000")
    assert (rows["n_used"] == 0).all() and st["n_no_beams"] == len(starts) and st["n_moved"] == 0 and out.tobytes() == starts.tobytes()
    assert np.all(rows["cost_before"] == F(len(beams)) * p["max_dist"] * p["max_dist"])


def test_premise_of_the_update_cases(ra, orc):
    """the vectorised end points are field_ref.end_points' bytes; end points fall inside and outside cadmix20k's lattice; every shape
    is there; on chain2000 every error is NaN and the chain says so"""
    from rmcl_amd import types as T
    info, lat, _ = fc.oracle_lattice(orc, "cadmix20k")
    assert set(fc.UPDATE_SHAPES) == {(n, b) for n in (1, 5, 257) for b in (1, 257, 2048, 2049, 8192)} - {(257, 8192)}
    for n, b in ((5, 257), (1, 2049)):
        poses, attrs, beams, Tsb = fc.update_case(ra, orc, n, b)
        ends = fc.end_points(poses, Tsb, beams)
        assert ends.tobytes() == fr.end_points(poses, Tsb, beams).tobytes()
    poses, attrs, beams, Tsb = fc.update_case(ra, orc, 257, 257)
    ends = fc.end_points(poses, Tsb, beams)
    lo = np.array(info["origin"], np.float64)
    hi = lo + (np.array(info["n"]) - 1) * float(info["cell"])
    inside = ((ends >= lo) & (ends <= hi)).all(axis=2)
    assert 0.2 < inside.mean() < 0.9
    e = fr.lookup(info, lat, ends.reshape(-1, 3))
    assert np.isfinite(e).all()
    info, lat, _ = fc.oracle_lattice(orc, "chain2000")
    poses, attrs, beams, Tsb = fc.chain2000_update_case(ra, orc)
    ends = fc.end_points(poses, Tsb, beams)
    assert fc.same_bits(ends, fr.end_points(poses, Tsb, beams)) is None and np.isfinite(ends).all()
    e = fr.lookup(info, lat, ends.reshape(-1, 3)).reshape(len(poses), len(beams))
    assert np.isnan(e).all()
    p = T.pf_params(correspondence_type=1)
    mean, sigma, n_meas = fr.chain(attrs, e, p.dist_sigma, p.max_n_meas)
    assert np.isnan(mean).all() and np.array_equal(n_meas, attrs["likelihood"]["n_meas"] + len(beams))


def test_same_bits():
    a = np.array([1.0, np.nan, 3.0], F)
    b = a.copy()
    b.view(np.uint32)[1] = 0xFFC00000                                  # the other NaN
    assert fc.same_bits(a, b) is None and a.tobytes() != b.tobytes()
    b[2] = np.nextafter(F(3.0), F(4.0))
    assert "1 of 3 differ" in fc.same_bits(a, b)
    b[2] = np.nan
    assert "NaN pattern" in fc.same_bits(a, b)
    assert fc.same_bits(np.array([0.0], F), np.array([-0.0], F)) is not None
