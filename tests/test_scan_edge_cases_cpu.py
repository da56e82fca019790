"""tests/scan_edge_cases.py pinned on the restatements alone (no GPU): every named point reaches the cell, counter or branch it is
named for in tests/pc2scan_ref.py, the condition the GPU's byte parity rests on holds for every point the GPU tests use, and
segmentation_ref.segment_f32 (the float32 restatement tests/test_gpu_segmentation_exact.py compares bits with) agrees with the float64
rule on every ray of the cube scene that `undecided` does not mark."""
import math

import numpy as np
import pytest

import pc2scan_ref as pr
import scan_edge_cases as ec
import segmentation_ref as sr

f32 = np.float32
IMG, OUT, NF = ec.IMG, ec.OUT, ec.NF


def _alone(p, m, flags, T=None):
    """what a single point is, binned alone: its cell, IMG, OUT or NF -- and the range the image then holds there"""
    res = pr.bin_points(np.asarray(p, np.float64).astype(f32).reshape(1, 3), *m, flags=flags, T=T)
    s = res["stats"]
    if not s["n_finite"]:
        assert s["n_in_image"] == s["n_in_range"] == s["n_cells_filled"] == 0
        return NF, None
    if not s["n_in_image"]:
        assert s["n_in_range"] == 0
        return OUT, None
    if not s["n_in_range"]:
        assert s["n_cells_filled"] == 0 and (res["ranges"] == res["empty"]).all()
        return IMG, None
    cell = int(res["cell"][0])
    assert s["n_cells_filled"] == 1 and (np.delete(res["ranges"], cell) == res["empty"]).all()
    return cell, res["ranges"][cell]


def _named(model, name):
    hits = [c for c in ec.case_points(model) if c[0] == name]
    assert len(hits) == 1, (model, name)
    return hits[0][1]


@pytest.mark.parametrize("model", ec.MODEL_ORDER)
def test_every_named_point_is_what_it_is_named_for(model):
    m = ec.MODELS[model]
    cases = ec.case_points(model)
    assert len({c[0] for c in cases}) == len(cases)
    pinned = 0
    for name, p, expect in cases:
        for flags, want in expect.items():
            got, _ = _alone(p, m, flags)
            assert got == want, "%s %s flags %d: %r, named %r" % (model, name, flags, got, want)
            pinned += 1
    assert pinned >= len(cases)
    # every cell that a point can reach has a point of its own, by the reference's rule and by true elevation
    H, W = m[2], m[5]
    for flags, tag in ((0, "own["), (7, "own_el[")):
        cells = {next(iter(e.values())) for n, _, e in cases if n.startswith(tag) and n.endswith("+0.00+0.00")}
        for v in range(H):
            for h in range(W):
                phi = float(m[0]) + v * float(m[1])
                reachable = abs(phi) <= (math.pi / 4 if flags == 0 else math.pi / 2) + 1e-6
                assert (v * W + h in cells) == reachable, (model, flags, v, h)


def test_the_seam_the_poles_and_the_origin_by_hand():
    """the named facts, written out by hand: theta = +pi on a model from -pi has id W (lost; column 0 with WRAP_THETA), on "half" it is
    lost either way, a wrap flag changes nothing on "nowrap"; the poles are +-pi/4 by the reference's rule and +-pi/2 by true elevation"""
    tiny, odd, half, poles, zmin = (ec.MODELS[k] for k in ("tiny", "odd", "half", "poles", "zero_min"))
    for m, W in ((tiny, 8), (odd, 37)):
        mid = (m[2] // 2) * W
        for name in ("seam(-1,+0,0)", "seam(-0,+0,0)"):
            p = _named("tiny" if W == 8 else "odd", name)
            want = (OUT, mid) if p[0] != 0 else (OUT, IMG)          # (-0, +0, 0) is the origin: range 0 < range.min
            assert (_alone(p, m, 0)[0], _alone(p, m, 4)[0]) == want, (W, name)
            assert _alone(p, m, 2)[0] == OUT and _alone(p, m, 7)[0] == want[1] and _alone(p, m, 15)[0] == want[1]
        # -pi is column 0 without any flag
        assert _alone((-1.0, -0.0, 0.0), m, 0)[0] == mid and _alone((-1.0, -0.0, 1.0), m, 0)[0] // W > m[2] // 2
        # the axes: +-pi/2 are columns W/4 and 3W/4 (rounded) of a model from -pi
        assert _alone((0.0, 1.0, 0.0), m, 0)[0] == mid + int(0.75 * W + 0.5) and _alone((0.0, -1.0, 0.0), m, 0)[0] == mid + int(0.25 * W + 0.5)
        assert _alone((0.0, -0.0, 0.0), m, 0)[0] == IMG
    assert _alone((-0.0, 0.0, 0.0), zmin, 4) == (2 * 8, f32(0.0)) and _alone((-0.0, 0.0, 0.0), zmin, 0)[0] == OUT
    # "half": theta = +pi has id 48, one period less is 16 = W: outside with and without the flag; -pi has id -16 (+32: 16)
    for p in ((-1.0, 0.0, 0.0), (-1.0, -0.0, 0.0)):
        for flags in ec.FLAGS:
            assert _alone(p, half, flags)[0] == OUT, (p, flags)
    assert ec.period(half) == 32 and ec.period(ec.MODELS["nowrap"]) == 0 and ec.period(odd) == 37 and ec.period(tiny) == 8
    for name, p, _ in ec.case_points("nowrap"):
        assert _alone(p, ec.MODELS["nowrap"], 4) == _alone(p, ec.MODELS["nowrap"], 0), name
        assert _alone(p, ec.MODELS["nowrap"], 7) == _alone(p, ec.MODELS["nowrap"], 3), name
    # "turned" (theta from -pi + 2, full circle): theta_est = -pi + 1 lies 1 rad BELOW theta.min, which is 2 pi - 1 = 10.09 columns above
    # it: lost without the flag, column 10 with floor + wrap (floor(-1.91 + 0.5) = -2, + 12), column 11 with truncation + wrap (-1 + 12)
    turned = ec.MODELS["turned"]
    p = ec.aim(-0.1, -math.pi + 1, 2.0)                   # (row 1: phi = -0.1)
    assert ec.period(turned) == 12 == turned[5]
    assert [_alone(p, turned, fl)[0] for fl in (0, 2, 4, 6, 7, 15)] == [OUT, OUT, 1 * 12 + 11, 1 * 12 + 10, 1 * 12 + 10, 1 * 12 + 10]
    wrapped = [e for n, _, e in ec.case_points("turned") if n.startswith("own") and set(e) in ({6}, {7, 15}) and next(iter(e.values())) % 12 >= 9]
    assert len(wrapped) >= 3 * 4 * 2 * 3                  # columns 9 to 11 of every row are reached through the negative-id branch only
    # poles: rows 6 / 2 by the reference's rule (atan2(2, 2) = pi/4), rows 8 / 0 by true elevation; theta = atan2(+0, +0) = 0: column 4
    assert [_alone((0.0, 0.0, z), poles, fl)[0] for z in (2.0, -2.0) for fl in (0, 7)] == [6 * 8 + 4, 8 * 8 + 4, 2 * 8 + 4, 0 * 8 + 4]
    # the origin: range 0, stored only where range.min is 0, as the bytes 00 00 00 00; (-0, -0, -0) has theta = -pi: column 0
    for p, cell in (((0.0, 0.0, 0.0), 2 * 8 + 4), ((-0.0, -0.0, -0.0), 2 * 8 + 0)):
        assert _alone(p, tiny, 0)[0] == IMG
        got, r = _alone(p, zmin, 0)
        assert got == cell and r.tobytes() == b"\0\0\0\0"
    # at buffer index 0 the default key is (0 + 1) << 32 | 0 and the nearest key 0 << 32 | 0: neither is its rule's "nobody"
    assert ec.case_points("zero_min")[0][0] == "origin(+0)"


@pytest.mark.parametrize("model", ["tiny", "zero_min", "odd"])
def test_range_bounds_overflow_and_subnormals(model):
    m = ec.MODELS[model]
    for label, r, inside in ec.bound_values(m):
        r = f32(r)
        # the chosen values survive square and root -- but for the float above a range.min of 0: its square is 0, so is its range
        survives = not (m[6] == 0 and label == "rmin+")
        assert (np.sqrt(r * r) == r) if survives else (r > 0 and np.sqrt(r * r) == 0), label
        got, stored = _alone((r, 0.0, 0.0), m, 0)
        assert (got >= 0) == inside and (not inside or stored == (r if survives else 0)), label
    # (3e38, 3e38, 0): finite, range inf: in the image (theta = pi/4, phi = atan2(0, inf) = 0), not in range
    res = pr.bin_points(np.array([[3e38, 3e38, 0]], f32), *m)
    assert res["stats"] == dict(n_points=1, n_finite=1, n_in_image=1, n_in_range=0, n_cells_filled=0)
    # ... and with a translation of 1 m the finite test still sees the FIELDS
    res = pr.bin_points(np.array([[3e38, 3e38, 0]], f32), *m, T=translation_1m())
    assert res["stats"]["n_finite"] == 1 and res["stats"]["n_in_range"] == 0
    # ... and even where T * p is no longer finite (a quarter turn about z: y' = 3e38 * sqrt(2))
    turned = translation_1m()
    turned["R"]["z"], turned["R"]["w"] = math.sin(math.pi / 8), math.cos(math.pi / 8)
    with np.errstate(all="ignore"):
        assert not np.isfinite(pr.apply_transform(turned, np.array([[3e38, 3e38, 0]], f32))).all()
    res = pr.bin_points(np.array([[3e38, 3e38, 0]], f32), *m, T=turned)
    assert res["stats"] == dict(n_points=1, n_finite=1, n_in_image=0, n_in_range=0, n_cells_filled=0)
    # squares that are subnormal / zero
    x = f32(1e-20)
    assert 0 < x * x < np.finfo(f32).tiny and abs(float(np.sqrt(x * x)) / 1e-20 - 1) < 1e-3
    assert f32(1e-42) > 0 and f32(1e-42) * f32(1e-42) == 0
    got, stored = _alone((1e-20, 0.0, 0.0), m, 0)
    if m[6] == 0:
        assert got >= 0 and stored == np.sqrt(x * x) and stored != 0
        got, stored = _alone((1e-42, 0.0, 0.0), m, 0)
        assert got >= 0 and stored.tobytes() == b"\0\0\0\0"
    else:
        assert got == IMG


def translation_1m():
    T = np.zeros(1, np.dtype([("R", [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")]), ("t", [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]),
                              ("stamp", "<u4")]))
    T["R"]["w"] = 1.0
    T["t"]["x"] = 1.0
    return T


def test_float64_records_cast_as_named():
    xyz, want = ec.f64_cloud("tiny")
    data, lay = pr.make_cloud(ec.REC29, xyz)
    assert lay["point_step"] == 29 and lay["offset_x"] == 3 and lay["datatype"] == pr.FLOAT64
    got = pr.xyz_from_bytes(data, **lay)
    k = len(ec.F64_VALUES)
    assert got[:k, 0].tobytes() == want.astype(f32).tobytes()
    assert np.isinf(got[0, 0]) and got[1, 0] == np.finfo(f32).max and np.isinf(got[2, 0]) and np.isinf(got[3, 0])
    assert 0 < got[4, 0] < np.finfo(f32).tiny and got[5, 0] == 1 and got[6, 0] == f32(1 + 2.0 ** -22) and got[7, 0] == f32(1 + 2.0 ** -23)
    res = pr.bin_points(got[:k], *ec.MODELS["tiny"])
    # inf x: skipped; FLT_MAX: finite, its square overflows; 1e-40: finite, range 0 < range.min; the three near 1: stored
    assert list(res["fin"]) == [False, True, False, False, True, True, True, True]
    assert list(res["inimg"]) == [False, True, False, False, True, True, True, True] and list(res["ok"]) == [False] * 5 + [True] * 3
    # the widened case points are no floats: the cast rounds
    assert (xyz[k:].astype(f32).astype(np.float64) != xyz[k:])[np.isfinite(xyz[k:])].mean() > 0.5


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("order", ["asc", "desc", "tail"])
@pytest.mark.parametrize("model", ["odd", "tiny"])
def test_winner_rule(model, order, two):
    m = ec.MODELS[model]
    xyz, winners = ec.winner_cloud(model, order, two_cells=two)
    n = len(xyz)
    assert len(winners) == (2 if two else 1)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(invalid="ignore"):
        r = np.sqrt((x * x + y * y) + z * z).astype(f32)
    last, near = pr.bin_points(xyz, *m, flags=0), pr.bin_points(xyz, *m, flags=pr.NEAREST)
    for k, (cell, w_last, w_near) in enumerate(winners):
        rivals = np.nonzero(last["cell"] == cell)[0]
        slots = sorted((s + k if s in (0, 64, 256) else s - k) % n for s in ec.RIVAL_SLOTS)
        assert list(rivals) == (slots[:4] if order == "tail" else slots)
        assert {i // 64 for i in slots} == {0, 1, 3, 4} and {i // 256 for i in slots} == {0, 1}    # four waves, two workgroups
        assert w_last == rivals.max() and last["ranges"][cell] == r[w_last]
        assert near["ranges"][cell] == r[w_near] == r[rivals].min()
        if order == "asc" and k == 0 or order == "desc" and k == 1:
            assert w_last != w_near and r[w_last] > r[w_near]        # the largest index wins although it is not the nearest
        if order == "tail":
            assert w_last == slots[3] and np.isnan(xyz[slots[4]]).any() and r[slots[5]] > m[7]


def test_ulp_condition_holds_for_every_point_the_gpu_tests_use():
    """a point whose double atan2, moved by +-4 double ulps, casts to a float that falls into another cell would make byte parity depend
    on the last bits of the device's atan2: there must be none (a failing point is to be REPLACED here, never excused on the GPU)"""
    checked = 0
    for model in ec.MODEL_ORDER:
        m = ec.MODELS[model]
        clouds = [ec.edge_cloud(model), ec.edge_cloud(model, 1025), ec.f64_cloud(model)[0].astype(f32)]
        clouds += [ec.winner_cloud(model, o, two_cells=t)[0] for o in ("asc", "desc", "tail") for t in (False, True) if model in ("odd", "tiny")]
        for xyz in clouds:
            for flags in ec.FLAGS:
                ok = ec.ulp_condition(xyz, m, flags)
                assert ok.all(), "%s flags %d: points %s change their cell within %d ulps" % (model, flags, np.nonzero(~ok)[0][:5], ec.ULPS)
                checked += len(ok)
    assert checked > 50000
    # the check can fail: a point a hair's breadth from a cell edge
    m = ec.MODELS["tiny"]
    th = -math.pi + 2.501 * float(m[4])
    near_edge = np.array([[2 * math.cos(th), 2 * math.sin(th), 0]])
    assert ec.ulp_condition(near_edge, m, 0).all() and not ec.ulp_condition(near_edge, m, 0, ulps=1 << 44).all()


def test_record_layouts_and_truncations():
    pts = ec.edge_cloud("tiny", 1025)
    k = len(ec.case_points("tiny"))
    assert len(pts) == 1025 and 257 < k < 1025 < len(ec.case_points("odd"))
    assert pr.bin_points(pts[k:], *ec.MODELS["tiny"])["stats"]["n_in_range"] == 1025 - k        # the padding is inside image and range
    pts = ec.edge_cloud("odd", 1025)
    for n in (1, 63, 64, 65, 255, 256, 257):
        assert ec.edge_cloud("odd", n).tobytes() == ec.edge_cloud("odd")[:n].tobytes()
    data, lay = pr.make_cloud(ec.REC13, pts)
    assert (lay["point_step"], lay["offset_x"], lay["offset_y"], lay["offset_z"]) == (13, 8, 4, 0)
    assert pr.xyz_from_bytes(data, **lay).tobytes() == pts.tobytes()
    cut = ec.cut_to_last_coordinate(data, lay)
    assert len(cut) == len(data) - 1 and pr.xyz_from_bytes(cut, **lay).tobytes() == pts.tobytes()
    with pytest.raises(ValueError):
        pr.xyz_from_bytes(cut[:-1], **lay)
    org = ec.edge_cloud("odd", 37 * 28)
    data, lay = pr.make_cloud(ec.REC12, org, height=28, row_pad=5)
    assert lay["width"] == 37 and lay["row_step"] == 37 * 12 + 5 and pr.xyz_from_bytes(data, **lay).tobytes() == org.tobytes()
    assert len(ec.cut_to_last_coordinate(data, lay)) == len(data) - 5


def test_down_model_counts_rows_from_the_top():
    """phi.min > 0 with phi.inc < 0: (est - min) / inc is positive below phi.min -- row 0 is the TOP row, nothing is refused"""
    m = ec.MODELS["down"]
    for v in range(6):
        p = ec.aim(0.5 - 0.2 * v, 0.3, 2.0)
        assert _alone(p, m, 0)[0] // 12 == v and _alone(p, m, 2)[0] // 12 == v
    assert _alone(ec.aim(0.66, 0.3, 2.0), m, 0)[0] // 12 == 0 and _alone(ec.aim(0.66, 0.3, 2.0), m, 2)[0] == OUT


def test_spherical_table_is_close_to_numpys():
    """the libm table (bits may differ from numpy's float32 trig in the last place; that is why the GPU tests use this one)"""
    for model in ("odd", "poles"):
        m = ec.MODELS[model]
        d = ec.spherical_dirs(m)
        assert np.abs(d - pr.model_dirs(*m[:6])).max() < 3e-7
        pts, mask = ec.dataset_of(np.full(m[2] * m[5], 2.0, f32), m)
        assert mask.all() and pts.tobytes() == (d * f32(2.0)).tobytes()
    assert not ec.dataset_of(np.array([11.0], f32), ec.MODELS["one"])[1].any()


# ---- segmentation: the float32 restatement against the float64 rule ---------------------------------------------------------------------
@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("thr", [(0.15, 0.15), (0.10, 0.30)])
def test_segment_f32_agrees_with_the_float64_rule_away_from_its_thresholds(orc, thr, flag):
    from rmcl_amd import synthetic as syn, types as T
    (mv, mf), (rv, rf), model, Tsb, truth, est = sr.cube_scene(syn, T)
    dirs = syn.model_directions(model)
    orig = np.array([0.05, -0.02, 0.4], f32)
    rng = (model.range.min, model.range.max)
    real = orc.Mesh(rv, rf).simulate_o1dn(32, 32, rng[0], rng[1], orig, dirs, Tsb, truth, bvh=False, want=("ranges",))["ranges"]
    real = sr.invalidate_some(sr.doctor_cube_scan(real), rng[1], 0.05)
    sim = orc.Mesh(mv, mf).simulate_o1dn(32, 32, rng[0], rng[1], orig, dirs, Tsb, est, bvh=False, want=("ranges", "normals"))
    kw = dict(min_dist_outlier_scan=thr[0], min_dist_outlier_map=thr[1], pint_with_origin=flag)
    ref = sr.segment(real, sim["ranges"], sim["normals"], dirs, orig, rng[0], rng[1], **kw)
    und = sr.undecided(real, sim["ranges"], sim["normals"], dirs, orig, rng[0], rng[1], **kw)
    got = sr.segment_f32(real, sim["ranges"], sim["normals"], dirs, orig, rng[0], rng[1], add_origin=True, **kw)
    assert und.sum() < 0.01 * len(real) and np.bincount(ref["labels"], minlength=4)[1:].min() >= 10
    assert np.array_equal(got["labels"][~und], ref["labels"][~und])
    if not und.any():
        for k in ("outlier_scan", "outlier_map"):
            assert got[k].dtype == f32 and np.allclose(got[k], ref[k], rtol=1e-6, atol=1e-6), k
    # without an origin (spherical, pinhole) the flag changes nothing
    a = sr.segment_f32(real, sim["ranges"], sim["normals"], dirs, orig, rng[0], rng[1], add_origin=False, **kw)
    b = sr.segment_f32(real, sim["ranges"], sim["normals"], dirs, np.zeros(3), rng[0], rng[1], add_origin=True, **kw)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("labels", "outlier_scan", "outlier_map"))
    # the pinhole directions against the oracle's
    pd = sr.pinhole_dirs_f32(40, 30, 18.0, 18.0, 19.5, 14.5)
    assert np.abs(pd - orc.pinhole_directions(40, 30, (18.0, 18.0), (19.5, 14.5))).max() < 2e-7
