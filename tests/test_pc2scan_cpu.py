"""PointCloud2 -> spherical scan, CPU side: tests/pc2scan_ref.py (the yardstick of tests/test_gpu_pc2scan.py) pinned by hand cases for
each statement of Pc2ToScanNode::convert (pc2_to_scan.cpp:105-213), by a plain sequential loop, by the committed fixture
tests/golden/g9_pc2scan.npz and by the round trip dir(vid, hid) * r -> bin on the C1 and C2 models."""
import math
import os
import subprocess

import numpy as np
import pytest

import pc2scan_ref as pr

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_pc2scan.npz")
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("time", "<f4")])   # 22 B, unaligned
REC64 = np.dtype([("pad", "<u4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8")])                                          # 28 B

# a small model whose cells are easy to aim at: 3 rows at phi = -0.4, 0, 0.4 rad, 8 columns from theta = -pi in steps of pi / 4
SMALL = (f32(-0.4), f32(0.4), 3, f32(-math.pi), f32(math.pi / 4), 8, f32(0.5), f32(10.0))
EMPTY = f32(11.0)


def _pt(phi, theta, r):
    """a point whose REFERENCE angles are (phi, theta): phi_est = atan2(z, range) = atan(sin(elevation))"""
    el = math.asin(math.tan(phi))
    return [r * math.cos(el) * math.cos(theta), r * math.cos(el) * math.sin(theta), r * math.sin(el)]


def _bin(pts, flags=0, model=SMALL, T=None):
    return pr.bin_points(np.asarray(pts, f32).reshape(-1, 3), *model, flags=flags, T=T)


def test_empty_cells_hold_range_max_plus_one_and_an_empty_cloud_is_all_empty():
    res = _bin(np.zeros((0, 3)))
    assert res["ranges"].shape == (24,) and (res["ranges"] == EMPTY).all()
    assert res["stats"] == dict(n_points=0, n_finite=0, n_in_image=0, n_in_range=0, n_cells_filled=0)
    res = _bin([_pt(0.0, 0.0, 2.0)])
    assert res["ranges"][1 * 8 + 4] == f32(2.0) and (np.delete(res["ranges"], 12) == EMPTY).all()
    # the value is (float)((double)range.max + 1.0): for a range.max where that is not range.max + 1 in float it still is what the cast gives
    big = SMALL[:7] + (f32(3e8),)
    assert _bin(np.zeros((0, 3)), model=big)["empty"] == f32(np.float64(f32(3e8)) + 1.0) == f32(3e8)


def test_last_point_wins_and_an_out_of_range_later_point_does_not_overwrite():
    a, b, far, near = _pt(0.0, 0.1, 2.0), _pt(0.05, 0.0, 3.0), _pt(0.0, 0.0, 50.0), _pt(0.0, 0.0, 0.2)
    assert _bin([a, b])["ranges"][12] == f32(np.sqrt(f32(b[0]) ** 2 + f32(b[1]) ** 2 + f32(b[2]) ** 2)) and abs(_bin([a, b])["ranges"][12] - 3.0) < 1e-6
    assert abs(_bin([b, a])["ranges"][12] - 2.0) < 1e-6
    res = _bin([a, far, near])                      # :201 -- the range test guards the store, the cell keeps the earlier point
    assert abs(res["ranges"][12] - 2.0) < 1e-6
    assert res["stats"] == dict(n_points=3, n_finite=3, n_in_image=3, n_in_range=1, n_cells_filled=1)
    # NEAREST: the smallest range whatever the order; ties go to the smaller index (the same value either way)
    for order in ([a, b], [b, a], [b, a, b]):
        assert abs(_bin(order, pr.NEAREST)["ranges"][12] - 2.0) < 1e-6
    # the bounds are inside (Interval::inside is <= on both sides)
    assert _bin([[0.5, 0, 0]])["stats"]["n_in_range"] == 1 and _bin([[10.0, 0, 0]])["stats"]["n_in_range"] == 1


def test_nan_and_inf_are_skipped():
    good = _pt(0.0, 0.0, 2.0)
    pts = [good, [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan, np.nan, np.nan]]
    res = _bin(pts)
    assert res["stats"] == dict(n_points=5, n_finite=1, n_in_image=1, n_in_range=1, n_cells_filled=1)
    assert (res["ranges"] != EMPTY).sum() == 1
    # finite fields whose transform overflows: counted finite (:186 tests x, y, z), rejected by the NaN angles / inf range
    T = np.zeros(1, np.dtype([("R", [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")]), ("t", [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]), ("stamp", "<u4")]))
    T["R"]["w"] = 1.0
    T["t"]["x"] = 3e38
    res = _bin([[3e38, 0, 0]], T=T)
    assert res["stats"]["n_finite"] == 1 and res["stats"]["n_in_range"] == 0


def test_truncation_takes_minus_one_cells_into_cell_zero_and_floor_does_not():
    # phi_est = -0.72 rad: q = -0.8, q + 0.5 = -0.3 -> (int) 0, floor -1: every q in (-1.5, -0.5) lands in cell 0 by default
    low = _pt(-0.72, 0.0, 2.0)
    res = _bin([low])
    assert res["stats"]["n_in_image"] == 1 and abs(res["ranges"][0 * 8 + 4] - 2.0) < 1e-6
    res = _bin([low], pr.FLOOR)
    assert res["stats"]["n_in_image"] == 0 and (res["ranges"] == EMPTY).all()
    # the theta axis likewise: theta just below theta.min cannot occur for -pi, so use a model that starts at 0
    m = (f32(-0.4), f32(0.4), 3, f32(0.0), f32(math.pi / 4), 4, f32(0.5), f32(10.0))
    left = _pt(0.0, -0.8 * math.pi / 4, 2.0)
    assert abs(_bin([left], model=m)["ranges"][1 * 4 + 0] - 2.0) < 1e-6
    assert _bin([left], pr.FLOOR, model=m)["stats"]["n_in_image"] == 0
    # above the last cell nothing differs: q + 0.5 = size + 0.2 is outside either way; size - 0.3 is the last cell either way
    assert _bin([_pt(0.0, 3.7 * math.pi / 4, 2.0)], model=m)["stats"]["n_in_image"] == 0
    assert _bin([_pt(0.0, 3.2 * math.pi / 4, 2.0)], model=m)["ranges"][1 * 4 + 3] != EMPTY


def test_the_first_column_of_a_model_from_minus_pi_is_lost_unless_theta_wraps():
    # dir(vid = 1, hid = 0) of SMALL points along -x: atan2(+-0, -x) = +-pi.  y = +0 gives +pi: q = 8, outside (:196-199)
    back = [-2.0, 0.0, 0.0]
    res = _bin([back])
    assert res["stats"]["n_in_image"] == 0
    res = _bin([back], pr.WRAP_THETA)
    assert res["stats"]["n_in_image"] == 1 and res["ranges"][1 * 8 + 0] == f32(2.0)
    # y = -0 gives -pi: column 0 with or without the wrap; a point a little before +pi rounds up to id 8 and wraps to 0 as well
    assert _bin([[-2.0, -0.0, 0.0]])["ranges"][8] == f32(2.0)
    almost = _pt(0.0, math.pi - 0.1, 2.0)
    assert _bin([almost])["stats"]["n_in_image"] == 0 and _bin([almost], pr.WRAP_THETA)["ranges"][8] != EMPTY
    # no wrap when the circle is not a whole number of columns
    odd = SMALL[:4] + (f32(0.8), 8) + SMALL[6:]
    assert _bin([[-2.0, 0.0, 0.0]], pr.WRAP_THETA, model=odd)["stats"]["n_in_image"] == 0


def test_true_elevation_is_the_inverse_of_the_models_direction():
    # the edge between rows 1 and 2 lies at phi = 0.2.  Elevation 0.202: the reference computes atan(sin(0.202)) = 0.1980 -> q + 0.5 =
    # 1.995 -> row 1; the true elevation gives 2.005 -> row 2, the row whose direction dir(2, hid) is the nearest to the point
    el = 0.202
    p = [2.0 * math.cos(el), 0.0, 2.0 * math.sin(el)]
    assert _bin([p])["cell"][0] == 1 * 8 + 4 and _bin([p], pr.TRUE_ELEVATION)["cell"][0] == 2 * 8 + 4


def test_zero_increment_needs_size_one():
    flat = (f32(0.0), f32(0.0), 1, f32(-math.pi), f32(math.pi / 4), 8, f32(0.5), f32(10.0))    # the 2-D scanner of scan_to_scan.cpp:92-94
    res = _bin([_pt(0.3, 0.0, 2.0), _pt(-0.6, math.pi / 2, 3.0)], model=flat)
    assert res["stats"]["n_in_image"] == 2 and res["ranges"][4] != EMPTY and res["ranges"][6] != EMPTY
    with pytest.raises(ValueError):
        _bin([[1, 0, 0]], model=(f32(0.0), f32(0.0), 2) + flat[3:])
    with pytest.raises(ValueError):
        _bin([[1, 0, 0]], flags=16)


def test_float64_fields_row_padding_and_layout_errors():
    rng = np.random.RandomState(3)
    p = rng.uniform(-5, 5, (24, 3))
    p[3, 0] = 1e300                                                   # finite as a double, inf as a float: skipped
    with np.errstate(over="ignore"):
        p32 = p.astype(f32)
    p32[3, 0] = 1.0
    d32, l32 = pr.make_cloud(REC, p32)
    d64, l64 = pr.make_cloud(REC64, p, height=4, row_pad=10)
    assert l32["point_step"] == 22 and l64["row_step"] == 6 * 28 + 10 and l64["datatype"] == 8
    x64 = pr.xyz_from_bytes(d64, **l64)
    assert np.isinf(x64[3, 0]) and np.array_equal(np.delete(x64, 3, 0), np.delete(p32, 3, 0))
    a, b = pr.convert(d32, model=SMALL, **l32), pr.convert(d64, model=SMALL, **l64)
    assert a["stats"]["n_finite"] == 24 and b["stats"]["n_finite"] == 23
    keep = pr.bin_points(np.delete(p32, 3, 0), *SMALL)
    assert b["ranges"].tobytes() == keep["ranges"].tobytes()
    with pytest.raises(ValueError):
        pr.xyz_from_bytes(d64[:-11], **l64)                           # the last point's z is cut (the padding behind it may be missing)
    assert len(pr.xyz_from_bytes(d64[:-10], **l64)) == 24
    with pytest.raises(ValueError):
        pr.xyz_from_bytes(d32, **dict(l32, datatype=2))


def _sequential(xyz, model, flags):
    """the node's loop as it stands (pc2_to_scan.cpp:160-210), one point after the other, with Python scalars"""
    phi_min, phi_inc, H, th_min, th_inc, W, rmin, rmax = model
    ranges = np.full(H * W, f32(np.float64(rmax) + 1.0), f32)
    for p in xyz:
        x, y, z = (f32(v) for v in p)
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            continue
        r = f32(np.sqrt(f32(f32(x * x) + f32(y * y)) + f32(z * z)))
        th = f32(math.atan2(float(y), float(x)))
        den = f32(np.sqrt(f32(f32(x * x) + f32(y * y)))) if flags & pr.TRUE_ELEVATION else r
        ph = f32(math.atan2(float(z), float(den)))
        cp, ct = float(f32(f32(ph - phi_min) / phi_inc)) + 0.5, float(f32(f32(th - th_min) / th_inc)) + 0.5
        pi, ti = (math.floor(cp), math.floor(ct)) if flags & pr.FLOOR else (int(cp), int(ct))
        if flags & pr.WRAP_THETA:
            P = round(2 * math.pi / float(th_inc))
            ti = ti - P if ti >= W else ti + P if ti < 0 else ti
        if 0 <= pi < H and 0 <= ti < W and rmin <= r <= rmax:
            c = pi * W + ti
            if not flags & pr.NEAREST or ranges[c] == f32(np.float64(rmax) + 1.0) or r < ranges[c]:
                ranges[c] = r
    return ranges


def test_golden_fixture_and_the_sequential_loop():
    from rmcl_amd import synthetic as syn
    g = np.load(GOLDEN)
    lay = dict(zip(("width", "height", "point_step", "row_step", "offset_x", "offset_y", "offset_z", "datatype"), (int(v) for v in g["layout"])))
    assert lay["point_step"] == 22 and lay["height"] == 1
    mt = pr.model_tuple(syn.model_c1())
    xyz = pr.xyz_from_bytes(g["data"].tobytes(), **lay)
    names = ("n_points", "n_finite", "n_in_image", "n_in_range", "n_cells_filled")
    for fl in (0, 7, 8):
        res = pr.convert(g["data"].tobytes(), model=mt, flags=fl, **lay)
        assert res["ranges"].tobytes() == g["ranges_%d" % fl].tobytes(), fl
        assert [res["stats"][k] for k in names] == [int(v) for v in g["stats_%d" % fl]], fl
        assert res["stats"]["n_cells_filled"] == int((res["ranges"] != res["empty"]).sum())
        assert _sequential(xyz, mt, fl).tobytes() == res["ranges"].tobytes(), fl
    assert g["ranges_0"].tobytes() != g["ranges_7"].tobytes() and g["ranges_0"].tobytes() != g["ranges_8"].tobytes()
    assert _sequential(xyz, mt, 15).tobytes() == pr.bin_points(xyz, *mt, flags=15)["ranges"].tobytes()


@pytest.mark.parametrize("name,own_default", [("c1", 0.484), ("c2", 0.468)])
def test_round_trip_of_the_models_own_directions(name, own_default):
    """dir(vid, hid) * r, shuffled, binned: the reference's rule finds under half of the points in their own cell (atan2(z, range) is
    not the elevation; the hid = 0 column falls out), the corrected one all of them, also with the points moved +-0.3 cell in angle"""
    from rmcl_amd import synthetic as syn
    mt = pr.model_tuple(syn.model_c1() if name == "c1" else syn.model_c2())
    H, W = mt[2], mt[5]
    rng = np.random.RandomState(5)
    for jitter in (0.0, 0.3):
        d = pr.model_dirs(*mt[:6], jitter=jitter, rng=rng)
        rr = rng.uniform(1, 50, H * W).astype(f32)
        pts = (d * rr[:, None]).astype(f32)
        perm = rng.permutation(H * W)
        res = pr.bin_points(pts[perm], *mt, flags=7)
        assert (res["cell"] == perm).all()
        assert res["stats"]["n_cells_filled"] == H * W
        assert np.abs(res["ranges"] - rr).max() / 1.0 <= 50 * 4e-7 and (np.abs(res["ranges"] - rr) / rr).max() < 1e-6
        if jitter == 0.0:
            res0 = pr.bin_points(pts[perm], *mt, flags=0)
            own = (res0["cell"] == perm).mean()
            assert abs(own - own_default) < 0.01, own
            assert res0["stats"]["n_in_image"] == H * W - H           # the hid = 0 column computes theta_est = +pi
    pts_d, mask = pr.dataset(res["ranges"], mt)
    assert mask.all() and pts_d.shape == (H * W, 3)


def test_edge_cells_rule():
    """a point 5e-5 cell widths from a phi edge marks the cells on both sides of that edge and no other"""
    q = 1.5 - 5e-5                                                     # q + 0.5 just below 2: row 1, the edge to row 2
    p = _pt(float(SMALL[0]) + q * float(SMALL[1]), 0.0, 2.0)
    res = _bin([p, _pt(0.0, math.pi / 2, 3.0)])
    assert res["cell"][0] == 1 * 8 + 4
    out, n = pr.edge_cells(res, 8, 3)
    assert n == 1 and sorted(np.nonzero(out)[0]) == [1 * 8 + 4, 2 * 8 + 4]


def test_cpp_example_compiles_without_gpu_and_the_adapter_is_spherical_only(ra, tmp_path):
    import os
    from test_cpp_adapters import ROOT, _build
    exe = _build(tmp_path, "pc2_to_scan_cpp_example.cpp")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    src = tmp_path / "o1dn.cpp"
    body = '#include "rmcl_hip/rmcl_hip.hpp"\nvoid f(rmcl_hip::%s& r, const rmclhip_pointcloud2_layout& l) { r.setInputPointCloud2(nullptr, 0, l); }\nint main() { return 0; }\n'
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)]
    src.write_text(body % "RCCHipSpherical")
    subprocess.check_call(cmd)
    src.write_text(body % "RCCHipO1Dn")
    bad = subprocess.run(cmd, capture_output=True, text=True)
    assert bad.returncode != 0 and "RCCHipSpherical only" in bad.stderr
