"""GPU parity: spherical scans from unordered PointCloud2 bytes on the device (rmclhip_pointcloud2_to_scan,
rmclhip_rcc_set_input_pointcloud2_scan; RCCHipSpherical.setInputPointCloud2, wire.pointcloud2_to_scan) -- the reference's
Pc2ToScanNode::convert (rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213) and the four switches that correct it.

The expected images come from tests/pc2scan_ref.py (numpy; pinned on the CPU by tests/test_pc2scan_cpu.py and a committed fixture).
Without a transform every step is the same IEEE operation in the same order on both sides (-ffp-contract=off, correctly rounded float
divide and sqrt, atan2 in double rounded to float), so images and counts are compared BYTE FOR BYTE.  With a transform the library's
T * p and numpy's may differ in the last bit, which can move a point that sits on a cell edge; test 3 states the rule for that.
"""
import ctypes as C
import math
import struct
import subprocess

import numpy as np
import pytest

import pc2scan_ref as pr

pytestmark = pytest.mark.gpu

f32 = np.float32
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("time", "<f4")])  # 22 B, unaligned
REC64 = np.dtype([("pad", "<u4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8")])                                      # 28 B
STAT_NAMES = ("n_points", "n_finite", "n_in_image", "n_in_range", "n_cells_filled")
_cache = {}


def _model(name):
    from rmcl_amd import synthetic as syn
    return syn.model_c1() if name == "c1" else syn.model_c2()


def _random_cloud():
    if "cloud" not in _cache:
        _cache["cloud"] = pr.random_cloud(400000, seed=5)
    return _cache["cloud"]


def _bytes(rec, organised):
    """the 400 000-point cloud as PointCloud2 bytes: unorganised (height 1), or 250 rows with 6 bytes of padding behind each"""
    key = (rec.itemsize, organised)
    if key not in _cache:
        p = _random_cloud()
        if rec is REC64:
            # doubles that are no floats: the cast to float has to round
            with np.errstate(invalid="ignore"):
                p = p.astype(np.float64) * (1.0 + 1e-9 * np.arange(1, 4)[None, :])
        _cache[key] = pr.make_cloud(rec, p, height=250 if organised else 1, row_pad=6 if organised else 0, seed=1)
    return _cache[key]


def _fnv(buf):
    h = 1469598103934665603
    for b in bytes(buf):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _write_mesh(path, v, f):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())


# ---- 1: bit parity without a transform ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name", ["c1", "c2"])
@pytest.mark.parametrize("organised", [False, True])
@pytest.mark.parametrize("rec", [REC, REC64], ids=["rec22", "rec64"])
def test_image_and_counts_equal_the_restatement_byte_for_byte(ra, ctx, rec, organised, model_name):
    data, lay = _bytes(rec, organised)
    model = _model(model_name)
    xyz = pr.xyz_from_bytes(data, **lay)
    for flags in (0, 7, 8, 15):
        ref = pr.bin_points(xyz, *pr.model_tuple(model), flags=flags)
        got, stats = ra.wire.pointcloud2_to_scan(ctx, data, model=model, flags=flags, **lay)
        print("flags %2d %s: %s" % (flags, model_name, stats))
        assert stats == ref["stats"], (flags, stats, ref["stats"])
        diff = got.reshape(-1).view(np.uint32) != ref["ranges"].view(np.uint32)
        assert not diff.any(), "flags %d: %d of %d cells differ (first: cell %d, %r vs %r)" % (
            flags, diff.sum(), diff.size, np.argmax(diff), got.reshape(-1)[np.argmax(diff)], ref["ranges"][np.argmax(diff)])
    # many points per cell: the winner rule is exercised
    assert ref["stats"]["n_in_range"] > 2.5 * ref["stats"]["n_cells_filled"]


def test_device_source_and_device_destination(ra, ctx):
    data, lay = _bytes(REC, False)
    model = _model("c2")
    want, wstats = ra.wire.pointcloud2_to_scan(ctx, data, model=model, flags=7, **lay)
    d_raw = ra.DeviceArray.from_host(ctx, np.frombuffer(data, np.uint8))
    d_out = ra.DeviceArray.from_host(ctx, np.full(want.size + 64, -7.0, f32))
    stats = ra.wire.pointcloud2_to_scan(ctx, d_raw, model=model, flags=7, device=True, nbytes=len(data), into=d_out, **lay)
    out = d_out.download()
    assert stats == wstats and out[:want.size].tobytes() == want.tobytes()
    assert (out[want.size:] == f32(-7.0)).all()            # nothing is written beyond the image


# ---- 2: the operator path -----------------------------------------------------------------------------------------------------------
def _room(orc, ra, ctx, meshes):
    if "room" not in _cache:
        from rmcl_amd import synthetic as syn, types as T
        v, f = meshes("room30k")
        # a pose whose hits all lie inside the range interval of both models (nearest surface 0.35 m away): the simulator reports a hit
        # below range.min as a hit, the binning rule does not store it
        truth = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
        _cache["room"] = dict(v=v, f=f, mesh=orc.Mesh(v, f), truth=truth, est=T.mult(truth, syn.pose_c2_perturbation()), sims={})
    return _cache["room"]


def _sim(room, model_name):
    """the room seen from the true pose (Tsb = identity): ranges, points (NaN where the scan missed), hits"""
    from rmcl_amd import types as T
    if model_name not in room["sims"]:
        room["sims"][model_name] = room["mesh"].simulate_spherical(_model(model_name), T.identity(), room["truth"], bvh=True)
    return room["sims"][model_name]


def _hit_cloud(sim, seed=3):
    """the hit points in a random order, as an unorganised cloud of 22-byte records -> (bytes, layout, permutation of the hit rays)"""
    hit = np.nonzero(sim["hits"] > 0)[0]
    perm = np.random.RandomState(seed).permutation(hit)
    data, lay = pr.make_cloud(REC, sim["points"][perm].astype(f32), seed=seed)
    return data, lay, perm


def _operator(ra, ctx, room, model_name, max_dist=0.5):
    from rmcl_amd import types as T
    hm = room.setdefault("hm", None) or ra.import_hip_map(ctx, room["v"], room["f"])
    room["hm"] = hm
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(_model(model_name))
    rcc.params.max_dist = max_dist
    return rcc


@pytest.mark.parametrize("flags", [0, 7])
def test_operator_input_equals_model_plus_dataset_from_the_restatements_image(ra, orc, ctx, meshes, flags):
    from rmcl_amd import types as T
    room = _room(orc, ra, ctx, meshes)
    data, lay, _ = _hit_cloud(_sim(room, "c2"))
    model = _model("c2")
    ref = pr.convert(data, model=model, flags=flags, **lay)
    a, b = _operator(ra, ctx, room, "c2"), _operator(ra, ctx, room, "c2")
    stats = a.setInputPointCloud2(data, flags=flags, **lay)
    nv = b.set_dataset_from_ranges(ref["ranges"])
    assert stats == ref["stats"] and stats["n_cells_filled"] == nv > 1000
    assert a.rangesView().download().tobytes() == ref["ranges"].tobytes()
    outs = []
    for rcc in (a, b):
        rcc.find(room["est"])
        outs.append((rcc.modelView(), rcc.computeCrossStatistics(T.identity())))
    for k in ("hits", "face_ids", "ranges", "points", "normals"):
        assert outs[0][0][k].tobytes() == outs[1][0][k].tobytes(), k
    assert outs[0][1].tobytes() == outs[1][1].tobytes() and int(outs[0][1]["n_meas"]) > 1000
    # the cloud may already live on the device: the same bytes
    d_raw = ra.DeviceArray.from_host(ctx, np.frombuffer(data, np.uint8))
    stats2 = a.setInputPointCloud2(d_raw, flags=flags, device=True, nbytes=len(data), **lay)
    assert stats2 == stats and a.rangesView().download().tobytes() == ref["ranges"].tobytes()
    a.find(room["est"])
    assert a.computeCrossStatistics(T.identity()).tobytes() == outs[1][1].tobytes()
    a.close()
    b.close()


# ---- 3: with a transform ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 7, 8, 15])
def test_with_a_transform_cells_agree_away_from_cell_edges(ra, ctx, flags):
    """Rule (the library's T * p and numpy's may differ in the last bit): a cell is left out of the comparison if, by the restatement, a
    point within 1e-4 of a cell width of a cell edge falls into it or into the cell across that edge -- 1e-4 is five times the 2e-5 cell
    widths one float ulp of position moves an angle in the C2 model.  Everywhere else cells agree exactly in occupancy and to 1e-6
    relative in range; at most 0.5 % of the filled cells may be left out; the counts differ by at most the number of such points."""
    from rmcl_amd import synthetic as syn
    data, lay = _bytes(REC, False)
    model = _model("c2")
    Tsc = syn.tsb_offset()
    ref = pr.convert(data, model=model, flags=flags, T=Tsc, **lay)
    got, stats = ra.wire.pointcloud2_to_scan(ctx, data, model=model, flags=flags, T=Tsc, **lay)
    got = got.reshape(-1)
    H, W = int(model.phi.size), int(model.theta.size)
    skip, n_near = pr.edge_cells(ref, W, H)
    filled_ref, filled_got = ref["ranges"] != ref["empty"], got != ref["empty"]
    share = (skip & filled_ref).sum() / filled_ref.sum()
    exact = int((got.view(np.uint32) == ref["ranges"].view(np.uint32)).sum())
    print("flags %2d: %d points near an edge, %.4f %% of the filled cells left out, %d of %d cells equal bit for bit; stats %s vs %s"
          % (flags, n_near, 100 * share, exact, got.size, stats, ref["stats"]))
    assert share <= 0.005
    keep = ~skip
    assert np.array_equal(filled_got[keep], filled_ref[keep])
    both = keep & filled_ref
    assert (np.abs(got[both].astype(np.float64) - ref["ranges"][both]) <= 1e-6 * ref["ranges"][both]).all()
    assert stats["n_points"] == ref["stats"]["n_points"] and stats["n_finite"] == ref["stats"]["n_finite"]
    for k in ("n_in_image", "n_in_range", "n_cells_filled"):
        assert abs(stats[k] - ref["stats"][k]) <= n_near, k
    # a different image than without the transform (the transform is applied)
    plain, _ = ra.wire.pointcloud2_to_scan(ctx, data, model=model, flags=flags, **lay)
    assert plain.tobytes() != got.tobytes()


# ---- 4: round trip through the real path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name", ["c1", "c2"])
def test_round_trip_of_a_simulated_scan(ra, orc, ctx, meshes, model_name):
    """simulate at a true pose, hand the hit points over as a shuffled unorganised cloud: with the three corrections every hit ray's
    cell holds its simulated range (1e-6 relative: 8 float ulps for normalise, multiply, square and root), every missed ray's cell is
    empty, and correctOnce from the cloud equals correctOnce from the simulated ranges to the project's 1e-5 on the pose.  With the
    reference's rule the image is the restatement's and NOT the simulated one."""
    from rmcl_amd import types as T
    room = _room(orc, ra, ctx, meshes)
    sim = _sim(room, model_name)
    model = _model(model_name)
    data, lay, perm = _hit_cloud(sim)
    hit = sim["hits"] > 0
    empty = f32(np.float64(f32(model.range.max)) + 1.0)
    assert 0 < hit.sum() < hit.size and ((sim["ranges"] == empty) == ~hit).all()
    assert (sim["ranges"][hit] >= f32(model.range.min)).all() and (sim["ranges"][hit] <= f32(model.range.max)).all()
    a = _operator(ra, ctx, room, model_name, max_dist=1.0)
    a.adaptive_max_dist_min = 0.15
    stats = a.setInputPointCloud2(data, flags=7, **lay)
    img = a.rangesView().download()
    assert stats["n_cells_filled"] == int(hit.sum()) == stats["n_in_range"] == stats["n_points"]
    assert (img[~hit] == empty).all()
    rel = np.abs(img[hit].astype(np.float64) - sim["ranges"][hit]) / sim["ranges"][hit]
    print("%s flags 7: max relative range error %.3g over %d hit rays" % (model_name, rel.max(), hit.sum()))
    assert rel.max() <= 1e-6
    b = _operator(ra, ctx, room, model_name, max_dist=1.0)
    b.adaptive_max_dist_min = 0.15
    assert b.set_dataset_from_ranges(sim["ranges"]) == int(hit.sum())
    Ta, sa = a.correct_once(T.identity(), room["est"], 5)
    Tb, sb = b.correct_once(T.identity(), room["est"], 5)
    assert int(sa["n_meas"]) == int(sb["n_meas"]) > 0.5 * hit.sum()
    assert np.allclose([float(Ta["t"][k]) for k in "xyz"], [float(Tb["t"][k]) for k in "xyz"], atol=1e-5)
    qa, qb = (np.array([float(q["R"][k]) for k in "xyzw"]) for q in (Ta, Tb))
    assert np.allclose(qa, qb * np.sign(np.dot(qa, qb)), atol=1e-5)
    # the reference's rule: what the restatement says, and not the scan the cloud came from
    stats0 = a.setInputPointCloud2(data, flags=0, **lay)
    img0 = a.rangesView().download()
    ref0 = pr.convert(data, model=model, flags=0, **lay)
    assert img0.tobytes() == ref0["ranges"].tobytes() and stats0 == ref0["stats"]
    own = float((ref0["cell"] == perm).mean())
    same = float((img0[hit] == img[hit]).mean())
    assert img0.tobytes() != img.tobytes() and own < 1.0 and same < 1.0, \
        "%s flags 0: %.1f %% of the hit rays found in their own cell, %.1f %% of the hit cells hold the same range" % (model_name, 100 * own, 100 * same)
    print("%s flags 0: %.1f %% of the hit rays found in their own cell (flags 7: 100 %%), %.1f %% of the hit cells hold the flags-7 range"
          % (model_name, 100 * own, 100 * same))
    a.close()
    b.close()


# ---- 5: the image stays on the device -----------------------------------------------------------------------------------------------
def test_ranges_view_feeds_segment_without_leaving_the_device(ra, orc, ctx, meshes):
    room = _room(orc, ra, ctx, meshes)
    data, lay, _ = _hit_cloud(_sim(room, "c2"))
    ref = pr.convert(data, model=_model("c2"), flags=7, **lay)
    a, b = _operator(ra, ctx, room, "c2"), _operator(ra, ctx, room, "c2")
    a.setInputPointCloud2(data, flags=7, **lay)
    view = a.rangesView()
    assert view.count == ref["ranges"].size and view.ptr
    dev = a.segment(room["est"], view)
    host = b.segment(room["est"], ref["ranges"])
    assert dev["counts"] == host["counts"] and sum(dev["counts"]) > 100
    for k in ("labels", "outlier_scan", "outlier_map"):
        assert dev[k].tobytes() == host[k].tobytes(), k
    # ... and segment did not disturb the image or the dataset made of it
    assert view.download().tobytes() == ref["ranges"].tobytes()
    a.close()
    b.close()


# ---- 6: the model is left alone -----------------------------------------------------------------------------------------------------
def test_model_stays_and_results_do_not_depend_on_arrival_order(ra, orc, ctx, meshes):
    room = _room(orc, ra, ctx, meshes)
    sim = _sim(room, "c2")
    data, lay, _ = _hit_cloud(sim)
    a = _operator(ra, ctx, room, "c2")
    a.setInputPointCloud2(data, flags=7, **lay)
    shape, variant = a._model_shape, a.find_variant(1)
    a.find(room["est"])
    before = a.modelView()
    a.setInputPointCloud2(data, flags=7, **lay)
    assert a._model_shape == shape and a.find_variant(1) == variant
    a.find(room["est"])
    after = a.modelView()
    assert after["face_ids"].tobytes() == before["face_ids"].tobytes() and after["hits"].tobytes() == before["hits"].tobytes()
    a.close()
    # five calls, five identical images, for the reference's rule and for the nearest rule, on the cloud with many points per cell
    rdata, rlay = _bytes(REC, False)
    model = _model("c2")
    for flags in (0, 8):
        imgs = [ra.wire.pointcloud2_to_scan(ctx, rdata, model=model, flags=flags, **rlay) for _ in range(5)]
        assert all(i[0].tobytes() == imgs[0][0].tobytes() and i[1] == imgs[0][1] for i in imgs[1:]), flags
    # NEAREST does not depend on the buffer order; the reference's last-point-wins does
    p = _random_cloud()
    sh = np.random.RandomState(11).permutation(len(p))
    sdata, slay = pr.make_cloud(REC, p[sh], seed=1)
    near, _ = ra.wire.pointcloud2_to_scan(ctx, rdata, model=model, flags=8, **rlay)
    near_s, _ = ra.wire.pointcloud2_to_scan(ctx, sdata, model=model, flags=8, **slay)
    assert near.tobytes() == near_s.tobytes()
    last, _ = ra.wire.pointcloud2_to_scan(ctx, rdata, model=model, flags=0, **rlay)
    last_s, _ = ra.wire.pointcloud2_to_scan(ctx, sdata, model=model, flags=0, **slay)
    assert last_s.tobytes() == pr.bin_points(p[sh], *pr.model_tuple(model), flags=0)["ranges"].tobytes()
    assert last.tobytes() != last_s.tobytes() and (near <= last).all()


# ---- 7: errors ----------------------------------------------------------------------------------------------------------------------
def test_error_cases_and_the_empty_cloud(ra, orc, ctx, meshes):
    from rmcl_amd import _capi, synthetic as syn, types as T
    L = _capi.lib()
    model = _model("c1")
    n = 64
    p = np.random.RandomState(2).uniform(-5, 5, (n, 3)).astype(f32)
    data, lay = pr.make_cloud(REC, p)
    buf = np.frombuffer(data, np.uint8)
    dp = buf.ctypes.data_as(C.c_void_p)
    out = np.zeros(1024, f32)
    op = out.ctypes.data_as(C.c_void_p)
    st = _capi.Pc2ScanStats()

    def layout(**kw):
        d = dict(lay, **kw)
        return _capi.PointCloud2Layout(*(d[k] for k in ("width", "height", "point_step", "row_step", "offset_x", "offset_y", "offset_z", "datatype")))

    def call(data_p=dp, nbytes=len(data), lay_=None, T_p=None, model_=model, flags=0, out_p=op, null_layout=False, null_model=False):
        lp = None if null_layout else C.byref(lay_ if lay_ is not None else layout())
        mp = None if null_model else C.byref(model_)
        return L.rmclhip_pointcloud2_to_scan(ctx.handle, data_p, nbytes, lp, 0, T_p, mp, flags, out_p, 0, C.byref(st))

    assert call() == _capi.OK and st.n_points == n
    assert call(flags=16) == _capi.ERR_INVALID and b"flag" in L.rmclhip_last_error()
    assert call(null_layout=True) == _capi.ERR_INVALID
    assert call(null_model=True) == _capi.ERR_INVALID
    assert call(data_p=None) == _capi.ERR_INVALID
    assert call(nbytes=len(data) - 11) == _capi.ERR_INVALID and b"shorter" in L.rmclhip_last_error()     # the last point's z is cut
    assert call(nbytes=len(data) - 10) == _capi.OK                                                      # its trailing fields may be
    for dt in (1, 2, 6, 9):
        assert call(lay_=layout(datatype=dt)) == _capi.ERR_UNSUPPORTED
    bad = np.ascontiguousarray(T.identity(), dtype=T.TRANSFORM).reshape(1).copy()
    for field, val in (("t", np.nan), ("t", np.inf), ("R", np.nan)):
        Tb = bad.copy()
        Tb[field]["x"] = val
        assert call(T_p=Tb.ctypes.data_as(C.c_void_p)) == _capi.ERR_INVALID
    assert call(lay_=layout(width=1 << 16, height=(1 << 15) + 1, row_step=22 << 16), nbytes=1 << 62) == _capi.ERR_INVALID   # > 2^31 points
    assert b"2^31" in L.rmclhip_last_error()
    zero_inc = T.spherical_model(0.0, 0.0, 2, -math.pi, 2 * math.pi / 32, 32, 0.1, 100.0)
    assert call(model_=zero_inc) == _capi.ERR_INVALID
    flat = T.spherical_model(0.0, 0.0, 1, -math.pi, 2 * math.pi / 32, 32, 0.1, 100.0)       # the 2-D scanner: every point in row 0
    assert call(model_=flat) == _capi.OK
    ref = pr.bin_points(p, *pr.model_tuple(flat))
    assert st.as_dict() == ref["stats"] and out[:32].tobytes() == ref["ranges"].tobytes()
    assert call(out_p=None) == _capi.ERR_INVALID
    # the empty cloud: no error, an all-empty image, zero counts; its data pointer may be null
    out[:] = 0
    assert call(data_p=None, nbytes=0, lay_=layout(width=0, row_step=0)) == _capi.OK
    assert st.as_dict() == dict.fromkeys(STAT_NAMES, 0) and (out == f32(101.0)).all()
    img, stats = ra.wire.pointcloud2_to_scan(ctx, b"", 0, 1, 22, 0, 0, 4, 8, model)
    assert img.shape == (32, 32) and (img == f32(101.0)).all() and stats["n_cells_filled"] == 0

    # the operator form: a spherical model is needed
    v, f = meshes("cube")
    hm = ra.import_hip_map(ctx, v, f)
    rp = C.c_void_p()

    def op_call(h, flags=0, nbytes=len(data)):
        return L.rmclhip_rcc_set_input_pointcloud2_scan(h, dp, nbytes, C.byref(layout()), 0, None, flags, C.byref(rp), C.byref(st))

    o1 = ra.RCCHipO1Dn(hm)
    o1.setModel(32, 32, 0.1, 100.0, (0, 0, 0), syn.model_directions(model))
    assert op_call(o1._h) == _capi.ERR_INVALID and b"spherical" in L.rmclhip_last_error()
    fresh = ra.RCCHipSpherical(hm)
    assert op_call(fresh._h) == _capi.ERR_INVALID                                   # no model yet
    fresh.setModel(model)
    assert op_call(fresh._h) == _capi.OK and rp.value and st.n_points == n
    assert op_call(fresh._h, flags=32) == _capi.ERR_INVALID and op_call(fresh._h, nbytes=100) == _capi.ERR_INVALID
    assert L.rmclhip_rcc_set_input_pointcloud2_scan(None, dp, len(data), C.byref(layout()), 0, None, 0, None, None) == _capi.ERR_INVALID
    with pytest.raises(ra.RmclHipError) as e:
        fresh.setInputPointCloud2(data, **dict(lay, datatype=3))
    assert e.value.status == _capi.ERR_UNSUPPORTED
    # stats and the ranges pointer are optional; the empty cloud empties the dataset's mask
    assert L.rmclhip_rcc_set_input_pointcloud2_scan(fresh._h, dp, len(data), C.byref(layout()), 0, None, 0, None, None) == _capi.OK
    stats = fresh.setInputPointCloud2(b"", 0, 1, 22, 0, 0, 4, 8)
    assert stats == dict.fromkeys(STAT_NAMES, 0) and (fresh.rangesView().download() == f32(101.0)).all()
    fresh.find(T.identity())
    assert int(fresh.computeCrossStatistics(T.identity())["n_meas"]) == 0
    for h in (o1, fresh):
        h.close()


# ---- 8: the C++ adapters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 7])
def test_cpp_example_matches_the_python_path(ra, orc, ctx, meshes, tmp_path, flags):
    """examples/pc2_to_scan_cpp_example.cpp: cloud bytes -> RCCHipSpherical::setInputPointCloud2 -> correctOnce, and cloud bytes ->
    Pc2ToScanHip -> ScanMapSegmentationHipNode; image digest, counts, corrected pose and segment counts against the Python path"""
    from rmcl_amd import synthetic as syn, types as T
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "pc2_to_scan_cpp_example.cpp")
    v, f = meshes("cube")
    _write_mesh(tmp_path / "mesh.bin", v, f)
    model = syn.model_c1()
    truth = T.transform_from_rpy((0.5, -0.3, 0.2), (0.02, -0.03, 0.4))
    est = T.mult(truth, T.transform_from_rpy((0.2, 0.1, 0.05), (0, 0, 2.0 * math.pi / 180)))
    sim = orc.Mesh(v, f).simulate_spherical(model, T.identity(), truth, bvh=False)
    data, lay, _ = _hit_cloud(sim)
    (tmp_path / "cloud.bin").write_bytes(data)
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "cloud.bin"), str(flags)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}

    hm = ra.import_hip_map(ctx, v, f)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    rcc.params.max_dist = 1.0
    rcc.adaptive_max_dist_min = 0.15
    stats = rcc.setInputPointCloud2(data, flags=flags, **lay)
    img = rcc.rangesView().download()
    ref = pr.convert(data, model=model, flags=flags, **lay)
    assert img.tobytes() == ref["ranges"].tobytes()
    assert [int(x) for x in out["stats"]] == [stats[k] for k in STAT_NAMES] == [int(x) for x in out["node_stats"]]
    assert int(out["image_digest"][0]) == _fnv(img.tobytes()) == int(out["image_digest_again"][0]) == int(out["node_image_digest"][0])
    To, so = rcc.correct_once(T.identity(), est, 5)
    assert int(out["correct_once_n_meas"][0]) == int(so["n_meas"]) > 100
    assert np.allclose([float(x) for x in out["correct_once_t"]], [float(To["t"][k]) for k in "xyz"], atol=1e-6)
    q, q_ref = np.array([float(x) for x in out["correct_once_q"]]), np.array([float(To["R"][k]) for k in "xyzw"])
    assert np.allclose(q, q_ref * np.sign(np.dot(q, q_ref)), atol=1e-6)
    seg = rcc.segment(est, rcc.rangesView(), want=())
    assert [int(x) for x in out["segment_counts"]] == list(seg["counts"])
    Tsc = T.transform_from_rpy((0.1, 0.0, 0.3), (0.0, 0.0, 10.0 * math.pi / 180))
    moved, mstats = ra.wire.pointcloud2_to_scan(ctx, data, model=model, flags=flags, T=Tsc, **lay)
    assert [int(x) for x in out["node_transformed"]] == [_fnv(moved.tobytes()), mstats["n_cells_filled"]]
    rcc.close()
