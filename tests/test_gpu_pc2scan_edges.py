"""GPU parity at the edges: the hand-built clouds of tests/scan_edge_cases.py on its small spherical models, through
rmclhip_pointcloud2_to_scan and rmclhip_rcc_set_input_pointcloud2_scan, BYTE FOR BYTE against tests/pc2scan_ref.py -- image, the five
statistics, and for the operator form the image view and the dataset's points and mask.  tests/test_scan_edge_cases_cpu.py pins what
every point is there for (poles, the +-pi seam, signed zeros, the origin, the range bounds, overflow, subnormals, non-finite fields,
FLOAT64 values that only become inf / FLT_MAX / subnormal in the cast, rivals of one cell in different waves and workgroups) and shows
the one condition this parity rests on: no point changes its cell when the double atan2 results move by +-4 double ulps.  No cell is
excused here.  Every call of this file runs on ONE context and ONE operator, so the grow-only scratch of both (pc2scan_scratch) sees
clouds and models grow and shrink in turn; the free function writes into a guarded device buffer.
"""
import math

import numpy as np
import pytest

import pc2scan_ref as pr
import scan_edge_cases as ec

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64
_cache = {}


def _operator(ra, ctx, meshes):
    """the file's one operator (a map is needed to make one; the cube)"""
    if "rcc" not in _cache:
        from rmcl_amd import types as T
        v, f = meshes("cube")
        rcc = ra.RCCHipSpherical(ra.import_hip_map(ctx, v, f))
        rcc.setTsb(T.identity())
        _cache["rcc"], _cache["model"] = rcc, None
    return _cache["rcc"]


def _set_model(rcc, name):
    if _cache["model"] != name:
        rcc.setModel(ec.model_struct(name))
        _cache["model"] = name


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    diff = got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)
    bad = diff.any(1)
    assert not bad.any(), "%s: %d of %d differ (first at %d: %r vs %r)" % (what, bad.sum(), bad.size, np.argmax(bad), got[np.argmax(bad)],
                                                                            want[np.argmax(bad)])


def _check(ra, ctx, rcc, name, data, lay, flags, T=None, device=False, what=""):
    """one cloud, one flag word, both entry points, everything compared with the restatement byte for byte -> the restatement's result"""
    m = ec.MODELS[name]
    n_cells = m[2] * m[5]
    ref = pr.convert(data, model=m, flags=flags, T=T, **lay)
    what = "%s %s flags %d" % (name, what, flags)
    src, kw = data, {}
    if device:
        src, kw = ra.DeviceArray.from_host(ctx, np.frombuffer(data, np.uint8)), dict(device=True, nbytes=len(data))
    # the free function, into a guarded device buffer
    d_out = ra.DeviceArray.from_host(ctx, np.full(n_cells + GUARD, -7.0, f32))
    stats = ra.wire.pointcloud2_to_scan(ctx, src, model=ec.model_struct(name), flags=flags, T=T, into=d_out, **dict(lay, **kw))
    out = d_out.download()
    d_out.free()
    assert stats == ref["stats"], (what, stats, ref["stats"])
    _same(out[:n_cells], ref["ranges"], what + " image")
    assert (out[n_cells:] == f32(-7.0)).all(), what + ": written beyond W * H"
    # ... and to the host
    img, stats = ra.wire.pointcloud2_to_scan(ctx, src, model=ec.model_struct(name), flags=flags, T=T, **dict(lay, **kw))
    assert stats == ref["stats"] and img.shape == (m[2], m[5])
    _same(img, ref["ranges"], what + " host image")
    # the operator: image view, dataset points and mask
    _set_model(rcc, name)
    stats = rcc.setInputPointCloud2(src, flags=flags, T=T, **dict(lay, **kw))
    assert stats == ref["stats"], (what, "operator", stats, ref["stats"])
    _same(rcc.rangesView().download(), ref["ranges"], what + " rangesView")
    pts, mask = ec.dataset_of(ref["ranges"], m)
    iv = rcc.inputView()
    _same(iv["points"], pts, what + " dataset points")
    _same(iv["mask"], mask, what + " dataset mask")
    assert int(mask.sum()) == ref["stats"]["n_cells_filled"]
    if device:
        src.free()
    return ref


def _f32_cloud(xyz, rec=ec.REC12, **kw):
    return pr.make_cloud(rec, np.asarray(xyz, f32), **kw)


# ---- 1: every model, every named point, every flag word -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.MODEL_ORDER)
def test_named_points_on_every_model(ra, ctx, meshes, name):
    rcc = _operator(ra, ctx, meshes)
    data, lay = _f32_cloud(ec.edge_cloud(name))
    seen = set()
    for flags in ec.FLAGS:
        ref = _check(ra, ctx, rcc, name, data, lay, flags)
        seen.add(ref["ranges"].tobytes())
    m = ec.MODELS[name]
    if ec.period(m) == 0:
        # a wrap flag the library drops (no whole-number period, or a zero increment) changes nothing
        for a, b in ((4, 0), (6, 2), (12, 8)):
            ref_a, ref_b = (pr.convert(data, model=m, flags=fl, **lay) for fl in (a, b))
            got_a, st_a = ra.wire.pointcloud2_to_scan(ctx, data, model=ec.model_struct(name), flags=a, **lay)
            got_b, st_b = ra.wire.pointcloud2_to_scan(ctx, data, model=ec.model_struct(name), flags=b, **lay)
            assert st_a == st_b == ref_b["stats"] == ref_a["stats"] and got_a.tobytes() == got_b.tobytes() == ref_b["ranges"].tobytes()
    elif name in ("tiny", "odd", "poles"):
        assert len(seen) >= 4        # the flags do different things to this cloud


# ---- 2: clouds smaller than a wave, than a workgroup, and just beyond ------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_truncated_clouds(ra, ctx, meshes, n):
    rcc = _operator(ra, ctx, meshes)
    for name in ("zero_min", "odd"):
        data, lay = _f32_cloud(ec.edge_cloud(name, n))
        assert lay["width"] == n
        for flags in ec.FLAGS:
            ref = _check(ra, ctx, rcc, name, data, lay, flags, what="n=%d" % n)
            assert ref["stats"]["n_points"] == n
            if name == "zero_min" and n == 1:
                # the origin alone at buffer index 0: its keys are (0 + 1) << 32 | 0 and 0 << 32 | 0 -- neither is "nobody": range 0 is
                # stored in the cell of phi = theta = 0
                assert ref["stats"]["n_cells_filled"] == 1 and ref["ranges"][2 * 8 + 4].tobytes() == b"\0\0\0\0"


# ---- 3: record layouts, host and device sources ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_record_layouts(ra, ctx, meshes, device):
    rcc = _operator(ra, ctx, meshes)
    for name in ("tiny", "odd"):
        pts = ec.edge_cloud(name, 1025)
        clouds = [("z-y-x in 13 bytes", pr.make_cloud(ec.REC13, pts, seed=2)),
                  ("organised, 37 wide, 5 bytes of row padding", pr.make_cloud(ec.REC12, ec.edge_cloud(name, 37 * 28), height=28, row_pad=5, seed=3)),
                  ("FLOAT64 at offset 3 of 29 bytes", pr.make_cloud(ec.REC29, ec.f64_cloud(name)[0], seed=4))]
        for label, (data, lay) in clouds:
            cut = ec.cut_to_last_coordinate(data, lay)
            assert len(cut) < len(data)
            for flags in (0, 7, 8, 15):
                ref = _check(ra, ctx, rcc, name, cut, lay, flags, device=device, what=label)
            assert ref["stats"]["n_finite"] < ref["stats"]["n_points"] and ref["stats"]["n_cells_filled"] > 10


def test_float64_values_that_change_in_the_cast(ra, ctx, meshes):
    """1e300 and the doubles at and above FLT_MAX + 1/2 ulp become inf (skipped), the one below becomes FLT_MAX (finite, range inf),
    1e-40 a subnormal float, the half-way doubles round to even: one point per cloud, so the statistics show each cast"""
    rcc = _operator(ra, ctx, meshes)
    for k, (label, value, as_float) in enumerate(ec.F64_VALUES):
        data, lay = pr.make_cloud(ec.REC29, np.array([[value, 0.0, 0.0]], np.float64))
        for name in ("tiny", "zero_min"):
            ref = _check(ra, ctx, rcc, name, data, lay, 0, what=label)
            assert ref["stats"]["n_finite"] == int(np.isfinite(as_float)), label
        if np.isfinite(as_float) and as_float < 10:
            # (ref: zero_min) the stored range is the float the cast made, squared and rooted -- 0 for the subnormal 1e-40
            x = f32(as_float)
            assert ref["stats"]["n_in_range"] == 1 and np.sqrt(x * x) in ref["ranges"]


# ---- 4: the winner rule, rivals placed on purpose ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_cell", "two_cells"])
@pytest.mark.parametrize("order", ["asc", "desc", "tail"])
def test_winner_rule_across_waves_and_workgroups(ra, ctx, meshes, order, two):
    rcc = _operator(ra, ctx, meshes)
    for name in ("odd", "tiny"):
        xyz, winners = ec.winner_cloud(name, order, two_cells=two)
        data, lay = _f32_cloud(xyz)
        with np.errstate(invalid="ignore"):
            r = np.sqrt((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2]).astype(f32)
        last = _check(ra, ctx, rcc, name, data, lay, 0, what=order)
        near = _check(ra, ctx, rcc, name, data, lay, pr.NEAREST, what=order)
        for cell, w_last, w_near in winners:
            # (the restatement's images equal the device's: checked above; these say WHICH rival that is)
            assert last["ranges"][cell] == r[w_last] and near["ranges"][cell] == r[w_near]


# ---- 5: a finite point whose range overflows, with and without a transform --------------------------------------------------------------
def test_overflowing_point_with_a_translation(ra, ctx, meshes):
    """(3e38, 3e38, 0) is finite, its range is inf: in the image, not in range.  With T = a translation of 1 m (identity rotation: every
    product of qrot is exact, the sums are single IEEE additions on both sides) the finite test still looks at the FIELDS"""
    from rmcl_amd import types as T
    rcc = _operator(ra, ctx, meshes)
    Tx = T.transform_from_rpy((1.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    pts = np.array([[3e38, 3e38, 0], [np.nan, 1, 1], [1, np.inf, 1], [2, 0, 0], [-3.4e38, 1, 1], [0, 0, 0]], f32)
    data, lay = _f32_cloud(pts)
    for name in ("tiny", "zero_min"):
        for flags in ec.FLAGS:
            plain = _check(ra, ctx, rcc, name, data, lay, flags)
            moved = _check(ra, ctx, rcc, name, data, lay, flags, T=Tx, what="translated")
            assert plain["stats"]["n_finite"] == moved["stats"]["n_finite"] == 4
            assert plain["stats"]["n_in_image"] > plain["stats"]["n_in_range"] >= 1
    # a quarter turn about z on top: T * (3e38, 3e38, 0) is no longer finite (y' = 3e38 * sqrt(2) overflows) -- the point still counts
    # in n_finite, because the test comes before the transform.  One point per cloud, so the count is this point's
    Tr = T.transform_from_rpy((1.0, 0.0, 0.0), (0.0, 0.0, math.pi / 4))
    data, lay = _f32_cloud(pts[:1])
    with np.errstate(all="ignore"):
        assert not np.isfinite(pr.apply_transform(Tr, pts[:1])).all()
    for flags in ec.FLAGS:
        moved = _check(ra, ctx, rcc, "tiny", data, lay, flags, T=Tr, what="turned")
        assert moved["stats"] == dict(n_points=1, n_finite=1, n_in_image=0, n_in_range=0, n_cells_filled=0)


# ---- 6: one context, one operator, from the largest case to the smallest and back ------------------------------------------------------
def test_scratch_carries_nothing_over(ra, ctx, meshes):
    """models by falling cell count, each with a 1025-point and then a one-point cloud, and back up: keys, per-workgroup counts, the
    staged bytes and the image of an earlier, larger call must not show in a later, smaller one (and growing again must work)"""
    rcc = _operator(ra, ctx, meshes)
    order = list(ec.MODEL_ORDER) + list(ec.MODEL_ORDER[::-1])
    for name in order:
        for n in (1025, 1):
            data, lay = _f32_cloud(ec.edge_cloud(name, n))
            for flags in (0, 15):
                _check(ra, ctx, rcc, name, data, lay, flags, what="n=%d" % n)
    # the empty cloud last: an all-empty image on the smallest and on the largest model
    for name in ("one", "odd"):
        ref = _check(ra, ctx, rcc, name, b"", dict(lay, width=0, row_step=0), 8)
        assert ref["stats"]["n_cells_filled"] == 0
