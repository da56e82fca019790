"""GPU parity: map segmentation on the device (rmclhip_rcc_segment, CorrespondencesHIP.segment) -- labels and the two compacted outlier
clouds of the reference's ScanMapSegmentationEmbreeNode / O1DnMapSegmentationEmbreeNode (scan_map_segmentation_embree.cpp:76-185).

The oracle has no segmentation entry: the expected labels come from tests/segmentation_ref.py (the decision rule in numpy / float64)
fed with the ORACLE's simulated ranges and normals.  Simulated ranges agree with the oracle to 1e-5 relative (face ids and hits bit for
bit), so a ray whose decision sits that close to a threshold may fall either way: a ray is *undecided* if the restatement's label
changes when r_sim, or r_real, is scaled by 1 +- 3e-5; every other ray's label must be equal.  The clouds are then checked against the
GPU's own labels exactly: counts, order, coordinates, nothing written beyond the counted points.
"""
import struct
import subprocess

import numpy as np
import pytest

import segmentation_ref as sr
from conftest import assert_close_rel, find_kinds

pytestmark = pytest.mark.gpu

THRESHOLDS = [(0.15, 0.15), (0.10, 0.30)]
O1DN_ORIGIN = np.array([0.05, -0.02, 0.4], np.float32)
_cache = {}


def _scene(orc, which):
    """the cube / room scene of segmentation_ref with the oracle's meshes (cached: the room takes a second to build)"""
    from rmcl_amd import synthetic as syn, types as T
    if which not in _cache:
        (mv, mf), (rv, rf), model, Tsb, truth, est = (sr.cube_scene if which == "cube" else sr.room_scene)(syn, T)
        _cache[which] = dict(map_vf=(mv, mf), map_mesh=orc.Mesh(mv, mf), real_mesh=orc.Mesh(rv, rf), model=model, Tsb=Tsb, truth=truth,
                             est=est, bvh=(which != "cube"), dirs=syn.model_directions(model))
    return _cache[which]


def _spherical_case(orc, which):
    """-> (scene, real ranges, the oracle's simulation of the map at the estimate)"""
    s = _scene(orc, which)
    key = which + "/spherical"
    if key not in _cache:
        real = s["real_mesh"].simulate_spherical(s["model"], s["Tsb"], s["truth"], bvh=s["bvh"], nthreads=8, want=("ranges",))["ranges"]
        if which == "room":
            real = sr.invalidate_some(real, s["model"].range.max)
        sim = s["map_mesh"].simulate_spherical(s["model"], s["Tsb"], s["est"], bvh=s["bvh"], nthreads=8, want=("ranges", "normals"))
        _cache[key] = (real, sim)
    return (s,) + _cache[key]


def _expect(real, sim, dirs, origs, rng, thr=(0.15, 0.15), flag=False):
    kw = dict(min_dist_outlier_scan=thr[0], min_dist_outlier_map=thr[1], pint_with_origin=flag)
    ref = sr.segment(real, sim["ranges"], sim["normals"], dirs, origs, rng[0], rng[1], **kw)
    und = sr.undecided(real, sim["ranges"], sim["normals"], dirs, origs, rng[0], rng[1], **kw)
    assert und.sum() <= 0.001 * len(real), "%d undecided rays: the scene does not pin the labels" % und.sum()
    return ref, und


def _labels_agree(got, ref, und, what):
    bad = (got != ref["labels"]) & ~und
    assert not bad.any(), "%s: %d labels differ from the restatement (first at ray %d: %d vs %d)" % (
        what, bad.sum(), np.argmax(bad), got[np.argmax(bad)], ref["labels"][np.argmax(bad)])


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_clouds(out, real, r_sim_gpu, dirs, origs, rng, flag, what):
    """test 2: counts, order and coordinates of both clouds follow from the GPU's own labels"""
    L = out["labels"]
    n_scan, n_map = int((L == 2).sum()), int((L == 3).sum())
    assert tuple(out["counts"]) == (n_scan, n_map), what
    assert out["outlier_scan"].shape == (n_scan, 3) and out["outlier_map"].shape == (n_map, 3)
    d64, o64 = dirs.astype(np.float64), np.broadcast_to(np.asarray(origs, np.float64).reshape(-1, 3), dirs.shape)
    preal = d64 * real.astype(np.float64)[:, None] + o64
    assert_close_rel(out["outlier_scan"], preal[L == 2], 1e-5, 1e-6, what + " outlier_scan")
    real_ok = (np.float32(rng[0]) <= real) & (real <= np.float32(rng[1]))
    pint = d64 * r_sim_gpu.astype(np.float64)[:, None] + np.where((~real_ok | flag)[:, None], o64, 0.0)
    assert_close_rel(out["outlier_map"], pint[L == 3], 1e-5, 1e-6, what + " outlier_map")


def _spherical_operator(ra, ctx, s, kind=None):
    hm = ra.import_hip_map(ctx, *s["map_vf"])
    rcc = ra.RCCHipSpherical(hm)
    if kind is not None:
        rcc.set_traversal(kind)
    rcc.setTsb(s["Tsb"])
    rcc.setModel(s["model"])
    return rcc


def _gpu_ranges(ra, rcc, pose):
    return ra.CorrespondencesHIP.download_bundle(rcc.simulate(pose, attributes=("ranges",)))["ranges"]


# ---- 1 + 2: labels against the restatement, clouds against the labels ---------------------------------------------------------------
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("which", ["cube", "room"])
def test_labels_match_the_restatement_and_clouds_match_the_labels(ra, orc, ctx, which, thr):
    s, real, sim = _spherical_case(orc, which)
    rng = (s["model"].range.min, s["model"].range.max)
    ref, und = _expect(real, sim, s["dirs"], np.zeros(3), rng, thr)
    hist = np.bincount(ref["labels"], minlength=4)
    if which == "room":
        assert (hist >= 0.01 * len(real)).all(), hist           # all four branches carry weight
    else:
        assert hist[0] == 0 and hist[2] >= 20 and hist[3] >= 20, hist
    rcc = _spherical_operator(ra, ctx, s)
    out = rcc.segment(s["est"], real, thr[0], thr[1])
    _labels_agree(out["labels"], ref, und, "%s %s" % (which, thr))
    _check_clouds(out, real, _gpu_ranges(ra, rcc, s["est"]), s["dirs"], np.zeros(3), rng, False, "%s %s" % (which, thr))
    rcc.close()


def test_nothing_is_written_beyond_the_counts(ra, orc, ctx):
    """caller-owned, canary-filled buffers twice the capacity: labels end at W*H, a cloud at its count"""
    s, real, _ = _spherical_case(orc, "room")
    n = len(real)
    rcc = _spherical_operator(ra, ctx, s)
    into = dict(labels=ra.DeviceArray.from_host(ctx, np.full(2 * n, 77, np.uint8)),
                outlier_scan=ra.DeviceArray.from_host(ctx, np.full(6 * n, -7.0, np.float32)),
                outlier_map=ra.DeviceArray.from_host(ctx, np.full(6 * n, -7.0, np.float32)),
                counts=ra.DeviceArray.from_host(ctx, np.full(4, 0xABCDEF, np.uint32)))
    counts = rcc.segment(s["est"], real, into=into)
    L = into["labels"].download()
    assert (L[n:] == 77).all() and (L[:n] <= 3).all()
    assert counts == (int((L[:n] == 2).sum()), int((L[:n] == 3).sum())) and min(counts) > 1000
    for a, k in (("outlier_scan", counts[0]), ("outlier_map", counts[1])):
        pts = into[a].download()
        assert (pts[3 * k:] == -7.0).all(), "%s: written beyond its %d points" % (a, k)
        assert np.isfinite(pts[:3 * k]).all()
    c = into["counts"].download()
    assert tuple(c[:2]) == counts and (c[2:] == 0xABCDEF).all()
    fresh = rcc.segment(s["est"], real)
    assert _same_bits(fresh["labels"], L[:n])
    assert _same_bits(fresh["outlier_scan"].reshape(-1), into["outlier_scan"].download()[:3 * counts[0]])
    assert _same_bits(fresh["outlier_map"].reshape(-1), into["outlier_map"].download()[:3 * counts[1]])
    rcc.close()


# ---- 3: all four sensor models ------------------------------------------------------------------------------------------------------
def test_o1dn_with_an_offset_origin_flag_off_and_on(ra, orc, ctx):
    """the reference leaves the ray origin out of pint_s when both ranges are valid; RMCLHIP_SEG_PINT_WITH_ORIGIN adds it.  Each mode
    against the restatement in the same mode -- and the modes differ in more than 1 % of the rays, so the flag does something"""
    s = _scene(orc, "room")
    model, dirs = s["model"], s["dirs"]
    H, W, rng = int(model.phi.size), int(model.theta.size), (model.range.min, model.range.max)
    real = s["real_mesh"].simulate_o1dn(W, H, rng[0], rng[1], O1DN_ORIGIN, dirs, s["Tsb"], s["truth"], bvh=True, nthreads=8, want=("ranges",))["ranges"]
    real = sr.invalidate_some(real, rng[1])
    sim = s["map_mesh"].simulate_o1dn(W, H, rng[0], rng[1], O1DN_ORIGIN, dirs, s["Tsb"], s["est"], bvh=True, nthreads=8, want=("ranges", "normals"))
    hm = ra.import_hip_map(ctx, *s["map_vf"])
    rcc = ra.RCCHipO1Dn(hm)
    rcc.setTsb(s["Tsb"])
    rcc.setModel(W, H, rng[0], rng[1], O1DN_ORIGIN, dirs)
    r_gpu = _gpu_ranges(ra, rcc, s["est"])
    labels = {}
    for flag in (False, True):
        ref, und = _expect(real, sim, dirs, O1DN_ORIGIN, rng, flag=flag)
        out = rcc.segment(s["est"], real, pint_with_origin=flag)
        _labels_agree(out["labels"], ref, und, "o1dn flag %s" % flag)
        _check_clouds(out, real, r_gpu, dirs, O1DN_ORIGIN, rng, flag, "o1dn flag %s" % flag)
        labels[flag] = out["labels"]
    assert (labels[False] != labels[True]).sum() > 0.01 * len(real)
    rcc.close()


def test_pinhole_and_ondn(ra, orc, ctx):
    s = _scene(orc, "room")
    model, dirs = s["model"], s["dirs"]
    rng = (model.range.min, model.range.max)
    hm = ra.import_hip_map(ctx, *s["map_vf"])
    # OnDn: the spherical directions, every ray with an origin of its own
    H, W = int(model.phi.size), int(model.theta.size)
    origs = (np.random.RandomState(11).uniform(-0.05, 0.05, dirs.shape) + O1DN_ORIGIN).astype(np.float32)
    real = s["real_mesh"].simulate_ondn(W, H, rng[0], rng[1], origs, dirs, s["Tsb"], s["truth"], bvh=True, nthreads=8, want=("ranges",))["ranges"]
    real = sr.invalidate_some(real, rng[1])
    sim = s["map_mesh"].simulate_ondn(W, H, rng[0], rng[1], origs, dirs, s["Tsb"], s["est"], bvh=True, nthreads=8, want=("ranges", "normals"))
    on = ra.RCCHipOnDn(hm)
    on.setTsb(s["Tsb"])
    on.setModel(W, H, rng[0], rng[1], origs, dirs)
    ref, und = _expect(real, sim, dirs, origs, rng)
    out = on.segment(s["est"], real)
    _labels_agree(out["labels"], ref, und, "ondn")
    _check_clouds(out, real, _gpu_ranges(ra, on, s["est"]), dirs, origs, rng, False, "ondn")
    assert min(out["counts"]) > 1000
    on.close()
    # pinhole 256 x 192
    PW, PH = 256, 192
    f, c = (PW * 0.45, PW * 0.45), ((PW - 1) / 2.0, (PH - 1) / 2.0)
    pdirs = orc.pinhole_directions(PW, PH, f, c).astype(np.float32)
    real = s["real_mesh"].simulate_pinhole(PW, PH, rng[0], rng[1], f, c, s["Tsb"], s["truth"], bvh=True, nthreads=8, want=("ranges",))["ranges"]
    real = sr.invalidate_some(real, rng[1])
    sim = s["map_mesh"].simulate_pinhole(PW, PH, rng[0], rng[1], f, c, s["Tsb"], s["est"], bvh=True, nthreads=8, want=("ranges", "normals"))
    ph = ra.RCCHipPinhole(hm)
    ph.setTsb(s["Tsb"])
    ph.setModel(PW, PH, rng[0], rng[1], f[0], f[1], c[0], c[1])
    ref, und = _expect(real, sim, pdirs, np.zeros(3), rng)
    out = ph.segment(s["est"], real)
    _labels_agree(out["labels"], ref, und, "pinhole")
    _check_clouds(out, real, _gpu_ranges(ra, ph, s["est"]), pdirs, np.zeros(3), rng, False, "pinhole")
    assert out["counts"][0] > 1000
    ph.close()


# ---- 4: every product find kind -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", find_kinds(0, 2, 23, 24, 32))
def test_every_find_kind_gives_the_same_bits(ra, orc, ctx, kind):
    s, real, _ = _spherical_case(orc, "cube")
    base = _spherical_operator(ra, ctx, s, 15)
    want = base.segment(s["est"], real)
    rcc = _spherical_operator(ra, ctx, s, kind)
    got = rcc.segment(s["est"], real)
    assert got["counts"] == want["counts"] and min(want["counts"]) >= 20
    for a in ("labels", "outlier_scan", "outlier_map"):
        assert _same_bits(got[a], want[a]), "kind %d: %s differs from kind 15's" % (kind, a)
    base.close()
    rcc.close()


# ---- 5: shapes that stress the compaction -------------------------------------------------------------------------------------------
def test_model_that_is_no_multiple_of_a_wave_or_a_workgroup(ra, orc, ctx):
    from rmcl_amd import types as T
    s = _scene(orc, "cube")
    f32 = np.float32
    model = T.spherical_model(f32(-0.6), f32(1.2 / 36), 37, f32(-np.pi), f32(2 * np.pi / 53), 53, f32(0.1), f32(100.0))
    from rmcl_amd import synthetic as syn
    dirs = syn.model_directions(model)
    real = sr.invalidate_some(s["real_mesh"].simulate_spherical(model, s["Tsb"], s["truth"], bvh=False, want=("ranges",))["ranges"], 100.0, 0.05)
    sim = s["map_mesh"].simulate_spherical(model, s["Tsb"], s["est"], bvh=False, want=("ranges", "normals"))
    ref, und = _expect(real, sim, dirs, np.zeros(3), (0.1, 100.0))
    rcc = _spherical_operator(ra, ctx, s)
    rcc.setModel(model)
    out = rcc.segment(s["est"], real)
    assert len(out["labels"]) == 37 * 53
    _labels_agree(out["labels"], ref, und, "37 x 53")
    _check_clouds(out, real, _gpu_ranges(ra, rcc, s["est"]), dirs, np.zeros(3), (0.1, 100.0), False, "37 x 53")
    assert min(out["counts"]) >= 20
    rcc.close()


def test_all_or_nothing_scans(ra, ctx, meshes):
    """the plain cube room (every ray hits): every ray a scan outlier (the cloud fills its whole capacity), every ray a map outlier, none,
    an all-invalid scan (zeros, NaNs: the sim-only branch), and a model of one ray"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cube")
    hm = ra.import_hip_map(ctx, v, f)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    model = syn.model_c1()
    rcc.setModel(model)
    pose = syn.pose_c2_truth()
    n = 32 * 32
    r_sim = _gpu_ranges(ra, rcc, pose)
    assert ((r_sim > 1.0) & (r_sim < 40.0)).all()
    dirs = syn.model_directions(model).astype(np.float64)
    into = dict(labels=ra.DeviceArray.from_host(ctx, np.full(n + 64, 77, np.uint8)),
                outlier_scan=ra.DeviceArray.from_host(ctx, np.full(3 * n + 64, -7.0, np.float32)),
                outlier_map=ra.DeviceArray.from_host(ctx, np.full(3 * n + 64, -7.0, np.float32)))
    half = (r_sim * np.float32(0.5)).astype(np.float32)
    assert rcc.segment(pose, half, into=into) == (n, 0)
    assert (into["labels"].download()[:n] == 2).all() and (into["labels"].download()[n:] == 77).all()
    pts = into["outlier_scan"].download()
    assert_close_rel(pts[:3 * n].reshape(n, 3), dirs * half.astype(np.float64)[:, None], 1e-5, 1e-6, "all scan outliers")
    assert (pts[3 * n:] == -7.0).all() and (into["outlier_map"].download() == -7.0).all()
    double = (r_sim * np.float32(2.0)).astype(np.float32)
    out = rcc.segment(pose, double)
    assert out["counts"] == (0, n) and (out["labels"] == 3).all() and out["outlier_scan"].shape == (0, 3)
    assert_close_rel(out["outlier_map"], dirs * r_sim.astype(np.float64)[:, None], 1e-5, 1e-6, "all map outliers")
    out = rcc.segment(pose, r_sim)
    assert out["counts"] == (0, 0) and (out["labels"] == 1).all()
    for bad in (np.zeros(n, np.float32), np.full(n, np.nan, np.float32)):
        out = rcc.segment(pose, bad)
        assert out["counts"] == (0, n) and (out["labels"] == 3).all()
        assert_close_rel(out["outlier_map"], dirs * r_sim.astype(np.float64)[:, None], 1e-5, 1e-6, "all-invalid scan")
    f32 = np.float32
    rcc.setModel(T.spherical_model(f32(0.1), f32(0.0), 1, f32(0.3), f32(0.0), 1, f32(0.1), f32(100.0)))
    one = _gpu_ranges(ra, rcc, pose)
    assert len(one) == 1
    out = rcc.segment(pose, one * np.float32(0.5))
    assert out["counts"] == (1, 0) and list(out["labels"]) == [2]
    out = rcc.segment(pose, np.zeros(1, np.float32))
    assert out["counts"] == (0, 1) and list(out["labels"]) == [3]
    rcc.close()


# ---- 6: plumbing --------------------------------------------------------------------------------------------------------------------
def test_host_and_device_ranges_null_outputs_async_and_repeat(ra, orc, ctx):
    s, real, _ = _spherical_case(orc, "room")
    n = len(real)
    rcc = _spherical_operator(ra, ctx, s)
    a = rcc.segment(s["est"], real)
    b = rcc.segment(s["est"], real)                                       # two calls: the same bits
    d_real = ra.DeviceArray.from_host(ctx, real)
    c = rcc.segment(s["est"], d_real)                                     # ranges in device memory
    for k in ("labels", "outlier_scan", "outlier_map"):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), k
    assert a["counts"] == b["counts"] == c["counts"]
    # every subset of the outputs, the counts always
    assert rcc.segment(s["est"], real, want=())["counts"] == a["counts"]
    only = rcc.segment(s["est"], real, want=("outlier_map",))
    assert sorted(only) == ["counts", "outlier_map"] and _same_bits(only["outlier_map"], a["outlier_map"])
    only = rcc.segment(s["est"], real, want=("labels",))
    assert _same_bits(only["labels"], a["labels"])
    assert rcc.segment(s["est"], real, into={}) == a["counts"]
    # async + sync + counts_dev
    into = dict(labels=ra.DeviceArray(ctx, np.uint8, n), outlier_scan=ra.DeviceArray(ctx, np.float32, 3 * n),
                outlier_map=ra.DeviceArray(ctx, np.float32, 3 * n), counts=ra.DeviceArray.from_host(ctx, np.zeros(2, np.uint32)))
    assert rcc.segment(s["est"], d_real, into=into, sync=False) is None
    rcc.sync()
    cnt = tuple(int(x) for x in into["counts"].download())
    assert cnt == a["counts"]
    assert _same_bits(into["labels"].download(), a["labels"])
    assert _same_bits(into["outlier_scan"].download()[:3 * cnt[0]], a["outlier_scan"].reshape(-1))
    assert _same_bits(into["outlier_map"].download()[:3 * cnt[1]], a["outlier_map"].reshape(-1))
    rcc.close()


def test_segment_leaves_the_operator_alone_and_grows_with_the_model(ra, orc, ctx):
    """like simulate: model buffers, dataset and the statistics served from them are untouched; a larger model after setModel works"""
    from rmcl_amd import synthetic as syn, types as T
    s, real, sim = _spherical_case(orc, "cube")
    rcc = _spherical_operator(ra, ctx, s)
    rcc.find(s["truth"])
    own = rcc.modelView()
    rcc.set_dataset((own["points"] + np.float32(0.02)).astype(np.float32), own["hits"])
    rcc.params.max_dist = 1.0
    s0 = rcc.computeCrossStatistics(T.identity(), 0.0)
    first = rcc.segment(s["est"], real)
    after = rcc.modelView()
    for a in ("hits", "ranges", "points", "normals", "face_ids"):
        assert _same_bits(after[a], own[a]), "segment touched the operator's own %s" % a
    assert rcc.computeCrossStatistics(T.identity(), 0.0).tobytes() == s0.tobytes()
    # grow: the room model (128 x 1024) on the same operator, then back
    big = sr.room_model(syn)
    rcc.setModel(big)
    nb = 128 * 1024
    r_big = _gpu_ranges(ra, rcc, s["est"])
    out = rcc.segment(s["est"], (r_big * np.float32(0.5)).astype(np.float32))
    hit = (r_big >= np.float32(0.3)) & (r_big <= np.float32(12.0))
    assert out["counts"] == (int(hit.sum()), 0) and hit.sum() > nb // 2
    assert np.array_equal(out["labels"], np.where(hit, 2, 0).astype(np.uint8))
    rcc.setModel(s["model"])
    again = rcc.segment(s["est"], real)
    for a in ("labels", "outlier_scan", "outlier_map"):
        assert _same_bits(again[a], first[a])
    rcc.close()


def test_error_cases(ra, orc, ctx):
    import ctypes as C
    from rmcl_amd import _capi, types as T
    s, real, _ = _spherical_case(orc, "cube")
    rcc = _spherical_operator(ra, ctx, s)
    for kw in (dict(min_dist_outlier_scan=float("nan")), dict(min_dist_outlier_map=float("nan")), dict(min_dist_outlier_scan=-0.1),
               dict(min_dist_outlier_map=-1e-6)):
        with pytest.raises(ra.RmclHipError) as e:
            rcc.segment(s["est"], real, **kw)
        assert e.value.status == _capi.ERR_INVALID
    L = _capi.lib()
    Tm = np.ascontiguousarray(s["est"], dtype=T.TRANSFORM).reshape(1)
    rp = real.ctypes.data_as(C.c_void_p)
    tp = Tm.ctypes.data_as(C.c_void_p)
    good = _capi.SegmentationParams(0.15, 0.15, 0)
    views = _capi.SegmentationViews()
    counts = (C.c_uint32 * 2)(5, 5)
    assert L.rmclhip_rcc_segment(rcc._h, tp, rp, 0, C.byref(_capi.SegmentationParams(0.15, 0.15, 2)), C.byref(views), counts) == _capi.ERR_INVALID
    assert b"flag" in L.rmclhip_last_error()
    assert L.rmclhip_rcc_segment(rcc._h, None, rp, 0, C.byref(good), C.byref(views), counts) == _capi.ERR_INVALID
    assert L.rmclhip_rcc_segment(rcc._h, tp, None, 0, C.byref(good), C.byref(views), counts) == _capi.ERR_INVALID
    assert L.rmclhip_rcc_segment(rcc._h, tp, rp, 0, None, C.byref(views), counts) == _capi.ERR_INVALID
    assert L.rmclhip_rcc_segment_async(rcc._h, tp, rp, 0, None, C.byref(views)) == _capi.ERR_INVALID
    # a null views struct means "counts only"; an operator without a model: no-op, counts 0
    assert L.rmclhip_rcc_segment(rcc._h, tp, rp, 0, C.byref(good), None, counts) == _capi.OK
    assert tuple(counts) == rcc.segment(s["est"], real, want=())["counts"]
    with pytest.raises(ValueError):
        rcc.segment(s["est"], real[:-1])
    empty = ra.RCCHipSpherical(rcc.map)
    assert L.rmclhip_rcc_segment(empty._h, tp, rp, 0, C.byref(good), C.byref(views), counts) == _capi.OK and tuple(counts) == (0, 0)
    empty.close()
    rcc.close()


# ---- 7: the C++ adapters --------------------------------------------------------------------------------------------------------------
def test_segmentation_cpp_example_matches_the_restatement(ra, orc, ctx, tmp_path):
    """examples/segmentation_cpp_example.cpp: the two node classes of include/rmcl_hip/rmcl_hip.hpp, one call per scan -- counts and
    coordinate sums against the restatement (the cube scene has no undecided ray)"""
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "segmentation_cpp_example.cpp")
    s, real, sim = _spherical_case(orc, "cube")
    mv, mf = s["map_vf"]
    mesh_bin, scan_bin = tmp_path / "mesh.bin", tmp_path / "scan.bin"
    with open(mesh_bin, "wb") as fh:
        fh.write(struct.pack("<II", len(mv), len(mf)))
        fh.write(np.ascontiguousarray(mv, np.float32).tobytes())
        fh.write(np.ascontiguousarray(mf, np.uint32).tobytes())
    real.astype(np.float32).tofile(scan_bin)
    est = s["est"]
    pose = ["%.9g" % float(est["R"][k]) for k in "xyzw"] + ["%.9g" % float(est["t"][k]) for k in "xyz"]
    r = subprocess.run([exe, str(mesh_bin), str(scan_bin)] + pose, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    model, dirs = s["model"], s["dirs"]
    rng = (model.range.min, model.range.max)

    def check(prefix, ref, und):
        assert not und.any()
        for cloud, label in (("outlier_scan", 2), ("outlier_map", 3)):
            got = out["%s_%s" % (prefix, cloud)]
            assert int(got[0]) == int((ref["labels"] == label).sum()) >= 20, (prefix, cloud)
            assert np.allclose([float(x) for x in got[1:]], ref[cloud].sum(axis=0), rtol=1e-5, atol=1e-3), (prefix, cloud)

    # the example's pose is the scene's estimate; Tsb identity
    check("seg", *_expect(real, sim, dirs, np.zeros(3), rng))
    assert out["seg_labels"] == [str(int(x)) for x in np.bincount(_expect(real, sim, dirs, np.zeros(3), rng)[0]["labels"], minlength=4)]
    check("seg_host_ranges", *_expect(real, sim, dirs, np.zeros(3), rng))
    sim1 = s["map_mesh"].simulate_o1dn(32, 32, rng[0], rng[1], O1DN_ORIGIN, dirs, s["Tsb"], s["est"], bvh=False, want=("ranges", "normals"))
    check("o1dn", *_expect(real, sim1, dirs, O1DN_ORIGIN, rng))
    check("o1dn_with_origin", *_expect(real, sim1, dirs, O1DN_ORIGIN, rng, flag=True))
