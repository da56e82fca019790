"""GPU parity, bit for bit: segment.hip's own arithmetic -- k_segment_classify's comparisons at their thresholds and k_segment_scatter's
order and points -- against segmentation_ref.segment_f32, the kernels' float32 operations restated in numpy in the kernels' order.

tests/test_gpu_segmentation.py judges the labels through a tolerance, because it feeds its restatement the ORACLE's trace.  Here the
restatement is fed the LIBRARY's own trace: rcc.simulate(pose, attributes=("ranges", "normals")) is rmclhip_rcc_simulate ->
simulate_enqueue (capi_rcc.cpp), which for one host pose fills FindParams with fill_find_params(r, p, 1), sets only the ranges and
normals outputs, composes Tsm = Tbm * Tsb and Tms = xinv(Tsm) on the host and calls launch_find(p, r->kind, find_variant(r, 1), stream)
-- statement for statement what segment_enqueue (capi_segment.cpp:38-45) does with its scratch as the bundle.  Same kernel, same
variant, same inputs, no atomics in the trace: the same bits, so nothing is left undecided and every label and every cloud byte must be
equal.  Directions: O1Dn / OnDn are the caller's arrays; pinhole is seg_pinhole_direction restated in float32; spherical is the table of
rmclhip_rcc_set_model_spherical restated with the C library's cosf / sinf through ctypes (scan_edge_cases.spherical_dirs).
"""
import math

import numpy as np
import pytest

import scan_edge_cases as ec
import segmentation_ref as sr

pytestmark = pytest.mark.gpu

f32 = np.float32
THRESHOLDS = [(0.15, 0.15), (0.10, 0.30)]
ORIGIN = np.array([0.05, -0.02, 0.4], f32)
RNG = (f32(0.1), f32(100.0))
SPH_37x53 = (f32(-0.6), f32(1.2 / 36), 37, f32(-math.pi), f32(2 * math.pi / 53), 53, RNG[0], RNG[1])
SPH_BIG = (f32(-math.pi / 4), f32((math.pi / 2) / 1025), 1026, f32(-math.pi), f32(2 * math.pi / 1024), 1024, RNG[0], RNG[1])
SPH_ONE = (f32(0.1), f32(0.0), 1, f32(0.3), f32(0.0), 1, RNG[0], RNG[1])
PIN = dict(w=40, h=30, f=(18.0, 18.0), c=(19.5, 14.5))
_cache = {}


def _scene(orc):
    from rmcl_amd import synthetic as syn, types as T
    if "scene" not in _cache:
        (mv, mf), (rv, rf), model, Tsb, truth, est = sr.cube_scene(syn, T)
        _cache["scene"] = dict(map_vf=(mv, mf), real_mesh=orc.Mesh(rv, rf), Tsb=Tsb, truth=truth, est=est, c1_dirs=syn.model_directions(model))
    return _cache["scene"]


def _case(ra, orc, ctx, kind):
    """-> (operator, measured ranges, dirs float32 (n, 3), origs, add_origin): the cube scene seen through one of the four models; the
    measured scan is the oracle's view of the reality mesh from the true pose with 5 % of the rays invalidated"""
    s = _scene(orc)
    key = "case/" + kind
    if key in _cache:
        return _cache[key]
    hm = _cache.setdefault("map", None) or ra.import_hip_map(ctx, *s["map_vf"])
    _cache["map"] = hm
    rm = s["real_mesh"]
    if kind == "spherical":
        rcc = ra.RCCHipSpherical(hm)
        rcc.setModel(ec.model_struct(SPH_37x53))
        real = rm.simulate_spherical(ec.model_struct(SPH_37x53), s["Tsb"], s["truth"], bvh=False, want=("ranges",))["ranges"]
        dirs, origs, add = ec.spherical_dirs(SPH_37x53), np.zeros(3, f32), False
    elif kind == "o1dn":
        rcc = ra.RCCHipO1Dn(hm)
        dirs, origs, add = s["c1_dirs"], ORIGIN, True
        rcc.setModel(32, 32, RNG[0], RNG[1], ORIGIN, dirs)
        real = rm.simulate_o1dn(32, 32, RNG[0], RNG[1], ORIGIN, dirs, s["Tsb"], s["truth"], bvh=False, want=("ranges",))["ranges"]
    elif kind == "ondn":
        rcc = ra.RCCHipOnDn(hm)
        dirs, add = s["c1_dirs"], True
        origs = (np.random.RandomState(11).uniform(-0.05, 0.05, dirs.shape) + ORIGIN).astype(f32)
        rcc.setModel(32, 32, RNG[0], RNG[1], origs, dirs)
        real = rm.simulate_ondn(32, 32, RNG[0], RNG[1], origs, dirs, s["Tsb"], s["truth"], bvh=False, want=("ranges",))["ranges"]
    else:
        rcc = ra.RCCHipPinhole(hm)
        rcc.setModel(PIN["w"], PIN["h"], RNG[0], RNG[1], PIN["f"][0], PIN["f"][1], PIN["c"][0], PIN["c"][1])
        real = rm.simulate_pinhole(PIN["w"], PIN["h"], RNG[0], RNG[1], PIN["f"], PIN["c"], s["Tsb"], s["truth"], bvh=False, want=("ranges",))["ranges"]
        dirs, origs, add = sr.pinhole_dirs_f32(PIN["w"], PIN["h"], PIN["f"][0], PIN["f"][1], PIN["c"][0], PIN["c"][1]), np.zeros(3, f32), False
        # the camera sees neither box of the reality mesh: an obstacle (a block of pixels 40 % shorter) and a hole in the map (1.5 m longer)
        real = real.reshape(PIN["h"], PIN["w"]).copy()
        real[5:12, 4:14] *= f32(0.6)
        real[18:25, 22:34] += f32(1.5)
        real = real.reshape(-1)
    rcc.setTsb(s["Tsb"])
    real = sr.invalidate_some(real, RNG[1], 0.05)
    _cache[key] = (rcc, real, np.ascontiguousarray(dirs, f32), origs, add)
    return _cache[key]


def _trace(ra, rcc, pose):
    """the library's own simulated ranges and normals at `pose` (see the module docstring: the launch segment() makes)"""
    b = ra.CorrespondencesHIP.download_bundle(rcc.simulate(pose, attributes=("ranges", "normals")))
    return b["ranges"], b["normals"]


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.reshape(len(got), -1).view(np.uint8) != want.reshape(len(want), -1).view(np.uint8)).any(1))[0]
        raise AssertionError("%s: %d of %d differ, first at %d: %r vs %r" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def _exact(out, ref, what):
    _same(out["labels"], ref["labels"], what + " labels")
    assert tuple(out["counts"]) == (len(ref["outlier_scan"]), len(ref["outlier_map"])), what
    _same(out["outlier_scan"], ref["outlier_scan"], what + " outlier_scan")
    _same(out["outlier_map"], ref["outlier_map"], what + " outlier_map")


# ---- 1: the four models on the cube scene -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("kind", ["spherical", "o1dn", "ondn", "pinhole"])
def test_labels_and_clouds_equal_the_float32_restatement(ra, orc, ctx, kind, thr):
    rcc, real, dirs, origs, add = _case(ra, orc, ctx, kind)
    est = _scene(orc)["est"]
    r_sim, nrm = _trace(ra, rcc, est)
    labels = {}
    for flag in (False, True):
        ref = sr.segment_f32(real, r_sim, nrm, dirs, origs, RNG[0], RNG[1], thr[0], thr[1], flag, add_origin=add)
        out = rcc.segment(est, real, thr[0], thr[1], pint_with_origin=flag)
        _exact(out, ref, "%s %s flag %s" % (kind, thr, flag))
        labels[flag] = out["labels"]
        hist = np.bincount(ref["labels"], minlength=4)
        assert hist[1] >= 100 and hist[2] >= 20 and hist[3] >= 20, hist          # inliers and both kinds of outliers
    if add:
        assert (labels[False] != labels[True]).any()                            # the flag moves pint_s by the origin
    else:
        assert (labels[False] == labels[True]).all()


# ---- 2: hand-made measured ranges on every comparison -------------------------------------------------------------------------------------
def _bits_step(r, k):
    """the float k steps above (below for k < 0) positive finite floats"""
    return (np.asarray(r, f32).view(np.int32) + np.int32(k)).view(f32)


def _on_threshold(r_sim, nrm, dirs, origs, add, flag, thr, side, target, span=24):
    """for every ray a measured range on `side` of r_sim (-1: in front, +1: behind) whose restated float32 plane_distance equals
    `target` exactly, found among the floats around the solution of |(r - r_sim) s + c| = thr in double -> (bool found (n,), r (n,))"""
    n = len(r_sim)
    d, nn = dirs.astype(np.float64), nrm.astype(np.float64)
    unit = nn / np.sqrt((nn * nn).sum(1))[:, None]
    s = (d * unit).sum(1)
    o = np.broadcast_to(np.asarray(origs, np.float64).reshape(-1, 3), (n, 3))
    c = (o * unit).sum(1) if (add and not flag) else np.zeros(n)
    found, best = np.zeros(n, bool), np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for sign in (-1.0, 1.0):
            r0 = (r_sim.astype(np.float64) + (sign * thr - c) / s).astype(f32)
            for k in range(-span, span + 1):
                r = _bits_step(r0, k)
                ok = np.isfinite(r) & (r > RNG[0]) & (r < RNG[1]) & ((r < r_sim) if side < 0 else (r > r_sim))
                plane = sr.segment_f32(np.where(ok, r, f32(1.0)), r_sim, nrm, dirs, origs, RNG[0], RNG[1], pint_with_origin=flag,
                                       add_origin=add)["plane"]
                hit = ok & (plane == target) & ~found
                best[hit], found[hit] = r[hit], True
    return found, best


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("kind", ["spherical", "o1dn"])
def test_measured_ranges_on_every_comparison(ra, orc, ctx, kind, thr):
    """r_real == r_sim and one float to either side (`<` against `<=`), plane_distance exactly ON a threshold and on the next float
    above it (`>` against `>=`), the range interval's bounds and the floats just outside, NaN, +inf, -0.0 -- and thresholds 0 and +inf"""
    rcc, _, dirs, origs, add = _case(ra, orc, ctx, kind)
    est = _scene(orc)["est"]
    r_sim, nrm = _trace(ra, rcc, est)
    n = len(r_sim)
    assert ((r_sim > 1.0) & (r_sim < 20.0)).all()                    # the closed room: every ray hits
    for flag in (False, True):
        real = r_sim.copy()
        i = np.arange(n)
        real[i % 4 == 1] = _bits_step(r_sim, -1)[i % 4 == 1]
        real[i % 4 == 2] = _bits_step(r_sim, +1)[i % 4 == 2]
        marks, taken = {}, np.zeros(n, bool)
        for side, t, name in ((-1, thr[0], "scan"), (+1, thr[1], "map")):
            for target, tag in ((f32(t), "on"), (np.nextafter(f32(t), f32(1)), "above")):
                found, r = _on_threshold(r_sim, nrm, dirs, origs, add, flag, t, side, target)
                found &= ~taken                                                     # disjoint rays for the four targets
                found[np.nonzero(found)[0][20:]] = False
                assert found.sum() >= 1, "no ray found with plane_distance %s the %s threshold %r" % (tag, name, t)
                print("%s flag %s: %d rays with plane_distance %s the %s threshold %r" % (kind, flag, found.sum(), tag, name, t))
                real[found] = r[found]
                marks[(name, tag)] = found
                taken |= found
        special = [RNG[0], np.nextafter(RNG[0], f32(0)), RNG[1], np.nextafter(RNG[1], f32(np.inf)), f32(np.nan), f32(np.inf), f32(-0.0)]
        free = np.nonzero(~np.logical_or.reduce(list(marks.values())))[0][5:5 + len(special)]
        real[free] = special
        ref = sr.segment_f32(real, r_sim, nrm, dirs, origs, RNG[0], RNG[1], thr[0], thr[1], flag, add_origin=add)
        out = rcc.segment(est, real, thr[0], thr[1], pint_with_origin=flag)
        _exact(out, ref, "%s %s flag %s hand-made" % (kind, thr, flag))
        L = out["labels"]
        # what the rule says at each of them, written out
        assert (L[marks[("scan", "on")]] == sr.INLIER).all() and (L[marks[("scan", "above")]] == sr.OUTLIER_SCAN).all()
        assert (L[marks[("map", "on")]] == sr.INLIER).all() and (L[marks[("map", "above")]] == sr.OUTLIER_MAP).all()
        assert list(L[free]) == [ref["labels"][free[0]], sr.OUTLIER_MAP, ref["labels"][free[2]], sr.OUTLIER_MAP, sr.OUTLIER_MAP,
                                 sr.OUTLIER_MAP, sr.OUTLIER_MAP]
        assert L[free[0]] in (sr.INLIER, sr.OUTLIER_SCAN) and L[free[2]] in (sr.INLIER, sr.OUTLIER_MAP)        # the bounds are inside
        if not add or flag:
            # r_real == r_sim is the `else` branch with a distance of exactly 0: a map-side decision, an inlier at any threshold
            equal = np.nonzero(real == r_sim)[0]
            assert len(equal) > 50 and (L[equal] == sr.INLIER).all()
        for t0, t1 in ((0.0, 0.0), (float("inf"), float("inf")), (0.0, float("inf"))):
            ref = sr.segment_f32(real, r_sim, nrm, dirs, origs, RNG[0], RNG[1], t0, t1, flag, add_origin=add)
            out = rcc.segment(est, real, t0, t1, pint_with_origin=flag)
            _exact(out, ref, "%s thresholds (%r, %r) flag %s" % (kind, t0, t1, flag))
            both = np.isfinite(ref["plane"])
            if t0 == t1 == float("inf"):
                assert (out["labels"][both] == sr.INLIER).all()
            if t0 == t1 == 0.0 and (not add or flag):
                assert (out["labels"][both & (real == r_sim)] == sr.INLIER).all() and (out["labels"][both] != sr.INLIER).any()


# ---- 3: a simulated hit below range.min -----------------------------------------------------------------------------------------------------
def test_simulated_hit_below_range_min(ra, orc, ctx):
    """the sensor 5 cm from the wall x = 5: the trace reports those hits with their range (0.05 .. 0.1 m), Interval::inside says the
    simulated range is invalid, and the ray is a scan outlier when measured and nothing otherwise -- the reference's
    `if(range_real_valid) { ... if(range_sim_valid) { ... } else { push preal_s to outlier_scan } }` (scan_map_segmentation_embree.cpp:
    123-170); there the simulated range of such a ray is whatever rmagine's simulator stores for it, which this repository cannot run."""
    from rmcl_amd import types as T
    rcc, _, dirs, origs, add = _case(ra, orc, ctx, "spherical")
    pose = T.transform_from_rpy((4.95, 0.3, 0.2), (0.0, 0.0, 0.0))
    r_sim, nrm = _trace(ra, rcc, pose)
    close = (r_sim > 0) & (r_sim < RNG[0])
    assert close.sum() >= 20 and (r_sim[close] >= f32(0.0499)).all(), (close.sum(), r_sim.min())
    real = np.full(len(r_sim), 3.0, f32)
    real[::3] = 0.0
    real[1::3] = r_sim[1::3]
    ref = sr.segment_f32(real, r_sim, nrm, dirs, origs, RNG[0], RNG[1])
    out = rcc.segment(pose, real)
    _exact(out, ref, "5 cm from the wall")
    valid = (real >= RNG[0]) & (real <= RNG[1])
    assert (close & valid).sum() >= 10 and (close & ~valid).sum() >= 10
    assert (out["labels"][close & valid] == sr.OUTLIER_SCAN).all() and (out["labels"][close & ~valid] == sr.NONE).all()


# ---- 4: more than 1024 workgroups ---------------------------------------------------------------------------------------------------------
def _big(ra, orc, ctx):
    """1026 x 1024 rays = 1026 workgroups of 1024: the scatter's sum over earlier workgroups makes its second trip for the last two"""
    from rmcl_amd import synthetic as syn
    _case(ra, orc, ctx, "spherical")
    if "big_rcc" not in _cache:
        _cache["big_rcc"] = ra.RCCHipSpherical(_cache["map"])          # an operator of its own: the model changes on it
        _cache["big_rcc"].setTsb(_scene(orc)["Tsb"])
    rcc = _cache["big_rcc"]
    rcc.setModel(ec.model_struct(SPH_BIG))
    pose = syn.pose_c2_truth()
    if "big" not in _cache:
        r_sim, nrm = _trace(ra, rcc, pose)
        n = len(r_sim)
        kind = np.arange(n) % 3
        kind[1024 * 500 - 1500:1024 * 500 + 1500] = 0              # 3000 consecutive scan outliers across a workgroup boundary
        kind[1024 * 1025 - 300:1024 * 1025 + 300] = 1              # ... and 600 map outliers across the boundary of the last workgroup
        real = np.where(kind == 0, r_sim * f32(0.5), np.where(kind == 1, r_sim * f32(2.0), r_sim)).astype(f32)
        dirs = ec.spherical_dirs(SPH_BIG)
        _cache["big"] = (real, dirs, sr.segment_f32(real, r_sim, nrm, dirs, np.zeros(3, f32), RNG[0], RNG[1]))
    return (rcc, pose) + _cache["big"]


def test_more_than_1024_workgroups(ra, orc, ctx):
    rcc, pose, real, dirs, ref = _big(ra, orc, ctx)
    n = len(real)
    assert n == 1026 * 1024
    n_scan, n_map = len(ref["outlier_scan"]), len(ref["outlier_map"])
    assert n_scan > n // 4 and n_map > n // 4 and (ref["labels"] == sr.INLIER).sum() > n // 4
    # the workgroups behind the first 1024 have outliers of both kinds below them and of their own
    assert (ref["labels"][1024 * 1024:] == sr.OUTLIER_SCAN).sum() > 100 and (ref["labels"][1024 * 1024:] == sr.OUTLIER_MAP).sum() > 600
    into = dict(labels=ra.DeviceArray.from_host(ctx, np.full(n + 64, 77, np.uint8)),
                outlier_scan=ra.DeviceArray.from_host(ctx, np.full(3 * n + 64, -7.0, f32)),
                outlier_map=ra.DeviceArray.from_host(ctx, np.full(3 * n + 64, -7.0, f32)),
                counts=ra.DeviceArray.from_host(ctx, np.full(4, 0xABCDEF, np.uint32)))
    counts = rcc.segment(pose, real, into=into)
    assert counts == (n_scan, n_map)
    L = into["labels"].download()
    _same(L[:n], ref["labels"], "labels")
    assert (L[n:] == 77).all()
    for name, k in (("outlier_scan", n_scan), ("outlier_map", n_map)):
        pts = into[name].download()
        _same(pts[:3 * k].reshape(-1, 3), ref[name], name)
        assert (pts[3 * k:] == f32(-7.0)).all(), "%s: written beyond its %d points" % (name, k)
    c = into["counts"].download()
    assert tuple(c[:2]) == counts and (c[2:] == 0xABCDEF).all()
    for d in into.values():
        d.free()


# ---- 5: a reused handle -------------------------------------------------------------------------------------------------------------------
def test_large_then_small_models_on_one_operator(ra, orc, ctx):
    """1026 x 1024, then 37 x 53, then 1 x 1 on one operator: the per-workgroup counts and labels of the larger call stay in the
    grow-only scratch -- none of them may leak into the smaller ones"""
    rcc, pose, real, dirs, ref = _big(ra, orc, ctx)
    out = rcc.segment(pose, real)
    _exact(out, ref, "1026 x 1024")
    for m in (SPH_37x53, SPH_ONE):
        rcc.setModel(ec.model_struct(m))
        r_sim, nrm = _trace(ra, rcc, pose)
        n = len(r_sim)
        small = np.where(np.arange(n) % 2 == 0, r_sim * f32(0.5), r_sim * f32(2.0)).astype(f32)
        ref_s = sr.segment_f32(small, r_sim, nrm, ec.spherical_dirs(m), np.zeros(3, f32), RNG[0], RNG[1])
        out = rcc.segment(pose, small)
        _exact(out, ref_s, "%d x %d after the large model" % (m[2], m[5]))
        assert len(out["labels"]) == n and sum(out["counts"]) > 0.9 * n and (n == 1 or min(out["counts"]) > 0.4 * n)
        out = rcc.segment(pose, r_sim)
        assert out["counts"] == (0, 0) and (out["labels"] == sr.INLIER).all()
