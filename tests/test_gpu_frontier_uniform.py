"""The frontier starts compute the tile's pyramid once per wave (traverse.hip.h wave_pyramid: lane l rotates plane l & 3, the values are
taken from lanes 0 - 3), k_find builds one RaySlab per ray and divides a scalar tile index.  None of it may change a bit: every
output of kinds 23, 24 and 32 (default knobs, and final_cap 0 = the plain third step) equals the oracle's and the other kinds' on the
same operator -- hits, ranges, points, normals and face ids, no tolerance anywhere.  The cases are the smallest at which each piece
can go wrong: lanes 0 - 3 without a usable ray, `reach` at its three regimes, a batch whose poses each rotate their own planes, and
the moment epilogue behind the shared slab."""
import math

import numpy as np
import pytest

import descent_cases as dc

pytestmark = pytest.mark.gpu

KINDS = (("kind 23", 23, None), ("kind 24", 24, None), ("kind 32", 32, dc.DEFAULT_KNOBS), ("kind 32 cap 0", 32, (0, 24, 24, False)))


def _view(op):
    mv = op.modelView()
    return {k: np.array(mv[k]) for k in dc.OUTPUT_KEYS}


def _same(got, want, what):
    """every output equal bit for bit (NaN = NaN), with the first differing rays named"""
    n = want["hits"].size
    for k in dc.OUTPUT_KEYS:
        a, b = np.asarray(got[k]).reshape(n, -1), np.asarray(want[k]).reshape(n, -1)
        if np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")):
            continue
        eq = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else (a == b)
        rays = np.flatnonzero(~eq.all(axis=1))
        raise AssertionError("%s: %s differs on %d of %d rays, first rays %s: %s, expected %s"
                             % (what, k, rays.size, n, rays[:8].tolist(), a[rays[:4]].tolist(), b[rays[:4]].tolist()))


def _every_kind(op, find, ref, what, tile_bits=(0,)):
    """`find` under every kind of KINDS and every tile shape of `tile_bits` on the one operator: each result against the oracle's
    `ref` and against the first one; -> the first result"""
    base = None
    for tile in tile_bits:
        for label, kind, knobs in KINDS:
            op.set_variant(dc.variant_word(kind, tile))
            if knobs is not None:
                dc.set_knobs(op, knobs)
            find()
            got = _view(op)
            _same(got, ref, "%s, %s, tile bits %d, against the oracle" % (what, label, tile))
            if base is None:
                base = got
            _same(got, base, "%s, %s, tile bits %d, against %s" % (what, label, tile, KINDS[0][0]))
    return base


def _map(name, meshes):
    """(vertices, faces, a pose inside, range.max with hits and misses)"""
    from rmcl_amd import types as T
    if name == "cube":
        v, f = meshes("cube")
        return v, f, T.transform_from_rpy((0.5, -0.4, 1.2), (0.05, -0.02, 0.7)), 6.0
    v, f = dc.tiny_map(4)
    return v, f, dc.tiny_pose(), 0.8


def _lanes_0_to_3(H, W):
    """the pixels that lanes 0 - 3 of a wave hold under ANY tile shape (2^k x 2^(6 - k) rays, k = 0 .. 6): boolean (H, W)"""
    mask = np.zeros((H, W), bool)
    for twl in range(7):
        tw, th = 1 << twl, 64 >> twl
        for lane in range(4):
            lx, ly = lane & (tw - 1), lane >> twl
            mask[ly::th, lx::tw] = True
    return mask


@pytest.mark.parametrize("name", ["cube", "tiny4"])
def test_waves_whose_first_lanes_carry_no_ray(ra, orc, ctx, meshes, name):
    """1 x 1, 1 x 3, 2 x 2 and 5 x 17 rays under every tile shape: lanes 0 - 3 compute the planes whether or not they hold a ray"""
    from rmcl_amd import types as T
    v, f, pose, far = _map(name, meshes)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    f32 = np.float32
    hits = 0
    for (H, W) in [(1, 1), (1, 3), (2, 2), (5, 17)]:
        model = T.spherical_model(f32(-0.6), f32(1.2 / max(H - 1, 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(far))
        ref = m.simulate_spherical(model, T.identity(), pose, bvh=False)
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        base = _every_kind(rcc, lambda: rcc.find(pose), ref, "%s %dx%d" % (name, H, W), dc.TILE_BITS)
        hits += int(base["hits"].sum())
        rcc.close()
    assert hits > 10
    hm.release()


def test_o1dn_whose_first_four_directions_of_every_tile_are_nan(ra, orc, ctx, meshes):
    """lanes 0 - 3 of every wave hold a NaN direction (ray_tfar < 0) under each tile shape, and still rotate the planes"""
    from rmcl_amd import synthetic as syn, types as T
    v, f, pose, _ = _map("cube", meshes)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    f32 = np.float32
    W, H = 64, 16
    sm = T.spherical_model(f32(-0.5), f32(1.0 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(6.0))
    dirs = syn.model_directions(sm).copy()
    dirs[_lanes_0_to_3(H, W).reshape(-1)] = np.nan
    orig = (0.0, 0.0, 0.0)
    ref = m.simulate_o1dn(W, H, 0.0, 6.0, orig, dirs, T.identity(), pose, bvh=False)
    assert ref["hits"].sum() > 10 and not ref["hits"].reshape(H, W)[_lanes_0_to_3(H, W)].any()
    ro = ra.RCCHipO1Dn(hm)
    ro.setTsb(T.identity())
    ro.setModel(W, H, 0.0, 6.0, orig, dirs)
    _every_kind(ro, lambda: ro.find(pose), ref, "cube o1dn with NaN first lanes", dc.TILE_BITS)
    ro.close()
    hm.release()


def _look_at(pos, target):
    """a pose at `pos` whose +x axis points at `target`"""
    from rmcl_amd import types as T
    d = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    yaw, pitch = math.atan2(d[1], d[0]), -math.atan2(d[2], math.hypot(d[0], d[1]))
    return T.transform_from_rpy(tuple(float(x) for x in pos), (0.0, pitch, yaw))


@pytest.mark.parametrize("name", ["cube", "tiny4"])
def test_reach_and_offsets_over_four_finds_on_one_operator(ra, orc, ctx, meshes, name):
    """`reach` = the distance to the map's bounding sphere (sensor at the centre, 3 m outside, 1 km outside looking at it; range.max
    1e12), then = the sensor's range (the first pose again, range.max 0.5 m): one operator, the finds in a row"""
    from rmcl_amd import types as T
    v, f, _, _ = _map(name, meshes)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    centre, half = np.unique(vv, axis=0).mean(0), 0.5 * (vv.max(0) - vv.min(0))     # (the centroid: inside both maps)
    f32 = np.float32
    H, W = 9, 32       # (an odd number of rows: the central ray of a sensor that looks at the map hits it from any distance)

    def model(far):
        return T.spherical_model(f32(-0.5), f32(1.0 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(far))

    at_centre = T.transform_from_rpy(tuple(float(x) for x in centre + 0.1 * half), (0.1, -0.05, 0.3))
    outside = _look_at(centre + np.array([half[0] + 3.0, 0.3, 0.2]), centre)
    far_out = _look_at(centre + np.array([600.0, -700.0, 400.0]) * (1000.0 / math.sqrt(600.0 ** 2 + 700.0 ** 2 + 400.0 ** 2)), centre)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model(1e12))
    hits = []
    for label, pose in (("at the centre", at_centre), ("3 m outside", outside), ("1 km outside", far_out)):
        ref = m.simulate_spherical(model(1e12), T.identity(), pose, bvh=False)
        hits.append(int(_every_kind(rcc, lambda: rcc.find(pose), ref, "%s %s" % (name, label))["hits"].sum()))
    assert min(hits) > 0, hits
    rcc.setModel(model(0.5))
    ref = m.simulate_spherical(model(0.5), T.identity(), at_centre, bvh=False)
    _every_kind(rcc, lambda: rcc.find(at_centre), ref, "%s at the centre, range.max 0.5" % name)
    rcc.close()
    hm.release()


def test_o1dn_with_an_origin_and_a_mount(ra, orc, ctx, meshes):
    """a non-zero ray origin through a non-identity Tsb: the wave's origin goes through xapply"""
    from rmcl_amd import synthetic as syn, types as T
    v, f, pose, _ = _map("cube", meshes)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    f32 = np.float32
    W, H = 32, 8
    sm = T.spherical_model(f32(-0.5), f32(1.0 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(6.0))
    dirs = syn.model_directions(sm).copy()
    orig, Tsb = (0.3, -0.2, 0.15), syn.tsb_offset()
    ref = m.simulate_o1dn(W, H, 0.0, 6.0, orig, dirs, Tsb, pose, bvh=False)
    assert 10 < ref["hits"].sum() < ref["hits"].size
    ro = ra.RCCHipO1Dn(hm)
    ro.setTsb(Tsb)
    ro.setModel(W, H, 0.0, 6.0, orig, dirs)
    _every_kind(ro, lambda: ro.find(pose), ref, "cube o1dn with origin and mount")
    ro.close()
    hm.release()


def _batch_case(ra, orc, ctx, meshes):
    from rmcl_amd import synthetic as syn, types as T
    v, f, pose, _ = _map("cube", meshes)
    f32 = np.float32
    H, W = 8, 16
    model = T.spherical_model(f32(-0.5), f32(1.0 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(6.0))
    poses = np.array([T.mult(pose, T.transform_from_rpy((0.2 * i, -0.1 * i, 0.05), rpy))
                      for i, rpy in enumerate([(0.0, 0.0, 0.0), (0.9, -0.4, 2.0), (-1.3, 0.7, -2.6)])], dtype=T.TRANSFORM)
    hm = ra.import_hip_map(ctx, v, f)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    rcc.setModel(model)
    ref = orc.Mesh(v, f).simulate_spherical(model, syn.tsb_offset(), poses, bvh=False)
    return hm, rcc, poses, ref, H * W


def _batch_checks(ra, ctx, rcc, poses, ref, n, what):
    """the batch from host poses and from a device array under every kind, against the oracle; pose i's slice = the single find"""
    assert 10 < ref["hits"].sum() < ref["hits"].size
    _every_kind(rcc, lambda: rcc.find_batch(poses), ref, what + " host poses")
    d_poses = ra.DeviceArray.from_host(ctx, poses)
    for label, kind, knobs in KINDS:
        rcc.set_variant(dc.variant_word(kind))
        if knobs is not None:
            dc.set_knobs(rcc, knobs)
        got = rcc.download_bundle(rcc.simulate(len(poses), attributes=dc.OUTPUT_KEYS, poses_dev=d_poses))
        _same(got, ref, "%s device poses, %s, against the oracle" % (what, label))
        for i in range(len(poses)):
            rcc.find(poses[i])
            one = _view(rcc)
            _same({k: np.asarray(got[k]).reshape(len(poses), n, -1)[i] for k in dc.OUTPUT_KEYS}, one,
                  "%s %s: pose %d of the batch against its single find" % (what, label, i))
    d_poses.free()


def test_each_pose_of_a_batch_rotates_its_own_planes(ra, orc, ctx, meshes):
    """three poses with three rotations, 8 x 16 rays, in world order (the default)"""
    hm, rcc, poses, ref, n = _batch_case(ra, orc, ctx, meshes)
    _batch_checks(ra, ctx, rcc, poses, ref, n, "cube 3 poses x 8x16, world order,")
    rcc.close()
    hm.release()


@pytest.mark.lab
def test_each_pose_of_a_pose_major_batch_rotates_its_own_planes(ra, orc, ctx, meshes):
    """... and launched pose-major (rmclhip_rcc_set_batch_order 0, include/rmclhip_lab.h)"""
    from rmcl_amd import _capi
    hm, rcc, poses, ref, n = _batch_case(ra, orc, ctx, meshes)
    _capi.check(_capi.lib().rmclhip_rcc_set_batch_order(rcc._h, 0))
    _batch_checks(ra, ctx, rcc, poses, ref, n, "cube 3 poses x 8x16, pose-major,")
    rcc.close()
    hm.release()


def test_moment_epilogue_is_the_same_under_kinds_23_and_32(ra, orc, ctx, meshes):
    """correct_once, 3 iterations on the cube: the pose and the CrossStatistics of kinds 23 and 32 are the same bits, and within each
    kind a second identical call returns the same bits"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cube")
    hm = ra.import_hip_map(ctx, v, f)
    truth = syn.pose_c2_truth()
    est = T.mult(truth, T.transform_from_rpy((0.03, -0.02, 0.015), (0.004, -0.003, 0.008)))
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    rcc.setModel(syn.model_c1())
    rcc.set_variant(dc.variant_word(23))
    rcc.find(truth)
    rcc.set_dataset_from_ranges(rcc.modelView()["ranges"])
    rcc.params.max_dist = 0.5
    out = {}
    for kind in (23, 32):
        rcc.set_variant(dc.variant_word(kind))
        if kind == 32:
            dc.set_knobs(rcc, dc.DEFAULT_KNOBS)
        for call in (0, 1):
            Tc, st = rcc.correct_once(est, T.identity(), 3, 0.0, False)
            out[(kind, call)] = (np.array(Tc).tobytes()[:28], np.array(st).tobytes(), int(st["n_meas"]))
        assert out[(kind, 0)] == out[(kind, 1)], "kind %d: a second identical call returns other bits" % kind
    assert out[(23, 0)][2] > 500, out[(23, 0)][2]
    assert out[(23, 0)][0] == out[(32, 0)][0], "the corrected pose differs between kinds 23 and 32"
    assert out[(23, 0)][1] == out[(32, 0)][1], "the CrossStatistics differ between kinds 23 and 32"
    rcc.close()
    hm.release()
