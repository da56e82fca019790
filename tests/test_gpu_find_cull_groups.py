"""Find kind 32 culls the frontier table by groups (traverse.hip.h frontier_descent_start): a wave tests the table's 16 group boxes
first and skips every block of 64 entries none of whose four groups touches its tile's pyramid, and its box tests are formed as wave
masks (box_in_pyramid_mask).  Neither may change a bit of a result: kind 32 against kind 23 and against the oracle, all five outputs
bit for bit, with 32 x 64 and 64 x 256 scans:

  (a) sphere-100k and room-100k from inside;
  (b) a sensor outside the map with the whole map inside ONE tile's pyramid: every group survives, all four blocks run;
  (c) a map whose table has <= 64 entries (a cube room of 4 x 4 cells per wall, 56 entries): no group table, every wave runs every block;
  (d) maps of 86 (5 x 5 cells) and 247 entries (the 972-triangle cube): short last groups;
  (e) frontiers that contain leaves: the four-triangle map, the chain and nest maps of tests/descent_cases.py's hard maps;
  (f) NaN directions (O1Dn) and an OnDn model (no pyramid: its rays start at the root);
  (g) a pose batch and the moment epilogue.

The witnesses read the per-wave word 15 of the clocked kind 32 (experiments library): bits 0..3 = the blocks of the cull a wave ran."""
import math

import numpy as np
import pytest

import descent_cases as dc

pytestmark = [pytest.mark.gpu, pytest.mark.lab]     # lab: the clocked kind 32 that witnesses the skip

f32 = np.float32
SHAPES = ((32, 64), (64, 256))
ROOM_POSE_RPY = ((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))


def _model(H, W, half_phi=math.pi / 4, rmin=0.0, rmax=120.0):
    from rmcl_amd import types as T
    return T.spherical_model(f32(-half_phi), f32(2 * half_phi / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(rmin), f32(rmax))


def _view(op):
    mv = op.modelView()
    return {k: np.array(mv[k]) for k in dc.OUTPUT_KEYS}


def _bit_equal(got, want, what):
    n = got["hits"].size
    for k in dc.OUTPUT_KEYS:
        a, b = got[k].reshape(n, -1), want[k].reshape(n, -1)
        eq = (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a == b)
        eq = eq | ((a != a) & (b != b))     # (NaN points / normals of a miss: any NaN)
        rays = np.flatnonzero(~eq.all(axis=1))
        assert rays.size == 0, "%s: %s differs on %d of %d rays, first rays %s: %s against %s" % (
            what, k, rays.size, n, rays[:8].tolist(), a[rays[:4]].tolist(), b[rays[:4]].tolist())


def _against_oracle(got, ref, what):
    """all five outputs against the oracle bit for bit; the figures are printed before they are asserted"""
    n = got["hits"].size
    diff = {}
    for k in dc.OUTPUT_KEYS:
        a, b = got[k].reshape(n, -1), np.asarray(ref[k]).reshape(n, -1)
        eq = (a == b) | ((a != a) & (b != b))
        diff[k] = int((~eq.all(axis=1)).sum())
    if any(diff.values()):
        print("%s against the oracle, rays that differ of %d: %s" % (what, n, diff))
    _bit_equal(got, {k: np.asarray(ref[k]).astype(got[k].dtype, copy=False) for k in dc.OUTPUT_KEYS}, what + " against the oracle")


KNOBS = (dc.DEFAULT_KNOBS, (64, 24, 24, True), (12, 24, 24, False))     # the 16-wide twins (<= 4 inner survivors per pass), four-wide nodes (<= 16), a short final list


def _kinds(op, find, ref, what, tile_bits=0):
    """kind 23 against the oracle; kind 32 under three knob sets against the oracle and against kind 23 bit for bit; -> kind 23's outputs"""
    op.set_variant(dc.variant_word(23, tile_bits))
    find()
    base = _view(op)
    _against_oracle(base, ref, what + " kind 23")
    for knobs in KNOBS:
        op.set_variant(dc.variant_word(32, tile_bits))
        dc.set_knobs(op, knobs)
        find()
        got = _view(op)
        label = "%s kind 32 %s" % (what, dc.knob_name(knobs))
        _against_oracle(got, ref, label)
        _bit_equal(got, base, label + " against kind 23")
    op.set_variant(dc.variant_word(32, tile_bits))
    dc.set_knobs(op, dc.DEFAULT_KNOBS)
    return base


def _flags(rcc, pose, knobs=dc.DEFAULT_KNOBS, tile_bits=0):
    """word 15 of every wave of one clocked kind-32 scan that ran"""
    rcc.set_variant(dc.variant_word(32, tile_bits))
    dc.set_knobs(rcc, knobs)
    w = rcc.debug_wave_clock(pose)
    ran = w[:, 1] != 0
    return rcc._last_descent_stamps[ran][:, 15].astype(np.int64)


def _spherical(ra, hm, model, Tsb):
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    return rcc


# ---- (a) the benchmark maps from inside ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere100k", "room100k"])
def test_inside_the_benchmark_maps(ra, orc, ctx, meshes, name):
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes(name)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    pose = syn.pose_c2_truth() if name == "sphere100k" else T.transform_from_rpy(*ROOM_POSE_RPY)
    for H, W in SHAPES:
        model = _model(H, W, half_phi=math.pi / 8)
        ref = m.simulate_spherical(model, T.identity(), pose, bvh=True, nthreads=16)
        rcc = _spherical(ra, hm, model, T.identity())
        base = _kinds(rcc, lambda: rcc.find(pose), ref, "%s %dx%d" % (name, H, W))
        assert base["hits"].sum() > H * W // 2
        rcc.close()
    hm.release()


# ---- (b) the whole map inside one tile's pyramid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["32x64", "64x256"])
def test_from_outside_every_group_survives(ra, orc, ctx, meshes, shape):
    """8 x 8 tiles (tile bits 4); the sensor stands where sphere-20k (radius 10 m, a full table) fills 0.8 of the smaller side of the
    tile whose centre looks at it: that wave keeps all 16 groups and all 256 entries"""
    from rmcl_amd import types as T
    H, W = shape
    v, f = meshes("sphere20k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = _model(H, W, half_phi=1.4, rmax=1000.0)
    phi = float(model.phi.min) + (8 * (H // 16 - 1) + 3.5) * float(model.phi.inc)       # the centre of the tile row below the horizon ...
    theta = float(model.theta.min) + 27.5 * float(model.theta.inc)                      # ... and of tile column 3
    side = 8.0 * min(float(model.phi.inc), float(model.theta.inc) * math.cos(phi))      # (columns close in towards the poles)
    d = 10.0 / math.sin(0.4 * side)
    look = np.array([math.cos(phi) * math.cos(theta), math.cos(phi) * math.sin(theta), math.sin(phi)])
    pose = T.transform_from_rpy(tuple((-d * look).tolist()), (0.0, 0.0, 0.0))
    ref = m.simulate_spherical(model, T.identity(), pose, bvh=True, nthreads=16)
    rcc = _spherical(ra, hm, model, T.identity())
    base = _kinds(rcc, lambda: rcc.find(pose), ref, "sphere20k from %.0f m, %dx%d" % (d, H, W), tile_bits=4)
    assert 8 <= base["hits"].sum() <= 64, "the sphere lies inside one tile"
    tiles = np.flatnonzero(base["hits"].reshape(H, W))
    assert len({(i // W // 8, i % W // 8) for i in tiles}) == 1, "every hit in ONE 8 x 8 tile"
    fl = _flags(rcc, pose, tile_bits=4)
    print("from outside %dx%d: blocks run %s" % (H, W, np.bincount(fl & 0xF, minlength=16).tolist()))
    assert ((fl & 0xF) == 0xF).sum() >= 1, "the wave that sees the whole map runs all four blocks"
    assert ((fl & 0xF) == 0).sum() >= fl.size // 2, "waves that look away keep no group at all"
    rcc.close()
    hm.release()


# ---- (c), (d), (e): small tables, short groups, leaves in the frontier -----------------------------------------------------------
def _small_maps(meshes):
    from rmcl_amd import synthetic as syn, types as T
    I = T.identity()
    inside = [syn.pose_c2_truth(), T.transform_from_rpy((-2.1, 1.3, -0.7), (0.3, -0.2, 2.5))]
    chain_model = lambda H, W: T.spherical_model(f32(-0.2), f32(0.4 / (H - 1)), H, f32(-0.3), f32(0.6 / W), W, f32(0.0), f32(1e30))
    nest_model = lambda H, W: T.spherical_model(f32(-0.4), f32(1.85 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(1e12))
    tiny_model = lambda H, W: T.spherical_model(f32(-math.pi / 4), f32((math.pi / 2) / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(0.8))
    return {
        # name: (mesh, model of a shape, Tsb, poses, entries of the map tree's table: (least, most), leaves in it)
        "cube4": (syn.cube_room(grid=4), _model, syn.tsb_offset(), inside, (1, 64), True),
        "cube5": (syn.cube_room(grid=5), _model, syn.tsb_offset(), inside, (65, 128), True),
        "cube": (meshes("cube"), _model, syn.tsb_offset(), inside, (129, 255), True),
        "four_triangles": (dc.tiny_map(4), tiny_model, I, [dc.tiny_pose()], (1, 1), True),
        "chain200": (meshes("chain200"), chain_model, I, [T.transform_from_rpy((-1.0, 0.04, 0.03), (0.0, 0.0, 0.0)), T.transform_from_rpy((-50.0, 2.0, 1.0), (0.0, 0.0, 0.0))], (2, 64), True),
        "nested200": (meshes("nested200"), nest_model, I, [T.transform_from_rpy((0.001, -0.002, -1.0), (0.0, 0.0, 0.3)), T.transform_from_rpy((0.8, 0.3, -2.5), (0.05, -0.1, 1.0))], (2, 64), True),
    }


@pytest.mark.parametrize("name", ["cube4", "cube5", "cube", "four_triangles", "chain200", "nested200"])
def test_small_tables_short_groups_and_leaves_in_the_frontier(ra, orc, ctx, meshes, name):
    (v, f), model_of, Tsb, poses, (least, most), leaves = _small_maps(meshes)[name]
    table, groups = ra.build_bvh_host_frontier(v, f)
    assert least <= len(table) <= most, "%s: %d entries" % (name, len(table))
    assert bool((table[:, 6] >> 31).any()) == leaves
    if name in ("cube5", "cube"):
        assert len(table) % 16 != 0 and int(groups[len(table) // 16, 6]) == len(table) % 16, "a short last group"
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    n_hits = 0
    for H, W in SHAPES:
        model = model_of(H, W)
        rcc = _spherical(ra, hm, model, Tsb)
        for i, pose in enumerate(poses):
            ref = m.simulate_spherical(model, Tsb, pose, bvh=False, nthreads=16)
            base = _kinds(rcc, lambda: rcc.find(pose), ref, "%s %dx%d pose %d" % (name, H, W, i))
            n_hits += int(base["hits"].sum())
        fl = _flags(rcc, poses[0])
        print("%s %dx%d: %d entries, blocks run %s" % (name, H, W, len(table), np.bincount(fl & 0xF, minlength=16).tolist()))
        if len(table) <= 64:
            assert ((fl & 0xF) == 0xF).all(), "a table of one block has no group table: nothing is skipped"
        rcc.close()
    assert n_hits > 100, "the scans must see the map"
    hm.release()


# ---- (f) NaN directions, and a model without a pyramid ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["32x64", "64x256"])
def test_nan_directions_and_ondn(ra, orc, ctx, meshes, shape):
    from rmcl_amd import synthetic as syn, types as T
    H, W = shape
    v, f = meshes("sphere20k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    dirs = syn.model_directions(_model(H, W)).copy()
    dirs[np.random.RandomState(5).randint(0, len(dirs), 40)] = np.nan
    dirs[100, 1] = np.nan
    orig = (0.05, -0.02, 0.11)
    Tsb, pose = syn.tsb_offset(), T.transform_from_rpy((-1.0, 0.7, 1.1), (0.02, 0.03, 1.9))
    ro = ra.RCCHipO1Dn(hm)
    ro.setTsb(Tsb)
    ro.setModel(W, H, 0.0, 40.0, orig, dirs)
    base = _kinds(ro, lambda: ro.find(pose), m.simulate_o1dn(W, H, 0.0, 40.0, orig, dirs, Tsb, pose, bvh=True, nthreads=16), "sphere20k o1dn %dx%d with NaN directions" % (H, W))
    assert (base["hits"] == 0).sum() >= 30 and base["hits"].sum() > H * W // 2
    ro.close()
    origs = np.random.RandomState(6).uniform(-0.3, 0.3, (W * H, 3)).astype(np.float32)
    rn = ra.RCCHipOnDn(hm)
    rn.setTsb(Tsb)
    rn.setModel(W, H, 0.0, 40.0, origs, dirs)
    base = _kinds(rn, lambda: rn.find(pose), m.simulate_ondn(W, H, 0.0, 40.0, origs, dirs, Tsb, pose, bvh=True, nthreads=16), "sphere20k ondn %dx%d" % (H, W))
    assert (base["hits"] == 0).sum() >= 30 and base["hits"].sum() > H * W // 2
    rn.close()
    hm.release()


# ---- (g) a pose batch, the moment epilogue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["32x64", "64x256"])
def test_pose_batch(ra, orc, ctx, meshes, shape):
    from rmcl_amd import synthetic as syn, types as T
    H, W = shape
    v, f = meshes("room30k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = _model(H, W, half_phi=math.pi / 8)
    rng = np.random.RandomState(18)
    base_pose = T.transform_from_rpy(*ROOM_POSE_RPY)
    poses = np.array([T.mult(base_pose, T.transform_from_rpy(tuple(rng.uniform(-1.5, 1.5, 3) * (1, 1, 0.2)), (0.0, 0.0, rng.uniform(-3, 3))))
                      for _ in range(3)], dtype=T.TRANSFORM)
    ref = m.simulate_spherical(model, syn.tsb_offset(), poses, bvh=True, nthreads=16)
    rcc = _spherical(ra, hm, model, syn.tsb_offset())
    base = _kinds(rcc, lambda: rcc.find_batch(poses), ref, "room30k 3 poses x %dx%d" % (H, W))
    assert base["hits"].size == 3 * H * W and 0 < base["hits"].sum() < base["hits"].size
    rcc.close()
    hm.release()


@pytest.mark.parametrize("shape", SHAPES, ids=["32x64", "64x256"])
def test_moment_epilogue(ra, ctx, meshes, shape):
    """a correction whose find forms the moments in its epilogue: kind 32 finds the correspondences kind 23 finds -- the same n_meas, the
    same pose to 1e-6 absolute (tests/test_gpu_find_descent.py: f64 partial sums in another order)"""
    from rmcl_amd import synthetic as syn, types as T
    H, W = shape
    v, f = meshes("room30k")
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy(*ROOM_POSE_RPY)
    est = T.mult(Tbm, T.transform_from_rpy((0.03, -0.02, 0.015), (0.004, -0.003, 0.008)))
    rcc = _spherical(ra, hm, _model(H, W, half_phi=math.pi / 8), syn.tsb_offset())
    rcc.set_traversal(23)
    rcc.find(Tbm)
    rcc.set_dataset_from_ranges(rcc.modelView()["ranges"])
    rcc.params.max_dist = 0.5

    def correct(kind, knobs=None):
        rcc.set_traversal(kind)
        if knobs is not None:
            dc.set_knobs(rcc, knobs)
        rcc.find(Tbm)
        Tc, st = rcc.correct_once(est, T.identity(), 4, 0.0, False)
        return np.frombuffer(np.array(Tc).tobytes()[:28], dtype=np.float32).astype(np.float64), int(st["n_meas"])

    want = correct(23)
    assert want[1] > H * W // 4
    for knobs in KNOBS:
        got = correct(32, knobs)
        print("moments %dx%d %s: n_meas %d (kind 23: %d), largest pose difference %.3g" % (H, W, dc.knob_name(knobs), got[1], want[1], np.abs(got[0] - want[0]).max()))
        assert got[1] == want[1], (dc.knob_name(knobs), got[1], want[1])
        assert np.allclose(got[0], want[0], rtol=0.0, atol=1e-6), (dc.knob_name(knobs), got[0], want[0])
    rcc.close()
    hm.release()


# ---- the witnesses -----------------------------------------------------------------------------------------------------------------
def test_waves_skip_blocks_inside_the_benchmark_maps(ra, ctx, meshes):
    """64 x 256 scans from inside the two benchmark maps (full tables): some wave skips blocks of the cull.  (Waves that run all four:
    test_from_outside_every_group_survives and the small tables above.)"""
    from rmcl_amd import synthetic as syn, types as T
    skipped = 0
    for name, pose in (("sphere100k", syn.pose_c2_truth()), ("room100k", T.transform_from_rpy(*ROOM_POSE_RPY))):
        hm = ra.import_hip_map(ctx, *meshes(name))
        rcc = _spherical(ra, hm, _model(64, 256, half_phi=math.pi / 8), T.identity())
        blocks = _flags(rcc, pose) & 0xF
        print("%s: %d waves, blocks run %s" % (name, blocks.size, np.bincount(blocks, minlength=16).tolist()))
        assert (blocks != 0).all(), "inside a closed map every tile sees some of it"
        skipped += int((blocks != 0xF).sum())
        rcc.close()
        hm.release()
    assert skipped > 0, "no wave skipped a block of the cull"
