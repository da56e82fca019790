"""GPU parity of find kind 32 (the cooperative descent below the frontier, traverse.hip.h frontier_descent_start<..., kCoop = true>) on
every path its knobs and its data open: each knob set of tests/descent_cases.py (final caps 64 / 32 / 12 / 0, 0 / 1 / 2 / all levels,
leaf caps 1 / 24 / 255, 16-wide and four-wide nodes) and each tile shape on the hard maps, against the oracle with the project's
bars (hits and face ids bit-exact; ranges, points and normals 1e-5 relative) AND against kind 23 on the same operator bit for bit
-- rmclhip_rcc_set_descent promises "results do not depend on any of them", the kernel "bit-identical to kind 23".

Which path a case takes is WITNESSED by test_reach_witness (clocked instantiation of the experiments library: the descent word and
two fallback flags of every wave); a failure message names the map, the scan, the knob set, the tile bits and the first rays."""
import math

import numpy as np
import pytest

import descent_cases as dc
from test_gpu_find import _compare, ROOM_POSE_RPY

pytestmark = pytest.mark.gpu


def _view(op):
    mv = op.modelView()
    return {k: np.array(mv[k]) for k in dc.OUTPUT_KEYS}


def _same(got, want, what):
    """np.array_equal(..., equal_nan=True) on all five outputs, with the rays named"""
    n = got["hits"].size
    for k in dc.OUTPUT_KEYS:
        if np.array_equal(got[k], want[k], equal_nan=True):
            continue
        a, b = got[k].reshape(n, -1), want[k].reshape(n, -1)
        eq = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else (a == b)
        rays = np.flatnonzero(~eq.all(axis=1))
        raise AssertionError("%s: %s differs from kind 23 on %d of %d rays, first rays %s: %s, kind 23 %s"
                             % (what, k, rays.size, n, rays[:8].tolist(), a[rays[:4]].tolist(), b[rays[:4]].tolist()))


def _check(got, ref, base, what):
    bad = np.flatnonzero((got["hits"] != ref["hits"]) | (got["face_ids"] != ref["face_ids"]))
    assert bad.size == 0, "%s: hits / face ids differ from the oracle on %d of %d rays, first rays %s: face ids %s, the oracle's %s" % (
        what, bad.size, got["hits"].size, bad[:8].tolist(), got["face_ids"][bad[:8]].tolist(), ref["face_ids"][bad[:8]].tolist())
    _compare(got, ref, what)
    _same(got, base, what)


def _sweep(op, find, ref, what, knob_sets=dc.KNOB_SETS, tile_knobs=dc.TILE_KNOBS, tile_bits=dc.TILE_BITS):
    """kind 23, then kind 32 with every knob set (automatic tile shape) and `tile_knobs` through every forced tile shape, all on the
    one operator `op` (`find` launches and leaves the result in its model buffers); -> kind 23's result"""
    op.set_variant(dc.variant_word(23))
    find()
    base = _view(op)
    _compare(base, ref, what + " kind 23")
    runs = [(k, 0) for k in knob_sets] + [(k, t) for t in tile_bits if t != 0 for k in tile_knobs]
    for knobs, tile in runs:
        op.set_variant(dc.variant_word(32, tile))
        dc.set_knobs(op, knobs)             # (a complete word: cap, levels, leaf cap, width; the tile-mapping override off)
        find()
        _check(_view(op), ref, base, "%s kind 32 %s tile bits %d" % (what, dc.knob_name(knobs), tile))
    op.set_variant(dc.variant_word(32))
    dc.set_knobs(op, dc.DEFAULT_KNOBS)
    return base


# ---- the hard maps: (vertices, faces, [(label, spherical model, Tsb, pose, the oracle's bvh argument)]) --------------------------
HARD_MAPS = ("sphere100k", "room100k", "turned_beams", "fan20k", "nested200", "chain200", "chain2000", "cube", "duplicates", "one_triangle",
             "four_triangles")


def _ragged_c2(syn, H, W):
    model = syn.model_c2()
    model.phi.inc = model.phi.inc * 128.0 / H
    model.phi.size = H
    model.theta.inc = model.theta.inc * 1024.0 / W
    model.theta.size = W
    return model


def _hard_map(name, meshes):
    from rmcl_amd import synthetic as syn, types as T
    f32 = np.float32
    I = T.identity()
    H, W = 48, 256
    if name == "sphere100k":        # the oracle's BVH walk is the authority on the two benchmark maps (itself pinned against brute force in test_gpu_find.py)
        v, f = meshes(name)
        scans = [("C2", syn.model_c2(), I, syn.pose_c2_truth(), True), ("100x1000", _ragged_c2(syn, 100, 1000), syn.tsb_offset(), syn.pose_c2_truth(), True)]
    elif name == "room100k":
        v, f = meshes(name)
        pose = T.transform_from_rpy(*ROOM_POSE_RPY)
        scans = [("C2", syn.model_c2(), I, pose, True), ("100x1000", _ragged_c2(syn, 100, 1000), syn.tsb_offset(), pose, True)]
    elif name == "turned_beams":    # spatial splits: a face in several leaves, the same record tested twice by one ray
        v, f = syn.cad_mix(20000, beam_yaw_deg=35.0, beam_tilt_deg=12.0, n_beams=60)
        scans = [("C2", syn.model_c2(), I, T.transform_from_rpy((-6.0, 0.5, 1.5), (0.3, 0.1, -1.0)), 2)]
    elif name == "fan20k":          # massively overlapping boxes: more than 64 survivors, rays that enter many leaves
        v, f = meshes(name)
        model = T.spherical_model(f32(-1.5), f32(3.0 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.01), f32(1e6))
        scans = [("pose %d" % i, model, I, p, False) for i, p in enumerate(
            [T.transform_from_rpy((1.0, 2.0, 3.0), (0.1, 0.2, 0.3)), T.transform_from_rpy((0.01, 0.02, -0.5), (0.0, 0.0, 1.0))])]
    elif name == "nested200":       # stack_need 57 / 56 (chain200): a preload of 7 / 8; 64 (chain2000): no room for a preload, the table is switched off
        v, f = meshes(name)
        model = T.spherical_model(f32(-0.4), f32(1.85 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(1e12))
        scans = [("pose %d" % i, model, I, p, False) for i, p in enumerate(
            [T.transform_from_rpy((0.001, -0.002, -1.0), (0.0, 0.0, 0.3)), T.transform_from_rpy((0.8, 0.3, -2.5), (0.05, -0.1, 1.0))])]
    elif name in ("chain200", "chain2000"):
        v, f = meshes(name)
        model = T.spherical_model(f32(-0.2), f32(0.4 / (H - 1)), H, f32(-0.3), f32(0.6 / W), W, f32(0.0), f32(1e30))
        scans = [("pose %d" % i, model, I, p, False) for i, p in enumerate(
            [T.transform_from_rpy((-1.0, 0.04, 0.03), (0.0, 0.0, 0.0)), T.transform_from_rpy((-1e-6, 2e-8, 1e-8), (0.0, 0.0, 0.0)),
             T.transform_from_rpy((-50.0, 2.0, 1.0), (0.0, 0.0, 0.0))])]
    elif name == "cube":            # 972 triangles: the frontier is mostly leaves
        v, f = meshes(name)
        scans = [("pose %d" % i, syn.model_c1(), syn.tsb_offset(), p, False) for i, p in enumerate(
            [syn.pose_c2_truth(), T.transform_from_rpy((-2.1, 1.3, -0.7), (0.3, -0.2, 2.5)), T.transform_from_rpy((3.9, -3.3, 2.2), (-0.1, 0.25, -1.2))])]
    elif name == "duplicates":      # every hit is a tie: the smaller face id wins wherever the two copies sit
        v, f = dc.random_map("duplicates")
        model = T.spherical_model(f32(-1.2), f32(2.4 / 63), 64, f32(-math.pi), f32(2 * math.pi / 256), 256, f32(0.0), f32(100.0))
        scans = [("c1", syn.model_c1(), syn.tsb_offset(), T.transform_from_rpy((0.3, -0.2, 0.1), (0.13, -0.27, 0.9)), False),
                 ("64x256", model, I, T.transform_from_rpy((-3.0, 2.5, -1.0), (0.4, 0.2, -2.0)), False)]
    elif name in ("one_triangle", "four_triangles"):    # the smallest maps
        v, f = dc.tiny_map(1 if name == "one_triangle" else 4)
        scans = [("tiny", dc.tiny_model(), I, dc.tiny_pose(), False), ("c1", syn.model_c1(), syn.tsb_offset(), T.transform_from_rpy((0.4, 0.3, 3.0), (0.0, 0.6, 0.2)), False)]
    else:
        raise KeyError(name)
    return v, f, scans


@pytest.mark.parametrize("name", HARD_MAPS)
def test_every_knob_set_and_tile_shape_on_the_hard_maps(ra, orc, ctx, meshes, name):
    """every knob set, and three of them through six tile shapes, on one hard map: the oracle (brute force where the map is small
    enough or the oracle's own tree is not the point) and kind 23"""
    v, f, scans = _hard_map(name, meshes)
    hm = ra.import_hip_map(ctx, v, f)           # (a refused upload is a finding: no mesh is refused)
    info = hm.info()
    assert info["stack_need"] <= 64
    m = orc.Mesh(v, f)
    n_hits = 0
    for label, model, Tsb, pose, bvh in scans:
        ref = m.simulate_spherical(model, Tsb, pose, bvh=bvh, nthreads=16)
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(Tsb)
        rcc.setModel(model)
        base = _sweep(rcc, lambda: rcc.find(pose), ref, "%s %s" % (name, label))
        n_hits += int(base["hits"].sum())
        rcc.close()
    assert n_hits > (100 if name != "one_triangle" else 10), "the scans must see the map"
    if name == "duplicates":
        ids = np.concatenate([m.simulate_spherical(model, Tsb, pose, bvh=False, nthreads=16)["face_ids"] for _, model, Tsb, pose, _ in scans])
        assert len(np.unique(ids[ids != 0xFFFFFFFF])) > 100
    if name in ("nested200", "chain200"):
        assert 50 < info["stack_need"] < 63, "a deep tree: room for a small preload only"
    if name == "chain2000":
        assert info["stack_need"] >= 63, "no room for a preload: the frontier table is switched off, every ray starts at the root"
    hm.release()


def test_tiny_and_ragged_models(ra, orc, ctx, meshes):
    """1 x 1, 1 x 360, 7 x 33 and 65 x 9 rays on room-30k: waves with one ray, ragged tiles, lanes without a ray"""
    from rmcl_amd import types as T
    v, f = meshes("room30k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy((0.5, -0.4, 1.2), (0.05, -0.02, 0.7))
    f32 = np.float32
    for (H, W) in [(1, 1), (1, 360), (7, 33), (65, 9)]:
        model = T.spherical_model(f32(-0.3), f32(0.6 / max(H - 1, 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.1), f32(30.0))
        ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False)
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        _sweep(rcc, lambda: rcc.find(Tbm), ref, "room30k %dx%d" % (H, W))
        rcc.close()


def test_other_sensor_models(ra, orc, ctx, meshes):
    """an O1Dn model with NaN directions, a 97 x 33 pinhole and an OnDn model (no common pyramid: its rays start at the root with the
    default seed) on room-30k"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room30k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    f32 = np.float32
    W, H = 64, 24
    sm = T.spherical_model(f32(-0.4), f32(0.9 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.2), f32(40.0))
    dirs = syn.model_directions(sm).copy()
    dirs[np.random.RandomState(5).randint(0, len(dirs), 20)] = np.nan
    orig = (0.05, -0.02, 0.11)
    Tsb = syn.tsb_offset()
    Tbm = T.transform_from_rpy((-1.0, 0.7, 1.1), (0.02, 0.03, 1.9))
    ro = ra.RCCHipO1Dn(hm)
    ro.setTsb(Tsb)
    ro.setModel(W, H, 0.2, 40.0, orig, dirs)
    base = _sweep(ro, lambda: ro.find(Tbm), m.simulate_o1dn(W, H, 0.2, 40.0, orig, dirs, Tsb, Tbm, bvh=False), "room30k o1dn")
    assert (base["hits"] == 0).sum() >= 20 and base["hits"].sum() > 1000
    ro.close()
    rp = ra.RCCHipPinhole(hm)
    rp.setTsb(Tsb)
    w, h = 97, 33
    rp.setModel(w, h, 0.1, 100.0, 0.8 * w, 0.8 * w, 0.5 * w, 0.5 * h)
    ref = m.simulate_pinhole(w, h, 0.1, 100.0, (0.8 * w, 0.8 * w), (0.5 * w, 0.5 * h), Tsb, Tbm, bvh=False)
    base = _sweep(rp, lambda: rp.find(Tbm), ref, "room30k pinhole 97x33")
    assert base["hits"].sum() > 1000
    rp.close()
    origs = (np.random.RandomState(6).uniform(-0.3, 0.3, (W * H, 3))).astype(np.float32)
    rn = ra.RCCHipOnDn(hm)
    rn.setTsb(Tsb)
    rn.setModel(W, H, 0.2, 40.0, origs, dirs)
    base = _sweep(rn, lambda: rn.find(Tbm), m.simulate_ondn(W, H, 0.2, 40.0, origs, dirs, Tsb, Tbm, bvh=False), "room30k ondn")
    assert (base["hits"] == 0).sum() >= 20 and base["hits"].sum() > 1000
    rn.close()


def test_pose_batch(ra, orc, ctx, meshes):
    """kind 32 forced on 5 poses x a ragged 30 x 500 scan (the automatic rule never picks it for a batch)"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = _ragged_c2(syn, 30, 500)
    rng = np.random.RandomState(18)
    base_pose = T.transform_from_rpy(*ROOM_POSE_RPY)
    poses = np.array([T.mult(base_pose, T.transform_from_rpy(tuple(rng.uniform(-1.5, 1.5, 3) * (1, 1, 0.2)), (0.0, 0.0, rng.uniform(-3, 3))))
                      for _ in range(5)], dtype=T.TRANSFORM)
    ref = m.simulate_spherical(model, syn.tsb_offset(), poses, bvh=True, nthreads=16)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    rcc.setModel(model)
    base = _sweep(rcc, lambda: rcc.find_batch(poses), ref, "room100k 5 poses x 30x500", knob_sets=dc.BATCH_KNOBS, tile_knobs=())
    assert base["hits"].size == 5 * 30 * 500 and 0 < base["hits"].sum() < base["hits"].size
    rcc.close()


def test_moment_epilogue_counts_and_corrects_the_same_under_every_knob_set(ra, orc, ctx, meshes):
    """a correction whose find forms the moments in its epilogue: the knobs decide which leaves a wave tests together, never which
    correspondences are found -- the same n_meas as under the default knobs, the same pose to 1e-6 absolute (the tolerance of the
    dealing test in test_gpu_find.py for f64 partial sums in another order)"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room100k")
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy(*ROOM_POSE_RPY)
    est = T.mult(Tbm, T.transform_from_rpy((0.03, -0.02, 0.015), (0.004, -0.003, 0.008)))
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    rcc.setModel(syn.model_c2())
    rcc.set_traversal(32)
    dc.set_knobs(rcc, dc.DEFAULT_KNOBS)
    rcc.find(Tbm)
    rcc.set_dataset_from_ranges(rcc.modelView()["ranges"])
    rcc.params.max_dist = 0.5

    def correct(knobs):
        dc.set_knobs(rcc, knobs)
        rcc.find(Tbm)
        Tc, st = rcc.correct_once(est, T.identity(), 4, 0.0, False)
        return np.frombuffer(np.array(Tc).tobytes()[:28], dtype=np.float32).astype(np.float64), int(st["n_meas"])   # quaternion + translation

    want = correct(dc.DEFAULT_KNOBS)
    assert want[1] > 50000
    for knobs in dc.MOMENT_KNOBS:
        got = correct(knobs)
        print("moments %s: n_meas %d (default %d), largest pose difference %.3g" % (dc.knob_name(knobs), got[1], want[1], np.abs(got[0] - want[0]).max()))
        assert got[1] == want[1], (dc.knob_name(knobs), got[1], want[1])
        assert np.allclose(got[0], want[0], rtol=0.0, atol=1e-6), (dc.knob_name(knobs), got[0], want[0])
    rcc.close()


def test_final_cap_above_64_is_refused(ra, ctx, meshes):
    from rmcl_amd import _capi
    v, f = meshes("cube")
    rcc = ra.RCCHipSpherical(ra.import_hip_map(ctx, v, f))
    assert _capi.lib().rmclhip_rcc_set_descent(rcc._h, 65, 24) == _capi.ERR_INVALID
    assert _capi.lib().rmclhip_rcc_set_descent(rcc._h, 64, 24) == _capi.OK
    rcc.close()


def test_randomised_scans(ra, orc, ctx):
    """the randomised set of tests/descent_cases.py (proved to contain hits and misses, and BVH walk == brute force, by
    tests/test_find_descent_cases_cpu.py): four knob sets against the oracle's BVH walk on all rays and kind 23 bit for bit"""
    per_map = {}
    for name in dc.RANDOM_MAPS:
        v, f = dc.random_map(name)
        m = orc.Mesh(v, f)
        hm = ra.import_hip_map(ctx, v, f)
        per_map[name] = []
        for s in dc.random_scans(name, v):
            ref = s.oracle(m, bvh=True, nthreads=16)
            op = s.operator(ra, hm)
            base = _sweep(op, lambda: op.find(s.pose), ref, s.name, knob_sets=dc.RANDOM_KNOBS, tile_knobs=())
            per_map[name].append(base["hits"])      # (kind 32's under every knob set, bit for bit)
            op.close()
        hm.release()
    assert all(len(x) == dc.N_RANDOM_SCANS for x in per_map.values())
    dc.hit_share_conditions(per_map)        # (equal to the oracle's by now: this guards against an emptied case list)


# ---- which paths the cases above take --------------------------------------------------------------------------------------------
def _descent_words(rcc, pose, knobs):
    """-> (descent word, leaf-cap fallback flag, stack-room fallback flag) of every wave of one clocked kind-32 scan"""
    rcc.set_variant(dc.variant_word(32))
    dc.set_knobs(rcc, knobs)
    w = rcc.debug_wave_clock(pose)
    ran = w[:, 1] != 0
    d = w[ran, 7].astype(np.int64)
    stamps = rcc._last_descent_stamps[ran]
    return d, stamps[:, 13] != 0, stamps[:, 14] != 0


@pytest.mark.lab
def test_reach_witness(ra, ctx, meshes):
    """The parity tests prove nothing about a path no wave took.  The clocked instantiation of kind 32 (experiments library) leaves per
    wave the descent word -- min(survivors, 63) | entries after level 1 << 6 | 2 << 12 | 3 << 18 | final entries << 24, nothing above
    bit 24 for a wave that did not descend -- and two flags: the wave fell back to the root because a ray entered more final leaves
    than the leaf cap / because a lane's stack was left without room.  Over the spherical scans of the hard maps: waves that
    descended and waves that did not, final lists beyond 32 entries (the mask's high half), 63 or more survivors, levels 0 keeping
    the survivors as they are, a smaller cap giving shorter lists, both fallbacks taken AND not taken (the stack-room one also after
    the leaves were tested, i.e. with a seed; not taken on the deep maps whose preload is 7 or 8 entries), and the table switched off."""
    seen = dict(descended=0, not_descended=0, final_gt_32=0, surv_ge_63=0, leaf_fallback=0, no_leaf_fallback=0, room_fallback=0,
                room_fallback_with_a_seed=0, no_room_fallback_on_a_deep_map=0, table_off=0)
    for name in HARD_MAPS:
        v, f, scans = _hard_map(name, meshes)
        hm = ra.import_hip_map(ctx, v, f)
        for label, model, Tsb, pose, _ in scans:
            rcc = ra.RCCHipSpherical(hm)
            rcc.setTsb(Tsb)
            rcc.setModel(model)
            what = "%s %s" % (name, label)
            mean_final = {}
            for knobs in dc.KNOB_SETS:
                d, leaf_fb, room_fb = _descent_words(rcc, pose, knobs)
                surv, final = d & 63, (d >> 24) & 127
                desc = final != 0
                mean_final[knobs] = float(final[desc].mean()) if desc.any() else 0.0
                print("%-22s %-24s waves %5d descended %5d final mean %5.1f max %2d survivors max %2d leaf-cap fallbacks %5d stack-room fallbacks %5d"
                      % (what, dc.knob_name(knobs), d.size, desc.sum(), mean_final[knobs], final.max() if d.size else 0, surv.max() if d.size else 0,
                         leaf_fb.sum(), room_fb.sum()))
                assert (final <= 64).all()
                seen["descended"] += int(desc.sum())
                seen["not_descended"] += int((~desc).sum())
                seen["final_gt_32"] += int((final > 32).sum())
                seen["surv_ge_63"] += int((surv == 63).sum())
                seen["room_fallback"] += int(room_fb.sum())
                seen["room_fallback_with_a_seed"] += int((room_fb & desc).sum())       # (the leaves were tested before the wave gave up)
                seen["no_room_fallback_on_a_deep_map"] += int((~room_fb & ~leaf_fb & (d != 0)).sum()) if name in ("nested200", "chain200") else 0
                if name == "chain2000":     # no table: no wave enters the frontier start at all
                    assert d.size > 0 and not d.any() and not room_fb.any() and not leaf_fb.any(), what
                    seen["table_off"] += int(d.size)
                assert not (leaf_fb & ~desc).any(), what             # only a wave that descended counts leaves per ray
                if knobs[1] == 0:       # levels 0: the final list is the survivors (the word saturates the survivors at 63)
                    assert ((final == surv) | ((surv == 63) & (final >= 63)))[desc].all(), (what, dc.knob_name(knobs))
                if knobs[2] == 255:     # no ray can enter more than 64 leaves
                    assert not leaf_fb.any(), (what, dc.knob_name(knobs))
                    seen["no_leaf_fallback"] += int(desc.sum())
                if knobs[2] == 1:
                    seen["leaf_fallback"] += int(leaf_fb.sum())
            if (name, label) == ("sphere100k", "C2"):
                assert mean_final[(12, 24, 24, False)] < mean_final[dc.DEFAULT_KNOBS], mean_final
                assert mean_final[(12, 24, 24, True)] < mean_final[(64, 24, 24, True)], mean_final
            rcc.close()
        hm.release()
    print(seen)
    for k, n in seen.items():
        assert n > 0, "no wave of any case: %s (%s)" % (k, seen)
