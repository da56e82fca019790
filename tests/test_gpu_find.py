"""GPU parity: RCC*::find (ray-casting correspondences) through the C ABI vs the CPU oracle.

Reads like the reference's call pattern: setTsb, setModel, find(Tbm_est), modelView()
(rmcl/src/rmcl/registration/RCCEmbree.cpp:8-36).  Bar: hits / face ids bit-exact; ranges, points,
normals within 1e-5 relative (BASELINE.json north_star).
"""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import descent_cases as dc
from conftest import find_kinds, assert_close_rel, golden_path

pytestmark = pytest.mark.gpu


def _compare(gpu, ref, what):
    assert np.array_equal(gpu["hits"], ref["hits"]), what + ": hits differ"
    bad = gpu["face_ids"] != ref["face_ids"]
    assert not bad.any(), "%s: %d of %d face ids differ" % (what, bad.sum(), bad.size)
    assert_close_rel(gpu["ranges"], ref["ranges"], 1e-5, 0, what + " ranges")
    assert_close_rel(gpu["points"], ref["points"], 1e-5, 1e-6, what + " points")
    assert_close_rel(gpu["normals"], ref["normals"], 1e-5, 1e-6, what + " normals")


def _brute_force_sample(orc, m, model, Tbm, gpu, n_sample, seed=0):
    """`n_sample` of the scan's OWN rays against every triangle of the map (no BVH at all: the authority the oracle's BVH walk is
    itself checked against), face ids and hits bit-exact, ranges to 1e-5.  The rays go through the oracle's O1Dn entry with the
    spherical model's own direction values and a zero origin: the same arithmetic as simulate_spherical."""
    from rmcl_amd import types as T
    dirs = orc.spherical_directions(model)
    idx = np.sort(np.random.RandomState(1234 + int(seed)).choice(len(dirs), size=min(n_sample, len(dirs)), replace=False))
    sub = m.simulate_o1dn(len(idx), 1, model.range.min, model.range.max, (0.0, 0.0, 0.0), dirs[idx], T.identity(), Tbm, bvh=False,
                          nthreads=8, want=("hits", "ranges", "face_ids"))
    assert np.array_equal(gpu["hits"][idx], sub["hits"]), "brute-force sample: hits differ"
    bad = gpu["face_ids"][idx] != sub["face_ids"]
    assert not bad.any(), "brute-force sample: %d of %d face ids differ from the exhaustive test" % (bad.sum(), bad.size)
    assert_close_rel(gpu["ranges"][idx], sub["ranges"], 1e-5, 0, "brute-force sample ranges")


def _poses(syn, T):
    return [
        syn.pose_c2_truth(),
        T.transform_from_rpy((-2.1, 1.3, -0.7), (0.3, -0.2, 2.5)),
        T.transform_from_rpy((3.9, -3.3, 2.2), (-0.1, 0.25, -1.2)),
    ]


@pytest.mark.parametrize("variant", find_kinds(0, 1, 2, 4, 5, 6, 8, 10, 11, 12, 13, 14, 16, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32))
def test_c1_cube_32x32(ra, orc, ctx, meshes, variant):
    """config C1: 32x32 scan, 972-triangle cube, every output attribute, 3 poses, Tsb != I."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cube")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c1()
    for Tsb in (T.identity(), syn.tsb_offset()):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(variant)
        rcc.setTsb(Tsb)
        rcc.setModel(model)
        for i, Tbm in enumerate(_poses(syn, T)):
            rcc.find(Tbm)
            gpu = rcc.modelView()
            ref = m.simulate_spherical(model, Tsb, Tbm, bvh=False)
            _compare(gpu, ref, "cube pose %d" % i)
            assert gpu["hits"].all()
        rcc.close()


def test_c1_matches_committed_golden(ra, ctx, meshes):
    """GPU vs the committed fixture (tests/golden/g2_cube_32x32.npz, made by tests/golden/make_golden.py)."""
    from rmcl_amd import synthetic as syn, types as T
    g = np.load(golden_path("g2_cube_32x32.npz"))
    v, f = meshes("cube")
    hm = ra.import_hip_map(ctx, v, f)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(g["Tsb"].view(T.TRANSFORM)[0])
    rcc.setModel(syn.model_c1())
    poses = g["Tbm"].view(T.TRANSFORM)
    n = 32 * 32
    for i in range(len(poses)):
        rcc.find(poses[i])
        gpu = rcc.modelView()
        ref = {k: g[k][i * n:(i + 1) * n] for k in ("hits", "ranges", "points", "normals", "face_ids")}
        _compare(gpu, ref, "golden pose %d" % i)


@pytest.mark.parametrize("variant", find_kinds(0, 1, 2, 4, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32))
def test_c2_sphere100k_full_size(ra, orc, ctx, meshes, variant):
    """config C2 at BASELINE.json's full size: 128x1024 rays, 100k triangles; oracle BVH on all rays,
    brute force on a sample, and the committed SHA-256 of the face-id array (G7)."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("sphere100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.set_traversal(variant)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    Tbm = syn.pose_c2_truth()
    rcc.find(Tbm)
    gpu = rcc.modelView()
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=True, nthreads=8)
    _compare(gpu, ref, "C2")
    assert gpu["hits"].all()
    if variant in (0, 2, 15, 23, 24, 32):     # (the product's kinds; the experiments of the lab library are pinned by _compare + the digest)
        _brute_force_sample(orc, m, model, Tbm, gpu, 2048, seed=variant)
    with open(golden_path("g7_digests.json")) as fh:
        dig = json.load(fh)
    assert hashlib.sha256(gpu["face_ids"].tobytes()).hexdigest() == dig["c2_sphere100k_face_ids_sha256"]
    # size-independent property: every hit point lies on the radius-10 sphere seen from the sensor
    Tsm = Tbm
    t = np.array([Tsm["t"]["x"], Tsm["t"]["y"], Tsm["t"]["z"]], dtype=np.float64)
    # |R p_s + t| == 10 up to faceting (chord sag of a 250x200 UV sphere < 1 cm at 10 m)
    from scipy.spatial.transform import Rotation
    R = Rotation.from_quat([Tsm["R"]["x"], Tsm["R"]["y"], Tsm["R"]["z"], Tsm["R"]["w"]]).as_matrix()
    pm = gpu["points"].astype(np.float64) @ R.T + t
    r = np.linalg.norm(pm, axis=1)
    assert np.all(r <= 10.0 + 1e-4) and np.all(r >= 10.0 - 0.02)


@pytest.mark.parametrize("kinds", [(15, 23, 2, 24, 32), pytest.param((19, 22), marks=pytest.mark.lab)], ids=["product", "round-2 kinds"])
def test_ragged_and_tiny_models(ra, orc, ctx, meshes, kinds):
    """edge cases: 1x1, 1x360 (2-D scanner), 7x33 (ragged tiles), empty model (find is a no-op,
    RCCOptix.cpp:30-34)."""
    from rmcl_amd import types as T
    v, f = meshes("room30k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy((0.5, -0.4, 1.2), (0.05, -0.02, 0.7))
    Tsb = T.identity()
    f32 = np.float32
    for (H, W) in [(1, 1), (1, 360), (7, 33), (65, 9)]:
        model = T.spherical_model(f32(-0.3), f32(0.6 / max(H - 1, 1)), H, f32(-math.pi), f32(2 * math.pi / W), W,
                                  f32(0.1), f32(30.0))
        ref = m.simulate_spherical(model, Tsb, Tbm, bvh=False)
        for kind in kinds:
            rcc = ra.RCCHipSpherical(hm)
            rcc.set_traversal(kind)
            rcc.setTsb(Tsb)
            rcc.setModel(model)
            rcc.find(Tbm)
            gpu = rcc.modelView()
            _compare(gpu, ref, "ragged %dx%d kind %d" % (H, W, kind))
            rcc.close()
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(T.spherical_model(f32(0), f32(0), 0, f32(0), f32(0), 0, f32(0.1), f32(30.0)))
    rcc.find(Tbm)  # must not raise
    assert rcc.modelView()["hits"].size == 0


def test_misses_and_range_limit(ra, orc, ctx, meshes):
    """rays leaving through the open ceiling and hits beyond range.max are misses:
    hits 0, range = range.max + 1, NaN point/normal, face id 0xFFFFFFFF."""
    from rmcl_amd import types as T
    v, f = meshes("room30k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    f32 = np.float32
    model = T.spherical_model(f32(-0.6), f32(1.8 / 47), 48, f32(-math.pi), f32(2 * math.pi / 200), 200, f32(0.1), f32(6.0))
    Tbm = T.transform_from_rpy((1.0, 2.0, 1.5), (0.0, 0.1, -0.3))
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False)
    for kind in (15, 32):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(kind)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        rcc.find(Tbm)
        gpu = rcc.modelView()
        _compare(gpu, ref, "misses kind %d" % kind)
        miss = gpu["hits"] == 0
        assert miss.any() and (~miss).any()
        assert np.all(gpu["ranges"][miss] == f32(7.0))
        assert np.all(gpu["face_ids"][miss] == 0xFFFFFFFF)
        assert np.isnan(gpu["points"][miss]).all() and np.isnan(gpu["normals"][miss]).all()
        rcc.close()


@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32))
def test_o1dn_model(ra, orc, ctx, meshes, variant):
    """RCCEmbreeO1Dn::find (RCCEmbree.cpp:89-99): one origin, N explicit directions, with NaN
    directions (invalid points of an organised cloud) which must come back as misses."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room30k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    base = syn.model_pf16()
    W, H = 64, 24
    rng = np.random.RandomState(5)
    f32 = np.float32
    sm = T.spherical_model(f32(-0.4), f32(0.9 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.2), f32(40.0))
    dirs = syn.model_directions(sm).copy()
    dirs[rng.randint(0, len(dirs), 20)] = np.nan
    orig = (0.05, -0.02, 0.11)
    Tsb = syn.tsb_offset()
    Tbm = T.transform_from_rpy((-1.0, 0.7, 1.1), (0.02, 0.03, 1.9))
    rcc = ra.RCCHipO1Dn(hm)
    rcc.set_traversal(variant)
    rcc.setTsb(Tsb)
    rcc.setModel(W, H, 0.2, 40.0, orig, dirs)
    rcc.find(Tbm)
    gpu = rcc.modelView()
    ref = m.simulate_o1dn(W, H, 0.2, 40.0, orig, dirs, Tsb, Tbm, bvh=False)
    _compare(gpu, ref, "o1dn")
    assert (gpu["hits"] == 0).sum() >= 20
    _ = base


def test_grow_only_buffers_and_refind(ra, orc, ctx, meshes):
    """model buffers are grow-only (RCCEmbree.cpp:28-33): big model, then small, then big again."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cube")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    Tbm = syn.pose_c2_truth()
    for model in (syn.model_c1(), syn.model_pf16(), syn.model_c1()):
        rcc.setModel(model)
        rcc.find(Tbm)
        _compare(rcc.modelView(), m.simulate_spherical(model, T.identity(), Tbm, bvh=False), "regrow")


@pytest.mark.parametrize("kind", [23, 24, 32])
def test_frontier_plane_table_follows_model_and_tiling(ra, orc, ctx, meshes, kind):
    """The frontier start (kinds 23 / 24, and kind 32's cooperative descent below it) reads the pyramid of every tile from a table that belongs to (model, tiling) and is
    rebuilt by the model setters and by set_variant's tile shape.  One operator walks through spherical models of three sizes,
    an O1Dn model with NaN directions, a pinhole model and three tile shapes; every scan must equal the scan of the packet
    traversal (kind 0: no table, no frontier) bit for bit -- a stale table would cull boxes the new tiles' rays enter."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room30k")
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))

    def scan(op, tile_bits=0):
        out = {}
        for k in (kind, 0):
            op.set_variant((k & 15) | (((k >> 4) & 1) << 13) | (((k >> 5) & 1) << 14) | (tile_bits << 4))
            op.find(Tbm)
            out[k] = op.modelView()
        for key in ("hits", "ranges", "points", "normals", "face_ids"):
            assert np.array_equal(out[kind][key], out[0][key], equal_nan=True), key
        return int(out[0]["hits"].sum())

    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    hits = []
    for model in (syn.model_c2(), syn.model_c1(), syn.model_pf16(), syn.model_c2()):
        rcc.setModel(model)
        hits.append(scan(rcc))
        for tile_bits in (1, 3, 5, 0):          # 1 + log2(tile width): 1x64, 4x16, 16x4 rays per wave, then automatic again
            assert scan(rcc, tile_bits) == hits[-1]
    assert hits[0] == hits[-1] and hits[0] > 100000
    rcc.close()
    # O1Dn on the same map: directions are data (every 7th one NaN), then a different size on the same operator
    model = syn.model_c2()
    dirs = syn.model_directions(model).reshape(-1, 3).copy()
    dirs[::7] = np.nan
    ro = ra.RCCHipO1Dn(hm)
    ro.setTsb(T.identity())
    ro.setModel(model.theta.size, model.phi.size, 0.3, 120.0, (0.1, 0.0, 0.2), dirs)
    n1 = scan(ro)
    half = (model.phi.size // 2) * model.theta.size
    ro.setModel(model.theta.size, model.phi.size // 2, 0.3, 120.0, (0.1, 0.0, 0.2), dirs[:half])
    n2 = scan(ro)
    assert 0 < n2 < n1
    ro.close()
    rp = ra.RCCHipPinhole(hm)
    rp.setTsb(T.identity())
    for (w, h) in ((640, 480), (97, 33)):
        rp.setModel(w, h, 0.1, 100.0, 0.8 * w, 0.8 * w, 0.5 * w, 0.5 * h)
        assert scan(rp) > 0
    rp.close()


def test_autotune_chooses_a_product_kind_and_changes_no_result(ra, orc, ctx, meshes):
    """rmclhip_rcc_autotune: the single-scan traversal is MEASURED on the operator's own map and model; the choice is one of the
    product's kinds, the scan is the same bit for bit, a new model forgets the measurement, a forced kind refuses it."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room30k")
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    for model in (syn.model_vlp16_900(), syn.model_c2()):
        rcc.setModel(model)
        rule = rcc.find_variant(1)
        rcc.find(Tbm)
        before = rcc.modelView()
        kind, ms = rcc.autotune(Tbm)
        assert kind in (2, 19, 22, 23, 24, 32) and 0.0 < ms < 1.0       # 19 / 22: kinds 23 / 24 without the frontier start
        assert rcc.find_variant(1) == {19: 23, 22: 24}.get(kind, kind)
        assert rcc.find_variant(64) in (23, 24)           # batches keep the rule ...
        rcc.find(Tbm)
        after = rcc.modelView()
        for key in ("hits", "ranges", "points", "normals", "face_ids"):
            assert np.array_equal(before[key], after[key], equal_nan=True), key
        # ... until they are measured too: same results before and after
        poses = np.array([T.mult(Tbm, T.transform_from_rpy((0.01 * k, -0.02 * k, 0.0), (0.0, 0.0, 0.05 * k))) for k in range(6)], dtype=T.TRANSFORM)
        rcc.find_batch(poses)
        b0 = rcc.modelView()
        bkind, bms = rcc.autotune_batch(poses)
        assert bkind in (19, 22, 23, 24) and 0.0 < bms < 10.0
        assert rcc.find_variant(6) == {19: 23, 22: 24}.get(bkind, bkind)
        rcc.find_batch(poses)
        b1 = rcc.modelView()
        for key in ("hits", "ranges", "points", "normals", "face_ids"):
            assert np.array_equal(b0[key], b1[key], equal_nan=True), key
        rcc.setModel(model)                               # a (re)set model forgets the measurements
        assert rcc.find_variant(1) == rule and rcc.find_variant(6) == rcc.find_variant(6)
    rcc.set_traversal(23)
    with pytest.raises(RuntimeError, match="forced"):
        rcc.autotune(Tbm)
    rcc.close()


def test_far_from_origin_mesh(ra, orc, ctx):
    """conservative slab test: a mesh 5 km from the origin (large absolute coordinates) must still
    give brute-force-identical face ids."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = syn.uv_sphere(5000, radius=8.0)
    off = np.array([5000.0, -3000.0, 120.0], dtype=np.float32)
    v = (v + off).astype(np.float32)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c1()
    Tbm = T.transform_from_rpy(tuple(off + np.array([0.4, -0.3, 0.2], dtype=np.float32)), (0.1, 0.2, 0.3))
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False)
    for kind in (15, 32):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(kind)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        rcc.find(Tbm)
        _compare(rcc.modelView(), ref, "far mesh kind %d" % kind)
        rcc.close()


def test_c5_mesh_one_million_triangles(ra, orc, ctx):
    """config C5's map size: 1M-triangle sphere (BVH4 depth 15, traversal stack 46 -> LDS + scratch spill path),
    a 128x1024 scan and a small particle-filter update against the oracle."""
    import math
    from rmcl_amd import synthetic as syn, types as T
    v, f = syn.uv_sphere(1000000)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    info = hm.info()
    assert info["n_faces"] == 1000000 and info["stack_need"] <= 64
    model = syn.model_c2()
    Tbm = syn.pose_c2_truth()
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=True, nthreads=8)
    for variant in (0, 2, 23, 24, 32):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(variant)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        rcc.find(Tbm)
        _compare(rcc.modelView(), ref, "sphere-1M variant %d" % variant)
        rcc.close()
    poses, attrs = syn.uniform_particles(2000, seed=4, bb_min=(-6, -6, -2, 0, 0, -math.pi), bb_max=(6, 6, 2, 0, 0, math.pi))
    beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::4] * np.float32(7.0))
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.init()
    upd.setInput(beams, T.identity())
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    upd.update(d_poses, d_attrs)
    a_ref = attrs.copy()
    m.pf_update(poses, a_ref, beams, T.identity(), orc.pf_params(), bvh=True, nthreads=8)
    a_gpu = d_attrs.download()
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], a_ref["likelihood"]["n_meas"])
    assert_close_rel(a_gpu["likelihood"]["mean"], a_ref["likelihood"]["mean"], 1e-5, 1e-12, "1M pf mean")


ROOM_POSE_RPY = ((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))   # the pose of tests/golden/make_golden.py:g7_digests


@pytest.mark.parametrize("variant", find_kinds(0, 2, 15, 23, 24, 19, 22, 25, 26, 27, 28, 29, 30, 31, 32))
def test_c2_room100k_full_size(ra, orc, ctx, meshes, variant):
    """config C2's scan on a REALISTIC map (room-100k: occluders, vertex noise, open ceiling => misses): every
    traversal incl. the automatic one (15) vs the oracle on all 131 072 rays + the committed G7 digests
    (face ids, hits, hit count).  RCCEmbree.cpp:26-36 / RCCOptix.cpp:28-43."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.set_traversal(variant)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    Tbm = T.transform_from_rpy(*ROOM_POSE_RPY)
    rcc.find(Tbm)
    gpu = rcc.modelView()
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=True, nthreads=8)
    _compare(gpu, ref, "C2 room-100k variant %d" % variant)
    with open(golden_path("g7_digests.json")) as fh:
        dig = json.load(fh)
    assert hashlib.sha256(gpu["face_ids"].tobytes()).hexdigest() == dig["c2_room100k_face_ids_sha256"]
    assert hashlib.sha256(gpu["hits"].tobytes()).hexdigest() == dig["c2_room100k_hits_sha256"]
    assert int(gpu["hits"].sum()) == dig["c2_room100k_n_hits"]
    assert 0 < int(gpu["hits"].sum()) < gpu["hits"].size   # the scan really contains misses
    rcc.close()


def _o1dn_c2(syn, n_nan=37, seed=11):
    """the documented deployment model: C2's 128x1024 directions as DATA (+12 B/ray read), a few NaNs"""
    model = syn.model_c2()
    dirs = syn.model_directions(model).copy()
    rng = np.random.RandomState(seed)
    dirs[rng.randint(0, len(dirs), n_nan)] = np.nan
    return model, dirs


@pytest.mark.parametrize("mesh,variant", [("sphere100k", 15), ("room100k", 15), ("room100k", 24), ("room100k", 2)])
def test_o1dn_c2_size_single_pose(ra, orc, ctx, meshes, mesh, variant):
    """RCCEmbreeO1Dn::find (RCCEmbree.cpp:89-99) at C2's full size: 131 072 explicit directions, sensor origin and
    Tsb != identity, NaN directions come back as misses."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes(mesh)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model, dirs = _o1dn_c2(syn)
    W, H = model.theta.size, model.phi.size
    orig = (0.03, -0.01, 0.08)
    Tsb = syn.tsb_offset()
    Tbm = syn.pose_c2_truth() if mesh == "sphere100k" else T.transform_from_rpy(*ROOM_POSE_RPY)
    rcc = ra.RCCHipO1Dn(hm)
    rcc.set_traversal(variant)
    rcc.setTsb(Tsb)
    rcc.setModel(W, H, float(model.range.min), float(model.range.max), orig, dirs)
    rcc.find(Tbm)
    gpu = rcc.modelView()
    ref = m.simulate_o1dn(W, H, float(model.range.min), float(model.range.max), orig, dirs, Tsb, Tbm, bvh=True, nthreads=8)
    _compare(gpu, ref, "o1dn C2 %s variant %d" % (mesh, variant))
    assert (gpu["hits"] == 0).sum() >= 30
    rcc.close()


def test_o1dn_c2_size_pose_batch(ra, orc, ctx, meshes):
    """8 poses x 131 072 explicit directions in one launch (pose-major model buffers), automatic traversal
    (> 262 144 rays in flight => quantised nodes)."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model, dirs = _o1dn_c2(syn, seed=12)
    W, H = model.theta.size, model.phi.size
    orig = (0.0, 0.02, 0.05)
    Tsb = syn.tsb_offset()
    rng = np.random.RandomState(3)
    base = T.transform_from_rpy(*ROOM_POSE_RPY)
    poses = np.array([T.mult(base, T.transform_from_rpy(tuple(rng.uniform(-1.5, 1.5, 3) * (1, 1, 0.2)),
                                                        (0.0, 0.0, rng.uniform(-3, 3)))) for _ in range(8)],
                     dtype=T.TRANSFORM)
    rcc = ra.RCCHipO1Dn(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(W, H, float(model.range.min), float(model.range.max), orig, dirs)
    rcc.find_batch(poses)
    gpu = rcc.modelView()
    ref = m.simulate_o1dn(W, H, float(model.range.min), float(model.range.max), orig, dirs, Tsb, poses, bvh=True, nthreads=8)
    _compare(gpu, ref, "o1dn C2 batch")
    rcc.close()


def test_context_creation_asks_for_eight_hardware_queues(ra, ctx):
    """Round 6: operators run on streams of their own and count on overlapping; the HIP runtime deals streams onto GPU_MAX_HW_QUEUES
    hardware queues (default 4) and a fifth stream shares one (a two-sensor correction 46 -> 63 us).  rmclhip_ctx_create sets the
    variable to 8 unless the caller chose a value (the C environment: os.environ is Python's copy)."""
    import ctypes
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    v = libc.getenv(b"GPU_MAX_HW_QUEUES")
    assert v is not None and int(v) >= 1
    if "GPU_MAX_HW_QUEUES" not in os.environ:
        assert int(v) == 8


@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32))
def test_every_dealing_of_the_tiles_gives_the_same_scan_and_the_same_correction(ra, orc, ctx, meshes, variant):
    """Round 6: which workgroup computes which tile of a single scan (FindParams::xcd_mapping: 0 as the hardware deals workgroups --
    the default --, 1 an eighth of the image per XCD as in rounds 1-5, 2 a CU's two workgroups from the image's halves) decides
    where a tile runs, never what it computes: 128 x 1024 (mapping 2's own shape: 64 workgroups per XCD), a ragged 100 x 1000 and
    64 x 512, every output bit-equal across the three, the default equal to the oracle; and a correction whose find forms the
    moments in its epilogue (partial rows and mask words follow the dealing) counts the same correspondences and returns the same
    pose to 1e-6 (the f64 partial rows are summed in workgroup order, which is what the dealing changes: last bits only)."""
    from rmcl_amd import synthetic as syn, types as T, _capi
    v, f = meshes("room100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    Tbm = T.transform_from_rpy(*ROOM_POSE_RPY)
    est = T.mult(Tbm, T.transform_from_rpy((0.03, -0.02, 0.015), (0.004, -0.003, 0.008)))
    for H, W in ((128, 1024), (100, 1000), (64, 512)):
        model = syn.model_c2()
        model.phi.inc = model.phi.inc * 128.0 / H
        model.phi.size = H
        model.theta.inc = model.theta.inc * 1024.0 / W
        model.theta.size = W
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(syn.tsb_offset())
        rcc.setModel(model)
        rcc.set_traversal(variant)
        rcc.find(Tbm)
        rcc.set_dataset_from_ranges(rcc.modelView()["ranges"])
        rcc.params.max_dist = 0.5
        out, corr = {}, {}
        for mapping in (0, 1, 2):
            _capi.check(_capi.lib().rmclhip_rcc_set_descent(rcc._h, 64, 24 | (24 << 8) | ((mapping + 1) << 29)))
            rcc.find(Tbm)
            mv = rcc.modelView()
            out[mapping] = {k: np.array(mv[k]) for k in ("hits", "ranges", "points", "normals", "face_ids")}
            Tc, st = rcc.correct_once(est, T.identity(), 4, 0.0, False)
            corr[mapping] = (np.frombuffer(np.array(Tc).tobytes()[:28], dtype=np.float32).astype(np.float64), int(st["n_meas"]))   # quaternion + translation
        for mapping in (1, 2):
            for k in out[0]:
                assert np.array_equal(out[0][k], out[mapping][k], equal_nan=True), (H, W, mapping, k)
            assert corr[mapping][1] == corr[0][1], (H, W, mapping)
            assert np.allclose(corr[mapping][0], corr[0][0], rtol=0.0, atol=1e-6), (H, W, mapping)
        if (H, W) == (100, 1000):
            _compare(out[0], m.simulate_spherical(model, syn.tsb_offset(), Tbm, bvh=True, nthreads=8), "dealing 0, kind %d" % variant)
        rcc.close()


@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32))
def test_pose_batch_in_world_order_equals_the_pose_major_launch_and_the_oracle(ra, orc, ctx, meshes, variant):
    """Round 6: a pose batch is launched in WORLD ORDER -- one key per workgroup (where the central ray of its tiles leaves the map's
    bounding box), a counting sort, k_find walks the sorted list (kernels.hip launch_batch_tile_order).  The order decides which
    workgroup computes a tile, never what is computed: 37 poses x a ragged 30 x 500 scan (a last workgroup with one tile, lanes
    without a ray) in both orders and with two granules, every output bit-equal, and equal to the oracle; the same for two poses (fewer
    workgroups than one turn of the XCDs)."""
    from rmcl_amd import synthetic as syn, types as T, _capi
    v, f = meshes("room100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    model.phi.inc = model.phi.inc * 128.0 / 30
    model.phi.size = 30
    model.theta.inc = model.theta.inc * 1024.0 / 500
    model.theta.size = 500
    rng = np.random.RandomState(17)
    base = T.transform_from_rpy(*ROOM_POSE_RPY)
    poses = np.array([T.mult(base, T.transform_from_rpy(tuple(rng.uniform(-1.5, 1.5, 3) * (1, 1, 0.2)), (0.0, 0.0, rng.uniform(-3, 3))))
                      for _ in range(37)], dtype=T.TRANSFORM)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    rcc.setModel(model)
    rcc.set_traversal(variant)
    far = np.array([T.transform_from_rpy((500.0, 20.0, 3.0), (0.0, 0.0, 1.0))] * 37, dtype=T.TRANSFORM)   # beyond the range limit: every ray misses
    out = {}
    for on in (0, 1, 3):     # pose-major, the default granule, three workgroups per XCD turn
        _capi.check(_capi.lib().rmclhip_rcc_set_batch_order(rcc._h, on))
        for P in (poses, poses[:2]):
            rcc.find_batch(far[:len(P)])   # what a slot that the measured launch never computes would keep: misses, not the call before's right answer
            assert not rcc.modelView(("hits",))["hits"].any()
            rcc.find_batch(P)
            mv = rcc.modelView()
            out[(on, len(P))] = {k: np.array(mv[k]) for k in ("hits", "ranges", "points", "normals", "face_ids")}
    for n in (37, 2):
        for on in (1, 3):
            for k in out[(0, n)]:
                assert np.array_equal(out[(0, n)][k], out[(on, n)][k], equal_nan=True), (on, n, k)
    ref = m.simulate_spherical(model, syn.tsb_offset(), poses, bvh=True, nthreads=8)
    _compare(out[(1, 37)], ref, "world-order batch, kind %d" % variant)
    rcc.close()


@pytest.mark.parametrize("mesh", ["sphere100k", "room100k"])
def test_automatic_variant_in_every_size_bracket(ra, orc, ctx, meshes, mesh):
    """variant 15 (the default) picks a traversal per rays-in-flight bracket (capi_rcc.cpp:find_variant): <= 57 344 four lanes
    per ray (kind 2); above, one lane per ray starting at the map's frontier -- kind 23 (full-precision nodes) up to 524 288
    rays, kind 24 (quantised nodes) beyond.  Each bracket is run explicitly with variant 15."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes(mesh)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    base = syn.pose_c2_truth() if mesh == "sphere100k" else T.transform_from_rpy(*ROOM_POSE_RPY)
    f32 = np.float32
    brackets = [(16, 900, 1), (64, 1024, 1), (96, 1024, 1), (128, 1024, 1), (128, 2048, 1), (256, 2048, 1), (128, 1024, 3), (128, 1024, 5), (16, 900, 40)]
    for (H, W, nposes) in brackets:
        model = T.spherical_model(f32(-0.39), f32(0.78 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.3), f32(120.0))
        rng = np.random.RandomState(H + W + nposes)
        poses = np.array([T.mult(base, T.transform_from_rpy(tuple(rng.uniform(-0.5, 0.5, 3)), (0.0, 0.0, rng.uniform(-3, 3))))
                          for _ in range(nposes)], dtype=T.TRANSFORM)
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_variant(15)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        rays = H * W * nposes
        assert rcc.find_variant(nposes) == (2 if rays <= 57344 else 23 if rays <= 262144 else 24)
        if nposes == 1:
            rcc.find(poses[0])
        else:
            rcc.find_batch(poses)
        gpu = rcc.modelView()
        ref = m.simulate_spherical(model, T.identity(), poses, bvh=True, nthreads=8)
        _compare(gpu, ref, "auto %s %dx%dx%d" % (mesh, H, W, nposes))
        rcc.close()


@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32, 6, 13, 19))
def test_sensor_origin_on_a_face(ra, orc, ctx, meshes, variant):
    """Embree's depth test is strict on the near side (absDen * tnear < T with tnear = 0): a ray that starts exactly ON a
    wall triangle does not hit that triangle -- the sensor sees the room, not t = 0 everywhere."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cube")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c1()
    Tbm = T.transform_from_rpy((5.0, 0.3, 0.2), (0.0, 0.0, 0.0))     # x = +5 is the wall plane of the side-10 cube
    rcc = ra.RCCHipSpherical(hm)
    rcc.set_traversal(variant)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    rcc.find(Tbm)
    gpu = rcc.modelView()
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False)
    _compare(gpu, ref, "origin on a face")
    hit = gpu["hits"] > 0
    assert hit.any() and (~hit).any()               # inward rays see the room, outward rays leave the cube
    assert gpu["ranges"][hit].min() > 1e-3          # nobody reports the wall it stands on at t = 0
    rcc.close()


def test_context_may_be_destroyed_before_its_children(ra, orc, meshes):
    """the context is reference counted: closing it first must not turn the later release of map / rcc /
    pf handles into a use-after-free."""
    from rmcl_amd import synthetic as syn, types as T
    c2 = ra.Context(0)
    v, f = meshes("cube")
    hm = ra.import_hip_map(c2, v, f)
    rcc = ra.RCCHipSpherical(hm)
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.init()
    c2.close()                                   # creator's reference gone; children keep the context alive
    rcc.setTsb(T.identity())
    rcc.setModel(syn.model_c1())
    rcc.find(syn.pose_c2_truth())
    ref = orc.Mesh(v, f).simulate_spherical(syn.model_c1(), T.identity(), syn.pose_c2_truth(), bvh=False)
    _compare(rcc.modelView(), ref, "after ctx close")
    upd.close()
    rcc.close()
    hm.release()


def test_c2_room100k_brute_force_sample(ra, orc, ctx, meshes):
    """C2's scan on the occluded room-100k map: the full scan against the oracle's BVH walk and 2 048 of its rays against every
    triangle (no BVH), for the product's automatic kind."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("room100k")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    Tbm = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
    rcc.find(Tbm)
    gpu = rcc.modelView()
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=True, nthreads=8)
    _compare(gpu, ref, "C2 room")
    _brute_force_sample(orc, m, model, Tbm, gpu, 2048)
    rcc.close()


def _nested_triangles(n, ratio, smallest):
    """n coaxial triangles of geometrically growing size stacked 1 cm apart: the SAH builder can only peel them off one by one, which
    makes the DEEPEST trees map_upload accepts out of a few hundred triangles"""
    vs, fs = [], []
    for k in range(n):
        s = smallest * ratio ** k
        vs += [[-s, -s, 0.01 * k], [s, -s, 0.01 * k], [0.0, s, 0.01 * k]]
        fs.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.array(vs, np.float32), np.array(fs, np.uint32)


@pytest.mark.parametrize("shape", [(160, 1.22), (140, 1.25), (120, 1.3)])
def test_deep_trees_do_not_overflow_the_frontier_start(ra, orc, ctx, shape):
    """the frontier start pre-loads up to 19 (kind 23) / 12 (kind 24) / more (quad kind) stack entries per lane, while
    map_upload's stack_need <= 64 only bounds a descent from the root.  Maps whose trees need 45..59 entries (stack_need of the main
    tree / of the filter's tree) must still trace correctly: the start is bounded by 64 - stack_need and falls back to the root.
    Rays from above the stack cross MANY of the nested boxes, so the frontier accepts as many entries as it can."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = _nested_triangles(shape[0], shape[1], 1e-3)
    info, _, _ = ra.build_bvh_host(v, f)
    info_pf, _, _ = ra.build_bvh_host_pf(v, f)
    assert max(info["stack_need"], info_pf["stack_need"]) > 45 and max(info["stack_need"], info_pf["stack_need"]) <= 64
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c1()
    model.phi.size, model.theta.size = 64, 256
    model.phi.inc, model.theta.inc = model.phi.inc * 32.0 / 64.0, model.theta.inc * 32.0 / 256.0
    model.phi.min = -0.4                                    # looks UP through the stack (smallest triangle first) as well as sideways
    model.phi.inc = (1.45 + 0.4) / 63.0
    model.range.max = 1.0e12
    poses = [T.transform_from_rpy((0.001, -0.002, -1.0), (0.0, 0.0, 0.3)), T.transform_from_rpy((0.8, 0.3, -2.5), (0.05, -0.1, 1.0))]
    for kind in (23, 24, 2, 15, 32):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(kind)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        for i, Tbm in enumerate(poses):
            rcc.find(Tbm)
            gpu = rcc.modelView()
            ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False, nthreads=8)
            _compare(gpu, ref, "nested %s kind %d pose %d" % (shape, kind, i))
            assert gpu["hits"].sum() > 1000 and len(np.unique(gpu["face_ids"][gpu["hits"] > 0])) > 20
        # the same map through a pose batch (kind 24 by rule)
        rcc.find_batch(np.array(poses, dtype=T.TRANSFORM))
        mvb = rcc.modelView()
        n = 64 * 256
        for i, Tbm in enumerate(poses):
            ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False, nthreads=8)
            assert np.array_equal(mvb["face_ids"][i * n:(i + 1) * n], ref["face_ids"])
        rcc.close()


# ---- the reference's own 1 M- and 10 M-face rows (lidar_corrector_optix_benchmark.cpp:161-169, ..._embree_benchmark.cpp:144-152): maps that
# ---- leave the 4 MB L2s (1 M faces: 128 MB on the device) and the 256 MB MALL (10 M faces: 1.29 GB)
def _hit_radius(gpu, Tbm):
    from scipy.spatial.transform import Rotation
    R = Rotation.from_quat([Tbm["R"]["x"], Tbm["R"]["y"], Tbm["R"]["z"], Tbm["R"]["w"]]).as_matrix()
    t = np.array([Tbm["t"]["x"], Tbm["t"]["y"], Tbm["t"]["z"]], dtype=np.float64)
    hit = gpu["hits"] > 0
    return np.linalg.norm(gpu["points"][hit].astype(np.float64) @ R.T + t, axis=1)


_FOUR_WIDE = 1 << 8    # (a flag of these tests, not of the library: kind 32 with the four-wide descent, rmclhip_rcc_set_descent bit 31)


@pytest.mark.parametrize("variant", [15, 24, 2, 32, pytest.param(32 | _FOUR_WIDE, id="32-four-wide")])
def test_c2_sphere1m_full_size(ra, orc, ctx, meshes, variant):
    """C2 scan on the 1 M-face sphere: the oracle's BVH4 walk on ALL 131 072 rays (hits, face ids AND ranges bit-equal), 2 048 of the
    scan's own rays against every triangle (no BVH), and every hit point on the radius-10 sphere."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("sphere1m")
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.set_traversal(variant & 63)
    if variant & _FOUR_WIDE:
        dc.set_knobs(rcc, (64, 24, 24, True))
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    for Tbm in (syn.pose_c2_truth(), T.transform_from_rpy((-2.1, 1.3, -0.7), (0.3, -0.2, 2.5))):
        rcc.find(Tbm)
        gpu = rcc.modelView()
        ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=2, nthreads=16)
        _compare(gpu, ref, "C2 sphere-1M")
        assert np.array_equal(gpu["ranges"], ref["ranges"])
        assert gpu["hits"].all()
        r = _hit_radius(gpu, Tbm)
        assert np.all(r <= 10.0 + 1e-4) and np.all(r >= 10.0 - 2e-3)     # chord sag of a 1000 x 500 UV sphere < 1 mm
    _brute_force_sample(orc, m, model, Tbm, gpu, 2048, seed=variant)
    rcc.close()


def test_c2_sphere10m_full_size(ra, orc, ctx, meshes):
    """C2 scan on the 10 M-face sphere (1.29 GB of nodes + records: past the MALL): 384 of the scan's own rays against all ten million
    triangles -- a random sample PLUS every ray the kernel reports as a miss (up to 128 of them: with 1 cm triangles at 10 m range a few
    rays in 10^5 slip through the fp32 edge tests of two neighbours, in the oracle's arithmetic exactly as in the kernel's) --, face ids
    and hits bit-exact; every hit point on the sphere; the automatic rule and the batch kind agree bit for bit."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("sphere10m")
    hm = ra.import_hip_map(ctx, v, f)
    info = hm.info()
    assert info["stack_need"] <= 64 and info["height_fallbacks"] == 0 and info["guarded_nodes"] == 0
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    Tbm = syn.pose_c2_truth()
    rcc.find(Tbm)
    gpu = rcc.modelView()
    rcc.set_traversal(24)
    rcc.find(Tbm)
    gpu24 = rcc.modelView()
    for k in ("hits", "face_ids", "ranges"):
        assert np.array_equal(gpu[k], gpu24[k]), k
    rcc.set_traversal(32)       # the cooperative descent on the 16-wide twins, then on the four-wide nodes (what maps beyond kMaxNodes16 run)
    for knobs in ((64, 24, 24, False), (64, 24, 24, True)):
        dc.set_knobs(rcc, knobs)
        rcc.find(Tbm)
        gpu32 = rcc.modelView()
        for k in ("hits", "face_ids", "ranges"):
            assert np.array_equal(gpu[k], gpu32[k]), (k, dc.knob_name(knobs))
    miss = np.flatnonzero(gpu["hits"] == 0)
    assert len(miss) < 1e-3 * gpu["hits"].size
    r = _hit_radius(gpu, Tbm)
    assert np.all(r <= 10.0 + 1e-4) and np.all(r >= 10.0 - 2e-4)
    # brute force: the oracle's intersector over all triangles, rays = its own spherical directions through the O1Dn entry
    m = orc.Mesh(v, f, build_bvh=False)
    dirs = orc.spherical_directions(model)
    idx = np.unique(np.concatenate([np.random.RandomState(4).choice(len(dirs), size=256, replace=False), miss[:128]]))
    sub = m.simulate_o1dn(len(idx), 1, model.range.min, model.range.max, (0.0, 0.0, 0.0), dirs[idx], T.identity(), Tbm, bvh=False,
                          nthreads=16, want=("hits", "ranges", "face_ids"))
    assert np.array_equal(gpu["hits"][idx], sub["hits"]), "brute-force sample: hits differ"
    assert np.array_equal(gpu["face_ids"][idx], sub["face_ids"]), "brute-force sample: face ids differ"
    assert np.array_equal(gpu["ranges"][idx], sub["ranges"])
    rcc.close()


@pytest.mark.parametrize("name", ["chain200", "chain2000", "nested200", "fan200k"])
def test_meshes_beyond_the_old_stack_limit_upload_and_trace(ra, orc, ctx, meshes, name):
    """VERDICT r4 'never refuse a valid mesh': maps whose SAH tree would need more than 64 stack entries (exponential chains: the
    builder's height budget and tallest-first collapse step in), a 200-deep nest (refused by rounds 1-4) and a 200 k-triangle sliver
    fan (massively overlapping boxes) upload, and every product kind traces them bit-exactly against brute force."""
    from rmcl_amd import types as T
    v, f = meshes(name)
    hm = ra.import_hip_map(ctx, v, f)
    info = hm.info()
    assert info["stack_need"] <= 64
    m = orc.Mesh(v, f)
    f32 = np.float32
    H, W = 48, 256
    if name == "fan200k":
        model = T.spherical_model(f32(-1.5), f32(3.0 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.01), f32(1e6))
        poses = [T.transform_from_rpy((1.0, 2.0, 3.0), (0.1, 0.2, 0.3)), T.transform_from_rpy((0.01, 0.02, -0.5), (0.0, 0.0, 1.0))]
    elif name.startswith("chain"):
        # look along +x from behind the small end, and sideways from the middle of the chain (sizes span 35 decades: range.max is huge)
        model = T.spherical_model(f32(-0.2), f32(0.4 / (H - 1)), H, f32(-0.3), f32(0.6 / W), W, f32(0.0), f32(1e30))
        poses = [T.transform_from_rpy((-1.0, 0.04, 0.03), (0.0, 0.0, 0.0)), T.transform_from_rpy((-1e-6, 2e-8, 1e-8), (0.0, 0.0, 0.0)),
                 T.transform_from_rpy((-50.0, 2.0, 1.0), (0.0, 0.0, 0.0))]
    else:
        model = T.spherical_model(f32(-0.4), f32(1.85 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(1e12))
        poses = [T.transform_from_rpy((0.001, -0.002, -1.0), (0.0, 0.0, 0.3)), T.transform_from_rpy((0.8, 0.3, -2.5), (0.05, -0.1, 1.0))]
    n_hits = 0
    for kind in (15, 23, 24, 2, 0, 32):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(kind)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        for i, Tbm in enumerate(poses):
            rcc.find(Tbm)
            gpu = rcc.modelView()
            ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=False, nthreads=16)
            _compare(gpu, ref, "%s kind %d pose %d" % (name, kind, i))
            n_hits += int(gpu["hits"].sum())
        if kind == 15:
            ms = rcc.time_find(poses[0], iters=20)
            print("\n[%s] %d faces, stack_need %d (height fallbacks %d, guarded nodes %d): find %d x %d = %.1f us"
                  % (name, len(f), info["stack_need"], info["height_fallbacks"], info["guarded_nodes"], H, W, ms * 1e3))
        rcc.close()
    assert n_hits > 500


def test_mixed_scale_map_hall_beams_and_a_fine_object(ra, orc, ctx, meshes):
    """a map whose triangles span four decades of size (a 40 m hall of twelve triangles, eight 30 m beams, a 20 k-triangle object of
    radius 3: what a CAD export next to scanned detail looks like): every product kind against the oracle's own tree on all rays and
    against brute force on a sample -- the hall's triangles sit in leaves near the root, beside subtrees five levels deep"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("cadmix20k")
    hm = ra.import_hip_map(ctx, v, f)
    m = orc.Mesh(v, f)
    model = syn.model_c2()
    dirs = orc.spherical_directions(model)
    idx = np.sort(np.random.RandomState(5).choice(len(dirs), size=1024, replace=False))
    for Tbm in (T.transform_from_rpy((9.0, -7.0, 0.5), (0.02, -0.03, 2.5)), T.transform_from_rpy((-6.0, 0.5, 1.5), (0.3, 0.1, -1.0))):
        ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=2, nthreads=16)
        sub = m.simulate_o1dn(len(idx), 1, model.range.min, model.range.max, (0.0, 0.0, 0.0), dirs[idx], T.identity(), Tbm, bvh=False,
                              nthreads=16, want=("hits", "ranges", "face_ids"))
        assert np.array_equal(ref["face_ids"][idx], sub["face_ids"])
        assert ref["hits"].all(), "a closed hall: every ray ends on something"
        for kind in (15, 23, 24, 2, 0, 32):
            rcc = ra.RCCHipSpherical(hm)
            rcc.set_traversal(kind)
            rcc.setTsb(T.identity())
            rcc.setModel(model)
            rcc.find(Tbm)
            _compare(rcc.modelView(), ref, "cad mix kind %d" % kind)
            rcc.close()
        small = ref["face_ids"] >= 108   # the hall and the beams are faces 0..107
        assert 1000 < small.sum() < small.size - 1000, "both poses see the object AND the hall"


def test_spatial_splits_leave_every_result_unchanged(ra, orc, ctx, meshes):
    """round 6 (SBVH): a CAD mix whose 60 beams are turned out of the axes -- long thin DIAGONAL triangles over scanned detail -- takes
    hundreds of spatial splits: faces referenced from several leaves through identical records.  Every product kind (and the cooperative
    descent) against the oracle's OWN tree (no spatial splits) on all rays and brute force on a sample: hits, face ids and ranges bit for
    bit; the particle filter's update and the closest-point query on the same map (they index records too) against the oracle."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = syn.cad_mix(20000, beam_yaw_deg=35.0, beam_tilt_deg=12.0, n_beams=60)
    hm = ra.import_hip_map(ctx, v, f)
    info = hm.info()
    assert info["spatial_splits"] > 50 and info["n_faces"] < info["n_tri_records"] <= 2 * info["n_faces"] and info["stack_need"] <= 64
    m = orc.Mesh(v, f)
    model = syn.model_c2()
    dirs = orc.spherical_directions(model)
    idx = np.sort(np.random.RandomState(6).choice(len(dirs), size=1024, replace=False))
    Tbm = T.transform_from_rpy((-6.0, 0.5, 1.5), (0.3, 0.1, -1.0))
    ref = m.simulate_spherical(model, T.identity(), Tbm, bvh=2, nthreads=16)
    sub = m.simulate_o1dn(len(idx), 1, model.range.min, model.range.max, (0.0, 0.0, 0.0), dirs[idx], T.identity(), Tbm, bvh=False,
                          nthreads=16, want=("hits", "ranges", "face_ids"))
    assert np.array_equal(ref["face_ids"][idx], sub["face_ids"])
    beam_faces = (ref["face_ids"] >= 12) & (ref["face_ids"] < 12 + 60 * 12)
    assert beam_faces.sum() > 2000, "the scan must see the turned beams"
    for kind in (15, 23, 32, 24, 2, 0):
        rcc = ra.RCCHipSpherical(hm)
        rcc.set_traversal(kind)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        rcc.find(Tbm)
        _compare(rcc.modelView(), ref, "turned beams kind %d" % kind)
        rcc.close()
    # the filter's tree is a cut of the same BVH2, its records the same array
    poses, attrs = syn.uniform_particles(300, seed=8, bb_min=(-8, -8, 0.0, 0, 0, -math.pi), bb_max=(8, 8, 3.0, 0, 0, math.pi))
    beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::4] * np.float32(6.0))
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.init()
    upd.setInput(beams, T.identity())
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    upd.update(d_p, d_a)
    a_gpu, a_ref = d_a.download(), attrs.copy()
    m.pf_update(poses, a_ref, beams, T.identity(), orc.pf_params(), bvh=True)
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], a_ref["likelihood"]["n_meas"])
    assert np.allclose(a_gpu["likelihood"]["mean"], a_ref["likelihood"]["mean"], rtol=1e-5, atol=1e-12)
    upd.close()
    # closest point: ties go to the smaller face id -- a face's duplicate records tie with themselves
    pts = (np.random.RandomState(3).uniform(-6, 6, (4000, 3)) + np.array([0, 0, 4.0])).astype(np.float32)
    want = m.cpc_find(T.identity(), T.identity(), pts, 2.0, bvh=False)
    for variant in (None, 1):       # the default (four lanes per point) and one lane per point
        cpc = ra.CPCHip(hm)
        if variant is not None:
            cpc.set_variant(variant)
        cpc.setTsb(T.identity())
        cpc.params.max_dist = 2.0
        cpc.set_dataset(pts, None)
        cpc.find(T.identity())
        got = cpc.modelView()
        assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["face_ids"], want["face_ids"]), variant
        cpc.close()


def test_prebound_find_callable_equals_find(ra, orc, ctx, meshes):
    """registration.find_async_fn (bench.py's timed step: the pose converted once, one C call per step) launches the same find as
    find() -- also when the caller's pose array is changed or dropped after the callable was made (it keeps its own copy)."""
    from rmcl_amd import synthetic as syn, types as T
    v, f = meshes("sphere20k")
    hm = ra.import_hip_map(ctx, v, f)
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(syn.model_c1())
    Tbm = np.array([T.transform_from_rpy((0.4, -0.2, 0.1), (0.02, -0.03, 0.4))], dtype=T.TRANSFORM)
    rcc.find(Tbm[0])
    want = {k: x.copy() for k, x in rcc.modelView().items()}
    step = rcc.find_async_fn(Tbm[0])
    Tbm["t"]["x"] = 5.0          # the caller's array changes afterwards
    rcc.find(T.transform_from_rpy((2.0, 1.0, 0.0), (0, 0, 1.0)))   # something else in between
    for _ in range(3):
        step()
    rcc.sync()
    got = rcc.modelView()
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    rcc.close()
