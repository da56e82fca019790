"""Find kind 32 can keep an accepted candidate undivided through its cooperative leaf loop (traverse.hip.h TriPending; bit 16 of
rmclhip_rcc_set_descent's word, which rmclhip_rcc_autotune sets where it measures faster) and divide once per ray behind the loop; a
lane that meets a second candidate resolves the first on the spot.  That may not change a bit of a result.  The loop runs only in
waves that DESCEND (inner nodes among the frontier's survivors), so the maps here are tessellated until their trees are deeper than
the frontier, and every spherical case reads the per-wave descent words of the clocked kind 32 (experiments library) and asserts that
waves descended and were not sent back to the root.  The cases:

  * stacked sheets: a ray crosses up to eight surfaces 1 cm apart -- candidates collide within a leaf and across rounds --, also with
    every face twice (exact ties);
  * random soups with coplanar overlapping stacks and zero-area triangles, and the same soup with every face twice;
  * a hit at exactly t == tfar (alone: against "no hit" in the resolve; and as a tie), an origin exactly on a wall, NaN directions;
  * one pose by value, as a batch of one and inside a batch of three, also from 500 m outside the map and with a range that ends
    before the map.  This guards the EXISTING pose paths only (the frontier starts' reach is computed on the device in all of them);
  * the moment epilogue behind kind 32 with pending candidates, and behind kind 23.

Every case runs kinds 23, 24 and 32 -- 32 with leaf caps 24 and 255 (long leaf loops that carry a candidate over many rounds), each
with the pending candidates off and on -- on one operator.  Against the oracle: hits, face ids and ranges bit-equal, points and
normals to the project's 1e-5; kinds 24 and 32 against kind 23: all five outputs bit-equal."""
import math

import numpy as np
import pytest

import descent_cases as dc
from test_gpu_find import _compare

pytestmark = [pytest.mark.gpu, pytest.mark.lab]     # lab: the clocked kind 32 that witnesses the descent

KNOBS_32 = ((64, 24, 24, False), (64, 24, 255, False))
f32 = np.float32


def _view(op, rows=None):
    mv = op.modelView()
    out = {k: np.array(mv[k]) for k in dc.OUTPUT_KEYS}
    if rows is not None:
        n = out["hits"].size
        out = {k: a.reshape(n, -1)[rows].reshape((-1,) + a.shape[1:]) if a.ndim > 1 else a[rows] for k, a in out.items()}
    return out


def _bits_equal(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _against_oracle(got, ref, what):
    for k in ("hits", "face_ids", "ranges"):
        if not _bits_equal(got[k], ref[k]):
            bad = np.flatnonzero(~((got[k] == ref[k]) | ((got[k] != got[k]) & (ref[k] != ref[k]))))
            raise AssertionError("%s: %s differs from the oracle on %d of %d rays, first rays %s: %s, the oracle's %s"
                                 % (what, k, bad.size, got[k].size, bad[:8].tolist(), got[k][bad[:8]].tolist(), ref[k][bad[:8]].tolist()))
    _compare(got, ref, what)


def _against_kind23(got, base, what):
    for k in dc.OUTPUT_KEYS:
        assert _bits_equal(got[k], base[k]), "%s: %s differs from kind 23" % (what, k)


def _set32(op, knobs, carry):
    """kind 32 with a complete descent word; carry: accepted candidates stay undivided through the cooperative leaf loop (bit 16)"""
    from rmcl_amd import _capi
    cap, levels, leaf_cap, four_wide = knobs
    op.set_variant(dc.variant_word(32))
    _capi.check(_capi.lib().rmclhip_rcc_set_descent(op._h, int(cap), dc.descent_word(levels, leaf_cap, four_wide) | ((1 << 16) if carry else 0)))


def _descended(rcc, pose, knobs=KNOBS_32[1]):
    """waves of one clocked kind-32 scan (spherical operators) that descended -- and so ran the cooperative leaf loop -- and were not
    sent back to the root afterwards (tests/test_gpu_find_descent.py test_reach_witness reads the same words)"""
    _set32(rcc, knobs, True)
    w = rcc.debug_wave_clock(pose)
    ran = w[:, 1] != 0
    d = w[ran, 7].astype(np.int64)
    stamps = rcc._last_descent_stamps[ran]
    ok = (((d >> 24) & 127) != 0) & (stamps[:, 13] == 0) & (stamps[:, 14] == 0)
    return int(ok.sum()), int(d.size)


def _kinds(op, find, ref, what):
    """kinds 23, 24 and 32 (both knob sets, pending candidates off and on) on the operator `op`; -> kind 23's outputs"""
    op.set_variant(dc.variant_word(23))
    find()
    base = _view(op)
    _against_oracle(base, ref, what + " kind 23")
    op.set_variant(dc.variant_word(24))
    find()
    got = _view(op)
    _against_oracle(got, ref, what + " kind 24")
    _against_kind23(got, base, what + " kind 24")
    for knobs in KNOBS_32:
        for carry in (False, True):
            _set32(op, knobs, carry)
            find()
            got = _view(op)
            label = "%s kind 32 %s%s" % (what, dc.knob_name(knobs), " pending" if carry else "")
            _against_oracle(got, ref, label)
            _against_kind23(got, base, label)
    dc.set_knobs(op, dc.DEFAULT_KNOBS)
    return base


def _witness(rcc, pose, what, at_least):
    n, of = _descended(rcc, pose)
    print("%s: %d of %d waves ran the cooperative leaf loop and kept its result" % (what, n, of))
    assert n >= at_least, "%s: only %d of %d waves descended (leaf cap 255): the case does not reach the leaf loop" % (what, n, of)
    dc.set_knobs(rcc, dc.DEFAULT_KNOBS)
    return n


# ---- 1. stacked sheets ------------------------------------------------------------------------------------------------------------
def _louvres(n=12):
    """eight 4 m squares at x = 3.00, 3.01, ... 3.07 m, each an n x n grid of cells of two triangles (2304 triangles: a tree deeper
    than the frontier, so the waves that see the sheets descend)"""
    lin = np.linspace(-2.0, 2.0, n + 1)
    v, f = [], []
    for k in range(8):
        x = 3.0 + 0.01 * k
        b = len(v)
        v += [(x, y, z) for z in lin for y in lin]
        for j in range(n):
            for i in range(n):
                p = b + j * (n + 1) + i
                f += [(p, p + 1, p + n + 2), (p, p + n + 2, p + n + 1)]
    return np.array(v, np.float32), np.array(f, np.uint32)


def _cube():
    """the cube room with 16 x 16 cells per wall (3072 triangles; the wall x = 5 exactly)"""
    from rmcl_amd import synthetic as syn
    return syn.cube_room(side=10.0, grid=16)


def _louvre_model():
    from rmcl_amd import types as T
    return T.spherical_model(f32(-math.pi / 4), f32((math.pi / 2) / 31), 32, f32(-math.pi), f32(2 * math.pi / 64), 64, f32(0.0), f32(20.0))


def _louvre_pose():
    from rmcl_amd import types as T
    return T.transform_from_rpy((0.2, -0.1, 0.3), (0.0, 0.0, 0.1))


def _crossings(v, f, origin, dirs, tmax):
    """float64: per ray the number of triangles crossed at 0 < t <= tmax (Moeller-Trumbore, edges inclusive)"""
    tri = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    d = np.asarray(dirs, np.float64)[:, None, :]
    p = np.cross(d, e2[None])
    det = (p * e1[None]).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = (np.asarray(origin, np.float64) - v0)[None]
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1[None])
        w = (d * q).sum(-1) * inv
        t = (q * e2[None]).sum(-1) * inv
        ok = (det != 0.0) & (u >= 0.0) & (w >= 0.0) & (u + w <= 1.0) & (t > 0.0) & (t <= tmax)
    return ok.sum(1)


def test_stacked_sheets_and_their_exact_ties(ra, orc, ctx):
    from rmcl_amd import synthetic as syn, types as T
    v, f = _louvres()
    model, pose = _louvre_model(), _louvre_pose()
    # the premise: lanes do collect several candidates
    yaw = 0.1
    R = np.array([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    dirs_m = syn.model_directions(model).astype(np.float64) @ R.T
    n_cross = _crossings(v, f, (0.2, -0.1, 0.3), dirs_m, 20.0)      # (a ray through a shared edge counts both triangles: rare)
    share2, share8 = float((n_cross >= 2).mean()), float((n_cross >= 8).mean())
    print("stacked sheets: %.1f %% of the rays cross two or more triangles, %.1f %% all eight sheets" % (100 * share2, 100 * share8))
    assert share2 >= 0.10
    for label, (vv, ff) in (("sheets", (v, f)), ("sheets twice", dc.duplicate_faces(v, f, seed=31))):
        m = orc.Mesh(vv, ff)
        hm = ra.import_hip_map(ctx, vv, ff)
        ref = m.simulate_spherical(model, T.identity(), pose, bvh=False)
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        base = _kinds(rcc, lambda: rcc.find(pose), ref, label)
        assert abs(float(base["hits"].mean()) - float((n_cross >= 1).mean())) < 0.02     # the scan sees what the count saw
        _witness(rcc, pose, label, at_least=2)      # (most of the 32 waves look away from the sheets and cull everything)
        rcc.close()
        hm.release()


# ---- 2. random soups --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "duplicates"])
def test_random_soups(ra, orc, ctx, name):
    v, f = dc.random_map(name)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    n_hits = n_desc = 0
    for s in dc.random_scans(name, v, n_scans=6):
        ref = s.oracle(m, bvh=True, nthreads=16)
        op = s.operator(ra, hm)
        base = _kinds(op, lambda: op.find(s.pose), ref, s.name)
        n_hits += int(base["hits"].sum())
        if s.kind == "spherical":
            n_desc += _witness(op, s.pose, s.name, at_least=0)
        op.close()
    assert n_hits > 1000, "the scans must see the map"
    assert n_desc >= 100, "the scans must reach the cooperative leaf loop"
    hm.release()


# ---- 3. the edges of the acceptance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("twice", [False, True], ids=["cube", "cube twice"])
def test_a_hit_at_exactly_tfar(ra, orc, ctx, twice):
    """range.max = the float32 range of one ray: that ray's hit sits at t == tfar and must be kept (t <= tfar; as an exact tie of two
    copies: 'a first hit at exactly tfar beats no hit', then the smaller face id), while the rays beyond it miss"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = _cube()
    if twice:
        v, f = dc.duplicate_faces(v, f, seed=32)
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    Tsb, pose = syn.tsb_offset(), T.transform_from_rpy((0.7, -1.1, 0.4), (0.02, -0.03, 0.6))
    wide = syn.model_c1()
    full = m.simulate_spherical(wide, Tsb, pose, bvh=False)
    assert full["hits"].all()
    ray = int(np.argsort(full["ranges"])[full["ranges"].size // 2])      # the ray of the median range
    tfar = f32(full["ranges"][ray])
    model = T.spherical_model(wide.phi.min, wide.phi.inc, wide.phi.size, wide.theta.min, wide.theta.inc, wide.theta.size, f32(0.1), tfar)
    ref = m.simulate_spherical(model, Tsb, pose, bvh=False)
    assert ref["hits"][ray] == 1 and ref["ranges"][ray] == tfar, "the premise: the oracle keeps the hit at exactly tfar"
    assert 0 < ref["hits"].sum() < ref["hits"].size
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    base = _kinds(rcc, lambda: rcc.find(pose), ref, "cube, tfar = the range of ray %d" % ray)
    assert base["hits"][ray] == 1 and base["ranges"][ray] == tfar
    _witness(rcc, pose, "cube, tfar", at_least=4)
    rcc.close()
    hm.release()


def test_origin_exactly_on_a_face(ra, orc, ctx):
    """the near side is strict (Tt > 0): a sensor standing exactly on the wall x = 5 does not hit that wall"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = _cube()
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    pose = T.transform_from_rpy((5.0, 0.3, -0.2), (0.0, 0.0, 0.0))
    model = syn.model_c1()
    model.range.min = f32(0.0)
    ref = m.simulate_spherical(model, T.identity(), pose, bvh=False)
    hit = ref["hits"] != 0
    assert hit.any() and (~hit).any() and float(ref["ranges"][hit].min()) > 0.1, "the premise: no hit on the wall the sensor stands on"
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    _kinds(rcc, lambda: rcc.find(pose), ref, "cube, origin on the wall x = 5")
    _witness(rcc, pose, "cube, origin on the wall", at_least=4)
    rcc.close()
    hm.release()


def test_nan_directions(ra, orc, ctx):
    """an O1Dn model with NaN directions; the clocked kernel is spherical only, so the witness is the spherical scan the directions
    were taken from, at the same mount and pose (the O1Dn origin is 12 cm off: the same tiles see the same walls)"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = _cube()
    m = orc.Mesh(v, f)
    hm = ra.import_hip_map(ctx, v, f)
    W, H = 64, 24
    sm = T.spherical_model(f32(-0.4), f32(0.9 / (H - 1)), H, f32(-math.pi), f32(2 * math.pi / W), W, f32(0.0), f32(40.0))
    dirs = syn.model_directions(sm).copy()
    dirs[np.random.RandomState(7).randint(0, len(dirs), 40)] = np.nan
    dirs[100, 1] = np.nan
    orig = (0.05, -0.02, 0.11)
    Tsb, pose = syn.tsb_offset(), T.transform_from_rpy((-1.0, 0.7, 1.1), (0.02, 0.03, 1.9))
    ref = m.simulate_o1dn(W, H, 0.0, 40.0, orig, dirs, Tsb, pose, bvh=False)
    op = ra.RCCHipO1Dn(hm)
    op.setTsb(Tsb)
    op.setModel(W, H, 0.0, 40.0, orig, dirs)
    base = _kinds(op, lambda: op.find(pose), ref, "cube o1dn with NaN directions")
    assert (base["hits"] == 0).sum() >= 30 and base["hits"].sum() > 1000
    op.close()
    rs = ra.RCCHipSpherical(hm)
    rs.setTsb(Tsb)
    rs.setModel(sm)
    _witness(rs, pose, "cube, the spherical twin of the o1dn scan", at_least=4)
    rs.close()
    hm.release()


# ---- 4. the pose by value, as a batch of one, inside a batch of three -------------------------------------------------------------
def _pose_paths(ra, hm, model, Tsb, pose, others, what):
    """-> kind 23's outputs of the single find; kind 32 runs with pending candidates.  A batch of several poses reads its poses from a
    device array; the single find (and a host batch of one, which the library also launches by value) carry theirs in the kernel's
    arguments.  These are the library's existing pose paths: the change adds none."""
    from rmcl_amd import types as T
    n = model.phi.size * model.theta.size
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    out = None
    for kind in (23, 32):
        if kind == 32:
            _set32(rcc, KNOBS_32[1], True)
        else:
            rcc.set_variant(dc.variant_word(kind))
        rcc.find(pose)
        single = _view(rcc)
        rcc.find_batch(np.array([pose], dtype=T.TRANSFORM))
        one = _view(rcc)
        rcc.find_batch(np.array([others[0], pose, others[1]], dtype=T.TRANSFORM))
        three = _view(rcc, rows=slice(n, 2 * n))
        for k in dc.OUTPUT_KEYS:
            assert single[k].tobytes() == one[k].tobytes(), "%s kind %d: %s of a batch of one differs from the single find" % (what, kind, k)
            assert single[k].tobytes() == three[k].tobytes(), "%s kind %d: %s inside a batch of three differs from the single find" % (what, kind, k)
        if out is None:
            out = single
        else:
            _against_kind23(single, out, what + " kind 32")
    rcc.close()
    return out


def test_pose_paths_agree(ra, orc, ctx, meshes):
    from rmcl_amd import synthetic as syn, types as T
    v, f = _louvres()
    hm = ra.import_hip_map(ctx, v, f)
    others = (T.transform_from_rpy((-1.0, 0.5, 0.2), (0.0, 0.1, -2.0)), T.transform_from_rpy((2.9, 0.0, 0.0), (0.1, 0.0, 3.0)))
    base = _pose_paths(ra, hm, _louvre_model(), T.identity(), _louvre_pose(), others, "sheets")
    assert 0 < base["hits"].sum() < base["hits"].size
    hm.release()
    # 500 m outside sphere-20k (radius 10 m), looking at it through a window of three times its angular size
    v, f = meshes("sphere20k")
    hm = ra.import_hip_map(ctx, v, f)
    H, W = 32, 64
    half = 3.0 * math.atan2(10.0, 500.0)
    pose = T.transform_from_rpy((500.0, 3.0, -2.0), (0.0, 0.0, math.pi))
    others = (T.transform_from_rpy((480.0, -3.0, 1.0), (0.0, 0.0, math.pi)), T.transform_from_rpy((1.0, 2.0, 3.0), (0.1, 0.2, 0.3)))
    for far, label in ((1000.0, "far outside"), (100.0, "far outside, the range ends before the map")):
        model = T.spherical_model(f32(-half), f32(2 * half / (H - 1)), H, f32(-half), f32(2 * half / W), W, f32(0.0), f32(far))
        base = _pose_paths(ra, hm, model, T.identity(), pose, others, "sphere20k " + label)
        if far > 500.0:
            assert 50 < base["hits"].sum() < base["hits"].size - 50, "the window must show the sphere and its surroundings"
            ref = orc.Mesh(v, f).simulate_spherical(model, T.identity(), pose, bvh=True, nthreads=16)
            _against_oracle(base, ref, "sphere20k " + label)
        else:
            assert base["hits"].sum() == 0
    hm.release()


# ---- 5. the moment epilogue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [32, 23])
def test_moment_epilogue_on_the_stacked_sheets(ra, orc, ctx, kind):
    """computeCrossStatistics served from the moments a speculating find forms in its epilogue == the streaming reduction of an
    operator with set_micp_fast(0) (the bars of tests/test_gpu_micp.py for this comparison)"""
    from rmcl_amd import types as T
    v, f = _louvres()
    hm = ra.import_hip_map(ctx, v, f)
    model, pose = _louvre_model(), _louvre_pose()
    est = T.mult(pose, T.transform_from_rpy((0.02, -0.01, 0.01), (0.0, 0.0, 0.004)))
    small = T.transform_from_rpy((0.002, 0.001, 0.0), (0.0, 0.0, 0.001))
    rcc, ref = ra.RCCHipSpherical(hm), ra.RCCHipSpherical(hm)
    for r, mode in ((rcc, 1), (ref, 0)):
        r.setTsb(T.identity())
        r.setModel(model)
        if kind == 32:
            _set32(r, KNOBS_32[1], True)
        else:
            r.set_variant(dc.variant_word(kind))
        r.set_micp_fast(mode)
        r.find(pose)
        r.set_dataset_from_ranges(r.modelView()["ranges"])
        r.params.max_dist, r.adaptive_max_dist_min = 0.5, 0.15

    def both(Tpre):
        a, b = rcc.computeCrossStatistics(Tpre, 0.0), ref.computeCrossStatistics(Tpre, 0.0)
        assert int(a["n_meas"]) == int(b["n_meas"]) and int(a["n_meas"]) > 100, (int(a["n_meas"]), int(b["n_meas"]), rcc.ccs_info())
        assert np.allclose(a["covariance"], b["covariance"], rtol=2e-5, atol=2e-6), rcc.ccs_info()
        for k in "xyz":
            assert abs(float(a["model_mean"][k]) - float(b["model_mean"][k])) < 2e-5
            assert abs(float(a["dataset_mean"][k]) - float(b["dataset_mean"][k])) < 2e-5

    for r in (rcc, ref):
        r.find(est)
    both(T.identity())
    both(small)
    for r in (rcc, ref):
        r.find(est)          # followed by calls last time: this find forms the moments itself
    both(T.identity())
    both(small)
    info = rcc.ccs_info()
    assert info["speculative_finds"] >= 1 and info["from_moments"] >= 3, info
    assert ref.ccs_info()["from_moments"] == 0
    if kind == 32:
        _witness(ref, est, "sheets, the find behind the moments", at_least=2)
    rcc.close()
    ref.close()
    hm.release()
