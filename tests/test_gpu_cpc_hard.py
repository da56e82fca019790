"""Closest-point queries (k_cpc_find: nearest_lane_ww and nearest_quad, the near grid, the particle filter's correspondence_type 1) on
deep, sliver, degenerate, planar, tiny and far-away maps against the brute-force oracle -- the inputs of tests/cpc_cases.py, which
tests/test_cpc_cases_cpu.py proves non-vacuous on the CPU.

Per map, pose, variant and mode: hits and face ids equal brute force exactly, distances within 1e-5 relative + 1e-7, points and normals
within 1e-5 + 1e-6 (the points' absolute term grows with the coordinates beyond 20 m: float32 rounding of the transform), the NaN
pattern identical, the special points `not found`.  One lane and four lanes per point, no seed, the near grid and tracking give the same
bytes; a bounded search gives them on every hit.  On the well-scaled maps the distance also lies within 1e-6 * scale of float64.

Wall time on an MI355X: see profiles/cpc_hard_cases.txt."""
import time

import numpy as np
import pytest

import cpc_cases as cc
from conftest import assert_close_rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(orc):
    """per map: mesh, points, gates, poses and the brute-force result at every pose (made when first asked for)"""
    cache = {}

    class Case:
        def __init__(self, name):
            self.name = name
            self.v, self.f = cc.build_map(name)
            self.m = orc.Mesh(self.v, self.f)
            self.pts = cc.query_points(name, self.v, self.f)
            self.special = cc.special_mask(self.pts)
            self.gates = cc.max_dists(self.v, self.f)
            self.poses = cc.poses(self.v)
            self._ref = {}

        def ref(self, k):
            if k not in self._ref:
                self._ref[k] = cc.oracle_cpc(self.m, self.poses[k], self.pts, self.gates[0], bvh=False, nthreads=12)
            return self._ref[k]

    def get(name):
        if name not in cache:
            cache[name] = Case(name)
        return cache[name]

    return get


def _view(op):
    mv = op.modelView()
    return {"hits": mv["hits"].reshape(-1).copy(), "ranges": mv["ranges"].reshape(-1).copy(), "points": mv["points"].reshape(-1, 3).copy(),
            "normals": mv["normals"].reshape(-1, 3).copy(), "face_ids": mv["face_ids"].reshape(-1).copy()}


def _same_bytes(a, b, what, rows=None):
    for k in cc.OUTPUT_KEYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert x.tobytes() == y.tobytes(), "%s: %s differs at %d of %d" % (
            what, k, (x.reshape(len(x), -1).view(np.uint8) != y.reshape(len(y), -1).view(np.uint8)).any(axis=1).sum(), len(x))


def _cmp(gpu, ref, pts, pose, gate, what):
    """against the oracle; `gate`: hits = (distance <= gate), which is all a gate does (tests/test_cpc_cases_cpu.py)"""
    hits = (ref["ranges"] <= np.float32(gate)).astype(np.uint8)
    assert np.array_equal(gpu["hits"], hits), "%s: hits differ at %d" % (what, (gpu["hits"] != hits).sum())
    bad = gpu["face_ids"] != ref["face_ids"]
    assert not bad.any(), "%s: face ids differ at %d of %d, first %s" % (what, bad.sum(), bad.size, np.nonzero(bad)[0][:8])
    assert_close_rel(gpu["ranges"], ref["ranges"], 1e-5, 1e-7, what + " distances")
    # float32 rounding of the transform at the magnitude of what it moves: 1e-6 within 20 m of the origin, beyond that 1e-6 * magnitude / 10
    mag = np.abs(np.concatenate([np.nan_to_num(pts.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0),
                                 np.nan_to_num(ref["points"].astype(np.float64), nan=0.0)], axis=1)).max(axis=1)
    mag = mag + max(abs(float(np.asarray(pose)["t"][c])) for c in "xyz")
    atol = np.where(mag <= 20.0, 1e-6, 1e-6 * mag / 10.0)[:, None]
    assert_close_rel(gpu["points"], ref["points"], 1e-5, atol, what + " points")
    assert_close_rel(gpu["normals"], ref["normals"], 1e-5, 1e-6, what + " normals")


def _assert_special(gpu, special, what):
    assert (gpu["hits"][special] == 0).all() and (gpu["face_ids"][special] == cc.INVALID_FACE).all(), what
    assert np.isnan(gpu["ranges"][special]).all() and np.isnan(gpu["points"][special]).all() and np.isnan(gpu["normals"][special]).all(), what


@pytest.mark.parametrize("name", cc.MAPS)
def test_every_mode_and_variant_against_brute_force(ra, orc, ctx, cases, name):
    t0 = time.time()
    c = cases(name)
    hm = ra.import_hip_map(ctx, c.v, c.f)
    n_poses = len(c.poses)
    out = {}
    for variant in cc.VARIANTS:
        ops = {mode: cc.make_operator(ra, hm, variant, mode, c.gates[0], c.pts) for mode in cc.MODES}
        for k in range(n_poses):            # the warm operator tracks: cold, two small steps, a 2 m jump
            for mode in cc.MODES:
                ops[mode].find(c.poses[k])
                out[variant, mode, k] = _view(ops[mode])
        for op in ops.values():
            op.close()
        for gi, gate in enumerate(c.gates):
            op = cc.make_operator(ra, hm, variant, "bounded", gate, c.pts)
            for k in (0, 1):
                op.find(c.poses[k])
                out[variant, "bounded%d" % gi, k] = _view(op)
            op.close()
    for k in range(n_poses):
        ref = c.ref(k)
        if k == 0:
            _assert_special(ref, c.special, name + " oracle")
        for variant in cc.VARIANTS:
            for mode in cc.MODES:
                what = "%s variant %d %s pose %d" % (name, variant, mode, k)
                _cmp(out[variant, mode, k], ref, c.pts, c.poses[k], c.gates[0], what)
                _assert_special(out[variant, mode, k], c.special, what)
                _same_bytes(out[variant, mode, k], out[1, "bare", k], what + " against variant 1 bare")
    # bounded: the hits of the unbounded search, and on every hit its bytes; beyond the gate the unbounded answer or `not found`
    for gi, gate in enumerate(c.gates):
        for k in (0, 1):
            ref = c.ref(k)
            hits = ref["ranges"] <= np.float32(gate)
            for variant in cc.VARIANTS:
                what = "%s variant %d bounded %g pose %d" % (name, variant, gate, k)
                b, a = out[variant, "bounded%d" % gi, k], out[1, "bare", k]
                assert np.array_equal(b["hits"], hits.astype(np.uint8)), what
                for key in ("ranges", "points", "normals", "face_ids"):
                    assert b[key][hits].tobytes() == a[key][hits].tobytes(), (what, key)
                nf = b["face_ids"] == cc.INVALID_FACE
                assert not (nf & hits).any(), what
                assert np.isnan(b["ranges"][nf]).all() and np.isnan(b["points"][nf]).all() and np.isnan(b["normals"][nf]).all(), what
                assert np.array_equal(b["face_ids"][~nf], a["face_ids"][~nf]), what
                _assert_special(b, c.special, what)
                _same_bytes(b, out[1, "bounded%d" % gi, k], what + " against variant 1")
            if gi == 0 and k == 0:
                assert (out[1, "bounded0", 0]["face_ids"] == cc.INVALID_FACE)[~c.special].any(), name + ": the small gate cuts no search"
    # the block edges: a prefix of the points gives a prefix of the results
    for n in cc.POINT_COUNTS:
        for variant in cc.VARIANTS:
            for mode in ("bare", "grid"):
                op = cc.make_operator(ra, hm, variant, mode, c.gates[0], c.pts[:n])
                op.find(c.poses[0])
                got = _view(op)
                op.close()
                for key in cc.OUTPUT_KEYS:
                    assert got[key].tobytes() == out[1, "bare", 0][key][:n].tobytes(), (name, n, variant, mode, key)
    # float64: the distance the kernel reports is as good as float32 can make it
    if name in cc.WELL_SCALED + cc.ONE_SIDED:
        g = out[2, "grid", 0]
        d64, _, _ = cc.ref64(c.v, c.f, c.pts, hint=g["face_ids"])
        ok = ~c.special
        bound = cc.f64_bound(c.v, c.pts)[ok]
        dev = g["ranges"][ok].astype(np.float64) - d64[ok]
        print("[cpc-hard] %-9s GPU - float64 in [%.3g, %.3g] m = [%.3g, %.3g] of the bound" % (
            name, dev.min(), dev.max(), (dev / bound).min(), (dev / bound).max()))
        assert (dev >= -bound).all(), name
        if name in cc.WELL_SCALED:
            assert (dev <= bound).all(), name
    info = hm.info()
    print("[cpc-hard] %-9s GPU map: n_faces %d max_depth %d stack_need %d; test wall time %.1f s" % (
        name, info["n_faces"], info["max_depth"], info["stack_need"], time.time() - t0))


def test_the_deepest_tree_runs_unseeded(ra, orc, ctx, cases):
    """an unseeded query starts at 3e38 and pushes every sibling of every level on its first descent: the map with the largest
    stack_need of all -- larger than that of every map the older closest-point tests use -- runs without tracking and without the grid in
    both variants, and the coarse pass of its grid build (always unseeded) as well"""
    need = {}
    for name in cc.DEEP_MAPS + cc.EARLIER_MAPS:
        hm = ra.import_hip_map(ctx, *cc.build_map(name))
        info = hm.info()
        need[name] = info["stack_need"]
        print("[cpc-hard] %-9s stack_need %d max_depth %d" % (name, info["stack_need"], info["max_depth"]))
        hm.release()
    deepest = max(cc.DEEP_MAPS, key=lambda k: need[k])
    assert need[deepest] > max(need[k] for k in cc.EARLIER_MAPS) and need[deepest] <= 64
    assert need[deepest] >= 56, "the builder's bound of 64 is (nearly) reached"
    c = cases(deepest)
    hm = ra.import_hip_map(ctx, c.v, c.f)
    for variant in cc.VARIANTS:
        for mode in ("bare", "grid"):
            op = cc.make_operator(ra, hm, variant, mode, c.gates[0], c.pts)
            op.find(c.poses[0])
            what = "%s variant %d %s" % (deepest, variant, mode)
            got = _view(op)
            _cmp(got, c.ref(0), c.pts, c.poses[0], c.gates[0], what)
            _assert_special(got, c.special, what)
            op.close()


def _run_filter(ra, ctx, hm, poses, attrs, beams, unseeded=False):
    from rmcl_amd import types as T
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.setInput(beams, T.identity())
    if unseeded:
        upd.set_mapping(256, 0, None)
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_e = ra.DeviceArray(ctx, np.float32, len(poses) * len(beams))
    upd.set_error_output(d_e)
    upd.update(d_p, d_a)
    a, e = d_a.download(), d_e.download().reshape(len(poses), len(beams))
    upd.close()
    return a, e


def _cmp_filter(orc, m, poses, attrs, beams, a_gpu, e_gpu, what):
    """the tolerances of tests/test_gpu_cpc.py:test_pf_update_with_closest_point_errors"""
    a_ref = attrs.copy()
    e_ref = m.pf_update(poses, a_ref, beams, cc.identity(), orc.pf_params(correspondence_type=1), bvh=False, nthreads=12, want_errors=True)
    assert_close_rel(e_gpu, e_ref, 1e-5, 1e-6, what + " errors")
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], a_ref["likelihood"]["n_meas"]), what
    assert_close_rel(a_gpu["likelihood"]["mean"], a_ref["likelihood"]["mean"], 1e-5, 1e-12, what + " mean")
    assert_close_rel(a_gpu["likelihood"]["sigma"], a_ref["likelihood"]["sigma"], 1e-4, 1e-10, what + " sigma")
    assert np.isfinite(e_ref).all()


@pytest.mark.parametrize("name", cc.FILTER_MAPS)
def test_filter_closest_point_mode(ra, orc, ctx, cases, name):
    t0 = time.time()
    c = cases(name)
    poses, attrs, beams = cc.filter_case(name, c.v, c.f)
    hm = ra.import_hip_map(ctx, c.v, c.f)
    a, e = _run_filter(ra, ctx, hm, poses, attrs, beams)
    _cmp_filter(orc, c.m, poses, attrs, beams, a, e, name + " filter")
    a2, e2 = _run_filter(ra, ctx, hm, poses, attrs, beams, unseeded=True)
    assert a2.tobytes() == a.tobytes() and e2.tobytes() == e.tobytes(), name + ": the grid's seed changes the filter's result"
    print("[cpc-hard] %-9s filter: test wall time %.1f s" % (name, time.time() - t0))


@pytest.mark.parametrize("name", cc.GRID_MAPS)
def test_grid_slots_in_both_orders(ra, orc, ctx, cases, name):
    """fresh maps: (a) the operator builds the sparse grid, the filter then the full one, which serves the operator from there on; (b) the
    filter builds the full grid first and the operator never builds its own.  Every result equals the unseeded one bit for bit."""
    c = cases(name)
    poses, attrs, beams = cc.filter_case(name, c.v, c.f)
    hm0 = ra.import_hip_map(ctx, c.v, c.f)          # no grid is ever built on this one
    bare = {}
    for variant in cc.VARIANTS:
        op = cc.make_operator(ra, hm0, variant, "bare", c.gates[0], c.pts)
        op.find(c.poses[1])
        bare[variant] = _view(op)
        op.close()
        _cmp(bare[variant], c.ref(1), c.pts, c.poses[1], c.gates[0], "%s variant %d bare" % (name, variant))
    a0, e0 = _run_filter(ra, ctx, hm0, poses, attrs, beams, unseeded=True)
    _cmp_filter(orc, c.m, poses, attrs, beams, a0, e0, name + " unseeded filter")

    def operator_equals_bare(hm, what):
        for variant in cc.VARIANTS:
            for mode in ("grid", "warm"):
                op = cc.make_operator(ra, hm, variant, mode, c.gates[0], c.pts)
                op.find(c.poses[0])
                op.find(c.poses[1])
                _same_bytes(_view(op), bare[variant], "%s %s variant %d %s" % (name, what, variant, mode))
                op.close()

    def filter_equals_unseeded(hm, what):
        a, e = _run_filter(ra, ctx, hm, poses, attrs, beams)
        assert a.tobytes() == a0.tobytes() and e.tobytes() == e0.tobytes(), "%s %s: filter" % (name, what)

    hm_a = ra.import_hip_map(ctx, c.v, c.f)
    operator_equals_bare(hm_a, "operator first (sparse grid)")
    filter_equals_unseeded(hm_a, "filter second (full grid)")
    operator_equals_bare(hm_a, "operator served by the full grid")
    hm_b = ra.import_hip_map(ctx, c.v, c.f)
    filter_equals_unseeded(hm_b, "filter first (full grid)")
    operator_equals_bare(hm_b, "operator second (full grid)")
    filter_equals_unseeded(hm_b, "filter again")
