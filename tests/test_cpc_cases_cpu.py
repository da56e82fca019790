"""The case generator of the closest-point tests on hard maps (tests/cpc_cases.py) through the CPU oracle alone: the inputs do what they
are for.  These are conditions, not measurements: the oracle's BVH walk equals brute force (or refuses the map, and then brute force is
the reference), every winner's distance stays where the kernel's start value 3e38 and the oracle's INFINITY are equivalent, and the
witnesses -- exact ties, degenerate winners, overflowed giant triangles, hits and misses at both gates -- are really there.  The
float32 oracle is held against a plain float64 restatement: within 1e-6 * scale on the well-scaled maps, never closer than float64 by
more than that on slivers and the CAD mix (there Ericson's barycentric branch loses digits: the largest deviation is printed)."""
import numpy as np
import pytest

import cpc_cases as cc


@pytest.fixture(scope="module")
def cases(orc):
    """per map: mesh, points, brute-force result at the identity pose with the small gate"""
    from rmcl_amd import types as T
    cache = {}

    def get(name):
        if name not in cache:
            v, f = cc.build_map(name)
            m = orc.Mesh(v, f)
            pts = cc.query_points(name, v, f)
            md = cc.max_dists(v, f)
            brute = cc.oracle_cpc(m, T.identity(), pts, md[0], bvh=False)
            cache[name] = (v, f, m, pts, md, brute)
        return cache[name]

    return get


def test_generator_is_deterministic_and_holds_every_kind():
    for name in ("cube", "chain200", "tri1", "degcube"):
        v, f = cc.build_map(name)
        a, b = cc.query_points(name, v, f), cc.query_points(name, v, f)
        assert a.tobytes() == b.tobytes() and a.dtype == np.float32 and a.shape == (cc.N_POINTS_DEFAULT, 3)
        sp = cc.special_mask(a)
        assert sp.sum() == len(cc.SPECIAL_POINTS) and sp[:63].any() and sp[257:].any()
        assert (np.abs(a[~sp]) <= cc.MAX_COORD).all()
        assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any() and (np.abs(a) == np.float32(1e20)).any()
    assert max(cc.POINT_COUNTS) < cc.N_POINTS["fan200k"] < cc.N_POINTS_DEFAULT
    v, f, deg = cc.degenerate_cube()
    assert deg.sum() == 3 * 6 * 4 and deg[0] and deg[-1] and not deg[len(cc.DEGENERATE_KINDS) * 6] and deg[len(f) // 2]
    vv = v.astype(np.float64)
    area = np.linalg.norm(np.cross(vv[f[:, 1]] - vv[f[:, 0]], vv[f[:, 2]] - vv[f[:, 0]]), axis=1)
    assert (area[deg] < 1e-5).all() and (area[~deg] > 0.1).all()
    for n in (1, 2, 3):
        assert len(cc.build_map("tri%d" % n)[1]) == n
    v, f = cc.build_map("floor")
    assert np.ptp(v[:, 2]) == 0.0
    assert np.abs(cc.build_map("farcube")[0]).max() > 5000.0 and np.abs(cc.build_map("farsoup")[0]).max() > 5000.0
    for name in cc.MAPS:
        assert name in cc.WELL_SCALED + cc.ONE_SIDED + cc.DEEP_MAPS + ("dupsoup", "tri1", "tri2", "tri3")


def test_float64_reference_on_hand_made_cases():
    a, b, c = (np.array([x], np.float64) for x in ([0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0]))
    for p, want in (([0.5, 0.5, 3.0], 9.0), ([-1.0, -1.0, 0.0], 2.0), ([1.0, -2.0, 0.0], 4.0), ([2.0, 2.0, 1.0], 3.0), ([3.0, 0.0, 0.0], 1.0)):
        assert abs(cc.tri_d2_64(p, a, b, c)[0] - want) < 1e-12
    assert abs(cc.tri_d2_64([1.0, 1.0, 0.0], a, b, b)[0] - 1.0) < 1e-12          # two equal vertices: a segment
    assert abs(cc.tri_d2_64([1.0, 1.0, 1.0], a, a, a)[0] - 3.0) < 1e-12          # three equal vertices: a point
    assert abs(cc.tri_d2_64([1.0, 1.0, 0.0], a, 0.5 * b, b)[0] - 1.0) < 1e-12    # collinear
    v, f = cc.build_map("tri3")
    pts = cc.query_points("tri3", v, f, 200)
    d, face, n_min = cc.ref64(v, f, pts)
    d_h, face_h, _ = cc.ref64(v, f, pts, hint=np.full(len(pts), 2))
    assert np.array_equal(face, face_h) and np.array_equal(d, d_h, equal_nan=True)      # the hint changes nothing
    fin = np.isfinite(pts).all(axis=1)
    assert (face[~fin] == -1).all() and np.isnan(d[~fin]).all() and (face[fin] >= 0).all() and (n_min[fin] >= 1).all()
    every = np.stack([cc.dist_to_face64(v, f, pts[fin], np.full(fin.sum(), k)) for k in range(3)])
    assert np.array_equal(every.min(0), d[fin]) and np.array_equal(every.argmin(0), face[fin])


@pytest.mark.parametrize("name", cc.MAPS)
def test_bvh_walk_equals_brute_force_and_winners_stay_in_range(orc, cases, name):
    from rmcl_amd import types as T
    v, f, m, pts, md, brute = cases(name)
    sp = cc.special_mask(pts)
    walk = cc.oracle_cpc(m, T.identity(), pts, md[0], bvh=True)
    refused = (walk["face_ids"][~sp] == cc.INVALID_FACE).all()
    if refused:
        # the oracle's 128-entry stack refuses this map (orc_closest_point returns -1: `not found` for every point): brute force is
        # the reference here, and nothing else is
        print("%s: the oracle's BVH walk refuses the map; brute force is the reference" % name)
        assert name in cc.DEEP_MAPS
    else:
        assert np.array_equal(walk["face_ids"], brute["face_ids"]) and np.array_equal(walk["hits"], brute["hits"]), name
    # winners: found, finite and below 1e15 for every ordinary point -- 3e38 and INFINITY are then the same start value
    assert (brute["face_ids"][~sp] != cc.INVALID_FACE).all()
    assert np.isfinite(brute["ranges"][~sp]).all() and (brute["ranges"][~sp] < 1e15).all()
    # hits and misses at both gates; a gate only compares the distance (what the GPU test derives the second gate's hits from)
    for gate in md:
        hits = brute["ranges"] <= np.float32(gate)
        assert hits[~sp].any() and not hits[~sp].all(), (name, gate)
    assert np.array_equal(brute["hits"], (brute["ranges"] <= np.float32(md[0])).astype(np.uint8))
    sub = m.cpc_find(T.identity(), T.identity(), pts[:300], md[1], bvh=False)
    assert np.array_equal(sub["hits"], (brute["ranges"][:300] <= np.float32(md[1])).astype(np.uint8))
    # every prefix the GPU test runs holds ordinary and special points (from 63 on)
    for n in cc.POINT_COUNTS[1:]:
        assert sp[:n].any() and not sp[:n].all()


@pytest.mark.parametrize("name", cc.MAPS)
def test_special_points_in_the_oracle(orc, cases, name):
    """NaN and infinite coordinates: `not found`.  A coordinate of 1e20 is finite, its squared distance to everything is not: nothing
    is closer than the start value, `not found` as well."""
    v, f, m, pts, md, brute = cases(name)
    sp = cc.special_mask(pts)
    assert (brute["hits"][sp] == 0).all() and (brute["face_ids"][sp] == cc.INVALID_FACE).all()
    assert np.isnan(brute["ranges"][sp]).all() and np.isnan(brute["points"][sp]).all() and np.isnan(brute["normals"][sp]).all()


def test_witnesses(orc, cases):
    # exact ties on the cube: distance 0 to two or more faces
    v, f, m, pts, md, brute = cases("cube")
    zero = np.nonzero(brute["ranges"] == 0)[0]
    vv = v.astype(np.float64)
    n_ties = 0
    for i in zero:
        d2 = cc.tri_d2_64(pts[i], vv[f[:, 0]], vv[f[:, 1]], vv[f[:, 2]])
        n_ties += int((d2 == 0).sum() >= 2)
    print("cube: %d exact ties among %d points" % (n_ties, len(pts)))
    assert n_ties >= 50
    # degenerate faces win
    v, f, deg = cc.degenerate_cube()
    _, _, m, pts, md, brute = cases("degcube")
    sp = cc.special_mask(pts)
    wins = deg[brute["face_ids"][~sp]]
    print("degcube: %d of %d winners are degenerate faces" % (wins.sum(), wins.size))
    assert wins.sum() >= 100
    kinds = set((np.nonzero(deg)[0][np.searchsorted(np.nonzero(deg)[0], brute["face_ids"][~sp][wins])] % 4).tolist())
    assert len(kinds) >= 3, "several kinds of degenerate face win"
    # overflow: Ericson's d1 * d4 - d3 * d2 is inf - inf for giant triangles, they drop out of the float32 race
    for name in ("chain200", "nested200"):
        v, f, m, pts, md, brute = cases(name)
        sp = cc.special_mask(pts)
        d64, f64, _ = cc.ref64(v, f, pts, hint=brute["face_ids"])
        differ = f64[~sp] != brute["face_ids"][~sp].astype(np.int64)
        print("%s: float32 and float64 winners differ at %d of %d points" % (name, differ.sum(), differ.size))
        assert differ.sum() >= 0.1 * differ.size, name


@pytest.mark.parametrize("name", cc.MAPS)
def test_oracle_against_float64(orc, cases, name):
    """the bound where the map is well scaled, its lower half on slivers and the CAD mix, figures only on the exponential maps (giant
    triangles overflow and drop out of the float32 race: no bound holds) -- and one line per map for profiles/cpc_hard_cases.txt"""
    from rmcl_amd import registration as reg
    v, f, m, pts, md, brute = cases(name)
    sp = cc.special_mask(pts)
    d64, f64, n_min = cc.ref64(v, f, pts, hint=brute["face_ids"])
    bound = cc.f64_bound(v, pts)[~sp]
    dev = brute["ranges"][~sp].astype(np.float64) - d64[~sp]
    info = reg.build_bvh_host(v, f)[0]
    n = float((~sp).sum())
    deg = cc.degenerate_cube()[2][brute["face_ids"][~sp]].sum() if name == "degcube" else 0
    lost = (f64[~sp] != brute["face_ids"][~sp].astype(np.int64)) & (dev > bound)
    print("[cpc-hard] %-9s n_faces %6d max_depth %2d stack_need %2d points %4d ties %.3f degenerate winners %.3f other winner and farther "
          "than float64 %.3f d32-d64 in [%.3g, %.3g] m = [%.3g, %.3g] of the bound" % (
              name, info["n_faces"], info["max_depth"], info["stack_need"], len(pts), (n_min[~sp] >= 2).sum() / n, deg / n, lost.sum() / n,
              dev.min(), dev.max(), (dev / bound).min(), (dev / bound).max()))
    assert info["stack_need"] <= 64
    if name in cc.WELL_SCALED + cc.ONE_SIDED:
        assert (dev >= -bound).all(), name
    if name in cc.WELL_SCALED:
        assert (dev <= bound).all(), name


@pytest.mark.parametrize("name", cc.FILTER_MAPS + cc.GRID_MAPS[:1])
def test_filter_cases(orc, name):
    """the filter's inputs: every beam error is a finite distance (never `not found`), small and large ones are there, and the oracle's
    BVH walk gives what brute force gives where it accepts the map"""
    v, f = cc.build_map(name)
    m = orc.Mesh(v, f)
    poses, attrs, beams = cc.filter_case(name, v, f)
    a = attrs.copy()
    e = m.pf_update(poses, a, beams, cc.identity(), orc.pf_params(correspondence_type=1), bvh=False, nthreads=8, want_errors=True)
    assert e.shape == (len(poses), len(beams)) and np.isfinite(e).all() and (e >= 0).all() and e.max() < 1e15
    assert (a["likelihood"]["n_meas"] > 0).all()
    gate = cc.max_dists(v, f)[0]
    assert (e < gate).any() and (e > gate).any()
    if name not in cc.DEEP_MAPS:
        a2 = attrs.copy()
        e2 = m.pf_update(poses, a2, beams, cc.identity(), orc.pf_params(correspondence_type=1), bvh=True, nthreads=8, want_errors=True)
        assert e2.tobytes() == e.tobytes() and a2.tobytes() == a.tobytes()


def test_stack_need_of_the_deep_maps():
    """host build: the deepest of the deep maps needs more stack than every map the older closest-point tests use"""
    from rmcl_amd import registration as reg
    need = {}
    for name in cc.DEEP_MAPS + cc.EARLIER_MAPS:
        info = reg.build_bvh_host(*cc.build_map(name))[0]
        need[name] = info["stack_need"]
        print("%s: n_faces %d max_depth %d stack_need %d" % (name, info["n_faces"], info["max_depth"], info["stack_need"]))
    assert max(need[k] for k in cc.DEEP_MAPS) > max(need[k] for k in cc.EARLIER_MAPS)
    assert max(need.values()) <= 64
