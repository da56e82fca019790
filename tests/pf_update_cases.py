"""Every map, cloud, beam set and parameter set of the sensor-update tests on hard maps (tests/test_gpu_pf_update_hard.py), made
deterministically from fixed seeds -- and proved non-vacuous on the CPU oracle alone by tests/test_pf_update_cases_cpu.py.

Map cases (update_case): the maps of cpc_cases.build_map plus two deep maps that stay inside 1e7 m (chain90, nested60).  The cloud is
AIMED: N_CLUSTERS faces are seeded, one from every size stratum of the map (an exponential map is sampled at every scale); a "truth"
pose stands off each face by 0.5 .. 3 of that face's own shortest altitude, on either side, and looks at it; PER_CLUSTER particles sit around each
truth (the first one on it) with small roll, pitch and yaw of their own.  The N_BEAMS beams are one set for the whole cloud: a cone
about the sensor's +x (forward: towards the seeded face) and one about -x (backward: past the map for a particle outside it).  Beam b
belongs to cluster b % N_CLUSTERS: its range is what the oracle's brute force sees along it from that cluster's truth, times a factor
in [0.5, 2] (every fourth: 1).  A fixed share of the beams has its range outside the sensor interval (real miss); the sensor
interval's lower end lies above the stand-off of the closest clusters, so their hits are `sim misses` under the Embree rule
t > range.min (modes 0, 2) and hits under the OptiX rule (mode 3).  Some beams start off the sensor origin.

The three penalties are NEGATIVE (-100, -101, -102): both sides only square them, a geometric error is fabsf(...) >= 0, so the class of
every beam can be read from the error output bit for bit (beam_class) whatever the scale of the map.

Envelope (in_envelope): DESIGN.md section 9 leaves the float32 overflow of the slab test for axis-parallel rays open in k_pf_update_v3.
The rule of make_ray_slab_guarded is restated here; tests/test_pf_update_cases_cpu.py asserts that EVERY ray of every case satisfies
it, so no ray is excluded from any comparison.

Edge table (edge_case), launch-shape table (shape_case), the two tfar maps of mode 3 (tfar_case) and the accumulator-range case
(sigma_case) live on the cube (walls at +-5) or on tri1.
"""
import math

import numpy as np

import cpc_cases as cc
import pf_cycle_cases as pc

MAPS = ("chain200", "chain2000", "nested200", "fan20k", "cadmix20k", "dupsoup", "farsoup", "farcube", "floor", "degcube",
        "tri1", "tri2", "tri3", "chain90", "nested60")
DEEP_MAPS = ("chain200", "chain2000", "nested200")                                        # filter-tree stack_need >= 59
SPILL_MAPS = DEEP_MAPS + ("fan20k", "cadmix20k", "chain90", "nested60")                   # stack_need > kPfRows = 20
DUPLICATE_MAPS = ("fan20k", "cadmix20k", "dupsoup", "degcube")                            # more records than faces
SMALL_MAPS = ("tri1", "tri2", "tri3", "floor")
MODES = (0, 2, 3)
PF_ROWS = 20
N_CLUSTERS, PER_CLUSTER, N_BEAMS = 10, 15, 32
RHSM, RMSH, RMSM = -100.0, -101.0, -102.0
GEO, C_RHSM, C_RMSH, C_RMSM, C_NAN = 0, 1, 2, 3, 4
CLASS_NAMES = ("geometric", "-100", "-101", "-102", "NaN")
MAX_N_MEAS = 10000

# variant bits of rmclhip_pf_set_variant (tests/test_gpu_pf.py)
BIG, MAPTREE, SLOT, STORED = 512, 1024, 2048, 4096
VARIANTS = (None, 64, 16, 64 | SLOT, 64 | MAPTREE, 64 | SLOT | MAPTREE, 64 | BIG, 64 | STORED, 64 | STORED | SLOT)


def is_stored(variant):
    return variant is not None and (variant & STORED) != 0


# ---- maps -----------------------------------------------------------------------------------------------------------------------
_maps = {}


def build_map(name):
    if name not in _maps:
        from rmcl_amd import synthetic as syn
        if name == "chain90":
            _maps[name] = syn.exp_chain(90, 1.19)                   # 4e-4 .. 3.2e3 m
        elif name == "nested60":
            _maps[name] = syn.nested_triangles(60, 1.2, 1e-3)       # 1e-3 .. 47 m
        else:
            _maps[name] = cc.build_map(name)
    return _maps[name]


def map_max_coord(v):
    return float(np.abs(np.asarray(v, np.float64)).max())


# ---- small helpers --------------------------------------------------------------------------------------------------------------------
def params(orc_or_types, case, mode, **over):
    """pf_params of either side (oracle.pf_params / rmcl_amd.types.pf_params take the same keywords)"""
    kw = dict(dist_sigma=case["dist_sigma"], real_hit_sim_miss_error=RHSM, real_miss_sim_hit_error=RMSH, real_miss_sim_miss_error=RMSM,
              range_min=case["range_min"], range_max=case["range_max"], max_n_meas=MAX_N_MEAS, correspondence_type=mode)
    kw.update(over)
    return orc_or_types.pf_params(**kw)


def beam_class(err):
    e = np.asarray(err, np.float32)
    out = np.full(e.shape, GEO, np.int8)
    out[e == np.float32(RHSM)] = C_RHSM
    out[e == np.float32(RMSH)] = C_RMSH
    out[e == np.float32(RMSM)] = C_RMSM
    out[np.isnan(e)] = C_NAN
    assert not ((out == GEO) & ~(e >= 0)).any(), "a negative error that is none of the three penalties"
    return out


def shares(err):
    c = beam_class(err)
    return [float((c == k).mean()) for k in range(5)]


def make_beams(dirs, ranges, origs=None):
    from rmcl_amd.types import RANGE_MEASUREMENT
    n = len(dirs)
    b = np.zeros(n, RANGE_MEASUREMENT)
    for i, k in enumerate("xyz"):
        b["dir"][k] = np.asarray(dirs)[:, i]
        if origs is not None:
            b["orig"][k] = np.asarray(origs)[:, i]
    b["range"] = ranges
    b["cov"][:, 0] = b["cov"][:, 4] = b["cov"][:, 8] = np.float32(0.1)
    return b


def make_attrs(n, seed):
    """two of three particles start from Gaussian1D::Identity with mean 1 (n_meas 0: the history has no weight, the mean after the update
    is the beams' alone), every third carries a history; state_sigma is random and must come back untouched"""
    a = pc.make_attrs(n, seed)
    fresh = np.arange(n) % 3 != 2
    a["likelihood"]["mean"][fresh] = 1.0
    a["likelihood"]["sigma"][fresh] = 0.0
    a["likelihood"]["n_meas"][fresh] = 0
    hist = np.flatnonzero(~fresh)
    a["likelihood"]["n_meas"][hist] = np.resize(np.array([1, 7, 9990, 9999, MAX_N_MEAS, 20000], np.uint32), len(hist))
    return a


def identity():
    from rmcl_amd import types as T
    return T.identity()


def _pose_arrays(poses):
    q = np.stack([poses["R"][k] for k in "xyzw"], 1).astype(np.float64)
    t = np.stack([poses["t"][k] for k in "xyz"], 1).astype(np.float64)
    return q, t


def rays(poses, beams):
    """(O, D) of every (particle, beam) in the map frame for Tsb = identity, in float64 from the float32 records: (n, nb, 3) each"""
    q, t = _pose_arrays(poses)
    d = np.stack([beams["dir"][k] for k in "xyz"], 1).astype(np.float64)
    o = np.stack([beams["orig"][k] for k in "xyz"], 1).astype(np.float64)
    n, nb = len(q), len(d)
    qq = np.broadcast_to(q[:, None, :], (n, nb, 4))
    with np.errstate(all="ignore"):
        D = pc.quat_rotate(qq, np.broadcast_to(d[None], (n, nb, 3)))
        O = pc.quat_rotate(qq, np.broadcast_to(o[None], (n, nb, 3))) + t[:, None, :]
    return O, D


def in_envelope(v, poses, beams):
    """the rule of make_ray_slab_guarded (traverse.hip.h) per ray and axis: |1 / D| * max(|O|, the map's largest |coordinate|) <= 1e37,
    1 / D as safe_inv forms it (+-1e30 for |D| < 1e-30).  Rays with a NaN in O or D are not traced (a miss on both sides) and count
    as inside.  -> bool (n, nb)"""
    O, D = rays(poses, beams)
    with np.errstate(all="ignore"):
        inv = np.where(np.abs(D) < 1e-30, 1e30, 1.0 / np.abs(D))
        reach = np.maximum(np.abs(O).max(-1), map_max_coord(v))[..., None]
        ok = (inv * reach <= 1e37).all(-1)
    return ok | np.isnan(O).any(-1) | np.isnan(D).any(-1)


def facing_rpy(fwd):
    """yaw and pitch (ZYX) that turn the sensor's +x onto the unit vectors fwd (n, 3)"""
    return np.zeros(len(fwd)), -np.arcsin(np.clip(fwd[:, 2], -1.0, 1.0)), np.arctan2(fwd[:, 1], fwd[:, 0])


# ---- the aimed cloud of a map -------------------------------------------------------------------------------------------------------
_cases = {}


def _cone(rng, n, a_max, sign):
    a, b = rng.uniform(0.02, a_max, n), rng.uniform(0.0, 2.0 * math.pi, n)
    return np.stack([sign * np.cos(a), np.sin(a) * np.cos(b), np.sin(a) * np.sin(b)], -1)


def update_case(name, orc):
    """-> dict(name, v, f, mesh, poses, attrs, beams, dist_sigma, range_min, range_max, cluster (per particle), standoff (per cluster),
    fwd (per beam), real_miss (per beam)).  poses / attrs are the INPUT: copy attrs before an in-place update."""
    if name in _cases:
        return _cases[name]
    v, f = build_map(name)
    rng = np.random.RandomState(12000 + MAPS.index(name))
    mesh = orc.Mesh(v, f)
    vv = np.asarray(v, np.float64)
    tri = vv[np.asarray(f, np.int64)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    nrm = np.cross(b - a, c - a)
    area2 = np.linalg.norm(nrm, axis=1)
    size = np.maximum(np.linalg.norm(b - a, axis=1), np.maximum(np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)))
    good = np.flatnonzero(area2 > 1e-9 * size * size)                        # (degcube: the spliced-in faces have no normal to stand off)
    good = good[np.argsort(size[good], kind="stable")]
    strata = np.array_split(good, N_CLUSTERS)
    seeds = np.array([int(rng.choice(s)) if len(s) else int(rng.choice(good)) for s in strata])
    w = rng.dirichlet((2.0, 2.0, 2.0), N_CLUSTERS)
    foot = (tri[seeds] * w[:, :, None]).sum(1)
    side = rng.choice([-1.0, 1.0], N_CLUSTERS)
    normal = nrm[seeds] / area2[seeds, None] * side[:, None]
    height = area2 / np.where(size > 0, size, 1.0)                                  # the shortest altitude: what a cone of beams has to land on
    standoff = height[seeds] * 10.0 ** rng.uniform(-0.3, 0.5, N_CLUSTERS)
    truth_t = foot + normal * standoff[:, None]
    _, pitch0, yaw0 = facing_rpy(-normal)
    truth_roll = rng.uniform(-0.3, 0.3, N_CLUSTERS)
    # (no Euler angle is ever exactly 0 or a multiple of pi / 2 after the noise: no direction component is exactly 0, see in_envelope)
    truth_pitch, truth_yaw = pitch0 + rng.uniform(0.01, 0.1, N_CLUSTERS), yaw0 + rng.uniform(0.01, 0.1, N_CLUSTERS)

    n = N_CLUSTERS * PER_CLUSTER
    cluster = np.repeat(np.arange(N_CLUSTERS), PER_CLUSTER)
    first = np.arange(n) % PER_CLUSTER == 0
    jit = np.where(first[:, None], 0.0, rng.uniform(-0.25, 0.25, (n, 3)))
    ang = np.where(first[:, None], 0.0, rng.uniform(-0.15, 0.15, (n, 3)))
    q = pc.quats_from_rpy(truth_roll[cluster] + ang[:, 0], truth_pitch[cluster] + ang[:, 1], truth_yaw[cluster] + ang[:, 2])
    poses = pc.make_poses(q, truth_t[cluster] + jit * standoff[cluster, None], 12000 + MAPS.index(name))
    order = rng.permutation(n)                         # clusters interleaved: a workgroup's particles are of every scale
    poses, cluster = poses[order].copy(), cluster[order]
    attrs = make_attrs(n, 12100 + MAPS.index(name))

    # beams: 18 forward real hits, 4 forward real misses, 6 backward real hits, 4 backward real misses -- shuffled
    fwd = np.array([True] * 22 + [False] * 10)
    real_miss = np.array([False] * 18 + [True] * 4 + [False] * 6 + [True] * 4)
    dirs = np.concatenate([_cone(rng, 22, 0.4, 1.0), _cone(rng, 10, 0.9, -1.0)])
    shuffle = rng.permutation(N_BEAMS)
    fwd, real_miss, dirs = fwd[shuffle], real_miss[shuffle], dirs[shuffle]
    origs = np.zeros((N_BEAMS, 3))
    origs[3::7] = rng.uniform(-0.3, 0.3, (len(origs[3::7]), 3)) * float(np.median(standoff))
    ds = np.sort(standoff)
    range_min = float(np.float32(1.3 * ds[1]))
    range_max = float(np.float32(8.0 * ds[-1]))
    beams = make_beams(dirs, np.zeros(N_BEAMS), origs)
    truth = pc.make_poses(pc.quats_from_rpy(truth_roll, truth_pitch, truth_yaw), truth_t)
    O, D = rays(truth, beams)
    rngs = np.zeros(N_BEAMS)
    for i in range(N_BEAMS):
        k = i % N_CLUSTERS
        hit, t, _ = mesh.intersect(O[k, i].astype(np.float32), D[k, i].astype(np.float32), bvh=False)
        r = (t if hit else standoff[k]) * (1.0 if i % 4 == 0 else rng.uniform(0.5, 2.0))
        if real_miss[i]:
            r = range_min * rng.uniform(0.1, 0.9) if i % 2 else range_max * rng.uniform(1.5, 10.0)
        else:
            r = min(max(r, range_min), range_max)
        rngs[i] = r
    beams["range"] = rngs
    rf = beams["range"]
    assert np.array_equal((rf >= np.float32(range_min)) & (rf <= np.float32(range_max)), ~real_miss)
    case = dict(name=name, v=v, f=f, mesh=mesh, poses=poses, attrs=attrs, beams=beams, dist_sigma=float(np.float32(0.5 * np.median(standoff))),
                range_min=range_min, range_max=range_max, cluster=cluster, standoff=standoff, fwd=fwd, real_miss=real_miss)
    _cases[name] = case
    return case


_refs = {}


def reference(case, orc, mode, bvh=False, **over):
    """the oracle's update of the case (brute force by default), cached: -> (attrs, errors), not to be modified"""
    key = (case["name"], mode, bool(bvh), tuple(sorted(over.items())))
    if key not in _refs:
        a = case["attrs"].copy()
        e = case["mesh"].pf_update(case["poses"], a, case["beams"], identity(), params(orc, case, mode, **over), bvh=bvh, nthreads=8, want_errors=True)
        _refs[key] = (a, e)
    return _refs[key]


def magnitude(case, mode, where):
    """M of the (particle, beam) pairs `where` (k, 2): the largest coordinate magnitude that enters the beam's error -- |O|, |preal| =
    |O + D range| and |pint| = |O + D t|, t the oracle's brute force (one call per pair: meant for the few beams that need it)"""
    O, D = rays(case["poses"], case["beams"])
    r = case["beams"]["range"].astype(np.float64)
    tfar = 1.0e4 if mode == 3 else np.inf
    M = np.zeros(len(where))
    for k, (i, j) in enumerate(where):
        o, d = O[i, j], D[i, j]
        hit, t, _ = case["mesh"].intersect(o.astype(np.float32), d.astype(np.float32), tfar=tfar, bvh=False)
        with np.errstate(all="ignore"):
            cand = [np.abs(o).max(), np.abs(o + d * r[j]).max()] + ([np.abs(o + d * t).max()] if hit else [])
        M[k] = max(x for x in cand if np.isfinite(x))
    return M


def ulp32(x):
    return np.spacing(np.asarray(x, np.float64).astype(np.float32)).astype(np.float64)


def first_beam_difference(what, got, want):
    """None, or a message naming the first beams whose error bits differ"""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    if len(bad) == 0:
        return None
    return "%s: %d of %d beam errors differ, first (particle, beam): %s" % (what, len(bad), g.size, "; ".join(
        "(%d, %d) got %r want %r" % (i, j, float(g[i, j]), float(w[i, j])) for i, j in bad[:5]))


# ---- filter tree ---------------------------------------------------------------------------------------------------------------------
def filter_tree(name):
    """(info, number of leaves with one record, with two) of the filter's own tree, built on the host"""
    from rmcl_amd import registration as reg
    info, nodes, _ = reg.build_bvh_host_pf(*build_map(name))
    n_children = nodes[:, 28]
    refs = np.concatenate([nodes[n_children > k, 24 + k] for k in range(4)])
    leaves = refs[(refs & 0x80000000) != 0]
    count = ((leaves >> 28) & 7) + 1
    return info, int((count == 1).sum()), int((count == 2).sum())


# ---- edge table on the cube ------------------------------------------------------------------------------------------------------------
EDGE_RANGE_MIN, EDGE_RANGE_MAX = 0.5, 8.0
EDGE_Y, EDGE_Z = 0.2, -0.3            # off the grid lines and the diagonals of the walls' quads
FAR_DIAGONALS = (10.0, 100.0, 1000.0)
FAR_AXIS = np.array([0.6, 0.64, 0.48])      # a unit vector (0.36 + 0.4096 + 0.2304 = 1) without a zero


def _f32(x):
    return np.float32(x)


def _up(x):
    return float(np.nextafter(_f32(x), _f32(np.inf)))


def _dn(x):
    return float(np.nextafter(_f32(x), _f32(-np.inf)))


def edge_case():
    """-> dict(v, f, poses, attrs, beams, rows, ...): `rows` is a list of (label, particle, beam, {mode: class}) -- the expectation the
    table carries; tests/test_pf_update_cases_cpu.py holds the oracle's brute force to it, the GPU test holds the device to the oracle on
    the WHOLE particle x beam matrix."""
    if "edge" in _cases:
        return _cases["edge"]
    v, f = build_map("cube")
    nan, inf = float("nan"), float("inf")
    lo, hi = EDGE_RANGE_MIN, EDGE_RANGE_MAX
    B = {}      # name -> (dir, range, orig)
    px = (1.0, 0.0, 0.0)
    for nm, r in (("plain", 2.0), ("r_min", lo), ("r_min_dn", _dn(lo)), ("r_min_up", _up(lo)), ("r_max", hi), ("r_max_up", _up(hi)),
                  ("r_max_dn", _dn(hi)), ("r_nan", nan), ("r_pinf", inf), ("r_ninf", -inf), ("r_zero", 0.0), ("r_neg", -1.0)):
        B[nm] = (px, r, (0, 0, 0))
    B["d_nan"] = ((1.0, nan, 0.0), 2.0, (0, 0, 0))
    B["d_zero"] = ((0.0, 0.0, 0.0), 2.0, (0, 0, 0))
    B["d_half"] = ((0.5, 0.0, 0.0), 2.0, (0, 0, 0))
    B["d_three"] = ((3.0, 0.0, 0.0), 2.0, (0, 0, 0))
    B["orig_1e3"] = (px, 2.0, (-1.0e3, 0.0, 0.0))
    B["back"] = ((-1.0, 0.0, 0.0), 2.0, (0, 0, 0))
    rng = np.random.RandomState(13001)
    for k in range(8):                                  # a narrow cone about +x: from 1000 diagonals out the cube is 6e-4 rad wide
        s = rng.uniform(-6e-4, 6e-4, 2)
        B["cone%d" % k] = ((1.0, float(s[0]), float(s[1])), 2.0, (0, 0, 0))
    bnames = list(B)
    beams = make_beams([B[k][0] for k in bnames], [B[k][1] for k in bnames], [B[k][2] for k in bnames])

    P = {}      # name -> (quaternion xyzw, translation)
    ident = (0.0, 0.0, 0.0, 1.0)
    P["centre"] = (ident, (0.0, EDGE_Y, EDGE_Z))
    P["wall_at_min"] = (ident, (4.5, EDGE_Y, EDGE_Z))               # 5 - 4.5 = 0.5 = range_min exactly
    P["wall_at_min_dn"] = (ident, (_dn(4.5), EDGE_Y, EDGE_Z))       # a little farther from the wall
    P["wall_at_min_up"] = (ident, (_up(4.5), EDGE_Y, EDGE_Z))       # a little closer
    P["q_nan"] = ((nan, 0.0, 0.0, 1.0), (0.0, EDGE_Y, EDGE_Z))
    P["t_nan"] = (ident, (nan, EDGE_Y, EDGE_Z))
    P["q_zero"] = ((0.0, 0.0, 0.0, 0.0), (0.0, EDGE_Y, EDGE_Z))
    P["q_norm2"] = ((0.0, 0.0, 0.0, 2.0), (0.0, EDGE_Y, EDGE_Z))    # q (p, 0) ~q without normalisation: directions four times as long
    P["on_face"] = (ident, (5.0, EDGE_Y, EDGE_Z))
    vv = np.asarray(v, np.float64)
    corner = vv[(vv[:, 0] == 5.0) & (np.abs(vv[:, 1]) < 4.0) & (np.abs(vv[:, 2]) < 4.0)][7]     # an inner vertex of the wall x = 5
    P["on_vertex"] = (ident, tuple(float(x) for x in corner))
    diag = 10.0 * math.sqrt(3.0)
    _, pitch, yaw = facing_rpy(FAR_AXIS[None])
    qfar = pc.quats_from_rpy(np.zeros(1), pitch, yaw)[0]
    for k in FAR_DIAGONALS:
        P["far%d" % int(k)] = (tuple(float(x) for x in qfar), tuple(float(x) for x in -FAR_AXIS * k * diag))
    pnames = list(P)
    poses = pc.make_poses(np.array([P[k][0] for k in pnames]), np.array([P[k][1] for k in pnames]), 13000)
    attrs = make_attrs(len(pnames), 13002)

    G, H, S, X = GEO, C_RHSM, C_RMSH, C_RMSM
    all3 = lambda c: {0: c, 2: c, 3: c}
    rows = [("range = range_min", "centre", "r_min", all3(G)), ("range just below range_min", "centre", "r_min_dn", all3(S)),
            ("range just above range_min", "centre", "r_min_up", all3(G)), ("range = range_max", "centre", "r_max", all3(G)),
            ("range just above range_max", "centre", "r_max_up", all3(S)), ("range just below range_max", "centre", "r_max_dn", all3(G)),
            ("range NaN", "centre", "r_nan", all3(S)), ("range +inf", "centre", "r_pinf", all3(S)), ("range -inf", "centre", "r_ninf", all3(S)),
            ("range 0", "centre", "r_zero", all3(S)), ("range negative", "centre", "r_neg", all3(S)),
            ("direction with a NaN component", "centre", "d_nan", all3(H)), ("zero direction", "centre", "d_zero", all3(H)),
            ("direction of length 0.5", "centre", "d_half", all3(G)), ("direction of length 3", "centre", "d_three", all3(G)),
            ("orig 1e3 m behind the sensor", "centre", "orig_1e3", all3(G)),
            ("wall exactly range_min away", "wall_at_min", "plain", {0: H, 2: H, 3: G}),
            ("wall a little more than range_min away", "wall_at_min_dn", "plain", all3(G)),
            ("wall a little less than range_min away", "wall_at_min_up", "plain", {0: H, 2: H, 3: G}),
            ("wall exactly range_min away, real miss", "wall_at_min", "r_nan", {0: X, 2: X, 3: S}),
            ("NaN quaternion component", "q_nan", "plain", all3(H)), ("NaN quaternion component, real miss", "q_nan", "r_neg", all3(X)),
            ("NaN translation", "t_nan", "plain", all3(H)), ("zero quaternion", "q_zero", "plain", all3(H)),
            ("quaternion of norm 2", "q_norm2", "plain", all3(G)),
            ("on a face, looking out", "on_face", "plain", all3(H)), ("on a face, looking in", "on_face", "back", all3(G)),
            ("on a vertex, looking out", "on_vertex", "plain", all3(H)), ("on a vertex, looking in", "on_vertex", "back", all3(G))]
    # (mode 3 ends its rays at 1e4 m: 1000 diagonals are 17 km)
    rows += [("%d diagonals out, looking at the cube" % int(k), "far%d" % int(k), "plain", all3(G) if k * diag < 1.0e4 else {0: G, 2: G, 3: H})
             for k in FAR_DIAGONALS]
    rows = [(lab, pnames.index(p), bnames.index(b), exp) for lab, p, b, exp in rows]
    # analytic errors of the unit-normal modes (walls at +-5, normals along x): |5 - (x + |d| range)|
    analytic = [(pnames.index("centre"), bnames.index("plain"), 3.0), (pnames.index("centre"), bnames.index("d_half"), 4.0),
                (pnames.index("centre"), bnames.index("d_three"), 1.0), (pnames.index("q_norm2"), bnames.index("plain"), 3.0),
                (pnames.index("centre"), bnames.index("orig_1e3"), 993.0), (pnames.index("on_face"), bnames.index("back"), 8.0)]
    case = dict(name="edge", v=v, f=f, poses=poses, attrs=attrs, beams=beams, rows=rows, analytic=analytic, pnames=pnames, bnames=bnames,
                dist_sigma=2.0, range_min=EDGE_RANGE_MIN, range_max=EDGE_RANGE_MAX)
    _cases["edge"] = case
    return case


def with_mesh(case, orc):
    if "mesh" not in case:
        case["mesh"] = orc.Mesh(case["v"], case["f"])
    return case


# ---- mode 3's tfar = 1e4 ---------------------------------------------------------------------------------------------------------------
TFAR_OFFSETS = (9999.5, 10000.5)


def tfar_case(offset):
    """tri1 (in the plane z = 0) lifted to z = offset; three particles below its inside at z = 0, identity orientation; beams along +z.
    Hit in mode 0 and 2 for both offsets; in mode 3 (tfar 1e4) a hit at 9999.5 and a miss at 10000.5"""
    key = ("tfar", offset)
    if key not in _cases:
        v, f = cc.build_map("tri1")
        v = v.copy()
        v[:, 2] += np.float32(offset)
        t = np.array([[0.5, 0.5, 0.0], [0.25, 1.0, 0.0], [1.2, 0.3, 0.0]])
        poses = pc.make_poses(np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)), t, 14000)
        beams = make_beams([(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0)], [9000.0, float(offset), 2.0e4])
        _cases[key] = dict(name="tfar%g" % offset, v=v, f=f, poses=poses, attrs=make_attrs(3, 14001), beams=beams, dist_sigma=2.0,
                           range_min=0.05, range_max=1.5e4, offset=offset)
    return _cases[key]


# ---- launch shapes ---------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 8192), (3, 8192), (5, 4097), (17, 255), (17, 256), (17, 257), (1025, 2), (1023, 1), (31, 128), (33, 128))
MAX_BEAMS = 8192


def shape_case(n_particles, n_beams):
    """a cloud inside the cube with roll and pitch and n_beams seeded directions all around; ranges 0.3 .. 9 against the interval
    [0.5, 8], so real misses occur; every ray hits a wall, some closer than range_min"""
    key = ("shape", n_particles, n_beams)
    if key not in _cases:
        v, f = build_map("cube")
        rng = np.random.RandomState(15000 + 7 * n_particles + n_beams)
        q = pc.quats_from_rpy(rng.uniform(-0.4, 0.4, n_particles), rng.uniform(-0.4, 0.4, n_particles), rng.uniform(-math.pi, math.pi, n_particles))
        poses = pc.make_poses(q, rng.uniform(-4.9, 4.9, (n_particles, 3)), 15000)
        d = rng.normal(size=(n_beams, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = rng.uniform(0.3, 9.0, n_beams)
        if n_beams >= 2:
            r[0] = 0.3                                  # (two beams: one of them a real miss)
        beams = make_beams(d, r)
        _cases[key] = dict(name="shape%dx%d" % (n_particles, n_beams), v=v, f=f, poses=poses, attrs=make_attrs(n_particles, 15001), beams=beams,
                           dist_sigma=2.0, range_min=EDGE_RANGE_MIN, range_max=EDGE_RANGE_MAX)
    return _cases[key]


# ---- accumulator range -------------------------------------------------------------------------------------------------------------------
SIGMA_MIN = float(np.float32(1e-10))                                   # the smallest dist_sigma rmclhip_pf_set_params accepts
SIGMA_BELOW = float(np.nextafter(np.float32(1e-10), np.float32(0)))    # the largest it refuses


def sigma_case(orc):
    """particles AT a truth pose in the cube (identity orientation: O and D are the pose's and the beam's own floats), beam ranges the
    oracle's own t at that pose: errors exactly 0, evals at the peak 1 / sqrt(2 pi sigma^2) = 3.99e9 for dist_sigma = 1e-10; and
    particles off the truth, whose evals underflow to 0"""
    if "sigma" not in _cases:
        v, f = build_map("cube")
        mesh = orc.Mesh(v, f)
        rng = np.random.RandomState(16000)
        d = rng.normal(size=(16, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d32 = d.astype(np.float32)
        truth = np.array([1.25, -0.75, 0.5], np.float32)
        r = []
        for k in range(16):
            hit, t, _ = mesh.intersect(truth, d32[k], bvh=False)
            assert hit
            r.append(t)
        n = 24
        t = np.tile(truth.astype(np.float64), (n, 1))
        t[16:] += rng.uniform(-0.5, 0.5, (8, 3))
        poses = pc.make_poses(np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)), t, 16001)
        _cases["sigma"] = dict(name="sigma", v=v, f=f, mesh=mesh, poses=poses, attrs=make_attrs(n, 16002), beams=make_beams(d32, r),
                               dist_sigma=SIGMA_MIN, range_min=0.05, range_max=80.0, n_truth=16)
    return _cases["sigma"]
