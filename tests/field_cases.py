"""Every map, lattice, point set, pose and beam set of the distance-field tests on hard maps (tests/test_gpu_field_hard.py), made
deterministically from fixed seeds -- and proved non-vacuous without a device by tests/test_field_cases_cpu.py.

Maps come from cpc_cases.build_map; the cells are explicit, so every lattice stays below 25 000 nodes and the brute-force oracle over it
takes seconds.  TABLE holds what include/rmclhip.h (DISTANCE FIELD) and capi_field.cpp's level schedule make of each map: the node
counts per axis and the number of levels of the dense field's coarse-to-fine build (k_field_level, which builds the banded field's
coarse lattice on the same maps too: band_layout).  "floor" is not in the table: its lattice (cell 0.5, margin 1.0,
so that it has volume) serves the rank-three refinement alone.

NaN.  The header says "NaN", never which one: an invalid operation makes 0xFFC00000 on x86 and 0x7FC00000 on the device, and a NaN
that passes through an addition keeps whatever payload it came with.  same_bits therefore asks for the same NaN PATTERN and the same
bytes everywhere else; which NaN it is is not part of the contract.

Not a test module."""
import math

import numpy as np

import band_field_ref as bfr
import cpc_cases as cc
import field_ref as fr
import refine_ref as rr

F = np.float32

# map: (cell, margin, nodes per axis, levels of the build, why)
TABLE = {
    "fan20k": (0.5, 0.5, (43, 43, 5), 3, "slivers"),
    "cadmix20k": (1.0, 0.0, (42, 42, 14), 3, "more records than faces"),
    "dupsoup": (0.75, 0.3, (28, 27, 28), 2, "every face twice, unequal axes"),
    "degcube": (0.5, 0.25, (22, 22, 22), 2, "degenerate faces"),
    "farsoup": (0.75, 0.0, (26, 26, 26), 2, "5 km from the origin"),
    "tri1": (0.5, 0.0, (5, 5, 2), 1, "one level, empty node slots, n_z = 2"),
    "tri3": (0.3, 0.1, (15, 14, 10), 2, "every n_k - 1 odd against 4 and 16"),
    "nested200": (5e11, 0.0, (24, 24, 2), 2, "deep tree, box 1e13 by 2 m"),
    "chain200": (1e16, 0.0, (42, 4, 4), 3, "deep tree, 1e-18 to 4e17, three levels along one axis only"),
    "chain2000": (1e20, 0.0, (24, 3, 3), 2, "squared distances overflow float32: NaN nodes"),
}
FLOOR = ("floor", 0.5, 1.0, (29, 29, 5))
MAPS = tuple(TABLE)
LOOKUP_MAPS = ("farsoup", "tri1", "chain200", "chain2000")
LOOKUP_PREFIXES = (1, 63, 65, 257)
N_LOOKUP_POINTS = 2560
REFINE_MAPS = ("cadmix20k", "degcube", "floor", "chain2000")
UPDATE_PARTICLES = (1, 5, 257)
UPDATE_BEAMS = (1, 257, 2048, 2049, 8192)        # 2048 / 2049: from several particles per workgroup to one, whose ray loop then strides
MAX_BEAMS = 8192
UPDATE_SHAPES = tuple((n, b) for n in UPDATE_PARTICLES for b in UPDATE_BEAMS if not (b == MAX_BEAMS and n > 5))
LIMIT_PARTICLES = (1, 4, 5)                       # 8192 beams x 64 iterations: one workgroup's worth of particles, and one more


def cell_margin(name):
    return (FLOOR[1], FLOOR[2]) if name == "floor" else TABLE[name][:2]


def expected_n(name):
    return FLOOR[3] if name == "floor" else TABLE[name][2]


_maps = {}


def build_map(name):
    """cpc_cases.build_map, made once per process"""
    if name not in _maps:
        _maps[name] = cc.build_map(name)
    return _maps[name]


def layout(name):
    v, _ = build_map(name)
    cell, margin = cell_margin(name)
    vv = np.asarray(v, F).reshape(-1, 3)
    return fr.layout(vv.min(0), vv.max(0), cell=cell, margin=margin)


# ---- the banded field on the same maps --------------------------------------------------------------------------------------------------
BAND_N_MAX_OVER_32 = ("fan20k", "cadmix20k", "chain200")     # the banded build runs its stride-16 level, with a clamped last node


def band_layout(name):
    """(logical, bricks) of band_field_ref.layout for the map's cell and margin at band = half a cell: every brick of every map is
    then within reach of the surface (tests/test_field_cases_cpu.py)"""
    v, _ = build_map(name)
    cell, margin = cell_margin(name)
    vv = np.asarray(v, F).reshape(-1, 3)
    return bfr.layout(vv.min(0), vv.max(0), cell=cell, margin=margin, band=0.5 * cell)


# ---- the level schedule of field_build (capi_field.cpp) ------------------------------------------------------------------------------
def schedule(n):
    """the strides field_build runs for a lattice of n = (n_x, n_y, n_z) nodes, coarsest first: 16, 4, 1, a coarse level skipped when
    n_max <= 2 * stride"""
    n_max = max(n)
    return [s for s in (16, 4, 1) if s == 1 or n_max > 2 * s]


def level_nodes(n, stride):
    """nodes per axis of the level with this stride: (n_k - 1) / stride + 1"""
    return tuple((k - 1) // stride + 1 for k in n)


def seed_index(i, pstride, pn):
    """the previous level's node (per axis) whose record seeds lattice index i: min((i + pstride / 2) / pstride, pn - 1)"""
    return min((i + pstride // 2) // pstride, pn - 1)


# ---- the oracle's lattice, brute force ---------------------------------------------------------------------------------------------------
_lattices = {}


def oracle_lattice(orc, name):
    """(info, lattice [n_z, n_y, n_x] float32, face ids [n_nodes]) of the oracle's BRUTE-FORCE closest-point query at every node (NaN
    and INVALID_FACE where it finds nothing), made once per process"""
    if name not in _lattices:
        v, f = build_map(name)
        info = layout(name)
        pos = fr.node_positions(info).reshape(-1, 3)
        out = cc.oracle_cpc(orc.Mesh(v, f), cc.identity(), pos, 1.0e30, bvh=False, nthreads=12)
        n = info["n"]
        _lattices[name] = (info, out["ranges"].astype(F).reshape(n[2], n[1], n[0]), out["face_ids"].copy())
    return _lattices[name]


def nan_holes(lattice, seed, n_holes=12):
    """a copy of the lattice with n_holes single nodes set to NaN (seeded): most cells keep eight finite corners, every hole poisons
    the (up to) eight cells around it"""
    rng = np.random.RandomState(seed)
    lat = np.array(lattice, F)
    flat = rng.permutation(lat.size)[:n_holes]
    lat.reshape(-1)[flat] = np.nan
    return lat


def cell_has_nan_corner(info, lattice, points):
    """per point: whether one of the eight corners of THE LOOKUP's cell is NaN (False for points that are not finite)"""
    info = fr.info_f32(info)
    n = info["n"]
    lat = np.asarray(lattice, F).reshape(n[2], n[1], n[0])
    P = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        fin = (np.abs(P) <= fr.FLT_MAX).all(axis=1)
        Q = np.where(fin[:, None], P, F(0))
        idx = []
        for k in range(3):
            u = (Q[:, k] - info["origin"][k]) * info["inv_cell"]
            c = np.minimum(np.maximum(u, F(0)), F(n[k] - 1))
            idx.append(np.minimum(np.floor(c).astype(np.int64), n[k] - 2))
    bad = np.zeros(len(P), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                bad |= np.isnan(lat[idx[2] + dz, idx[1] + dy, idx[0] + dx])
    return bad & fin


def same_bits(a, b):
    """None when a and b (float32, any shape) have the same NaN pattern and the same bytes wherever they are not NaN; otherwise a
    sentence about the first difference"""
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        i = int(np.flatnonzero(na != nb)[0])
        return "NaN pattern differs at %d of %d, first at %d: %r against %r" % ((na != nb).sum(), a.size, i, float(a[i]), float(b[i]))
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return "%d of %d differ, first at %d: %r against %r" % (bad.sum(), a.size, i, float(a[i]), float(b[i]))
    return None


def same_records(a, b):
    """same_bits over every float32 leaf of two structured arrays of one dtype, plain equality over the others"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype

    def walk(x, y, path):
        if x.dtype.names:
            for k in x.dtype.names:
                msg = walk(x[k], y[k], path + "." + k)
                if msg:
                    return msg
            return None
        if x.dtype == F:
            msg = same_bits(x, y)
            return None if msg is None else "%s: %s" % (path, msg)
        return None if np.array_equal(x, y) else "%s: %d of %d differ" % (path, (x != y).sum(), x.size)

    return walk(a, b, "")


# ---- lookup points, scaled to the lattice's own box ------------------------------------------------------------------------------------
def lookup_points(info, n_total=N_LOOKUP_POINTS, seed=21):
    """(points [n_total, 3] float32, kinds): the point kinds of test_gpu_field._lookup_points -- nodes, the max faces, the origin and
    its faces, all 26 outside directions, far, special, inside -- with every length a multiple of the lattice's own half extent, so that
    a box of 1e-18 .. 4e17 and one 5 km away are covered like the cube.  Shuffled: every prefix from 63 on holds most kinds."""
    info = fr.info_f32(info)
    rng = np.random.RandomState(seed)
    n, cell = info["n"], info["cell"]
    origin = np.array(info["origin"], F)
    top = np.array([info["origin"][k] + F(n[k] - 1) * cell for k in range(3)], F)
    centre, half = 0.5 * (origin.astype(np.float64) + top), 0.5 * (top.astype(np.float64) - origin)
    scale = float(half.max())
    inside = lambda k: (centre + rng.uniform(-1, 1, (k, 3)) * half).astype(F)
    parts, kinds = [], []

    def add(kind, p):
        with np.errstate(over="ignore"):
            p = np.asarray(p, np.float64).astype(F).reshape(-1, 3)
        parts.append(p)
        kinds.extend([kind] * len(p))

    pos = fr.node_positions(info).reshape(-1, 3)
    add("node", pos[rng.permutation(len(pos))[:300]])
    for k in range(3):
        p = inside(40)
        p[:, k] = top[k]
        add("maxface", p)
    add("maxface", top[None])
    add("origin", origin[None])
    for k in range(3):
        p = inside(10)
        p[:, k] = origin[k]
        add("origin", p)
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) == (0, 0, 0):
                    continue
                p = inside(10).astype(np.float64)
                for k, s in enumerate((sx, sy, sz)):
                    if s:
                        p[:, k] = centre[k] + s * (half[k] + rng.uniform(0.01, 3.0, 10) * scale)
                add("outside%+d%+d%+d" % (sx, sy, sz), p)
    far = 1e6 * scale
    add("far", [[centre[0] + far, centre[1], centre[2]], [centre[0], centre[1] - far, centre[2] + far]])
    add("special", [[np.nan, centre[1], centre[2]], [centre[0], np.nan, np.nan], [np.inf, centre[1], centre[2]], [centre[0], -np.inf, centre[2]],
                    [centre[0], centre[1], np.inf], [-np.inf, np.inf, np.nan], [1e38, centre[1], centre[2]], [centre[0], -1e38, centre[2]],
                    [1e38, 1e38, -1e38], [3.4028235e38, centre[1], centre[2]]])
    add("inside", inside(n_total - sum(len(p) for p in parts)))
    pts, kinds = np.concatenate(parts), np.array(kinds)
    order = rng.permutation(len(pts))
    return pts[order], kinds[order]


# ---- beams that end on the nodes: what the exact update is asked ---------------------------------------------------------------------------
def node_beams(positions):
    """RANGE_MEASUREMENT records whose end point under the identity pose is the position itself: orig = the node, range 0"""
    from rmcl_amd import types as T
    pos = np.asarray(positions, F).reshape(-1, 3)
    beams = np.zeros(len(pos), T.RANGE_MEASUREMENT)
    beams["orig"]["x"], beams["orig"]["y"], beams["orig"]["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    beams["dir"]["x"] = 1.0
    return beams


# ---- known poses ---------------------------------------------------------------------------------------------------------------------
def truth_pose(name):
    """[1] TRANSFORM: where the scan of a known-pose case is taken from"""
    from rmcl_amd import types as T
    xyz, rpy = {
        "cadmix20k": ((5.5, -4.0, 0.5), (0.02, -0.03, 0.6)),        # in the hall, 3 m from the sphere, under the turned beams
        "degcube": ((1.0, -1.5, 0.4), (0.03, -0.02, 0.5)),
        "floor": ((0.4, -0.3, 1.6), (0.02, -0.03, 0.5)),            # 0.85 m above the plane
        "chain2000": ((30.0, 1.5, 4.0), (0.0, 0.0, 0.3)),           # over the triangles of size 30: about a hundred rays hit
    }[name]
    return np.array([T.transform_from_rpy(xyz, rpy)]).reshape(1)


_scans = {}


def scan(orc, name):
    """(truth [1], Tsb, points of the oracle's simulated 32 x 32 spherical scan from the truth), made once per process"""
    from rmcl_amd import synthetic as syn
    if name not in _scans:
        v, f = build_map(name)
        truth, Tsb = truth_pose(name), syn.tsb_offset()
        cloud = orc.Mesh(v, f).simulate_spherical(syn.model_c1(), Tsb, truth[0], bvh=(name not in cc.DEEP_MAPS))["points"]
        _scans[name] = (truth, Tsb, cloud)
    return _scans[name]


# map: (n_beams, n_starts, seed, longest beam kept, keywords of perturbed_starts, keywords of refine_ref.params)
# floor: beams of at most 4 m end at least a cell inside the floor's edge from every start -- past the edge the distance to the floor
# grows with x and y, and the plane alone would no longer be what is seen
REFINE_CASES = {
    "cadmix20k": (256, 40, 41, None, dict(d_trans=0.3, d_yaw=0.1), dict(iterations=12, max_dist=1.5)),
    "degcube": (256, 40, 42, None, dict(d_trans=0.3, d_yaw=0.1), dict(iterations=12, max_dist=1.0)),
    "floor": (64, 40, 43, 4.0, dict(d_trans=0.45, d_yaw=0.15), dict(iterations=8, max_dist=2.0, max_step_trans=0.05, max_step_rot=0.02)),
    "chain2000": (64, 9, 44, None, dict(d_trans=0.3, d_yaw=0.15), dict()),
}


def refine_case(ra, orc, name):
    """(truth [1], Tsb, beams, starts, params): the truth pose, the oracle's scan from it sampled to beams, starts spread around it"""
    n_beams, n_starts, seed, longest, kw_starts, kw_params = REFINE_CASES[name]
    truth, Tsb, cloud = scan(orc, name)
    if longest is not None:
        with np.errstate(invalid="ignore"):
            cloud = cloud[np.sqrt((cloud.astype(np.float64) ** 2).sum(axis=1)) <= longest]
    beams = ra.sample_beams(cloud, n_beams, seed=seed)
    assert len(beams) == n_beams
    return truth, Tsb, beams, rr.perturbed_starts(truth, n_starts, seed=seed + 100, **kw_starts), rr.params(**kw_params)


def refine_trace(info, lattice, poses, beams, Tsb, p):
    """refine_ref.refine's loop once more, counting what it does not report: (poses', rows, dict(rejected = steps refused at a Cholesky
    pivot, limited = steps shortened by max_step_trans or max_step_rot, tried = particle-iterations)), over the particles that iterate.
    The poses and rows are refine_ref.refine's, byte for byte (tests/test_field_cases_cpu.py holds them against each other)."""
    D = np.float64
    poses = np.array(poses).reshape(-1)
    n = len(poses)
    R, t = rr.pose_arrays(poses)
    mask = p["dof_mask"] & 0x3F
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    C, A, b, n_used = rr.evaluate(info, lattice, R, t, Tsb, beams, p)
    C0 = C.copy()
    go = finite & (n_used != 0) & (p["iterations"] != 0) & (mask != 0)
    accepted = np.zeros(n, np.uint32)
    count = dict(rejected=0, limited=0, tried=0)
    unlimited = dict(p, max_step_trans=F(3e38), max_step_rot=F(3e38))
    lam = np.full(n, D(p["lambda0"]), D)
    for _ in range(p["iterations"] if go.any() else 0):
        delta, ok = rr.solve(A, b, mask, lam, p)
        free, _ = rr.solve(A, b, mask, lam, unlimited)
        count["tried"] += int(go.sum())
        count["rejected"] += int((go & ~ok).sum())
        with np.errstate(all="ignore"):
            count["limited"] += int((go & ok & (np.abs(delta) < np.abs(free)).any(axis=1)).sum())
        R2, t2 = rr.candidate(R, t, delta, mask)
        C2, A2, b2, n2 = rr.evaluate(info, lattice, R2, t2, Tsb, beams, p)
        with np.errstate(all="ignore"):
            acc = go & ok & (C2 < C)
        R, t = np.where(acc[:, None], R2, R), np.where(acc[:, None], t2, t)
        C, n_used = np.where(acc, C2, C), np.where(acc, n2, n_used)
        A, b = np.where(acc[:, None], A2, A), np.where(acc[:, None], b2, b)
        l3 = lam / 3.0
        lam = np.where(acc, np.where(l3 > 1e-6, l3, 1e-6), lam * 10.0)
        accepted += acc.astype(np.uint32)
    moved = accepted != 0
    for i, k in enumerate("xyzw"):
        poses["R"][k] = np.where(moved, R[:, i], poses["R"][k])
    for i, k in enumerate("xyz"):
        poses["t"][k] = np.where(moved, t[:, i], poses["t"][k])
    rows = np.zeros(n, rr.RESULT)
    with np.errstate(all="ignore"):
        rows["cost_before"], rows["cost_after"] = C0.astype(F), C.astype(F)
    rows["n_used"], rows["accepted"] = n_used, accepted
    return poses, rows, count


def yaw_error(poses, truth):
    """|yaw - yaw of the truth| per pose, radians, wrapped"""
    def yaw(p):
        R, _ = rr.pose_arrays(p)
        x, y, z, w = (R[:, k].astype(np.float64) for k in range(4))
        return np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
    d = yaw(poses) - yaw(truth)
    return np.abs((d + math.pi) % (2.0 * math.pi) - math.pi)


# ---- the update from the field ------------------------------------------------------------------------------------------------------------
def update_case(ra, orc, n_particles, n_beams):
    """cadmix20k: (poses, attrs, beams, Tsb) -- particles spread over the hall (some against its walls: end points outside the lattice,
    which has no margin), beams sampled from the oracle's scan at the truth pose (with repetition beyond its 1024 points)"""
    from rmcl_amd import synthetic as syn
    truth, Tsb, cloud = scan(orc, "cadmix20k")
    beams = ra.sample_beams(cloud, n_beams, seed=300 + n_beams)
    assert len(beams) == n_beams
    poses, attrs = syn.uniform_particles(n_particles, seed=400 + n_particles, bb_min=(-19.5, -19.5, -3.0, -0.1, -0.1, -math.pi),
                                         bb_max=(19.5, 19.5, 7.5, 0.1, 0.1, math.pi))
    return poses, attrs, beams, Tsb


def chain2000_update_case(ra, orc):
    """one small cloud on chain2000: 9 particles from the triangles of size 30 out to 1e21, 23 beams of the scan at the truth"""
    from rmcl_amd import synthetic as syn
    truth, Tsb, cloud = scan(orc, "chain2000")
    beams = ra.sample_beams(cloud, 23, seed=323)
    assert len(beams) == 23
    poses, attrs = syn.uniform_particles(9, seed=409, bb_min=(0, 0, 0, 0, 0, -math.pi), bb_max=(0, 0, 0, 0, 0, math.pi))
    x = np.array([30.0, 30.0, 900.0, 1e6, 1e12, 1e18, 3.1e19, 4.2e20, 1.3e21], F)
    poses["t"]["x"], poses["t"]["y"], poses["t"]["z"] = x, (0.04 * x).astype(F), (0.02 * x).astype(F)
    poses[0] = truth[0]
    return poses, attrs, beams, Tsb


def end_points(poses, Tsb, beams):
    """[n_particles, n_beams, 3]: field_ref.end_points' values from refine_ref's vectorised transform arithmetic (devmath.h's, which the
    device holds bit-exact to the oracle's) -- tests/test_field_cases_cpu.py holds the two against each other on these very inputs;
    field_ref's own loop takes a minute at 257 x 2049"""
    R, t = rr.pose_arrays(poses)
    with np.errstate(all="ignore"):
        return rr.end_points(R, t, Tsb, beams)
