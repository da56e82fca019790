"""Every map, query-point set, pose and mode of the closest-point tests on hard maps (tests/test_gpu_cpc_hard.py), made
deterministically from fixed seeds -- and proved non-vacuous on the CPU oracle alone by tests/test_cpc_cases_cpu.py.

Maps (build_map): the well-behaved ones of the older tests, the deep trees (chain200, chain2000, nested200: an unseeded closest-point
query pushes every sibling of every level on its first descent), the slivers (fan20k, fan200k), a CAD mix with turned beams (spatial
splits: duplicated records), a soup with every face twice, maps 5 km from the origin, a planar floor, maps of one to three triangles and
the cube with degenerate faces spliced in.

Query points (query_points): scaled to each triangle's own size, so the exponential maps are covered at every scale.  Finite points
farther than MAX_COORD from the origin are dropped by the generator: there the squared distance to everything overflows float32 and
the kernel's start value 3e38 and the oracle's INFINITY are no longer equivalent.  The SPECIAL points (NaN, +-inf, -1e20: on the far side of the origin from the chains, whose largest triangles reach 1e21) are appended
on purpose and are looked at apart (special_mask).

The float64 reference (ref64) restates point-to-triangle distance plainly; it is not bit-matched to anything.
"""
import math

import numpy as np

OUTPUT_KEYS = ("hits", "ranges", "points", "normals", "face_ids")
INVALID_FACE = 0xFFFFFFFF
FAR_OFFSET = (5000.0, -3000.0, 800.0)
MAX_COORD = 5.0e14          # finite query points stay inside: the distance to a triangle near the origin stays below 1e15, its square inside float32

MAPS = ("cube", "room30k", "sphere20k", "fan20k", "fan200k", "chain200", "chain2000", "nested200", "cadmix20k", "dupsoup", "farsoup",
        "farcube", "floor", "tri1", "tri2", "tri3", "degcube")
DEEP_MAPS = ("chain200", "chain2000", "nested200")
EARLIER_MAPS = ("cube", "room30k", "dupsoup", "cadmix20k")     # what the older closest-point tests run on (their soup has fewer faces)
WELL_SCALED = ("cube", "room30k", "sphere20k", "farsoup", "farcube", "floor", "degcube")    # two-sided bound against float64
ONE_SIDED = ("fan20k", "fan200k", "cadmix20k")                                             # d32 >= d64 - bound only
FILTER_MAPS = ("fan20k", "nested200", "chain200", "degcube", "farsoup")
GRID_MAPS = ("floor", "farsoup", "farcube", "tri1", "tri2", "tri3")
POINT_COUNTS = (1, 63, 65, 255, 257)        # around the block sizes 64 (four lanes per point) and 256 (one lane per point)
VARIANTS = (1, 2)                           # 1: one lane per point (nearest_lane_ww), 2: four lanes per point (nearest_quad)
F64_BOUND = 1e-6                            # times max(box diagonal, max |coordinate|), see f64_bound: ten times what the oracle needs


# ---- maps -----------------------------------------------------------------------------------------------------------------------
def _soup(seed, n_tri, offset=(0.0, 0.0, 0.0), scale=8.0):
    from descent_cases import soup
    return soup(seed, n_tri, offset, scale)


def floor_map(n=24, side=12.0, z=0.75):
    """a planar floor: n x n quads of two triangles, every z equal -- one extent of the map's box is exactly 0"""
    lin = np.linspace(-side / 2, side / 2, n + 1)
    X, Y = np.meshgrid(lin, lin)
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], -1).astype(np.float32)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    p00 = (j * (n + 1) + i).ravel()
    f = np.empty((2 * n * n, 3), np.uint32)
    f[0::2] = np.stack([p00, p00 + 1, p00 + n + 2], -1)
    f[1::2] = np.stack([p00, p00 + n + 2, p00 + n + 1], -1)
    return v, f


def few_triangles(n_tri):
    """one to three triangles that share no plane: node slots without a child stay at 1e30"""
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0],
                  [0.5, 0.5, 1.5], [2.5, 0.5, 1.0], [0.5, 2.5, 2.0],
                  [-1.0, -1.0, -0.5], [-1.0, 1.0, 0.5], [-1.5, 0.0, 2.0]], np.float32)
    f = np.arange(9, dtype=np.uint32).reshape(3, 3)
    return v[:3 * n_tri].copy(), f[:n_tri].copy()


DEGENERATE_KINDS = ("collinear", "two_equal", "three_equal", "cyclic")


def degenerate_cube():
    """the cube with degenerate faces spliced in at the start, in the middle and at the end of the face list (the ids of the cube's own
    faces shift): collinear with three distinct vertices, two equal vertices, three equal vertices and a cyclic repeat (b, c, a) of the
    same collinear face.  Returns (v, f, is_degenerate)."""
    from rmcl_amd import synthetic as syn
    v, f = syn.cube_room()
    rng = np.random.RandomState(61)
    nv = len(v)
    extra_v, groups = [], []
    for g in range(3):                      # start / middle / end
        faces = []
        for k in range(6):
            a = np.round(rng.uniform(-4.0, 4.0, 3) * 64.0) / 64.0      # multiples of 1/64: a, a + d and a + 2 d are exact in float32,
            d = np.round(rng.uniform(-0.9, 0.9, 3) * 64.0) / 64.0      # the three vertices exactly collinear
            d[k % 3] = (k + 1) / 8.0
            base = nv + len(extra_v)
            extra_v += [a, a + d, a + 2.0 * d]
            coll = [base, base + 1, base + 2]
            faces += [coll, [base, base, base + 2], [base + 1, base + 1, base + 1], [coll[1], coll[2], coll[0]]]
        groups.append(np.asarray(faces, np.uint32))
    vv = np.concatenate([v, np.asarray(extra_v, np.float32)])
    half = len(f) // 2
    ff = np.concatenate([groups[0], f[:half], groups[1], f[half:], groups[2]])
    deg = np.zeros(len(ff), bool)
    n0, n1 = len(groups[0]), len(groups[1])
    deg[:n0] = True
    deg[n0 + half:n0 + half + n1] = True
    deg[len(ff) - len(groups[2]):] = True
    return vv, ff, deg


def build_map(name):
    from rmcl_amd import synthetic as syn
    from descent_cases import duplicate_faces
    if name == "cube":
        return syn.cube_room()
    if name == "room30k":
        return syn.noisy_room(30000)
    if name == "sphere20k":
        return syn.uv_sphere(20000)
    if name == "fan20k":
        return syn.sliver_fan(20000)
    if name == "fan200k":
        return syn.sliver_fan(200000)
    if name == "chain200":
        return syn.exp_chain(200, 1.5)
    if name == "chain2000":
        return syn.exp_chain(2000, 1.05)
    if name == "nested200":
        return syn.nested_triangles(200, 1.2, 1e-3)
    if name == "cadmix20k":
        return syn.cad_mix(20000, beam_yaw_deg=35.0, beam_tilt_deg=12.0, n_beams=60)
    if name == "dupsoup":
        return duplicate_faces(*_soup(31, 1500), seed=32)
    if name == "farsoup":
        return _soup(33, 1500, offset=FAR_OFFSET)
    if name == "farcube":
        v, f = syn.cube_room()
        return (v.astype(np.float64) + np.asarray(FAR_OFFSET)).astype(np.float32), f
    if name == "floor":
        return floor_map()
    if name in ("tri1", "tri2", "tri3"):
        return few_triangles(int(name[3]))
    if name == "degcube":
        return degenerate_cube()[:2]
    raise KeyError(name)


def map_scale(v):
    """max(box diagonal, max |coordinate|): what float32 rounding of the map's coordinates is relative to"""
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    return float(max(np.linalg.norm(vv.max(0) - vv.min(0)), np.abs(vv).max()))


def f64_bound(v, pts):
    """per point: F64_BOUND * max(box diagonal, max |coordinate| of the map, max |coordinate| of the point) -- float32 rounding is
    relative to the largest magnitude that enters the distance, and a point 40 box sizes away brings its own"""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    return F64_BOUND * np.maximum(map_scale(v), np.abs(p).max(axis=1))


def map_centre(v):
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    return 0.5 * (vv.min(0) + vv.max(0))


# ---- query points ---------------------------------------------------------------------------------------------------------------
N_POINTS = {"fan200k": 384}         # brute force over 200 000 slivers is the expensive part
N_POINTS_DEFAULT = 2560

SPECIAL_POINTS = np.array([[np.nan, 0.0, 0.0], [0.0, np.nan, 1.0], [np.nan, np.nan, np.nan], [np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0],
                           [np.inf, np.inf, -np.inf], [0.5, 0.25, np.inf], [-1e20, 0.0, 0.0], [0.0, -1e20, 0.0], [-1e20, -1e20, -1e20]],
                          np.float32)


def special_mask(pts):
    """the points that carry NaN, an infinity or 1e20: they must come back as `not found`"""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    return ~(np.abs(p) < 1e19).all(axis=1)      # NaN compares false


def query_points(name, v, f, n=None):
    """float32 (n, 3), seeded per map: on faces, on shared edges and vertices, off a face by 0.3 and by 5 of ITS sizes, uniform in the
    inflated box, 40 box sizes outside, the box's centre (of the hollow sphere: everything equidistant), and the special points spread
    over the set (so that they fall into different blocks and quads).  Finite points beyond MAX_COORD are dropped and replaced by more
    of the rest; the order is shuffled so that any prefix (POINT_COUNTS) holds every kind."""
    n = N_POINTS.get(name, N_POINTS_DEFAULT) if n is None else n
    rng = np.random.RandomState(7000 + MAPS.index(name))
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    ff = np.asarray(f, np.int64).reshape(-1, 3)
    lo, hi = vv.min(0), vv.max(0)
    centre, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3 * max(float(np.linalg.norm(hi - lo)), 1e-3))
    n_gen = 4 * n + 64

    def on_faces(k):
        idx = rng.randint(len(ff), size=k)
        a, b, c = vv[ff[idx, 0]], vv[ff[idx, 1]], vv[ff[idx, 2]]
        u, w = rng.uniform(size=(2, k, 1))
        flip = (u + w) > 1.0
        u, w = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - w, w)
        size = np.maximum(np.linalg.norm(b - a, axis=1), np.maximum(np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)))
        return a + u * (b - a) + w * (c - a), size[:, None]

    def unit(k):
        d = rng.normal(size=(k, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    q = n_gen // 9
    parts = [on_faces(2 * q)[0]]
    idx = rng.randint(len(ff), size=q)
    corner = rng.randint(3, size=q)
    vert = vv[ff[idx, corner]]
    mid = 0.5 * (vert + vv[ff[idx, (corner + 1) % 3]])
    parts += [vert[: q // 2], mid[q // 2:]]
    for mult in (0.3, 5.0):
        p, size = on_faces(q)
        parts.append(p + unit(q) * size * mult)
    parts.append(centre + rng.uniform(-0.6, 0.6, (2 * q, 3)) * ext)
    parts.append(centre + unit(q) * 40.0 * float(np.linalg.norm(ext)) * rng.uniform(0.5, 1.0, (q, 1)))
    pts = np.concatenate(parts)
    pts = pts[(np.abs(pts) <= MAX_COORD).all(axis=1)]
    pts = pts[rng.permutation(len(pts))][: n - len(SPECIAL_POINTS) - 1]
    if np.abs(centre).max() > MAX_COORD:
        centre = np.zeros(3)
    pts = np.concatenate([centre[None], pts]).astype(np.float32)
    assert len(pts) == n - len(SPECIAL_POINTS), "%s: only %d usable points" % (name, len(pts))
    # the special points: one among the first 63, the others spread evenly
    where = np.unique(np.concatenate([[5], np.linspace(17, len(pts) - 1, len(SPECIAL_POINTS) - 1).astype(int)]))
    assert len(where) == len(SPECIAL_POINTS)
    special = SPECIAL_POINTS.copy()
    fin = np.isfinite(special) & (np.abs(special) < 1e19)
    special = np.where(fin, special + centre.astype(np.float32), special).astype(np.float32)
    return np.insert(pts, where - np.arange(len(where)), special, axis=0)


def max_dists(v, f):
    """the two gates of a map, from the median triangle size s: 0.25 s and 3 s -- points on faces and 0.3 sizes off hit, points 5 sizes off
    and far outside miss (tests/test_cpc_cases_cpu.py asserts both are there)"""
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    ff = np.asarray(f, np.int64).reshape(-1, 3)
    a, b, c = vv[ff[:, 0]], vv[ff[:, 1]], vv[ff[:, 2]]
    size = np.maximum(np.linalg.norm(b - a, axis=1), np.maximum(np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)))
    s = float(np.median(size[size > 0]))
    return float(np.float32(0.25 * s)), float(np.float32(3.0 * s))


def identity():
    from rmcl_amd import types as T
    return T.identity()


# ---- poses ----------------------------------------------------------------------------------------------------------------------
def poses(v):
    """identity (the query points are given in map coordinates: points on vertices stay exact ties), two small steps, a 2 m jump.  The
    rotations turn about the map's centre, so that a map 5 km away stays under its points."""
    from rmcl_amd import types as T
    c = map_centre(v)
    out = [T.identity()]
    for rpy, dt in (((0.004, -0.003, 0.006), (0.01, -0.015, 0.005)), ((0.008, -0.006, 0.012), (0.02, -0.03, 0.01)),
                    ((0.05, -0.02, 0.4), (1.6, -1.1, 0.5))):
        q = np.array(T.euler_to_quat(*rpy), np.float64)
        u, w = q[:3], q[3]
        rc = c + 2.0 * np.cross(u, np.cross(u, c) + w * c)
        out.append(T.transform(tuple(float(x) for x in q), tuple(float(x) for x in (c - rc + np.asarray(dt)))))
    return out


# ---- the oracle, on several threads (the C call releases the GIL; every point is independent) -------------------------------------
def oracle_cpc(m, pose, pts, max_dist, bvh=False, nthreads=8):
    import threading
    from rmcl_amd import types as T
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    nthreads = max(1, min(nthreads, len(pts) // 32))
    cuts = np.linspace(0, len(pts), nthreads + 1).astype(int)
    res = [None] * nthreads

    def work(k):
        res[k] = m.cpc_find(T.identity(), pose, pts[cuts[k]:cuts[k + 1]], max_dist, bvh=bvh)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(nthreads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return {k: np.concatenate([r[k] for r in res]) for k in OUTPUT_KEYS}


# ---- the float64 reference --------------------------------------------------------------------------------------------------------
def _seg_d2(p, a, b):
    ab, ap = b - a, p - a
    den = np.einsum("ij,ij->i", ab, ab)
    t = np.clip(np.einsum("ij,ij->i", ap, ab) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    d = ap - t[:, None] * ab
    return np.einsum("ij,ij->i", d, d)


def tri_d2_64(p, a, b, c):
    """squared distance of ONE point p (3,) to the triangles (a, b, c) (each (m, 3)), float64: the distance to the plane where the
    point's projection falls inside the triangle, else the smallest distance to the three edges.  Degenerate triangles have no inside."""
    p = np.asarray(p, np.float64)[None]
    ab, ac, ap = b - a, c - a, p - a
    nrm = np.cross(ab, ac)
    nn = np.einsum("ij,ij->i", nrm, nrm)
    safe = np.where(nn > 0, nn, 1.0)
    wc = np.einsum("ij,ij->i", np.cross(ab, ap), nrm) / safe
    wb = np.einsum("ij,ij->i", np.cross(ap, ac), nrm) / safe
    inside = (nn > 0) & (wb >= 0) & (wc >= 0) & (wb + wc <= 1)
    plane = np.einsum("ij,ij->i", ap, nrm) ** 2 / safe
    edge = np.minimum(_seg_d2(p, a, b), np.minimum(_seg_d2(p, b, c), _seg_d2(p, c, a)))
    return np.where(inside, plane, edge)


def ref64(v, f, pts, hint=None):
    """(distance, face id, number of faces at exactly that distance) of the closest triangle in float64, smallest id among exact ties;
    NaN / -1 / 0 for points that are not finite.
    `hint` (a face id per point, any) only saves work: the distance to that face bounds the answer, and a triangle whose box is farther
    cannot win.  The result does not depend on it."""
    vv = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    ff = np.asarray(f, np.int64).reshape(-1, 3)
    a, b, c = vv[ff[:, 0]], vv[ff[:, 1]], vv[ff[:, 2]]
    blo, bhi = np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))
    pts = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.full(len(pts), np.nan)
    face = np.full(len(pts), -1, np.int64)
    n_min = np.zeros(len(pts), np.int64)
    for i, p in enumerate(pts):
        if not np.isfinite(p).all():
            continue
        h = 0 if hint is None or not (0 <= int(hint[i]) < len(ff)) else int(hint[i])
        ub = float(tri_d2_64(p, a[h:h + 1], b[h:h + 1], c[h:h + 1])[0])
        gap = np.maximum(np.maximum(blo - p, p - bhi), 0.0)
        cand = np.nonzero(np.einsum("ij,ij->i", gap, gap) <= ub * (1.0 + 1e-9))[0]
        d2 = tri_d2_64(p, a[cand], b[cand], c[cand])
        k = int(np.argmin(d2))              # first of the minima: cand is sorted
        d[i], face[i], n_min[i] = math.sqrt(d2[k]), cand[k], int((d2 == d2[k]).sum())
    return d, face, n_min


def dist_to_face64(v, f, pts, faces):
    """float64 distance of every point to the face named for it"""
    vv = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    ff = np.asarray(f, np.int64).reshape(-1, 3)
    pts = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.empty(len(pts))
    for i, (p, k) in enumerate(zip(pts, np.asarray(faces, np.int64))):
        out[i] = math.sqrt(tri_d2_64(p, vv[ff[k:k + 1, 0]], vv[ff[k:k + 1, 1]], vv[ff[k:k + 1, 2]])[0])
    return out


# ---- the operator's modes ---------------------------------------------------------------------------------------------------------
MODES = ("bare", "grid", "warm")            # + bounded, at both gates of a map (max_dists)


def make_operator(ra, hm, variant, mode, max_dist, pts):
    """a fresh closest-point operator: bare = no tracking, no near grid (the reference's unseeded query); grid = the default cold path;
    warm = tracking (+ the grid for points without a record); bounded = the default with the search limited to max_dist"""
    from rmcl_amd import types as T
    op = ra.CPCHip(hm)
    op.set_variant(variant)
    op.setTsb(T.identity())
    op.params.max_dist = max_dist
    op.adaptive_max_dist_min = max_dist
    if mode == "bare":
        op.set_tracking(False)
        op.set_grid(False)
    elif mode == "grid":
        op.set_tracking(False)
    elif mode == "bounded":
        op.set_bounded(True)
    else:
        assert mode == "warm"
    op.set_dataset(pts, None)
    return op


# ---- the particle filter's closest-point mode -----------------------------------------------------------------------------------------
def filter_case(name, v, f, n_particles=150, n_beams=23):
    """(poses, attrs, beams) for PCDSensorUpdaterHip with correspondence_type = 1: particles stand on ordinary query points inside the
    map's box (so they are spread over every scale of an exponential map), headings random, small roll and pitch; the beams end 0.1 to
    5 median triangle sizes from the sensor"""
    from rmcl_amd import pf, synthetic as syn
    rng = np.random.RandomState(9000 + MAPS.index(name))
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    lo, hi = vv.min(0), vv.max(0)
    pts = query_points(name, v, f).astype(np.float64)
    inside = ~special_mask(pts) & ((pts >= lo) & (pts <= hi)).all(axis=1)
    pos = pts[inside][:n_particles]
    assert len(pos) == n_particles, "%s: only %d query points inside the box" % (name, len(pos))
    poses, attrs = syn.uniform_particles(n_particles, seed=9100 + MAPS.index(name), bb_min=(0, 0, 0, -0.2, -0.2, -math.pi),
                                         bb_max=(0, 0, 0, 0.2, 0.2, math.pi))
    poses["t"]["x"], poses["t"]["y"], poses["t"]["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    d = rng.normal(size=(n_beams, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = max_dists(v, f)[0] * 4.0 * 10.0 ** rng.uniform(-1.0, math.log10(5.0), (n_beams, 1))
    return poses, attrs, pf.beams_from_points((d * length).astype(np.float32))
