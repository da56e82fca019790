"""Every map, model, pose and knob set of the tests of find kind 32's cooperative descent (tests/test_gpu_find_descent.py), made
deterministically from fixed seeds -- and proved non-vacuous on the CPU oracle alone by tests/test_find_descent_cases_cpu.py.

Knobs: rmclhip_rcc_set_descent(rcc, final_cap, word) with word = levels | leaf_cap << 8 | four_wide << 31 (descent_word below).
Leaf-cap bits of 0 KEEP the operator's leaf cap, every call resets the tile-mapping override and the wide flag, and autotune leaves
its cap on the operator: always pass a complete word (set_knobs does) on a fresh operator or after an explicit reset.

Randomised scans: RANDOM_MAPS x N_RANDOM_SCANS `Scan`s (random_scans).  A Scan carries one sensor model (spherical, O1Dn or pinhole),
a mount and a pose; it knows how to ask the oracle for the whole scan, how to ask brute force for a sample of its OWN rays, and how
to configure a GPU operator.  Outside sensors are aimed at the map, their field of view follows the map's angular size and their
range reaches through it; on the sparse maps every range does.
"""
import math

import numpy as np

OUTPUT_KEYS = ("hits", "ranges", "points", "normals", "face_ids")

# ---- knob sets: (final_cap, levels, leaf_cap, four_wide) ------------------------------------------------------------------------
DEFAULT_KNOBS = (64, 24, 24, False)
KNOB_SETS = (
    DEFAULT_KNOBS,              # the default
    (32, 24, 24, False),        # autotune's other candidates
    (12, 24, 24, False),
    (64, 24, 24, True),         # the path of maps beyond kMaxNodes16: four-wide nodes
    (12, 24, 24, True),
    (64, 0, 24, False),         # nothing / one level / two levels expanded: unexpanded inner nodes on the stacks behind mask-tested leaves
    (64, 1, 24, False),
    (64, 2, 24, False),
    (0, 24, 24, False),         # the prediction break at the first level
    (64, 24, 1, False),         # nearly every wave that descends falls back to the root
    (64, 24, 255, False),       # no wave falls back to the root
)
TILE_KNOBS = (DEFAULT_KNOBS, (12, 24, 24, False), (64, 24, 24, True))      # the knob sets that go through every tile shape
TILE_BITS = (0, 1, 3, 4, 6, 7)              # set_variant bits 4..6: 0 automatic, else 1 + log2(tile width)
RANDOM_KNOBS = (DEFAULT_KNOBS, (12, 24, 24, False), (64, 24, 24, True), (64, 1, 24, False))
BATCH_KNOBS = ((12, 24, 24, False), (64, 24, 24, True))
MOMENT_KNOBS = ((12, 24, 24, False), (64, 24, 24, True), (64, 24, 1, False))


def descent_word(levels, leaf_cap, four_wide):
    """the second argument of rmclhip_rcc_set_descent"""
    assert 0 <= levels <= 255 and 0 < leaf_cap <= 255, "a leaf cap of 0 would keep the operator's old one"
    return int(levels) | (int(leaf_cap) << 8) | ((1 if four_wide else 0) << 31)


def knob_name(knobs):
    return "cap%d-lev%d-leaf%d-%s" % (knobs[0], knobs[1], knobs[2], "four" if knobs[3] else "wide")


def set_knobs(op, knobs):
    from rmcl_amd import _capi
    cap, levels, leaf_cap, four_wide = knobs
    _capi.check(_capi.lib().rmclhip_rcc_set_descent(op._h, int(cap), descent_word(levels, leaf_cap, four_wide)))


def variant_word(kind, tile_bits=0):
    """rmclhip_rcc_set_variant's word for a traversal kind (bits 4 and 5 of the kind travel in bits 13 and 14) and a tile shape"""
    return (kind & 15) | (((kind >> 4) & 1) << 13) | (((kind >> 5) & 1) << 14) | (tile_bits << 4)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
def soup(seed, n_tri, offset=(0.0, 0.0, 0.0), scale=8.0):
    """a random triangle soup: intersecting, sliver and zero-area triangles, a stack of coplanar overlapping ones"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-scale, scale, (n_tri, 1, 3))
    tri = c + rng.normal(size=(n_tri, 3, 3)) * rng.uniform(0.05, 0.7, (n_tri, 1, 1))
    tri[::17, 2] = tri[::17, 1]                                     # zero-area triangles (two equal vertices)
    tri[::23] = tri[::23] * (1.0, 1.0, 0.0) + (0.0, 0.0, 0.5)       # a stack of coplanar, overlapping triangles in z = 0.5
    v = (tri.reshape(-1, 3) + np.asarray(offset)).astype(np.float32)
    f = np.arange(3 * n_tri, dtype=np.uint32).reshape(-1, 3)
    return v, f


def duplicate_faces(v, f, seed):
    """every face twice, ids shuffled: all hits tie exactly"""
    rng = np.random.RandomState(seed)
    ff = np.concatenate([f, f])
    return v, ff[rng.permutation(len(ff))]


def tiny_map(n_tri):
    """the smallest maps: one triangle, or four (a tetrahedron's faces) -- a root with nothing below it"""
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, 0.5, 1.5]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]], np.uint32)
    return (v[:3].copy(), f[:1].copy()) if n_tri == 1 else (v, f)


def tiny_model():
    """32 x 32 rays, +-45 degrees, full circle; the range ends inside the four-triangle map: hits on every face, and misses"""
    from rmcl_amd import types as T
    f32 = np.float32
    return T.spherical_model(f32(-math.pi / 4), f32((math.pi / 2) / 31), 32, f32(-math.pi), f32(2 * math.pi / 32), 32, f32(0.0), f32(0.8))


def tiny_pose():
    """above the one triangle, inside the four"""
    from rmcl_amd import types as T
    return T.transform_from_rpy((0.6, 0.6, 0.5), (0.1, -0.05, 0.3))


RANDOM_MAPS = ("soup", "duplicates", "room", "tiny", "far", "fan", "cadmix")
SPARSE_MAPS = ("soup", "duplicates", "far", "fan", "tiny")      # most rays pass through (or by) these: every range reaches through the map
N_RANDOM_SCANS = 24


def random_map(name):
    from rmcl_amd import synthetic as syn
    if name == "soup":
        return soup(21, 2500)
    if name == "duplicates":
        return duplicate_faces(*soup(23, 1500), seed=24)
    if name == "room":
        return syn.noisy_room(20000)
    if name == "tiny":
        return syn.cube_room(side=0.2)
    if name == "far":
        return soup(22, 1500, offset=(4000.0, 2500.0, -700.0), scale=30.0)
    if name == "fan":
        return syn.sliver_fan(20000)
    if name == "cadmix":
        return syn.cad_mix(20000, beam_yaw_deg=35.0, beam_tilt_deg=12.0, n_beams=60)
    raise KeyError(name)


# ---- rotations in double (the generator never needs the native library) ---------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _qrot(q, p):
    u, w = np.asarray(q[:3]), q[3]
    p = np.asarray(p, np.float64)
    return p + 2.0 * np.cross(u, np.cross(u, p) + w * p)


def _qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def _q_rpy(roll, pitch, yaw):
    from rmcl_amd import types as T
    return np.array(T.euler_to_quat(roll, pitch, yaw), np.float64)


def _transform(q, t):
    from rmcl_amd import types as T
    return T.transform(tuple(float(x) for x in q), tuple(float(x) for x in t))


class Scan:
    """one scan of the randomised set: kind 'spherical' (model), 'o1dn' (W, H, far, orig, dirs) or 'pinhole' (W, H, far, f, c)"""

    def __init__(self, name, kind, Tsb, pose, **kw):
        self.name, self.kind, self.Tsb, self.pose = name, kind, Tsb, pose
        self.__dict__.update(kw)

    @property
    def n_rays(self):
        return self.model.phi.size * self.model.theta.size if self.kind == "spherical" else self.W * self.H

    def oracle(self, m, bvh=True, nthreads=8):
        """the whole scan from the oracle (m: oracle.Mesh)"""
        if self.kind == "spherical":
            return m.simulate_spherical(self.model, self.Tsb, self.pose, bvh=bvh, nthreads=nthreads)
        if self.kind == "o1dn":
            return m.simulate_o1dn(self.W, self.H, 0.0, self.far, self.orig, self.dirs, self.Tsb, self.pose, bvh=bvh, nthreads=nthreads)
        return m.simulate_pinhole(self.W, self.H, 0.0, self.far, self.f, self.c, self.Tsb, self.pose, bvh=bvh, nthreads=nthreads)

    def brute_force_sample(self, orc, m, n_sample=2048, nthreads=8):
        """(idx, hits, face ids) of at most n_sample of the scan's OWN rays against every triangle (no BVH): the rays go through the
        oracle's O1Dn entry with the model's own direction values, mount and pose -- the same arithmetic as the model's own entry"""
        if self.kind == "spherical":
            dirs, orig, rmin, rmax = orc.spherical_directions(self.model), (0.0, 0.0, 0.0), self.model.range.min, self.model.range.max
        elif self.kind == "o1dn":
            dirs, orig, rmin, rmax = self.dirs, self.orig, 0.0, self.far
        else:
            dirs, orig, rmin, rmax = orc.pinhole_directions(self.W, self.H, self.f, self.c), (0.0, 0.0, 0.0), 0.0, self.far
        n = len(dirs)
        idx = np.sort(np.random.RandomState(4321).choice(n, size=min(n_sample, n), replace=False))
        sub = m.simulate_o1dn(len(idx), 1, rmin, rmax, orig, dirs[idx], self.Tsb, self.pose, bvh=False, nthreads=nthreads,
                              want=("hits", "ranges", "face_ids"))
        return idx, sub["hits"], sub["face_ids"]

    def operator(self, ra, hm):
        """a fresh GPU operator with this scan's model and mount"""
        if self.kind == "spherical":
            op = ra.RCCHipSpherical(hm)
            op.setModel(self.model)
        elif self.kind == "o1dn":
            op = ra.RCCHipO1Dn(hm)
            op.setModel(self.W, self.H, 0.0, self.far, self.orig, self.dirs)
        else:
            op = ra.RCCHipPinhole(hm)
            op.setModel(self.W, self.H, 0.0, self.far, self.f[0], self.f[1], self.c[0], self.c[1])
        op.setTsb(self.Tsb)
        return op


_MODEL_OF_ROW = ("spherical", "spherical", "o1dn", "spherical", "o1dn", "pinhole")     # case // 4; case % 4 = where the sensor stands
_MAP_SEED = {name: 1000 + 17 * i for i, name in enumerate(RANDOM_MAPS)}


def random_scans(name, v, n_scans=N_RANDOM_SCANS):
    """the randomised scans of one map: sensor inside / just outside / far outside / on a face of the bounding box (case % 4);
    spherical models from 1 x 7 to 128 x 1024 rays with narrow and full fields of view, O1Dn models with NaN and repeated directions,
    pinhole models (case // 4); random mounts.  Cutting n_scans keeps the first cases: every stand and every model kind stay."""
    from rmcl_amd import types as T
    f32 = np.float32
    rng = np.random.RandomState(_MAP_SEED[name])
    vv = np.asarray(v, np.float64).reshape(-1, 3)
    lo, hi = vv.min(0), vv.max(0)
    centre, ext = 0.5 * (lo + hi), hi - lo
    diag = float(np.linalg.norm(ext))
    scans = []
    for case in range(n_scans):
        where, kind = case % 4, _MODEL_OF_ROW[(case // 4) % 6]
        if where == 0:
            pos = centre + rng.uniform(-0.45, 0.45, 3) * ext
        elif where == 1:
            pos = centre + rng.choice([-1.0, 1.0], 3) * rng.uniform(0.55, 0.9, 3) * ext
        elif where == 2:
            d = rng.normal(size=3)
            pos = centre + d / np.linalg.norm(d) * rng.uniform(15.0, 60.0) * diag
        else:
            pos = centre + rng.uniform(-0.5, 0.5, 3) * ext
            ax = rng.randint(3)
            pos[ax] = lo[ax] if rng.rand() < 0.5 else hi[ax]
        to_c = centre - pos
        dist = float(np.linalg.norm(to_c))
        ang = math.atan2(0.5 * diag, max(dist, 1e-9))            # angular radius of the map's bounding sphere seen from the sensor
        aimed = where in (1, 2) or (where == 3 and case % 8 == 3)
        if aimed:     # look at the map's centre: jitter of at most 0.2 rad, and no more than a third of the map's angular radius
            j = min(0.2, ang / 3.0)
            yaw = math.atan2(to_c[1], to_c[0]) + rng.uniform(-j, j)
            pitch = -math.atan2(to_c[2], math.hypot(to_c[0], to_c[1])) + rng.uniform(-j, j)
            q_s = _q_rpy(rng.uniform(-math.pi, math.pi), 0.0, 0.0)
            q_s = _qmul(_q_rpy(0.0, pitch, yaw), q_s)
        else:
            q_s = _q_rpy(*rng.uniform(-math.pi, math.pi, 3))
        # the mount is random; the body pose follows from where the SENSOR shall stand: Tbm = Tsm * inv(Tsb)
        t_sb, q_sb = rng.uniform(-0.3, 0.3, 3), _q_rpy(*rng.uniform(-0.5, 0.5, 3))
        q_b = _qmul(q_s, _qconj(q_sb))
        Tsb, pose = _transform(q_sb, t_sb), _transform(q_b, pos - _qrot(q_b, t_sb))
        far = float(10.0 ** rng.uniform(-0.5, 4.0))
        if where in (1, 2) or name in SPARSE_MAPS:
            far = max(far, 2.0 * dist + diag)                   # reaches through the map from wherever the sensor stands
        # the field of view: anything for a sensor in the map, the map's angular size (half to three times) for one that looks at it
        if aimed:
            fov_h = fov_v = float(min(2.0 * ang * rng.uniform(0.5, 3.0), 0.98 * math.pi))
        else:
            fov_v, fov_h = float(rng.uniform(0.03, math.pi)), float(rng.uniform(0.03, 2.0 * math.pi))
        tag = "%s/%02d/%s/%s" % (name, case, ("inside", "outside", "far", "face")[where], kind)
        if kind == "o1dn":
            W, H = int(rng.choice([1, 9, 64, 333])), int(rng.choice([1, 8, 17]))
            if aimed:           # a cone about +x
                r = math.tan(min(0.5 * fov_h, 1.4))
                d = np.concatenate([np.ones((W * H, 1)), rng.uniform(-r, r, (W * H, 2))], axis=1).astype(np.float32)
            else:
                d = rng.normal(size=(W * H, 3)).astype(np.float32)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            d[rng.rand(W * H) < 0.1] = np.nan
            d[rng.rand(W * H) < 0.1] = d[0]
            orig = tuple(float(x) for x in rng.uniform(-0.2, 0.2, 3) * min(1.0, 0.1 * diag))
            scans.append(Scan(tag, kind, Tsb, pose, W=W, H=H, far=far, orig=orig, dirs=d))
        elif kind == "pinhole":
            W, H = [(97, 33), (64, 48), (160, 120), (33, 17)][where]
            fov = min(fov_h, 2.6)
            fx = 0.5 * W / math.tan(0.5 * fov)
            scans.append(Scan(tag, kind, Tsb, pose, W=W, H=H, far=far, f=(fx, fx), c=(0.5 * W, 0.5 * H)))
        else:
            H, W = int(rng.choice([1, 3, 16, 64])), int(rng.choice([7, 64, 512]))
            if case == 0:
                H, W = 1, 7
            elif case == 4:         # the full size, full circle
                H, W, fov_h, fov_v = 128, 1024, 2.0 * math.pi, 0.5 * math.pi
            elif case == 5:         # ... and looking at the map from outside through a narrow window
                H, W = 128, 1024
            model = T.spherical_model(f32(-fov_v / 2), f32(fov_v / max(H - 1, 1)), H, f32(-fov_h / 2), f32(fov_h / W), W, f32(0.0), f32(far))
            scans.append(Scan(tag, kind, Tsb, pose, model=model))
    return scans


def hit_share_conditions(per_map):
    """per_map: {map name: [hits array of every scan]} -> asserts the conditions that keep the randomised tests from being vacuous:
    in each map at least half of the scans contain a hit and at least a third both hits and misses; over all scans the hit share lies
    between 10 % and 90 %"""
    n_hits = n_rays = 0
    for name, scans in per_map.items():
        some = sum(1 for h in scans if h.any())
        both = sum(1 for h in scans if h.any() and not h.all())
        assert 2 * some >= len(scans), "%s: only %d of %d scans contain a hit" % (name, some, len(scans))
        assert 3 * both >= len(scans), "%s: only %d of %d scans contain hits and misses" % (name, both, len(scans))
        n_hits += sum(int(h.sum()) for h in scans)
        n_rays += sum(h.size for h in scans)
    assert 0.1 * n_rays <= n_hits <= 0.9 * n_rays, "hit share %d of %d rays" % (n_hits, n_rays)
    return n_hits, n_rays
