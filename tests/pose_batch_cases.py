"""Every map, model and pose list of the pose-batch tests (tests/test_gpu_pose_batch.py), made from fixed seeds -- and proved fit for
their purpose on the CPU oracle alone by tests/test_pose_batch_cases_cpu.py.

Model: 21 x 150 rays (3150) in four forms -- spherical, pinhole, O1Dn with an origin that is not the sensor's, OnDn with per-ray origins
within +-0.2 m.  21 and 150 are multiples of no tile side (widths 4, 8, 16, 32 / heights 16, 8, 4, 2): every tile shape has ragged
right and bottom tiles, and at widths 8 and 32 the tile count (57, 55) is no multiple of four, so the last workgroup of a pose holds
fewer than four tiles.  The O1Dn and OnDn direction tables carry NaN rows: 20 drawn ones and, for every forced tile width, the
central ray of the middle tile of some workgroups (what k_batch_tile_keys makes a workgroup's key from).  Range limit 40 m.

Maps: room30k, cube, and `quad`: one 16 m x 16 m square of two triangles in z = 0 -- a bounding box without extent on one axis, a
tree without a frontier table.

Pose lists (TRANSFORM arrays): `spread` (37 all over the room, pitched and at every height), `edges` (nine, see EDGE_NAMES),
`one_cell` (40 with NaN translations: every key is 0) and the prefixes of `spread` the reduction tests use.

restated_keys() says in numpy float32, operation for operation, what k_batch_tile_keys (rmcl_amd/csrc/kernels.hip) computes for one
order entry.  It certifies the cases (how many sort cells `spread` occupies, that `one_cell` is one cell, that NaN / infinite / far
poses still get a cell) and nothing else: the GPU tests read the keys the device made.
"""
import math

import numpy as np

H, W = 21, 150
N_RAYS = H * W
RANGE_MIN, RANGE_MAX = 0.1, 40.0
TILE_BITS = (3, 4, 5, 6)                    # bits 4..7 of the variant word: 1 + log2(tile width) -> widths 4, 8, 16, 32
MODEL_KINDS = ("spherical", "pinhole", "o1dn", "ondn")
MAP_NAMES = ("room30k", "cube", "quad")
ORDER_SETTINGS = (0, 1, 2, 3, 7, 1000)      # rmclhip_rcc_set_batch_order: pose-major, granule 64, 2, 3, 7, one larger than any list here
REDUCE_COUNTS = (1, 2, 3, 4, 5, 9)          # both sides of reduce_num_blocks' switch at four poses
N_ORDER_CELLS = 4096
# the floors the GPU tests hold the device's keys of `spread` to (tests/test_pose_batch_cases_cpu.py shows the restated keys meet them
# with a factor of two to spare): distinct cells, and runs of sixteen cells (one thread of k_batch_cell_scan each) touched
MIN_DISTINCT_CELLS, MIN_SCAN_RUNS = 200, 100
O1DN_ORIG = (0.05, -0.02, 0.1)

EDGE_NAMES = ("interior A", "outside looking in", "interior B", "500 m away", "NaN translation", "interior A again",
              "NaN quaternion", "sensor on a bounding-box face", "interior A a third time")
EDGE_COPIES_OF_A = (0, 5, 8)
EDGE_NO_HIT = (3, 4, 6)
EDGE_INTERIOR = (0, 2, 5, 8)


def variant_word(kind, tile_bits=0):
    """rmclhip_rcc_set_variant's word for a traversal kind (bits 4 and 5 of the kind travel in bits 13 and 14) and a forced tile shape"""
    return (kind & 15) | (((kind >> 4) & 1) << 13) | (((kind >> 5) & 1) << 14) | (tile_bits << 4)


def group_of(kind):
    """tiles per workgroup of a find of this traversal kind: the quad kinds (2, and 25 = 2 with the frontier start) run one tile per
    workgroup"""
    return 1 if kind in (2, 25) else 4


def tiling(twl, h=H, w=W):
    """(tiles_x, tiles_y) of tiles 2^twl wide and 64 >> twl tall"""
    tw, th = 1 << twl, 64 >> twl
    return (w + tw - 1) // tw, (h + th - 1) // th


def n_groups(twl, group, h=H, w=W):
    tx, ty = tiling(twl, h, w)
    return (tx * ty + group - 1) // group


def central_ray(twl, group, g, h=H, w=W):
    """(cv, ch) of the ray k_batch_tile_keys reads for workgroup g: the centre of the middle tile of its `group` tiles, clamped"""
    tx_n, ty_n = tiling(twl, h, w)
    tile = min(g * group + (group >> 1), tx_n * ty_n - 1)
    ty, tx = divmod(tile, tx_n)
    return min((ty << (6 - twl)) + (32 >> twl), h - 1), min((tx << twl) + ((1 << twl) >> 1), w - 1)


# ---- maps -------------------------------------------------------------------------------------------------------------------------
def quad_map():
    v = np.array([[-8.0, -8.0, 0.0], [8.0, -8.0, 0.0], [8.0, 8.0, 0.0], [-8.0, 8.0, 0.0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


_MAPS, _BBOX = {}, {}


def map_arrays(name):
    from rmcl_amd import synthetic as syn
    if name not in _MAPS:
        _MAPS[name] = {"room30k": lambda: syn.noisy_room(30000), "cube": syn.cube_room, "quad": quad_map}[name]()
    return _MAPS[name]


def map_bbox(name):
    """(lo, hi) as float32[3]: the box the library's host build reports, which is what batch_order_enqueue hands to the key kernel"""
    import rmcl_amd as ra
    if name not in _BBOX:
        info, _, _ = ra.build_bvh_host(*map_arrays(name))
        _BBOX[name] = (np.array(info["bbox_min"], np.float32), np.array(info["bbox_max"], np.float32))
    return _BBOX[name]


# ---- models -----------------------------------------------------------------------------------------------------------------------
def spherical_model(h=H, w=W):
    from rmcl_amd import types as T
    f32 = np.float32
    return T.spherical_model(f32(-0.45), f32(0.9 / max(h - 1, 1)), h, f32(-math.pi), f32(2 * math.pi / w), w, f32(RANGE_MIN), f32(RANGE_MAX))


def nan_rows(h=H, w=W):
    """indices of the NaN rows of the O1Dn / OnDn direction tables"""
    rows = set(int(i) for i in np.random.RandomState(41).randint(0, h * w, 20))
    for twl in (2, 3, 4, 5):
        for group, gs in ((4, (0, 3, n_groups(twl, 4, h, w) - 1)), (1, (5, n_groups(twl, 1, h, w) - 1))):
            for g in gs:
                cv, ch = central_ray(twl, group, g, h, w)
                rows.add(cv * w + ch)
    return np.array(sorted(rows), np.int64)


def model(kind, h=H, w=W):
    """the model as tests/oracle_micp.py simulate_model takes it"""
    from rmcl_amd import synthetic as syn
    if kind == "spherical":
        return {"kind": "spherical", "model": spherical_model(h, w)}
    if kind == "pinhole":
        return {"kind": "pinhole", "width": w, "height": h, "range_min": RANGE_MIN, "range_max": RANGE_MAX,
                "f": (0.4 * w, 0.4 * w), "c": (0.5 * (w - 1), 0.5 * (h - 1))}
    dirs = syn.model_directions(spherical_model(h, w)).copy()
    if h * w > 64:
        dirs[nan_rows(h, w)] = np.nan
    if kind == "o1dn":
        return {"kind": "o1dn", "width": w, "height": h, "range_min": RANGE_MIN, "range_max": RANGE_MAX, "orig": O1DN_ORIG, "dirs": dirs}
    assert kind == "ondn"
    origs = np.random.RandomState(43).uniform(-0.2, 0.2, size=dirs.shape).astype(np.float32)
    return {"kind": "ondn", "width": w, "height": h, "range_min": RANGE_MIN, "range_max": RANGE_MAX, "origs": origs, "dirs": dirs}


def model_shape(m):
    if m["kind"] == "spherical":
        return int(m["model"].phi.size), int(m["model"].theta.size)
    return m["height"], m["width"]


def tsb():
    from rmcl_amd import synthetic as syn
    return syn.tsb_offset()


def operator(ra, hm, m, kind=None, tile_bits=0):
    """a fresh GPU operator with this model and the mount of the cases"""
    k = m["kind"]
    if k == "spherical":
        op = ra.RCCHipSpherical(hm)
        op.setModel(m["model"])
    elif k == "pinhole":
        op = ra.RCCHipPinhole(hm)
        op.setModel(m["width"], m["height"], m["range_min"], m["range_max"], m["f"][0], m["f"][1], m["c"][0], m["c"][1])
    elif k == "o1dn":
        op = ra.RCCHipO1Dn(hm)
        op.setModel(m["width"], m["height"], m["range_min"], m["range_max"], m["orig"], m["dirs"])
    else:
        op = ra.RCCHipOnDn(hm)
        op.setModel(m["width"], m["height"], m["range_min"], m["range_max"], m["origs"], m["dirs"])
    op.setTsb(tsb())
    if kind is not None:
        op.set_variant(variant_word(kind, tile_bits))
    return op


def simulate(mesh, m, poses, bvh=True, nthreads=8):
    """the oracle's scans of the model at every pose, pose-major"""
    k = m["kind"]
    if k == "spherical":
        return mesh.simulate_spherical(m["model"], tsb(), poses, bvh=bvh, nthreads=nthreads)
    size = (m["width"], m["height"], m["range_min"], m["range_max"])
    if k == "pinhole":
        return mesh.simulate_pinhole(*size, m["f"], m["c"], tsb(), poses, bvh=bvh, nthreads=nthreads)
    if k == "o1dn":
        return mesh.simulate_o1dn(*size, m["orig"], m["dirs"], tsb(), poses, bvh=bvh, nthreads=nthreads)
    return mesh.simulate_ondn(*size, m["origs"], m["dirs"], tsb(), poses, bvh=bvh, nthreads=nthreads)


def rays_s(m):
    """(origins [n, 3], directions [n, 3]) of the model's rays in the sensor frame, float32, as find_ray_s reads them"""
    import oracle as orc
    k = m["kind"]
    if k == "spherical":
        d = orc.spherical_directions(m["model"])
        return np.zeros_like(d), d
    if k == "pinhole":
        d = orc.pinhole_directions(m["width"], m["height"], m["f"], m["c"])
        return np.zeros_like(d), d
    d = np.asarray(m["dirs"], np.float32)
    if k == "o1dn":
        return np.tile(np.asarray(m["orig"], np.float32)[None, :], (len(d), 1)), d
    return np.asarray(m["origs"], np.float32), d


# ---- poses ------------------------------------------------------------------------------------------------------------------------
def _array(poses):
    from rmcl_amd import types as T
    return np.array(poses, dtype=T.TRANSFORM)


def spread():
    """37 poses all over the room: pitch up to +-0.5 rad, heights 0.3 .. 5.5 m, any yaw"""
    from rmcl_amd import types as T
    rng = np.random.RandomState(37)
    out = []
    for _ in range(37):
        x, y = rng.uniform(-9.0, 9.0, 2)
        out.append(T.transform_from_rpy((x, y, rng.uniform(0.3, 5.5)), (rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5), rng.uniform(-math.pi, math.pi))))
    return _array(out)


INTERIOR_A = ((1.0, -2.0, 1.2), (0.02, -0.03, 0.4))
INTERIOR_B = ((-6.5, 7.0, 2.4), (0.0, 0.1, -2.0))


def far_pose():
    from rmcl_amd import types as T
    return T.transform_from_rpy((500.0, 20.0, 3.0), (0.0, 0.0, 1.0))


def edges():
    """the nine poses of EDGE_NAMES, in that order"""
    from rmcl_amd import types as T
    nan = float("nan")
    a = T.transform_from_rpy(*INTERIOR_A)
    nan_t = T.transform_from_rpy((nan, 2.0, 1.0), (0.0, 0.0, 0.3))
    nan_q = T.transform((nan, 0.0, 0.0, 1.0), (2.0, 3.0, 1.0))
    # the SENSOR on the +x face of room30k's bounding box (to the rounding of the two compositions), looking along the wall
    import oracle as orc
    on_face = orc.tmult(T.transform_from_rpy((float(map_bbox("room30k")[1][0]), 0.0, 1.0), (0.0, 0.0, 1.5)), orc.tinv(tsb()))
    return _array([a, T.transform_from_rpy((30.0, 4.0, 1.0), (0.0, 0.0, 3.1)), T.transform_from_rpy(*INTERIOR_B), far_pose(), nan_t,
                   a.copy(), nan_q, on_face, a.copy()])


def edges_without_the_empty_ones():
    """`edges` without the far pose and the two NaN poses (EDGE_NO_HIT), and where each kept pose sits in `edges`"""
    keep = [i for i in range(len(EDGE_NAMES)) if i not in EDGE_NO_HIT]
    return edges()[keep], keep


def one_cell():
    """40 poses with NaN translations and 40 different rotations: every ray origin is NaN, every key the origin's cell 0"""
    from rmcl_amd import types as T
    nan = float("nan")
    rng = np.random.RandomState(40)
    return _array([T.transform_from_rpy((nan, nan, nan), tuple(rng.uniform(-1.0, 1.0, 3))) for _ in range(40)])


def far_poses(n):
    """n copies of a pose whose every ray misses every map here: what a batch is preceded by so that stale buffers hold misses"""
    return _array([far_pose()] * n)


def truth_and_estimates(n):
    """(truth, the first n poses of a list of nine estimates near it) of the reduction tests: the dataset is what the truth measures"""
    from rmcl_amd import types as T
    rng = np.random.RandomState(9)
    truth = T.transform_from_rpy(*INTERIOR_A)
    est = []
    for _ in range(9):
        dt, dr = rng.uniform(-0.08, 0.08, 3), rng.uniform(-0.02, 0.02, 3)
        est.append(T.transform_from_rpy((1.0 + dt[0], -2.0 + dt[1], 1.2 + dt[2]), (0.02 + dr[0], -0.03 + dr[1], 0.4 + dr[2])))
    return truth, _array(est)[:n]


def measure(mesh, m, Tbm):
    """(ranges, dataset points, mask) of one scan at Tbm: rmclhip_rcc_set_dataset_from_ranges' rule (point = origin + direction *
    range for every model but the spherical one, which has no origin; mask = range within the model's interval)"""
    sim = simulate(mesh, m, Tbm)
    r = np.asarray(sim["ranges"], np.float32)
    o, d = rays_s(m)
    with np.errstate(invalid="ignore", over="ignore"):
        pts = (d * r[:, None]).astype(np.float32) if m["kind"] == "spherical" else (d * r[:, None] + o).astype(np.float32)
    mask = ((r >= np.float32(RANGE_MIN)) & (r <= np.float32(RANGE_MAX))).astype(np.uint8)
    return r, pts, mask


# ---- the key of one order entry, restated ---------------------------------------------------------------------------------------------
def _qmul(a, b):
    """devmath.h qmul on float32 arrays [..., 4] = (x, y, z, w)"""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by - ax * bz) + ay * bw) + az * bx
    z = ((aw * bz + ax * by) - ay * bx) + az * bw
    return np.stack([x, y, z, w], axis=-1)


def _qrot(q, p):
    P = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float32)], axis=-1)
    qi = q * np.array([-1.0, -1.0, -1.0, 1.0], np.float32)
    return _qmul(_qmul(q, P), qi)[..., :3]


def _spread4(v):
    return (v & 1) | ((v & 2) << 2) | ((v & 4) << 4) | ((v & 8) << 6)


def restated_keys(m, poses, bbox, twl, group):
    """keys[pose * ngroups + g] of k_batch_tile_keys for the model `m` at the base poses `poses` (mount: tsb()), the map's bounding
    box (lo, hi), tiles 2^twl wide and `group` tiles per workgroup: float32 throughout, the kernel's order of operations.  Also returns
    ngroups."""
    import oracle as orc
    h, w = model_shape(m)
    ng = n_groups(twl, group, h, w)
    loc = np.array([cv * w + ch for cv, ch in (central_ray(twl, group, g, h, w) for g in range(ng))], np.int64)
    o_all, d_all = rays_s(m)
    o_s, d_s = o_all[loc].astype(np.float32), d_all[loc].astype(np.float32)                       # [ng, 3]
    Tsm = np.array([orc.tmult(p, tsb()) for p in np.asarray(poses).reshape(-1)], dtype=orc.TRANSFORM)
    q = np.stack([Tsm["R"][k] for k in "xyzw"], axis=-1).astype(np.float32)[:, None, :]          # [np, 1, 4]
    t = np.stack([Tsm["t"][k] for k in "xyz"], axis=-1).astype(np.float32)[:, None, :]
    lo, hi = np.asarray(bbox[0], np.float32), np.asarray(bbox[1], np.float32)
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q_b = np.broadcast_to(q, (len(Tsm), ng, 4))
        od = _qrot(q_b, np.broadcast_to(o_s[None], (len(Tsm), ng, 3))) + t                       # xapply(Tsm, orig_s)
        dd = _qrot(q_b, np.broadcast_to(d_s[None], (len(Tsm), ng, 3)))
        tt = np.full(od.shape[:2], 3.0e38, f32)
        for a in range(3):
            cand = np.fmax((np.where(dd[..., a] > 0, hi[a], lo[a]).astype(f32) - od[..., a]) / dd[..., a], f32(0.0))
            tt = np.where(dd[..., a] != 0, np.fmin(tt, cand), tt)
        tt = np.where(tt < f32(3.0e38), tt, f32(0.0)).astype(f32)
        cells = []
        for a in range(3):
            u = ((od[..., a] + tt * dd[..., a]) - lo[a]) / np.fmax(hi[a] - lo[a], f32(1e-20))
            cells.append((np.fmin(np.fmax(u, f32(0.0)), f32(1.0)) * f32(15.0)).astype(np.uint32))
    keys = _spread4(cells[0]) | (_spread4(cells[1]) << 1) | (_spread4(cells[2]) << 2)
    assert od.dtype == np.float32 and dd.dtype == np.float32 and tt.dtype == np.float32
    return keys.reshape(-1).astype(np.uint32), ng


def cells_and_runs(keys):
    """(distinct cells, runs of sixteen cells touched) of a key array"""
    k = np.unique(np.asarray(keys, np.int64))
    return len(k), len(np.unique(k >> 4))
