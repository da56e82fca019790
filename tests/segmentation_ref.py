"""The map segmentation's decision rule restated in numpy / float64 -- the yardstick of tests/test_segmentation_cpu.py and
tests/test_gpu_segmentation.py (the oracle has no segmentation entry; it supplies the simulated ranges and normals this is fed with).

The rule is the per-scan body of the reference's ScanMapSegmentationEmbreeNode / O1DnMapSegmentationEmbreeNode (include/rmclhip.h,
"map segmentation"): for ray bid = vid * W + hid, inside(r) = range.min <= r <= range.max (NaN is outside),

    both inside:  pint_s = dir * r_sim  (no origin unless pint_with_origin), n = normalize(normal_sim), preal_s = dir * r_real + orig,
                  plane_distance = |(preal_s - pint_s) . n|
                  r_real <  r_sim: plane_distance > min_dist_outlier_scan -> outlier_scan gets preal_s, else inlier
                  r_real >= r_sim: plane_distance > min_dist_outlier_map  -> outlier_map  gets pint_s,  else inlier
    real only:    outlier_scan gets preal_s
    sim only:     outlier_map gets dir * r_sim + orig
    neither:      nothing

Labels: 0 none, 1 inlier, 2 outlier_scan, 3 outlier_map; the clouds are in buffer order.  segment_f32 is the same rule in the kernels'
own float32 operations and order, for tests/test_gpu_segmentation_exact.py, which compares bits.  Also here: the two test scenes of the GPU
tests (meshes, poses, the doctored "real" scans), built from rmcl_amd.synthetic and the oracle alone.
"""
import numpy as np

NONE, INLIER, OUTLIER_SCAN, OUTLIER_MAP = 0, 1, 2, 3
UNDECIDED_REL = 3e-5   # three times the project's 1e-5 bar on simulated ranges


def segment(r_real, r_sim, normals_sim, dirs, origs, range_min, range_max, min_dist_outlier_scan=0.15, min_dist_outlier_map=0.15,
            pint_with_origin=False):
    """-> dict(labels uint8 (n,), outlier_scan (k, 3) float64, outlier_map (m, 3) float64, preal (n, 3), pint_sim_only (n, 3)).
    Inputs are taken as they are (float32 arrays are widened exactly); thresholds and range bounds are rounded to float32 first, the
    way the reference stores them."""
    r_real = np.asarray(r_real, np.float64).reshape(-1)
    r_sim = np.asarray(r_sim, np.float64).reshape(-1)
    n = len(r_real)
    dirs = np.asarray(dirs, np.float64).reshape(n, 3)
    origs = np.broadcast_to(np.asarray(origs, np.float64).reshape(-1, 3), (n, 3))
    nrm = np.asarray(normals_sim, np.float64).reshape(n, 3)
    lo, hi = float(np.float32(range_min)), float(np.float32(range_max))
    thr_scan, thr_map = float(np.float32(min_dist_outlier_scan)), float(np.float32(min_dist_outlier_map))
    with np.errstate(invalid="ignore", divide="ignore"):
        real_ok = (lo <= r_real) & (r_real <= hi)
        sim_ok = (lo <= r_sim) & (r_sim <= hi)
        preal = dirs * r_real[:, None] + origs
        pint_no = dirs * r_sim[:, None]
        pint_o = pint_no + origs
        pint_both = pint_o if pint_with_origin else pint_no
        unit = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]
        plane = np.abs(((preal - pint_both) * unit).sum(axis=1))
        both = real_ok & sim_ok
        front = r_real < r_sim
        labels = np.zeros(n, np.uint8)
        labels[both] = INLIER
        labels[both & front & (plane > thr_scan)] = OUTLIER_SCAN
        labels[both & ~front & (plane > thr_map)] = OUTLIER_MAP
        labels[real_ok & ~sim_ok] = OUTLIER_SCAN
        labels[~real_ok & sim_ok] = OUTLIER_MAP
    map_pts = np.where(real_ok[:, None], pint_both, pint_o)
    return dict(labels=labels, outlier_scan=preal[labels == OUTLIER_SCAN], outlier_map=map_pts[labels == OUTLIER_MAP],
                preal=preal, map_points=map_pts)


def pinhole_dirs_f32(width, height, fx, fy, cx, cy):
    """segment.hip seg_pinhole_direction in float32 numpy, buffer order (vid * width + hid)"""
    f = np.float32
    vid, hid = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    pX = ((hid - f(cx)) / f(fx)).astype(np.float32)
    pY = ((vid - f(cy)) / f(fy)).astype(np.float32)
    d = np.sqrt((pX * pX + pY * pY) + f(1.0) * f(1.0)).astype(np.float32)
    return np.stack([f(1.0) / d, -(pX / d), -(pY / d)], -1).astype(np.float32).reshape(-1, 3)


def segment_f32(r_real, r_sim, normals_sim, dirs, origs, range_min, range_max, min_dist_outlier_scan=0.15, min_dist_outlier_map=0.15,
                pint_with_origin=False, add_origin=False):
    """segment.hip's k_segment_classify and the two cloud points of k_segment_scatter in float32, one IEEE operation per step in the
    kernel's order (devmath.h: scale3 = (a.x * s, a.y * s, a.z * s), add3 / sub3 componentwise, dot_plain = (a.x * b.x + a.y * b.y) +
    a.z * b.z; the library is built with -ffp-contract=off, float divide and sqrt are correctly rounded).  add_origin: the model is O1Dn
    or OnDn -- seg_point adds an origin for these two only.  -> dict(labels uint8, outlier_scan, outlier_map (k, 3) float32 in buffer
    order, plane (n,) float32: plane_distance where both ranges are inside the interval, NaN elsewhere)."""
    f = np.float32
    r_real = np.asarray(r_real, f).reshape(-1)
    r_sim = np.asarray(r_sim, f).reshape(-1)
    n = len(r_real)
    d = np.asarray(dirs, f).reshape(n, 3)
    o = np.broadcast_to(np.asarray(origs, f).reshape(-1, 3), (n, 3))
    nr = np.asarray(normals_sim, f).reshape(n, 3)
    lo, hi, thr_scan, thr_map = f(range_min), f(range_max), f(min_dist_outlier_scan), f(min_dist_outlier_map)

    def point(r, with_origin):
        pt = (d * r[:, None]).astype(f)                                  # scale3(dir, r)
        return (pt + o).astype(f) if (with_origin and add_origin) else pt

    with np.errstate(all="ignore"):
        real_ok = (lo <= r_real) & (r_real <= hi)
        sim_ok = (lo <= r_sim) & (r_sim <= hi)
        preal = point(r_real, True)
        pint = point(r_sim, bool(pint_with_origin))
        nn = ((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]).astype(f) + nr[:, 2] * nr[:, 2]).astype(f)
        inv = (f(1.0) / np.sqrt(nn).astype(f)).astype(f)
        unit = (nr * inv[:, None]).astype(f)
        df = (preal - pint).astype(f)
        plane = np.abs(((df[:, 0] * unit[:, 0] + df[:, 1] * unit[:, 1]).astype(f) + df[:, 2] * unit[:, 2]).astype(f))
        both = real_ok & sim_ok
        front = r_real < r_sim
        labels = np.zeros(n, np.uint8)
        labels[both] = INLIER
        labels[both & front & (plane > thr_scan)] = OUTLIER_SCAN
        labels[both & ~front & (plane > thr_map)] = OUTLIER_MAP
        labels[real_ok & ~sim_ok] = OUTLIER_SCAN
        labels[~real_ok & sim_ok] = OUTLIER_MAP
        # k_segment_scatter: preal_s for a scan outlier; for a map outlier dir * r_sim, with the origin if the measured range is invalid
        map_pts = np.where(real_ok[:, None], pint, point(r_sim, True))
    return dict(labels=labels, outlier_scan=preal[labels == OUTLIER_SCAN], outlier_map=map_pts[labels == OUTLIER_MAP],
                plane=np.where(both, plane, f(np.nan)).astype(f))


def undecided(r_real, r_sim, normals_sim, dirs, origs, range_min, range_max, **kw):
    """rays whose label changes when r_sim, or r_real, is scaled by 1 +- UNDECIDED_REL: simulated ranges agree with the oracle to 1e-5
    relative only, so these may fall either way"""
    r_real = np.asarray(r_real, np.float64).reshape(-1)
    r_sim = np.asarray(r_sim, np.float64).reshape(-1)
    base = segment(r_real, r_sim, normals_sim, dirs, origs, range_min, range_max, **kw)["labels"]
    und = np.zeros(len(base), bool)
    for s in (1.0 - UNDECIDED_REL, 1.0 + UNDECIDED_REL):
        und |= segment(r_real, r_sim * s, normals_sim, dirs, origs, range_min, range_max, **kw)["labels"] != base
        und |= segment(r_real * s, r_sim, normals_sim, dirs, origs, range_min, range_max, **kw)["labels"] != base
    return und


def doctor_cube_scan(ranges_32x32):
    """the "real" scan of tests/test_cpp_adapters.py::test_simulator_example_matches_oracle: an obstacle (a block of beams 40 % shorter),
    a hole in the map (a block 1.5 m longer), two rows of invalid returns, four beams beyond the range"""
    real = np.array(ranges_32x32, np.float32).reshape(32, 32)
    real[4:9, 3:12] *= np.float32(0.6)
    real[20:24, 16:25] += np.float32(1.5)
    real[12:14, :] = np.float32(0.0)
    real[30, 5:9] = np.float32(150.0)
    return real.reshape(-1)


# ---- scenes of the GPU tests ----------------------------------------------------------------------------------------------------------
def box_mesh(centre, size):
    """12 triangles of an axis-aligned box"""
    c, h = np.asarray(centre, np.float64), np.asarray(size, np.float64) / 2
    v = np.array([[c[0] + sx * h[0], c[1] + sy * h[1], c[2] + sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.uint32)
    return v, f


def with_box(v, f, centre, size):
    bv, bf = box_mesh(centre, size)
    return np.concatenate([np.asarray(v, np.float32), bv]), np.concatenate([np.asarray(f, np.uint32), bf + np.uint32(len(v))])


def small_perturbation(T):
    """the estimate's offset from the truth pose in both scenes: 6 / 3 / 2 cm, 0.6 degrees of yaw"""
    return T.transform_from_rpy((0.06, 0.03, 0.02), (0.0, 0.0, np.deg2rad(0.6)))


def cube_scene(syn, T):
    """-> (map mesh, reality mesh, model, Tsb, truth, est): the 972-triangle cube room, a box only the map has, a box only reality has"""
    v, f = syn.cube_room()
    map_mesh = with_box(v, f, (2.5, 1.0, -1.0), (0.8, 0.8, 3.0))
    real_mesh = with_box(v, f, (-2.0, 2.0, 0.0), (1.0, 1.0, 2.0))
    truth = syn.pose_c2_truth()
    return map_mesh, real_mesh, syn.model_c1(), T.identity(), truth, T.mult(truth, small_perturbation(T))


def room_model(syn):
    """C2's 128 x 1024 grid with range [0.3, 12]: the far walls of the 20 m room are simulated misses"""
    m = syn.model_c2()
    m.range.min, m.range.max = np.float32(0.3), np.float32(12.0)
    return m


def room_scene(syn, T):
    v, f = syn.noisy_room(30000)
    map_mesh = with_box(v, f, (4.0, 3.0, 1.0), (0.8, 0.8, 2.0))
    real_mesh = with_box(v, f, (-3.0, 2.0, 0.6), (1.0, 0.6, 1.2))
    truth = T.transform_from_rpy((0.52, -0.30, 1.0), (0.02, -0.03, 0.4))
    return map_mesh, real_mesh, room_model(syn), syn.tsb_offset(), truth, T.mult(truth, small_perturbation(T))


def invalidate_some(real, range_max, fraction=0.02, seed=7):
    """`fraction` of the rays set to 0.0 or range.max + 1, alternating"""
    real = np.array(real, np.float32)
    rs = np.random.RandomState(seed)
    idx = rs.choice(len(real), int(round(fraction * len(real))), replace=False)
    real[idx[0::2]] = np.float32(0.0)
    real[idx[1::2]] = np.float32(range_max) + np.float32(1.0)
    return real
