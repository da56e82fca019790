"""Host restatement of the motion-compensated PointCloud2 input (include/rmclhip.h, MOTION-COMPENSATED INPUT; rmcl_amd/csrc/deskew.hip,
deskew_pose.h) in numpy float32 / float64, operation for operation, so the device's bytes can be compared with `==`.

The rules, restated:
  motion     K knots, 2 <= K <= 64; times[k] doubles, strictly increasing; knots[k] = T_sref_s(t_k), the sensor frame at t_k in the
             sensor frame at the reference time (the knot at that time is the identity)
  time       t = offset_s + scale * raw in double; raw = the point's time field, UINT32 (6) / FLOAT32 (7) / FLOAT64 (8)
  pose       k = the largest index with times[k] <= t, limited to [0, K - 2]
             s = float32((t - times[k]) / (times[k+1] - times[k])), quotient in double; s < 0 or s > 1: clamped, counted
             a = 1 - s;  q' = -q_{k+1} if ((x x' + y y') + z z') + w w' < 0;  q = a q_k + s q' per component, each divided by
             sqrt(((x x + y y) + z z) + w w);  tr = a t_k + s t_{k+1}           -- float32, one IEEE operation per step (nlerp)
             a non-finite t: knots[0], counted in n_time_nonfinite (not clamped), mask 0
  outputs    x, y, z as float32 (FLOAT64 cast); one non-finite: range 0, dir_local 0; else range = sqrt((x x + y y) + z z),
             dir_local = p / range;  orig = tr;  dir = q (dir_local, 0) q^-1 with devmath.h's Hamilton product;
             point = dir * range + orig;  mask = range in [range_min, range_max] and t finite
  cloud form point where mask, else NaN

slerp64_pose() is an INDEPENDENT float64 implementation (true slerp + lerp of two poses) the restatement is tested against.
"""
import numpy as np

F = np.float32
UINT32, FLOAT32, FLOAT64 = 6, 7, 8
_TIME_DTYPE = {UINT32: "<u4", FLOAT32: "<f4", FLOAT64: "<f8"}


# ---- cloud bytes --------------------------------------------------------------------------------------------------------------------
def gather_field(buf, rows, cols, row_step, point_step, offset, dtype):
    """field at `offset` of the records (row, col) for row in rows, col in cols: [len(rows) * len(cols)] values, any alignment"""
    buf = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
    size = np.dtype(dtype).itemsize
    base = (np.asarray(rows, np.int64)[:, None] * row_step + np.asarray(cols, np.int64)[None, :] * point_step + offset).reshape(-1)
    idx = base[:, None] + np.arange(size)[None, :]
    return np.ascontiguousarray(buf[idx]).view(dtype).reshape(-1)


def filtered(size, flt):
    """source indices the filter (skip_begin, skip_end, increment) keeps (scan_operations.cpp:41-52)"""
    sb, se, inc = flt if flt is not None else (0, 0, 1)
    return np.arange((size - sb - se) // inc) * inc + sb


def make_cloud(xyz, raw_time, time_dtype=FLOAT32, xyz_dtype=FLOAT32, point_step=None, row_pad=0, width=None, lead=0, gap=0):
    """bytes of a cloud with the fields [lead bytes] x y z [gap bytes] time (point_step >= that; row_pad extra bytes per row; lead 0,
    gap 6, FLOAT32: the 22-byte x y z intensity ring time record of a Velodyne driver, time at 18).
    Returns (uint8 array, layout dict, (time offset, time datatype))."""
    xyz = np.asarray(xyz)
    n = len(xyz)
    width = n if width is None else width
    height = n // width
    assert width * height == n
    ft = "<f4" if xyz_dtype == FLOAT32 else "<f8"
    fs = np.dtype(ft).itemsize
    tt = _TIME_DTYPE[time_dtype]
    toff = lead + 3 * fs + gap
    need = toff + np.dtype(tt).itemsize
    point_step = need if point_step is None else point_step
    assert point_step >= need
    row_step = width * point_step + row_pad
    buf = np.full(height * row_step, 0xA5, np.uint8)
    recs = np.zeros((n, point_step), np.uint8) + np.uint8(0x5A)
    for c in range(3):
        recs[:, lead + c * fs:lead + (c + 1) * fs] = np.ascontiguousarray(xyz[:, c].astype(ft)).view(np.uint8).reshape(n, fs)
    ts = np.dtype(tt).itemsize
    recs[:, toff:toff + ts] = np.ascontiguousarray(np.asarray(raw_time).astype(tt)).view(np.uint8).reshape(n, ts)
    for r in range(height):
        buf[r * row_step:r * row_step + width * point_step] = recs[r * width:(r + 1) * width].reshape(-1)
    layout = dict(width=width, height=height, point_step=point_step, row_step=row_step, offset_x=lead, offset_y=lead + fs,
                  offset_z=lead + 2 * fs, datatype=xyz_dtype)
    return buf, layout, (toff, time_dtype)


# ---- devmath.h, float32, vectorised ---------------------------------------------------------------------------------------------------
def qmul(a, b):
    """Hamilton product, devmath.h qmul; a, b: (x, y, z, w) tuples of float32 arrays"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by - ax * bz) + ay * bw) + az * bx
    z = ((aw * bz + ax * by) - ay * bx) + az * bw
    return x, y, z, w


def qrot(q, p):
    """devmath.h qrot: q (p, 0) q^-1"""
    zero = np.zeros_like(p[0])
    qi = (-q[0], -q[1], -q[2], q[3])
    r = qmul(qmul(q, (p[0], p[1], p[2], zero)), qi)
    return r[0], r[1], r[2]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def point_times(raw, time_dtype, scale=1.0, offset_s=0.0):
    return np.float64(offset_s) + np.float64(scale) * raw.astype(np.float64)


def poses(t, knot_q, knot_t, knot_times):
    """per-point pose (q [n, 4], tr [n, 3] float32) and the flags (clamped, nonfinite) of the times t (float64 [n])"""
    knot_q = np.asarray(knot_q, F).reshape(-1, 4)
    knot_t = np.asarray(knot_t, F).reshape(-1, 3)
    times = np.asarray(knot_times, np.float64)
    K = len(times)
    assert 2 <= K <= 64 and len(knot_q) == K and len(knot_t) == K
    bad = ~np.isfinite(t)
    tt = np.where(bad, times[0], t)
    k = np.clip(np.searchsorted(times, tt, side="right") - 1, 0, K - 2)
    with np.errstate(over="ignore", invalid="ignore"):
        s = ((tt - times[k]) / (times[k + 1] - times[k])).astype(F)
    s = np.where(bad, F(0), s)
    clamped = ((s < 0) | (s > 1)) & ~bad
    s = np.where(s < 0, F(0), np.where(s > 1, F(1), s)).astype(F)
    a = F(1) - s
    q0, q1 = knot_q[k], knot_q[k + 1]
    d = ((q0[:, 0] * q1[:, 0] + q0[:, 1] * q1[:, 1]) + q0[:, 2] * q1[:, 2]) + q0[:, 3] * q1[:, 3]
    q1 = np.where((d < 0)[:, None], -q1, q1)
    q = a[:, None] * q0 + s[:, None] * q1
    nrm = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    q = q / nrm[:, None]
    tr = a[:, None] * knot_t[k] + s[:, None] * knot_t[k + 1]
    assert q.dtype == F and tr.dtype == F
    return q, tr, clamped, bad


def deskew(buf, layout, time_field, knot_q, knot_t, knot_times, range_min=0.0, range_max=1e30, filter_height=None, filter_width=None):
    """the operator form's arrays: origs, dirs, points [n, 3] float32, mask [n] uint8, stats, and the per-point pose (q, tr); `cloud`
    is the cloud form (points, NaN where mask is 0).  time_field: (offset, datatype[, scale[, offset_s]])."""
    rows, cols = filtered(layout["height"], filter_height), filtered(layout["width"], filter_width)
    ft = "<f4" if layout["datatype"] == FLOAT32 else "<f8"
    g = lambda off, dt: gather_field(buf, rows, cols, layout["row_step"], layout["point_step"], off, dt)
    with np.errstate(over="ignore", invalid="ignore"):
        x, y, z = (g(layout[k], ft).astype(F) for k in ("offset_x", "offset_y", "offset_z"))
    toff, tdt = time_field[0], time_field[1]
    scale = time_field[2] if len(time_field) > 2 else 1.0
    offset_s = time_field[3] if len(time_field) > 3 else 0.0
    t = point_times(g(toff, _TIME_DTYPE[tdt]), tdt, scale, offset_s)
    n = len(x)
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rng = np.sqrt((x * x + y * y) + z * z)
        rng = np.where(fin, rng, F(0)).astype(F)
        dl = [np.where(fin, c / rng, F(0)).astype(F) for c in (x, y, z)]
    q, tr, clamped, bad = poses(t, knot_q, knot_t, knot_times)
    dx, dy, dz = qrot((q[:, 0], q[:, 1], q[:, 2], q[:, 3]), dl)
    dirs = np.stack([dx, dy, dz], axis=1).astype(F)
    points = (dirs * rng[:, None] + tr).astype(F)
    mask = (~((rng < F(range_min)) | (rng > F(range_max))) & ~bad).astype(np.uint8)
    cloud = np.where(mask[:, None] != 0, points, F(np.nan)).astype(F)
    stats = dict(n_points=n, n_finite=int(fin.sum()), n_valid=int(mask.sum()), n_time_clamped=int(clamped.sum()),
                 n_time_nonfinite=int(bad.sum()))
    return dict(origs=tr.astype(F), dirs=dirs, points=points, mask=mask, cloud=cloud, stats=stats, q=q, tr=tr, ranges=rng,
                width=len(cols), height=len(rows), t=t)


# ---- an independent float64 implementation --------------------------------------------------------------------------------------------
def _qmul64(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def rot64(q, p):
    """rotation matrix of the unit quaternion (x, y, z, w) applied to p, float64"""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(p, np.float64)


def slerp64_pose(q0, t0, q1, t1, u):
    """true slerp on the shorter arc + lerp, float64"""
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    q0, q1 = q0 / np.linalg.norm(q0), q1 / np.linalg.norm(q1)
    d = float(q0 @ q1)
    if d < 0:
        q1, d = -q1, -d
    om = np.arccos(min(1.0, d))
    if om < 1e-12:
        q = (1 - u) * q0 + u * q1
    else:
        q = (np.sin((1 - u) * om) * q0 + np.sin(u * om) * q1) / np.sin(om)
    return q / np.linalg.norm(q), (1 - u) * np.asarray(t0, np.float64) + u * np.asarray(t1, np.float64)


def pose_mul64(qa, ta, qb, tb):
    return _qmul64(qa, qb), rot64(qa, tb) + np.asarray(ta, np.float64)


def pose_inv64(q, t):
    qi = np.array([-q[0], -q[1], -q[2], q[3]])
    return qi, -rot64(qi, t)


def yaw_pose64(yaw, t):
    return np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]), np.asarray(t, np.float64)


def motion_knots64(S0, S1, times01, t_ref, subdivide, Tsb=None):
    """knots of the motion between two sensor-carrier poses S0 at times01[0] and S1 at times01[1] ((q, t) float64 pairs), by true
    slerp in float64: T_sref_s(t_k) = ~Tsb ~S(t_ref) S(t_k) Tsb at subdivide + 1 evenly spaced times.  Returns (q [K, 4] float32,
    t [K, 3] float32, times [K] float64) -- what rmclhip_scan_motion_from_base_poses_host computes for two poses."""
    t0, t1 = times01
    sb = Tsb if Tsb is not None else (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    ref = slerp64_pose(S0[0], S0[1], S1[0], S1[1], (t_ref - t0) / (t1 - t0))
    left = pose_mul64(*pose_inv64(*sb), *pose_inv64(*ref))
    qs, ts, tk = [], [], []
    for m in range(subdivide + 1):
        u = m / subdivide
        P = slerp64_pose(S0[0], S0[1], S1[0], S1[1], u)
        k = pose_mul64(*pose_mul64(*left, *P), *sb)
        qs.append(k[0] / np.linalg.norm(k[0]))
        ts.append(k[1])
        tk.append(t0 + u * (t1 - t0) if m else t0)
    return np.array(qs).astype(F), np.array(ts).astype(F), np.array(tk, np.float64)


# ---- the premise: what a moving sensor does to MICP, and what casting every ray from its own pose restores ----------------------------
PREMISE_START = dict(t=(0.1, 0.1, 0.0), yaw=0.05)   # offset of the first estimate from the truth
PREMISE_ITERATIONS = 40


def premise_scene(mesh, H=8, W=64):
    """Cube room, a full-circle H x W spherical scanner that moves 0.4 m and turns 0.15 rad during the scan (column time
    hid / (W - 1), reference time = the end of the scan).  `mesh`: an oracle Mesh of synthetic.cube_room().  Returns a dict: the
    truth pose (sensor in map at the reference time, TRANSFORM), the local directions, the cloud bytes a driver would publish (x y z
    FLOAT32 + time FLOAT32, points in the sensor's own frame at their own time), its layout, the knots, and the restatement of the
    compensated input."""
    import oracle as orc
    from rmcl_amd import synthetic as syn
    model = orc.spherical_model(F(-0.3), F(0.6 / (H - 1)), H, F(-np.pi), F(2 * np.pi / W), W, F(0.1), F(100.0))
    d_local = syn.model_directions(model)
    S1 = yaw_pose64(0.4, (0.5, -0.3, 0.2))                       # truth at the reference time
    D = yaw_pose64(0.15, (0.4, 0.0, 0.0))                        # the motion during the scan, in the frame of the start
    S0 = pose_mul64(*S1, *pose_inv64(*D))
    kq, kt, ktimes = motion_knots64(S0, S1, (0.0, 1.0), 1.0, 16)
    col_time = (np.arange(W, dtype=np.float32) / F(W - 1)).astype(F)
    raw_t = np.tile(col_time, H)
    q, tr, _, _ = poses(raw_t.astype(np.float64), kq, kt, ktimes)
    dx, dy, dz = qrot((q[:, 0], q[:, 1], q[:, 2], q[:, 3]), (d_local[:, 0], d_local[:, 1], d_local[:, 2]))
    dirs = np.stack([dx, dy, dz], axis=1).astype(F)
    truth = orc.transform(tuple(S1[0]), tuple(S1[1]))
    ident = orc.transform()
    sim = mesh.simulate_ondn(W, H, 0.1, 100.0, tr, dirs, ident, truth, bvh=False)
    assert sim["hits"].all(), "a closed room: every ray hits"
    xyz = (d_local * sim["ranges"][:, None]).astype(F)
    buf, layout, time_field = make_cloud(xyz, raw_t, FLOAT32, FLOAT32, width=W)
    comp = deskew(buf, layout, time_field, kq, kt, ktimes, 0.1, 100.0)
    return dict(truth=truth, d_local=d_local, cloud=buf, layout=layout, time_field=time_field, knots=(kq, kt, ktimes), comp=comp,
                xyz=xyz, W=W, H=H, range=(0.1, 100.0))


def premise_start(truth):
    import oracle as orc
    off = orc.transform((0.0, 0.0, np.sin(PREMISE_START["yaw"] / 2), np.cos(PREMISE_START["yaw"] / 2)), PREMISE_START["t"])
    return orc.tmult(truth, off)


def pose_error(T, truth):
    """(position error in metres, rotation error in radians) of two TRANSFORMs"""
    dt = np.array([float(T["t"][k]) - float(truth["t"][k]) for k in "xyz"])
    qa = np.array([float(T["R"][k]) for k in "xyzw"])
    qb = np.array([float(truth["R"][k]) for k in "xyzw"])
    d = min(1.0, abs(float(qa @ qb) / (np.linalg.norm(qa) * np.linalg.norm(qb))))
    return float(np.linalg.norm(dt)), float(2 * np.arccos(d))
