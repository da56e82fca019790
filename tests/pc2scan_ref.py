"""PointCloud2 -> spherical scan restated in numpy -- the yardstick of tests/test_pc2scan_cpu.py and tests/test_gpu_pc2scan.py (the
oracle has no such entry).  The rule is the per-cloud body of the reference's Pc2ToScanNode::convert
(rmcl_ros/src/nodes/conversion/pc2_to_scan.cpp:105-213; include/rmclhip.h, "Wire-format input of the SPHERICAL model"), per point i in
buffer order (i = row * width + col at row * row_step + col * point_step):

    1. x, y, z as float32 (FLOAT64 fields cast, :167-184); skipped unless all three are finite (:186)
    2. ps = T * (x, y, z) in float32 with the library's operation order (devmath.h qmul / qrot / xapply) (:188-189)
    3. range_est = sqrtf((x*x + y*y) + z*z); theta_est = (float)atan2((double)y, (double)x);
       phi_est = (float)atan2((double)z, (double)range_est) (:191-193)                       [TRUE_ELEVATION: sqrt(x*x + y*y)]
    4. id = (int)(((est - min) / inc) + 0.5): float quotient, + 0.5 in double, truncation toward zero, compared in double with
       [0, size) (:195-199); inc == 0 with size == 1: id 0                                    [FLOOR: floor; WRAP_THETA: +- one period]
    5. inside the image and range_est inside [range.min, range.max] (:201): candidate of cell phi_id * W + theta_id; the LARGEST i
       wins (:204, the sequential overwrite)                                                  [NEAREST: the smallest (range, i)]
    6. ranges[cell] = the winner's range_est, or (float)((double)range.max + 1.0) (fillEmpty, scan_operations.cpp:25-39)
    7. dataset(): points = dir(vid, hid) * range, mask = range inside the interval (MICPSphericalSensorCPU.cpp:181-233)

Every step is one IEEE operation in a pinned format, so a device result can be compared with this one bit for bit.
"""
import numpy as np

f32 = np.float32
TRUE_ELEVATION, FLOOR, WRAP_THETA, NEAREST = 1, 2, 4, 8
ALL_FLAGS = 15
FLOAT32, FLOAT64 = 7, 8
EDGE_TOL = 1e-4   # cell widths: five times the 2e-5 that one float ulp of position moves an angle in the C2 model


def model_tuple(model):
    """(phi_min, phi_inc, H, theta_min, theta_inc, W, range_min, range_max) of a SphericalModel struct"""
    return (f32(model.phi.min), f32(model.phi.inc), int(model.phi.size), f32(model.theta.min), f32(model.theta.inc),
            int(model.theta.size), f32(model.range.min), f32(model.range.max))


def xyz_from_bytes(data, width, height, point_step, row_step, offset_x, offset_y, offset_z, datatype=FLOAT32):
    """step 1: (n, 3) float32 in buffer order.  ValueError for the layouts the library answers with INVALID / UNSUPPORTED."""
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    if datatype not in (FLOAT32, FLOAT64):
        raise ValueError("Field X has unknown DataType")   # pc2_to_scan.cpp:183
    ft, size = ("<f4", 4) if datatype == FLOAT32 else ("<f8", 8)
    n = int(width) * int(height)
    out = np.empty((n, 3), f32)
    if n == 0:
        return out
    if (height - 1) * row_step + (width - 1) * point_step + max(offset_x, offset_y, offset_z) + size > buf.size:
        raise ValueError("cloud data shorter than its layout")
    row, col = np.divmod(np.arange(n, dtype=np.int64), int(width))
    base = row * int(row_step) + col * int(point_step)
    with np.errstate(over="ignore"):
        for c, off in enumerate((offset_x, offset_y, offset_z)):
            raw = buf[(base + off)[:, None] + np.arange(size)[None, :]]
            out[:, c] = np.ascontiguousarray(raw).view(ft).reshape(-1).astype(f32)
    return out


def _qmul(a, b):
    """devmath.h qmul on (x, y, z, w) tuples of float32 arrays, same association"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by - ax * bz) + ay * bw) + az * bx
    z = ((aw * bz + ax * by) - ay * bx) + az * bw
    return x, y, z, w


def apply_transform(T, xyz):
    """step 2: devmath.h xapply = qrot(R, p) + t, float32 throughout.  T: a TRANSFORM record (R.x .. R.w, t.x .. t.z) or None."""
    if T is None:
        return xyz
    T = np.asarray(T).reshape(-1)[0]
    q = tuple(f32(T["R"][k]) for k in "xyzw")
    t = tuple(f32(T["t"][k]) for k in "xyz")
    x, y, z = (xyz[:, k].astype(f32) for k in range(3))
    zero = np.zeros_like(x)
    with np.errstate(all="ignore"):
        qp = _qmul(tuple(np.broadcast_to(c, x.shape) for c in q), (x, y, z, zero))
        rx, ry, rz, _ = _qmul(qp, (-q[0], -q[1], -q[2], q[3]))
        return np.stack([rx + t[0], ry + t[1], rz + t[2]], -1).astype(f32)


def bin_points(xyz, phi_min, phi_inc, H, th_min, th_inc, W, rmin, rmax, flags=0, T=None):
    """steps 1 (the finite test) to 6 on (n, 3) points in buffer order.  -> dict(ranges (H*W,) float32, stats, cell (n,) int64 with -1
    for non-candidates, ok (n,) bool, edge_frac (n,): distance of the point's (phi, theta) bin coordinate from the nearest cell edge
    in cell widths, empty: the empty cells' value, cp / ct / pi / ti: the bin coordinates q + 0.5 and the ids of every point)."""
    if flags & ~ALL_FLAGS:
        raise ValueError("unknown flag bits")
    phi_min, phi_inc, th_min, th_inc, rmin, rmax = (f32(v) for v in (phi_min, phi_inc, th_min, th_inc, rmin, rmax))
    if (phi_inc == 0 and H != 1) or (th_inc == 0 and W != 1):
        raise ValueError("a zero increment needs size 1")
    raw = np.asarray(xyz, f32).reshape(-1, 3)
    fin = np.isfinite(raw).all(1)
    p = apply_transform(T, raw)
    x, y, z = (p[:, k] for k in range(3))
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z).astype(f32)
        th = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(f32)
        den = np.sqrt(x * x + y * y).astype(f32) if flags & TRUE_ELEVATION else r
        ph = np.arctan2(z.astype(np.float64), den.astype(np.float64)).astype(f32)
        cp = ((ph - phi_min) / phi_inc).astype(f32).astype(np.float64) + 0.5 if phi_inc != 0 else np.full(len(r), 0.5)
        ct = ((th - th_min) / th_inc).astype(f32).astype(np.float64) + 0.5 if th_inc != 0 else np.full(len(r), 0.5)
        rnd = np.floor if flags & FLOOR else np.trunc
        pi, ti = rnd(cp), rnd(ct)
        if flags & WRAP_THETA and th_inc != 0:
            P = 2 * np.pi / float(th_inc)
            if abs(P - round(P)) < 1e-3:
                P = float(round(P))
                ti = np.where(ti >= W, ti - P, np.where(ti < 0, ti + P, ti))
        inimg = fin & (pi >= 0) & (pi < H) & (ti >= 0) & (ti < W)     # NaN fails every comparison
        ok = inimg & (r >= rmin) & (r <= rmax)
    empty = f32(np.float64(rmax) + 1.0)
    ranges = np.full(H * W, empty, f32)
    cell = np.full(len(r), -1, np.int64)
    cell[ok] = (pi[ok] * W + ti[ok]).astype(np.int64)
    idx = np.nonzero(ok)[0]
    if flags & NEAREST:
        idx = idx[np.lexsort((-idx, -r[idx].astype(np.float64)))]   # farthest first, ties: larger i first -> the smallest (r, i) is written last
    ranges[cell[idx]] = r[idx]                                      # repeated indices: the last assignment wins
    with np.errstate(all="ignore"):
        edge = np.minimum(np.abs(cp - np.round(cp)), np.abs(ct - np.round(ct)))   # distance to the nearest cell edge, in cell widths
    stats = dict(n_points=len(r), n_finite=int(fin.sum()), n_in_image=int(inimg.sum()), n_in_range=int(ok.sum()),
                 n_cells_filled=int(len(np.unique(cell[idx]))))
    return dict(ranges=ranges, stats=stats, cell=cell, ok=ok, inimg=inimg, fin=fin, edge_frac=edge, empty=empty, pi=pi, ti=ti, cp=cp, ct=ct)


def convert(data, width, height, point_step, row_step, offset_x, offset_y, offset_z, model, datatype=FLOAT32, T=None, flags=0):
    """the whole node body on PointCloud2 bytes; model: a SphericalModel struct or the tuple of model_tuple()"""
    m = model if isinstance(model, tuple) else model_tuple(model)
    xyz = xyz_from_bytes(data, width, height, point_step, row_step, offset_x, offset_y, offset_z, datatype)
    return bin_points(xyz, *m, flags=flags, T=T)


def model_dirs(phi_min, phi_inc, H, th_min, th_inc, W, jitter=0.0, rng=None):
    """dir(vid, hid) of the spherical model (float32 trig of float32 angles), optionally moved by up to +-jitter cells in angle"""
    vid, hid = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    jv = rng.uniform(-jitter, jitter, vid.shape) if jitter else 0.0
    jh = rng.uniform(-jitter, jitter, vid.shape) if jitter else 0.0
    ph = (f32(phi_min) + (vid + jv).astype(f32) * f32(phi_inc)).astype(f32)
    th = (f32(th_min) + (hid + jh).astype(f32) * f32(th_inc)).astype(f32)
    cp, sp, ct, st = (fn(a).astype(f32) for fn, a in ((np.cos, ph), (np.sin, ph), (np.cos, th), (np.sin, th)))
    return np.stack([cp * ct, cp * st, sp], -1).astype(f32).reshape(-1, 3)


def dataset(ranges, model):
    """step 7: (points (H*W, 3) float32, mask uint8) of a range image, as k_dataset_from_ranges makes them for the spherical model"""
    m = model if isinstance(model, tuple) else model_tuple(model)
    d = model_dirs(*m[:6])
    r = np.asarray(ranges, f32).reshape(-1)
    return (d * r[:, None]).astype(f32), (~((r < m[6]) | (r > m[7]))).astype(np.uint8)


def edge_cells(res, W, H, tol=EDGE_TOL):
    """the cells left out of a comparison whose transform arithmetic may differ in the last bit: by the restatement, a finite point
    within `tol` cell widths of a cell edge falls into the cell or into the cell across that edge (four cells at a corner).  The
    bin coordinate c = q + 0.5 has its cell edges at the whole numbers: the edge near c is round(c), the cells on its two sides are
    round(c) - 1 and round(c); theta ids are taken modulo W (WRAP_THETA may join the two ends).  -> (bool (H*W,), number of such points)"""
    cp, ct = res["cp"], res["ct"]
    with np.errstate(all="ignore"):
        ep, et = np.round(cp), np.round(ct)
        near_p, near_t = np.abs(cp - ep) < tol, np.abs(ct - et) < tol
        sane = res["fin"] & (np.abs(cp) < 1e9) & (np.abs(ct) < 1e9)
    near = sane & (near_p | near_t)
    out = np.zeros(H * W, bool)
    idx = np.nonzero(near)[0]
    for dv in (-1, 0):
        for dh in (-1, 0):
            # the axis that is near an edge contributes both sides of it, the other one the point's own id
            v = np.where(near_p[idx], ep[idx] + dv, res["pi"][idx]).astype(np.int64)
            h = np.where(near_t[idx], et[idx] + dh, res["ti"][idx]).astype(np.int64) % W
            keep = (v >= 0) & (v < H)
            out[v[keep] * W + h[keep]] = True
    return out, len(idx)


def make_cloud(rec, xyz, height=1, row_pad=0, seed=0):
    """PointCloud2 bytes of `xyz` (n, 3) in a structured record `rec` with fields x, y, z (other fields get noise), as `height` rows of
    n / height points with `row_pad` bytes of padding behind each row.  -> (bytes, layout kwargs)"""
    n = len(xyz)
    assert n % height == 0
    width = n // height
    a = np.zeros(n, rec)
    rng = np.random.RandomState(seed)
    for name in rec.names:
        if name in "xyz":
            a[name] = xyz[:, "xyz".index(name)]
        else:
            a[name] = rng.randint(0, 200, n)
    rows = a.view(np.uint8).reshape(height, width * rec.itemsize)
    if row_pad:
        rows = np.concatenate([rows, rng.randint(0, 256, (height, row_pad)).astype(np.uint8)], 1)
    ft = rec.fields["x"][0]
    lay = dict(width=width, height=height, point_step=rec.itemsize, row_step=width * rec.itemsize + row_pad,
               offset_x=rec.fields["x"][1], offset_y=rec.fields["y"][1], offset_z=rec.fields["z"][1],
               datatype=FLOAT32 if ft == np.dtype("<f4") else FLOAT64)
    return np.ascontiguousarray(rows).tobytes(), lay


def random_cloud(n=400000, seed=5):
    """the unorganised test cloud: n points around the sensor (many per cell of the C2 model), NaN and inf sprinkled in"""
    rng = np.random.RandomState(seed)
    p = np.c_[rng.uniform(-12, 12, n), rng.uniform(-12, 12, n), rng.uniform(-4, 4, n)].astype(f32)
    k = max(1, n // 800)
    p[rng.randint(0, n, k), rng.randint(0, 3, k)] = np.nan
    p[rng.randint(0, n, max(1, k // 10)), 0] = np.inf
    p[rng.randint(0, n, max(1, k // 10)), 2] = -np.inf
    return p
