"""The refinement on the distance field (include/rmclhip.h, REFINE ON THE FIELD) restated in numpy: every operation in the header's
precision and order, vectorised over particles and beams (element-wise numpy arithmetic rounds every operation to the array's type,
which is the header's "unfused").  The transform arithmetic is devmath.h's (Hamilton product, q p q^-1 with the full products), which
the device holds bit-exact to the oracle's.  Not a test module.
"""
import numpy as np

F = np.float32
D = np.float64
FLT_MAX = F(3.4028234663852886e38)
MAX_BEAMS = 8192
MAX_ITERATIONS = 64
RESULT = np.dtype([("cost_before", np.float32), ("cost_after", np.float32), ("n_used", np.uint32), ("accepted", np.uint32)])
TRI = [(a, c) for a in range(6) for c in range(a, 6)]       # the upper triangle of A, row by row: 21 entries

# every parameter refusal: what rmclhip_field_refine answers with RMCLHIP_ERR_INVALID and check() with ValueError
BAD_PARAMS = [dict(iterations=65), dict(dof_mask=0x40)] + [{k: bad} for k in ("max_dist", "max_step_trans", "max_step_rot", "lambda0")
                                                           for bad in (0.0, -1.0, float("nan"), float("inf"))]


def params(iterations=8, dof_mask=0x3F, max_dist=0.5, max_step_trans=0.5, max_step_rot=0.25, lambda0=1e-3):
    """rmclhip_refine_params with the defaults of rmclhip_refine_params_default"""
    return dict(iterations=int(iterations), dof_mask=int(dof_mask), max_dist=F(max_dist), max_step_trans=F(max_step_trans),
                max_step_rot=F(max_step_rot), lambda0=F(lambda0))


def check(p, n_particles, n_beams):
    """the refusals of rmclhip_field_refine that do not concern pointers: ValueError where the library returns RMCLHIP_ERR_INVALID"""
    if not 0 <= p["iterations"] <= MAX_ITERATIONS:
        raise ValueError("iterations")
    if not 0 <= p["dof_mask"] <= 0x3F:
        raise ValueError("dof_mask")
    for k in ("max_dist", "max_step_trans", "max_step_rot", "lambda0"):
        if not (np.isfinite(p[k]) and p[k] > 0):
            raise ValueError(k)
    if n_particles > 0 and not 1 <= n_beams <= MAX_BEAMS:
        raise ValueError("n_beams")


# ---- devmath.h: quaternions are [..., 4] = (x, y, z, w), float32 ----------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by - ax * bz) + ay * bw) + az * bx
    z = ((aw * bz + ax * by) - ay * bx) + az * bw
    return np.stack([x, y, z, w], -1).astype(F)


def qrot(q, p):
    P = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), F)], -1)
    qi = q * np.array([-1, -1, -1, 1], F)
    return qmul(qmul(q, P), qi)[..., :3]


def qnormalise(q):
    nrm = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    return (q / nrm[..., None]).astype(F)


def pose_arrays(poses):
    """TRANSFORM records -> (R [n, 4], t [n, 3]) float32"""
    poses = np.asarray(poses).reshape(-1)
    return (np.stack([poses["R"][k] for k in "xyzw"], -1).astype(F), np.stack([poses["t"][k] for k in "xyz"], -1).astype(F))


def beam_arrays(beams):
    beams = np.asarray(beams).reshape(-1)
    return (np.stack([beams["orig"][k] for k in "xyz"], -1).astype(F), np.stack([beams["dir"][k] for k in "xyz"], -1).astype(F),
            beams["range"].astype(F))


def end_points(R, t, Tsb, beams):
    """[n, n_beams, 3]: Tsm = pose * Tsb; M = Tsm * orig + (Tsm.R * dir) * range"""
    Rb, tb = pose_arrays(Tsb)
    orig, dirs, rng = beam_arrays(beams)
    tsm_R = qmul(R, Rb)
    tsm_t = qrot(R, np.broadcast_to(tb, t.shape)) + t
    n, nb = len(R), len(orig)
    q = np.broadcast_to(tsm_R[:, None, :], (n, nb, 4))
    d = qrot(q, np.broadcast_to(dirs[None], (n, nb, 3)))
    o = qrot(q, np.broadcast_to(orig[None], (n, nb, 3))) + tsm_t[:, None, :]
    return (o + d * rng[None, :, None]).astype(F)


# ---- the lookup with its gradient ------------------------------------------------------------------------------------------------------
def lookup_grad(info, lattice, points):
    """(d, g [m, 3], valid) at points [m, 3]: THE LOOKUP's index, fraction and clamping; d is its value where the point is valid"""
    import field_ref as fr
    info = fr.info_f32(info)
    n = info["n"]
    lat = np.asarray(lattice, F).reshape(n[2], n[1], n[0])
    P = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        fin = (np.abs(P) <= FLT_MAX).all(axis=1)
        Q = np.where(fin[:, None], P, F(0))
        idx, fr_, clamped = [], [], np.zeros(len(P), bool)
        for k in range(3):
            top = F(n[k] - 1)
            u = (Q[:, k] - info["origin"][k]) * info["inv_cell"]
            c = np.minimum(np.maximum(u, F(0)), top)
            i = np.minimum(np.floor(c).astype(np.int64), n[k] - 2)
            idx.append(i)
            fr_.append((c - i.astype(F)).astype(F))
            clamped |= (u < 0) | (u > top)
        ix, iy, iz = idx
        fx, fy, fz = fr_
        v = {(x, y, z): lat[iz + z, iy + y, ix + x] for x in (0, 1) for y in (0, 1) for z in (0, 1)}

        def lerp(a, b, f):
            return (a + f * (b - a)).astype(F)

        x00, x10 = lerp(v[0, 0, 0], v[1, 0, 0], fx), lerp(v[0, 1, 0], v[1, 1, 0], fx)
        x01, x11 = lerp(v[0, 0, 1], v[1, 0, 1], fx), lerp(v[0, 1, 1], v[1, 1, 1], fx)
        d = lerp(lerp(x00, x10, fy), lerp(x01, x11, fy), fz)
        ic = info["inv_cell"]
        gx = lerp(lerp(v[1, 0, 0] - v[0, 0, 0], v[1, 1, 0] - v[0, 1, 0], fy), lerp(v[1, 0, 1] - v[0, 0, 1], v[1, 1, 1] - v[0, 1, 1], fy), fz) * ic
        gy = lerp(lerp(v[0, 1, 0] - v[0, 0, 0], v[1, 1, 0] - v[1, 0, 0], fx), lerp(v[0, 1, 1] - v[0, 0, 1], v[1, 1, 1] - v[1, 0, 1], fx), fz) * ic
        gz = lerp(lerp(v[0, 0, 1] - v[0, 0, 0], v[1, 0, 1] - v[1, 0, 0], fx), lerp(v[0, 1, 1] - v[0, 1, 0], v[1, 1, 1] - v[1, 1, 0], fx), fy) * ic
        g = np.stack([gx, gy, gz], -1).astype(F)
        valid = fin & ~clamped & (np.abs(d) <= FLT_MAX) & (np.abs(g) <= FLT_MAX).all(axis=1)
    return d.astype(F), g, valid


# ---- one pass: (C, A, b, n_used) of every pose -----------------------------------------------------------------------------------------
def wave_sum(contrib):
    """contrib [n, n_beams, k] float64 -> [n, k]: 64 partial sums, partial l over the beams l, l + 64, ... in increasing order from +0,
    then the rounds s = 32 ... 1 of partial_l + partial_(l xor s); the total is partial 0"""
    n, nb, k = contrib.shape
    rows = (nb + 63) // 64
    padded = np.zeros((n, rows * 64, k), D)
    padded[:, :nb] = contrib
    padded = padded.reshape(n, rows, 64, k)
    acc = np.zeros((n, 64, k), D)
    for r in range(rows):
        acc = acc + padded[:, r]
    lanes = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ s]
    return acc[:, 0]


def evaluate(info, lattice, R, t, Tsb, beams, p):
    """(C [n], A [n, 21], b [n, 6], n_used [n]) at the poses (R, t)"""
    n = len(R)
    with np.errstate(all="ignore"):
        M = end_points(R, t, Tsb, beams)
        nb = M.shape[1]
        d, g, valid = lookup_grad(info, lattice, M.reshape(-1, 3))
        d, g, valid = d.reshape(n, nb), g.reshape(n, nb, 3), valid.reshape(n, nb)
        used = valid & (d < p["max_dist"])
        m = np.where(used, d, p["max_dist"]).astype(F)
        L = (M - t[:, None, :]).astype(F)
        J = np.stack([g[..., 0], g[..., 1], g[..., 2],
                      L[..., 1] * g[..., 2] - L[..., 2] * g[..., 1],
                      L[..., 2] * g[..., 0] - L[..., 0] * g[..., 2],
                      L[..., 0] * g[..., 1] - L[..., 1] * g[..., 0]], -1).astype(F).astype(D)
        contrib = np.zeros((n, nb, 28), D)
        contrib[..., 0] = m.astype(D) * m.astype(D)
        for k, (a, c) in enumerate(TRI):
            contrib[..., 1 + k] = np.where(used, J[..., a] * J[..., c], 0.0)
        for a in range(6):
            contrib[..., 22 + a] = np.where(used, J[..., a] * d.astype(D), 0.0)
        S = wave_sum(contrib)
    return S[:, 0], S[:, 1:22], S[:, 22:28], used.sum(axis=1).astype(np.uint32)


# ---- the step --------------------------------------------------------------------------------------------------------------------------
def solve(A, b, mask, lam, p):
    """(delta [n, 6] float64, ok [n]): the damped, masked, length-limited step of every particle"""
    n = len(A)
    with np.errstate(all="ignore"):
        H = np.zeros((n, 6, 6), D)
        for k, (a, c) in enumerate(TRI):
            H[:, a, c] = A[:, k]
            H[:, c, a] = A[:, k]
        rhs = np.array(b, D)
        for a in range(6):
            if not (mask >> a) & 1:
                H[:, a, :] = 0.0
                H[:, :, a] = 0.0
                H[:, a, a] = 1.0
                rhs[:, a] = 0.0
        for a in range(6):
            H[:, a, a] = (H[:, a, a] + lam * H[:, a, a]) + 1e-9
        G = np.zeros((n, 6, 6), D)
        ok = np.ones(n, bool)
        for j in range(6):
            s = H[:, j, j].copy()
            for k in range(j):
                s = s - G[:, j, k] * G[:, j, k]
            ok &= s > 0.0
            G[:, j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                tt = H[:, i, j].copy()
                for k in range(j):
                    tt = tt - G[:, i, k] * G[:, j, k]
                G[:, i, j] = tt / G[:, j, j]
        y, x = np.zeros((n, 6), D), np.zeros((n, 6), D)
        for i in range(6):
            s = rhs[:, i].copy()
            for k in range(i):
                s = s - G[:, i, k] * y[:, k]
            y[:, i] = s / G[:, i, i]
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - G[:, k, i] * x[:, k]
            x[:, i] = s / G[:, i, i]
        delta = np.zeros((n, 6), D)
        for a in range(6):
            if (mask >> a) & 1:
                delta[:, a] = -x[:, a]
        nv = np.sqrt((delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]) + delta[:, 2] * delta[:, 2])
        nw = np.sqrt((delta[:, 3] * delta[:, 3] + delta[:, 4] * delta[:, 4]) + delta[:, 5] * delta[:, 5])
        scale = np.ones(n, D)
        q = np.where(nv > 0.0, D(p["max_step_trans"]) / nv, np.inf)
        scale = np.where(q < scale, q, scale)
        q = np.where(nw > 0.0, D(p["max_step_rot"]) / nw, np.inf)
        scale = np.where(q < scale, q, scale)
        delta = delta * scale[:, None]
    return delta, ok


def candidate(R, t, delta, mask):
    with np.errstate(all="ignore"):
        t2 = t.copy()
        for a in range(3):
            if (mask >> a) & 1:
                t2[:, a] = t[:, a] + delta[:, a].astype(F)
        R2 = R
        if mask & 0x38:
            dq = np.concatenate([(0.5 * delta[:, 3:6]).astype(F), np.ones((len(R), 1), F)], -1)
            R2 = qnormalise(qmul(dq, R))
    return R2, t2.astype(F)


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
def refine(info, lattice, poses, beams, Tsb, p=None):
    """rmclhip_field_refine: (poses', rows [n] of RESULT, stats dict) without touching its inputs"""
    p = params() if p is None else p
    poses = np.array(poses).reshape(-1)
    n = len(poses)
    check(p, n, len(np.asarray(beams).reshape(-1)))
    rows = np.zeros(n, RESULT)
    if n == 0:
        return poses, rows, dict(n_particles=0, n_moved=0, n_no_beams=0, n_not_finite=0, cost_before_sum=0.0, cost_after_sum=0.0)
    R, t = pose_arrays(poses)
    mask = p["dof_mask"] & 0x3F
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    C, A, b, n_used = evaluate(info, lattice, R, t, Tsb, beams, p)
    C0, n_start = C.copy(), n_used.copy()
    accepted = np.zeros(n, np.uint32)
    go = finite & (n_start != 0) & (p["iterations"] != 0) & (mask != 0)
    if go.any():
        lam = np.full(n, D(p["lambda0"]), D)
        for _ in range(p["iterations"]):
            delta, ok = solve(A, b, mask, lam, p)
            R2, t2 = candidate(R, t, delta, mask)
            C2, A2, b2, n2 = evaluate(info, lattice, R2, t2, Tsb, beams, p)
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
    with np.errstate(all="ignore"):
        rows["cost_before"], rows["cost_after"] = C0.astype(F), C.astype(F)
    rows["n_used"], rows["accepted"] = n_used, accepted
    stats = dict(n_particles=n, n_moved=int(moved.sum()), n_no_beams=int((finite & (n_start == 0)).sum()), n_not_finite=int((~finite).sum()),
                 cost_before_sum=float(np.cumsum(rows["cost_before"].astype(D))[-1]), cost_after_sum=float(np.cumsum(rows["cost_after"].astype(D))[-1]))
    return poses, rows, stats


def cost(info, lattice, poses, beams, Tsb, p=None):
    """C of every pose, float64"""
    p = params() if p is None else p
    R, t = pose_arrays(poses)
    return evaluate(info, lattice, R, t, Tsb, beams, p)[0]


def perturbed_starts(truth, n, seed, d_trans=0.3, d_yaw=0.15, z=True):
    """n TRANSFORM records around `truth`: uniformly +-d_trans per axis (z too unless z is False) and +-d_yaw about world z"""
    import math
    rng = np.random.RandomState(seed)
    poses = np.zeros(n, np.asarray(truth).dtype)
    R0, t0 = pose_arrays(truth)
    for i in range(n):
        dt = rng.uniform(-d_trans, d_trans, 3)
        if not z:
            dt[2] = 0.0
        yaw = rng.uniform(-d_yaw, d_yaw)
        dq = np.array([[0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)]], F)
        q = qnormalise(qmul(dq, R0))[0]
        for k, c in zip("xyzw", q):
            poses[i]["R"][k] = c
        for k, c in zip("xyz", (t0[0].astype(D) + dt).astype(F)):
            poses[i]["t"][k] = c
    return poses


def position_error(poses, truth):
    _, t = pose_arrays(poses)
    _, t0 = pose_arrays(truth)
    return np.sqrt(((t.astype(D) - t0.astype(D)) ** 2).sum(axis=1))


def build_example(tmp_path):
    """examples/field_refine_cpp_example.cpp compiled with plain g++ against the C ABI: the executable's path"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = "field_refine_cpp_example.cpp"
    exe = str(tmp_path / source.replace(".cpp", ""))
    libdir = os.path.join(root, "rmcl_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", source), "-L" + libdir, "-lrmclhip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe
