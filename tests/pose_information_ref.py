"""numpy restatement of the pose information (include/rmclhip.h, POSE COVARIANCE): the gate of rmclhip_statistics_p2l in float32,
operation for operation (devmath.h qmul / qrot / xapply / dot_plain; the oracle's p2l_element), then u = [N ; D x N ; r] and the sums
A, g, rss in float64 with math.fsum.  Every entry also comes with the sum of the magnitudes of its terms: n_meas * 2^-52 times that
bounds the error of ANY summation order in double (each partial sum is at most sum |terms| in magnitude, each of the n_meas - 1
additions rounds by at most half an ulp of it)."""
import math

import numpy as np

F = np.float32
EPS64 = 2.0 ** -52


def _qmul(a, b):
    """Hamilton product of (..., 4) float32 arrays {x, y, z, w}, in devmath.h's operation order"""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by - ax * bz) + ay * bw) + az * bx
    z = ((aw * bz + ax * by) - ay * bx) + az * bw
    return np.stack([x, y, z, w], axis=-1).astype(F)


def tapply_f32(T, P):
    """xapply(T, p) = qrot(T.R, p) + T.t on an (n, 3) float32 array, bit for bit what the kernels compute"""
    P = np.ascontiguousarray(P, dtype=F).reshape(-1, 3)
    q = np.array([T["R"][k] for k in "xyzw"], dtype=F)
    t = np.array([T["t"][k] for k in "xyz"], dtype=F)
    qi = np.array([-q[0], -q[1], -q[2], q[3]], dtype=F)
    Pq = np.concatenate([P, np.zeros((len(P), 1), F)], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        r = _qmul(_qmul(np.broadcast_to(q, Pq.shape), Pq), np.broadcast_to(qi, Pq.shape))
        return (r[:, :3] + t).astype(F)


def rotation_f64(T):
    """devmath.h quat_to_mat in float64, from the float32 quaternion normalised in float64 (rmclhip_pose_information_transform's R)"""
    q = np.array([float(T["R"][k]) for k in "xyzw"])
    x, y, z, w = q / math.sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]))
    return np.array([[2.0 * (w * w + x * x) - 1.0, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 2.0 * (w * w + y * y) - 1.0, 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 2.0 * (w * w + z * z) - 1.0]])


def adjoint(T):
    """X = [[R, 0], [[t]x R, R]]: J' = X J for correspondences moved by T"""
    R = rotation_f64(T)
    t = [float(T["t"][k]) for k in "xyz"]
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    X = np.zeros((6, 6))
    X[:3, :3] = R
    X[3:, 3:] = R
    X[3:, :3] = tx @ R
    return X


def gate(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist):
    """(kept, D, r): the float32 classification of rmclhip_statistics_p2l"""
    P = np.ascontiguousarray(dataset_points, dtype=F).reshape(-1, 3)
    I = np.ascontiguousarray(model_points, dtype=F).reshape(-1, 3)
    N = np.ascontiguousarray(model_normals, dtype=F).reshape(-1, 3)
    n = len(P)
    ok = np.ones(n, bool)
    if dataset_mask is not None:
        ok &= np.asarray(dataset_mask).reshape(-1)[:n] > 0
    if model_mask is not None:
        ok &= np.asarray(model_mask).reshape(-1)[:n] > 0
    D = tapply_f32(Tpre, P)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (I - D).astype(F)
        r = ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]).astype(F) + d[:, 2] * N[:, 2]).astype(F)
        kept = ok & (np.abs(r) < F(max_dist))
    return kept, D, r


def u_vectors(D, N, r):
    """u = [N ; D x N ; r] in float64 from float32 values (products exact, one rounding per difference: what the kernel computes)"""
    D, N = D.astype(np.float64), N.astype(np.float64)
    c = np.stack([D[:, 1] * N[:, 2] - D[:, 2] * N[:, 1], D[:, 2] * N[:, 0] - D[:, 0] * N[:, 2], D[:, 0] * N[:, 1] - D[:, 1] * N[:, 0]], axis=1)
    return np.concatenate([N, c, r.astype(np.float64)[:, None]], axis=1)


def sums_of(U):
    """(S, S_abs): the 7 x 7 matrix sum u u^T with math.fsum, and the sums of the terms' magnitudes"""
    S, Sa = np.zeros((7, 7)), np.zeros((7, 7))
    for a in range(7):
        for b in range(a, 7):
            terms = U[:, a] * U[:, b]
            S[a, b] = S[b, a] = math.fsum(terms.tolist())
            Sa[a, b] = Sa[b, a] = math.fsum(np.abs(terms).tolist())
    return S, Sa


def pose_information(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist):
    """dict A (6, 6), g (6), rss, n_meas, the same keys + '_abs' for the magnitudes' sums, kept (bool per element), U (kept u's)"""
    kept, D, r = gate(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist)
    N = np.ascontiguousarray(model_normals, dtype=F).reshape(-1, 3)
    U = u_vectors(D[kept], N[kept], r[kept])
    S, Sa = sums_of(U)
    return dict(A=S[:6, :6].copy(), g=S[:6, 6].copy(), rss=float(S[6, 6]), n_meas=int(kept.sum()),
                A_abs=Sa[:6, :6].copy(), g_abs=Sa[:6, 6].copy(), rss_abs=float(Sa[6, 6]), kept=kept, U=U)


def from_u(U):
    """the same record from ready-made u vectors (host-algebra tests)"""
    S, Sa = sums_of(U)
    return dict(A=S[:6, :6].copy(), g=S[:6, 6].copy(), rss=float(S[6, 6]), n_meas=len(U), A_abs=Sa[:6, :6].copy(), g_abs=Sa[:6, 6].copy(),
                rss_abs=float(Sa[6, 6]), U=U)


def as_record(T, ref):
    """a POSE_INFORMATION record holding a reference result"""
    rec = np.zeros((), dtype=T.POSE_INFORMATION)
    rec["A"], rec["g"], rec["rss"], rec["n_meas"] = ref["A"], ref["g"], ref["rss"], ref["n_meas"]
    return rec


def assert_matches(got, ref, what=""):
    """n_meas exact; every entry e of A, g, rss within n_meas * 2^-52 * sum |terms of e| of the reference"""
    assert int(got["n_meas"]) == ref["n_meas"], "%s: n_meas %d != %d" % (what, int(got["n_meas"]), ref["n_meas"])
    n = ref["n_meas"]
    for key in ("A", "g", "rss"):
        g, r, bound = np.asarray(got[key], np.float64), np.asarray(ref[key]), n * EPS64 * np.asarray(ref[key + "_abs"])
        err = np.abs(g - r)
        assert np.all(err <= bound), "%s: %s off by %.3g, bound %.3g" % (what, key, float(np.max(err - bound)), float(np.max(bound)))
    assert np.array_equal(np.asarray(got["A"]), np.asarray(got["A"]).T), "%s: A not symmetric" % what
