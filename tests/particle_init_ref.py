"""Host restatement (numpy only) of the particle cloud's initialisations and visualisation channels -- what
rmcl_amd/csrc/particles.hip and rmclhip_chol6_host compute, operation by operation in their order, so that the device results can be
compared bit for bit (transcendentals are evaluated in double and rounded to float on both sides: nearly always the same bits).

    philox4x32_10        the counter-based generator, with 64-bit products
    init_words           w0..w5 of global particle i: philox((i, epoch, 0, 1), seed), philox((i, epoch, 1, 1), seed)[0..1]
    uniform_values       the six uniform draws of RmclNode::initSamplesUniform
    gaussians            the three Box-Muller pairs of RmclNode::initSamples
    init_uniform / init_pose   the whole clouds (TRANSFORM, PARTICLE_ATTRIBUTES arrays)
    chol6                the covariance factor of the pose form and its "Cholesky Err"
    pack_visualization   the seven arrays RmclNode::visualize publishes
and the covariances the CPU and the GPU tests share (COVS).
"""
import math

import numpy as np

from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: [..., 4] uint32, key: [..., 2] uint32 (broadcast against each other) -> [..., 4] uint32 (Random123 philox4x32, 10 rounds)"""
    ctr = np.asarray(ctr, dtype=np.uint32)
    key = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., k], shape).astype(np.uint64) for k in range(4)]
    k0 = np.broadcast_to(key[..., 0], shape).astype(np.uint64)
    k1 = np.broadcast_to(key[..., 1], shape).astype(np.uint64)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        h0, l0, h1, l1 = p0 >> _S32, p0 & _LO, p1 >> _S32, p1 & _LO
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0, k1 = (k0 + np.uint64(_W0)) & _LO, (k1 + np.uint64(_W1)) & _LO
    return np.stack(c, axis=-1).astype(np.uint32)


def init_words(first, count, seed, epoch):
    """[count, 6] uint32: the random words of global particles first .. first+count-1"""
    i = (np.arange(count, dtype=np.uint64) + np.uint64(first)).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    ctr = np.zeros((count, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 3] = i, np.uint32(epoch), 1
    a = philox4x32_10(ctr, key)
    ctr[:, 2] = 1
    b = philox4x32_10(ctr, key)
    return np.concatenate([a, b[:, :2]], axis=1)


def _unit(w):
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def uniform_values(w, bb_min, bb_max):
    """[n, 6] float32: v_d = float(double(lo_d) + (double(hi_d) - double(lo_d)) * u_d)"""
    lo = np.asarray(bb_min, dtype=np.float32).astype(np.float64)
    hi = np.asarray(bb_max, dtype=np.float32).astype(np.float64)
    return (lo[None, :] + (hi - lo)[None, :] * _unit(w)).astype(np.float32)


def box_muller(a, b):
    u1, u2 = _unit(a), _unit(b)
    r, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925 * u2
    return (r * np.cos(ang)).astype(np.float32), (r * np.sin(ang)).astype(np.float32)


def gaussians(w):
    """[n, 6] float32 standard normals: (z0, z1) = box_muller(w0, w1), (z2, z3) = (w2, w3), (z4, z5) = (w4, w5)"""
    z = np.zeros(w.shape, dtype=np.float32)
    for k in (0, 2, 4):
        z[:, k], z[:, k + 1] = box_muller(w[:, k], w[:, k + 1])
    return z


def euler_to_quat(roll, pitch, yaw):
    """float32 arrays -> (x, y, z, w) float32: cos / sin of the float half angles in double, rounded to float, then float products"""
    two = np.float32(2.0)

    def cs(a):
        h = (np.asarray(a, dtype=np.float32) / two).astype(np.float64)
        return np.cos(h).astype(np.float32), np.sin(h).astype(np.float32)

    (cr, sr), (cp, sp), (cy, sy) = cs(roll), cs(pitch), cs(yaw)
    w = cr * cp * cy + sr * sp * sy
    x = sr * cp * cy - cr * sp * sy
    y = cr * sp * cy + sr * cp * sy
    z = cr * cp * sy - sr * sp * cy
    return x, y, z, w


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by - ax * bz) + ay * bw) + az * bx
    z = ((aw * bz + ax * by) - ay * bx) + az * bw
    return x, y, z, w


def _xmul_const(T, R, t):
    """T * {R, t}: T one TRANSFORM, R = (x, y, z, w) and t = (x, y, z) float32 arrays (devmath.h xmul / qrot / qmul)"""
    f = np.float32
    n = len(t[0])
    q = tuple(np.full(n, f(T["R"][k]), dtype=f) for k in "xyzw")
    qi = (-q[0], -q[1], -q[2], q[3])
    P = (t[0], t[1], t[2], np.zeros(n, dtype=f))
    PT = _qmul(_qmul(q, P), qi)
    tt = tuple(PT[k] + f(T["t"]["xyz"[k]]) for k in range(3))
    return _qmul(q, R), tt


def _attrs(n):
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = 1.0
    return a


def _poses(R, t, stamp=0):
    p = np.zeros(len(t[0]), dtype=TRANSFORM)
    for k, v in zip("xyzw", R):
        p["R"][k] = v
    for k, v in zip("xyz", t):
        p["t"][k] = v
    p["stamp"] = stamp
    return p


def init_uniform(first, count, bb_min, bb_max, seed, epoch=0):
    v = uniform_values(init_words(first, count, seed, epoch), bb_min, bb_max)
    return _poses(euler_to_quat(v[:, 3], v[:, 4], v[:, 5]), (v[:, 0], v[:, 1], v[:, 2])), _attrs(count)


def deform(L, z):
    """x_r = float(sum over c = 0..r, in increasing c, of double(L[r][c]) * double(z_c)), the sum starting at +0.0"""
    L = np.asarray(L, dtype=np.float32).reshape(6, 6).astype(np.float64)
    zd = z.astype(np.float64)
    x = np.zeros(z.shape, dtype=np.float32)
    for r in range(6):
        acc = np.zeros(len(z), dtype=np.float64)
        for c in range(r + 1):
            acc = acc + L[r, c] * zd[:, c]
        x[:, r] = acc.astype(np.float32)
    return x


def init_pose(first, count, Tlm, covariance, seed, epoch=0):
    L, _ = chol6(covariance)
    x = deform(L, gaussians(init_words(first, count, seed, epoch)))
    Tlm = np.asarray(Tlm, dtype=TRANSFORM).reshape(())
    R, t = _xmul_const(Tlm, euler_to_quat(x[:, 3], x[:, 4], x[:, 5]), (x[:, 0], x[:, 1], x[:, 2]))
    return _poses(R, t, int(Tlm["stamp"])), _attrs(count)


def chol6(covariance):
    """(L float32 [6, 6], err) of rmclhip_chol6_host; raises ValueError where that returns RMCLHIP_ERR_INVALID"""
    C = [float(v) for v in np.asarray(covariance, dtype=np.float64).reshape(36)]
    if not all(math.isfinite(v) for v in C):
        raise ValueError("covariance has a non-finite entry")
    A = [[(C[6 * r + c] + C[6 * c + r]) / 2.0 for c in range(6)] for r in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    tol = (36.0 / 16777216.0) * max(abs(A[j][j]) for j in range(6))
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if d < -tol:
            raise ValueError("covariance is not positive semidefinite")
        if d <= tol:
            continue
        ljj = math.sqrt(d)
        L[j][j] = ljj
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / ljj
    Lf = np.array(L, dtype=np.float64).astype(np.float32)
    Ld = [[float(Lf[r, c]) for c in range(6)] for r in range(6)]
    err = 0.0
    for r in range(6):
        for c in range(6):
            s = 0.0
            for k in range(6):
                s = s + Ld[r][k] * Ld[c][k]
            err = err + abs(s - A[r][c])
    return Lf, err / 36.0


def pack_visualization(poses, attrs, max_n_meas=10000):
    """dict of the seven float32 arrays of RmclNode::visualize (rmcl_localization.cpp:856-874)"""
    L = attrs["likelihood"]
    mean, sigma = L["mean"].astype(np.float32), L["sigma"].astype(np.float32)
    unc = (1.0 - L["n_meas"].astype(np.float64) / np.float64(max_n_meas)).astype(np.float32)
    return {"x": poses["t"]["x"].copy(), "y": poses["t"]["y"].copy(), "z": poses["t"]["z"].copy(), "likelihood": mean,
            "likelihood_sigma": sigma, "likelihood_n_meas": L["n_meas"].astype(np.float32), "badness": mean * (sigma * unc + unc)}


# ---- inputs the tests share -------------------------------------------------------------------------------
RVIZ_COV = np.diag([0.25, 0.25, 0.0, 0.0, 0.0, 0.0685])     # what RViz's "2D Pose Estimate" sends: x, y and yaw only


def full_rank_cov():
    """a pose covariance with every direction open and all of them correlated: S R S with S = the standard deviations"""
    rs = np.random.RandomState(11)
    A = rs.normal(size=(6, 6))
    R = A @ A.T + 6.0 * np.eye(6)
    d = np.sqrt(np.diag(R))
    R = R / d[:, None] / d[None, :]
    s = np.array([0.5, 0.4, 0.1, 0.03, 0.02, 0.25])
    return R * s[:, None] * s[None, :]


def rank3_cov():
    A = np.random.RandomState(12).normal(size=(6, 3)) * 0.3
    return A @ A.T


COVS = {"full": full_rank_cov(), "rviz": RVIZ_COV, "rank3": rank3_cov()}
