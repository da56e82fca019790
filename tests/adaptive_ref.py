"""Host restatement (numpy only) of the adaptive particle count -- what rmcl_amd/csrc/adaptive.hip (the bins), resample.hip (the
systematic resampler) and rmclhip_kld_bound_host compute, operation by operation in their order (include/rmclhip.h states the rules):

    quat_to_euler        the textbook ZYX extraction: float products, atan2 / asin in double, rounded to float
    likelihood_max       the maximum rmclhip_resampler_compute_stats returns (seeded with 0, NaN never taken)
    bin_tuples           counted mask and the six int32 of every particle's bin;  bin_margin: how far the coordinates are from a bin edge
    count_bins           (k, n_counted)
    kld_bound            the KLD-sampling bound in double (Python floats), ValueError where the library returns RMCLHIP_ERR_INVALID
    sys_weights / sys_sources   integer weights, exact prefix sums, the source of every slot and which slots start a run
    systematic           the new cloud (TRANSFORM, PARTICLE_ATTRIBUTES arrays) and its sources
and the clouds the CPU and the GPU tests share (weight_cases).
"""
import math

import numpy as np

from particle_init_ref import _qmul, box_muller, euler_to_quat, philox4x32_10
from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM

f32 = np.float32
PI_F = f32(3.14159265358979323846)


class Kld:
    """rmclhip_kld_params with the library's defaults"""

    def __init__(self, bin_xyz=(0.5, 0.5, 0.5), bin_rpy=(0.17453292,) * 3, min_likelihood_rel=0.01, epsilon=0.01, z=2.3263479, n_min=500,
                 n_max=0xFFFFFFFF):
        self.bin_xyz = [f32(v) for v in bin_xyz]
        self.bin_rpy = [f32(v) for v in bin_rpy]
        self.min_likelihood_rel = f32(min_likelihood_rel)
        self.epsilon, self.z, self.n_min, self.n_max = float(epsilon), float(z), int(n_min), int(n_max)


GLADIATOR_DEFAULTS = dict(min_noise_tx=0.03, min_noise_ty=0.03, min_noise_tz=0.0, min_noise_roll=0.0, min_noise_pitch=0.0, min_noise_yaw=0.01,
                          likelihood_forget_per_meter=0.3, likelihood_forget_per_radian=0.2, trans_dist_metric=0)


def gladiator_cfg(**kw):
    cfg = dict(GLADIATOR_DEFAULTS)
    cfg.update(kw)
    return cfg


def quat_to_euler(x, y, z, w):
    """float32 arrays -> (roll, pitch, yaw) float32"""
    x, y, z, w = (np.asarray(v, dtype=f32) for v in (x, y, z, w))
    two, one = f32(2.0), f32(1.0)
    sinr_cosp = two * (w * x + y * z)
    cosr_cosp = one - two * (x * x + y * y)
    sinp = two * (w * y - z * x)
    siny_cosp = two * (w * z + x * y)
    cosy_cosp = one - two * (y * y + z * z)
    with np.errstate(invalid="ignore"):
        roll = np.arctan2(sinr_cosp.astype(np.float64), cosr_cosp.astype(np.float64)).astype(f32)
        steep = np.abs(sinp) >= one
        pitch = np.where(steep, np.copysign(f32(3.14159265358979323846 / 2.0), sinp),
                         np.arcsin(np.where(steep, f32(0.0), sinp).astype(np.float64)).astype(f32)).astype(f32)
        yaw = np.arctan2(siny_cosp.astype(np.float64), cosy_cosp.astype(np.float64)).astype(f32)
    return roll, pitch, yaw


def likelihood_max(attrs):
    L = attrs["likelihood"]["mean"].astype(f32)
    L = L[~np.isnan(L)]
    return f32(max(f32(0.0), L.max())) if len(L) else f32(0.0)


def _coords(poses, p):
    """raw bin coordinates [n, 6] float32: t_d / bin_xyz[d] and (angle_d + pi_f) / bin_rpy[d]; 0 where the dimension is ignored"""
    n = len(poses)
    c = np.zeros((n, 6), dtype=f32)
    rpy = quat_to_euler(*(poses["R"][k] for k in "xyzw"))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for d in range(3):
            if p.bin_xyz[d] != 0:
                c[:, d] = poses["t"]["xyz"[d]].astype(f32) / p.bin_xyz[d]
            if p.bin_rpy[d] != 0:
                c[:, 3 + d] = (rpy[d] + PI_F) / p.bin_rpy[d]
    return c


def counted_mask(poses, attrs, p, max_l=None):
    max_l = likelihood_max(attrs) if max_l is None else f32(max_l)
    L = attrs["likelihood"]["mean"].astype(f32)
    fin = np.isfinite(L)
    for k in "xyzw":
        fin &= np.isfinite(poses["R"][k])
    for k in "xyz":
        fin &= np.isfinite(poses["t"][k])
    floor_l = f32(p.min_likelihood_rel * max_l)          # float product
    with np.errstate(invalid="ignore"):
        return fin & (L > 0) & (L >= floor_l)


def bin_tuples(poses, attrs, p, max_l=None):
    """(counted [n] bool, tuples [n, 6] int32; rows of particles that are not counted hold zeros)"""
    counted = counted_mask(poses, attrs, p, max_l)
    c = _coords(poses[counted], p)
    lo = np.array([-8192.0] * 3 + [0.0] * 3, dtype=f32)
    hi = np.array([8191.0] * 3 + [126.0] * 3, dtype=f32)
    idx = np.minimum(np.maximum(np.floor(c), lo[None, :]), hi[None, :]).astype(np.int32)
    out = np.zeros((len(poses), 6), dtype=np.int32)
    out[counted] = idx
    return counted, out


def bin_margin(poses, attrs, p, max_l=None):
    """smallest distance, in bins, of a counted particle's coordinate to an edge that separates two bin indices"""
    counted = counted_mask(poses, attrs, p, max_l)
    c = _coords(poses[counted], p).astype(np.float64)
    lo = np.array([-8192.0] * 3 + [0.0] * 3)
    hi = np.array([8192.0] * 3 + [127.0] * 3)
    frac = c - np.floor(c)
    inside = np.minimum(frac, 1.0 - frac)
    outside = np.where(c < lo[None, :], lo[None, :] - c, c - hi[None, :])
    m = np.where((c >= lo[None, :]) & (c < hi[None, :]), inside, outside)
    used = np.array([w != 0 for w in list(p.bin_xyz) + list(p.bin_rpy)])
    return float(m[:, used].min()) if m[:, used].size else 1.0


def count_bins(poses, attrs, p):
    counted, tup = bin_tuples(poses, attrs, p)
    k = len(np.unique(tup[counted], axis=0)) if counted.any() else 0
    return k, int(counted.sum())


def kld_bound(k, epsilon, z, n_min, n_max):
    if not (math.isfinite(epsilon) and math.isfinite(z) and epsilon > 0.0):
        raise ValueError("epsilon must be finite and > 0, z finite")
    if n_min == 0 or n_min > n_max:
        raise ValueError("1 <= n_min <= n_max required")
    if k < 2:
        return n_min
    km1 = float(k - 1)
    a = 2.0 / (9.0 * km1)
    x = (1.0 - a) + math.sqrt(a) * z
    n = math.ceil((km1 / (2.0 * epsilon)) * ((x * x) * x))
    return min(max(n, n_min), n_max)


def sys_weights(L, max_l):
    """python ints: w_i = uint64(rint(double(L_i) / double(max) * 2^24)), 0 for a negative or non-finite L_i"""
    L = np.asarray(L, dtype=f32)
    ok = np.isfinite(L) & (L > 0)
    w = np.zeros(len(L), dtype=np.float64)
    w[ok] = np.rint(L[ok].astype(np.float64) / np.float64(f32(max_l)) * 16777216.0)
    return [int(v) for v in w]


def _words(idx, step, draw, seed):
    idx = np.asarray(idx, dtype=np.uint32).reshape(-1)
    ctr = np.zeros((len(idx), 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = idx, np.uint32(step), np.uint32(draw)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32))


def sys_u0(seed, step):
    return (float(_words([0], step, 5, seed)[0, 0]) + 0.5) * (1.0 / 4294967296.0)


def sys_sources(L, n_new, seed, step, max_l=None):
    """(src [n_new] int64, first_of_run [n_new] bool, weights, T)"""
    L = np.asarray(L, dtype=f32)
    if max_l is None:
        Ln = L[~np.isnan(L)]
        max_l = f32(max(f32(0.0), Ln.max())) if len(Ln) else f32(0.0)
    if not (max_l > 0 and math.isfinite(max_l)) or n_new == 0:
        raise ValueError("nothing to resample from")
    w = sys_weights(L, max_l)
    C = np.cumsum(np.array(w, dtype=np.uint64), dtype=np.uint64)      # (T <= 2^56: exact)
    T = int(C[-1])
    u0 = sys_u0(seed, step)
    scale = float(T) / float(n_new)
    j = np.arange(n_new, dtype=np.float64)
    pos = np.minimum(np.floor((j + u0) * scale).astype(np.uint64), np.uint64(T - 1))
    src = np.searchsorted(C, pos, side="right").astype(np.int64)      # the first i with C[i] > pos
    first = np.ones(n_new, dtype=bool)
    first[1:] = src[1:] != src[:-1]
    return src, first, w, T


def _qrot(q, p):
    P = (p[0], p[1], p[2], np.zeros_like(p[0]))
    qi = (-q[0], -q[1], -q[2], q[3])
    r = _qmul(_qmul(q, P), qi)
    return r[0], r[1], r[2]


def n_meas_scaled(n_meas, rate):
    """uint32(float(n_meas) * rate) with the library's pinned conversion (pf_random.hip.h: n_meas_scaled): NaN or <= 0 -> 0,
    >= 2^32 -> 0xFFFFFFFF, otherwise truncate"""
    v = np.asarray(n_meas, dtype=np.uint32).astype(f32) * np.asarray(rate, dtype=f32)
    big, mid = v >= f32(4294967296.0), (v > 0) & (v < f32(4294967296.0))
    out = np.zeros(v.shape, dtype=np.uint32)
    out[big] = 0xFFFFFFFF
    out[mid] = v[mid].astype(np.int64).astype(np.uint32)
    return out


def perturb(poses, attrs, slots, cfg, seed, step):
    """the gladiator's winning enemy (resample.hip: k_gladiator_resample) with the Gaussians of the GLOBAL slot indices `slots` from
    draws 6 and 7; poses / attrs: the sources, one per slot"""
    a, b = _words(slots, step, 6, seed), _words(slots, step, 7, seed)
    Nd_tx, Nd_ty = box_muller(a[:, 1], a[:, 2])
    Nd_tz, Nd_rx = box_muller(a[:, 3], b[:, 0])
    Nd_ry, Nd_rz = box_muller(b[:, 1], b[:, 2])
    c = {k: f32(v) for k, v in cfg.items() if k != "trans_dist_metric"}
    q = tuple(poses["R"][k].astype(f32) for k in "xyzw")
    t = tuple(poses["t"][k].astype(f32) for k in "xyz")
    tn = (t[0] + Nd_tx * c["min_noise_tx"], t[1] + Nd_ty * c["min_noise_ty"], t[2] + Nd_tz * c["min_noise_tz"])
    roll, pitch, yaw = quat_to_euler(*q)
    roll = roll + Nd_rx * c["min_noise_roll"]
    pitch = pitch + Nd_ry * c["min_noise_pitch"]
    yaw = yaw + Nd_rz * c["min_noise_yaw"]
    qn = euler_to_quat(roll, pitch, yaw)
    # diff = ~pose * pose_new
    qi = (-q[0], -q[1], -q[2], q[3])
    ti = tuple(-v for v in _qrot(qi, t))
    dt = tuple(r + o for r, o in zip(_qrot(qi, tn), ti))
    dR = _qmul(qi, qn)
    t2 = (dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]
    trans_dist = t2 if cfg["trans_dist_metric"] == 1 else np.sqrt(t2)
    rot_dist = np.sqrt(((dR[3] * dR[3] + dR[0] * dR[0]) + dR[1] * dR[1]) + dR[2] * dR[2])
    frs = (1.0 - np.power(1.0 - np.float64(c["likelihood_forget_per_meter"]), trans_dist.astype(np.float64))).astype(f32)
    frr = (1.0 - np.power(1.0 - np.float64(c["likelihood_forget_per_radian"]), rot_dist.astype(np.float64))).astype(f32)
    forget = np.where(frs > frr, frs, frr)
    remember = (1.0 - forget.astype(np.float64)).astype(f32)
    pn, an = poses.copy(), attrs.copy()
    for k, v in zip("xyz", tn):
        pn["t"][k] = v
    for k, v in zip("xyzw", qn):
        pn["R"][k] = v
    an["likelihood"]["n_meas"] = n_meas_scaled(attrs["likelihood"]["n_meas"], remember)
    return pn, an


def systematic(poses, attrs, n_new, cfg, seed, step, first=0, count=None):
    """(poses_new, attrs_new, src) of slots first .. first+count-1 -- computed for those slots alone, the slot before them included"""
    count = n_new - first if count is None else count
    src, run_start, _, _ = sys_sources(attrs["likelihood"]["mean"], n_new, seed, step)
    sl = slice(first, first + count)
    s, fr = src[sl], run_start[sl]
    pn, an = poses[s].copy(), attrs[s].copy()
    if (~fr).any():
        slots = np.arange(first, first + count, dtype=np.uint32)[~fr]
        pp, aa = perturb(poses[s[~fr]], attrs[s[~fr]], slots, cfg, seed, step)
        pn[~fr], an[~fr] = pp, aa
    return pn, an, s


# ---- inputs the tests share -------------------------------------------------------------------------------
SYS_N = (1, 64, 65, 1025, 4097)


def sys_n_new(n):
    return sorted({v for v in (1, n // 7, n, 3 * n) if v >= 1})


def cloud(n, seed):
    """n particles in a room-sized box with distinct stamps (stamp = index: the source of a slot can be read back), likelihoods 1"""
    rs = np.random.RandomState(seed)
    v = rs.uniform((-9, -9, 0.2, -0.2, -0.2, -math.pi), (9, 9, 3.0, 0.2, 0.2, math.pi), size=(n, 6)).astype(f32)
    p = np.zeros(n, dtype=TRANSFORM)
    for k, q in zip("xyzw", euler_to_quat(v[:, 3], v[:, 4], v[:, 5])):
        p["R"][k] = q
    for d, k in enumerate("xyz"):
        p["t"][k] = v[:, d]
    p["stamp"] = np.arange(n, dtype=np.uint32)
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = 1.0
    a["likelihood"]["sigma"] = rs.uniform(0, 0.1, n)
    a["likelihood"]["n_meas"] = rs.randint(0, 10001, n)
    a["state_sigma"] = rs.uniform(0, 1, (n, 6))
    return p, a


def weight_cases(n, seed=3):
    """name -> likelihoods [n] float32"""
    rs = np.random.RandomState(seed + n)
    out = {"even": np.full(n, 0.37, dtype=f32)}
    one = np.zeros(n, dtype=f32)
    one[n // 2] = 0.8
    out["one_holds_all"] = one
    out["span_1e-6_1"] = (10.0 ** rs.uniform(-6, 0, n)).astype(f32)
    out["span_1e-6_1"][rs.randint(n)] = 1.0
    rz = rs.uniform(0.2, 1.0, n).astype(f32)
    rz[::3] = f32(1e-9)            # 1e-9 / max * 2^24 < 0.5: rounds to w = 0
    rz[n // 2] = 1.0
    out["rounds_to_zero"] = rz
    return out
