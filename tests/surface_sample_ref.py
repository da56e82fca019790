"""Host restatement (numpy only) of the surface sampler and the recovery rule (include/rmclhip.h, SURFACE SAMPLER): what
rmcl_amd/csrc/surface_sample.hip, the scan of resample.hip, surface_sample.hip.h, the two kernels of particles.hip and
rmclhip_recovery_update_host compute, operation by operation in their order, so that device results compare bit for bit.  Philox and the
Euler step come from particle_init_ref.  Not a test module.

    face_table       lowest record per face id, eligibility, areas, a_max, integer weights, prefix sums, T
    Sampler          the table of a (record array, parameters) with info() and draw(A, B)
    init_surface     the cloud of rmclhip_particles_init_surface
    inject_mask / inject   which slots rmclhip_particles_inject_surface replaces, and the cloud it leaves
    recovery_update / recovery_reset   the augmented-MCL averages
"""
import math

import numpy as np

import particle_init_ref as pir
from rmcl_amd.types import TRANSFORM

F = np.float32
PI_F = F(3.14159265358979323846)
NO_RECORD = 0xFFFFFFFF
TWO32 = 4294967296.0


def params(min_up_cos=0.7, height=0.0, align=0, region_min=(-np.inf,) * 3, region_max=(np.inf,) * 3, yaw_min=-PI_F, yaw_max=PI_F):
    """rmclhip_surface_sample_params with the defaults of rmclhip_surface_sample_params_default"""
    return dict(min_up_cos=F(min_up_cos), height=F(height), align=int(align), region_min=np.asarray(region_min, F),
                region_max=np.asarray(region_max, F), yaw_min=F(yaw_min), yaw_max=F(yaw_max))


def check_params(p):
    """raises ValueError where rmclhip_surface_sampler_create returns RMCLHIP_ERR_INVALID before any launch"""
    if not (p["min_up_cos"] >= 0 and p["min_up_cos"] <= 1):
        raise ValueError("min_up_cos")
    if not math.isfinite(p["height"]):
        raise ValueError("height")
    if p["align"] not in (0, 1):
        raise ValueError("align")
    if not all(p["region_min"][d] <= p["region_max"][d] for d in range(3)):
        raise ValueError("region")
    if not (math.isfinite(p["yaw_min"]) and math.isfinite(p["yaw_max"]) and p["yaw_min"] <= p["yaw_max"]):
        raise ValueError("yaw")


def face_table(tris, n_faces, p):
    """tris: the record array [n_records, 16] uint32 of registration.build_bvh_host -- the float Ng the device reads.
    Returns dict(rec, eligible, area, a_max, w, C, T)."""
    tris = np.asarray(tris, np.uint32).reshape(-1, 16)
    fid = tris[:, 15].astype(np.int64)
    rec = np.full(n_faces, NO_RECORD, np.int64)
    ok = fid < n_faces
    np.minimum.at(rec, fid[ok], np.nonzero(ok)[0])           # the lowest record index that carries the face id
    have = rec != NO_RECORD
    r = tris[np.where(have, rec, 0)].view(F)
    v0, e1, e2, Ng, n = (r[:, k:k + 3].astype(np.float64) for k in (0, 3, 6, 9, 12))
    with np.errstate(all="ignore"):
        eligible = have & (np.abs(r[:, 14]) >= p["min_up_cos"])
        c = v0 + (e2 - e1) / 3.0
        for d in range(3):
            eligible &= (c[:, d] >= np.float64(p["region_min"][d])) & (c[:, d] <= np.float64(p["region_max"][d]))
        area = 0.5 * np.sqrt((Ng[:, 0] * Ng[:, 0] + Ng[:, 1] * Ng[:, 1]) + Ng[:, 2] * Ng[:, 2])
        weighs = eligible & np.isfinite(area) & (area > 0.0)
        a_max = area[weighs].max() if weighs.any() else 0.0
        w = np.zeros(n_faces, np.uint64)
        if weighs.any():
            w[weighs] = np.rint(area[weighs] / a_max * TWO32).astype(np.uint64)
    C = np.cumsum(w, dtype=np.uint64)
    return dict(rec=rec, eligible=eligible, area=area, a_max=a_max, w=w, C=C, T=int(C[-1]) if n_faces else 0)


def _qmul(a, b):
    return pir._qmul(a, b)


def _qrot(q, p):
    """devmath.h qrot: (q (x) (p, 0)) (x) conj(q), float32"""
    P = (p[0], p[1], p[2], np.zeros_like(p[0]))
    r = _qmul(_qmul(q, P), (-q[0], -q[1], -q[2], q[3]))
    return r[0], r[1], r[2]


def _qnormalise(q):
    nrm = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q[0] / nrm, q[1] / nrm, q[2] / nrm, q[3] / nrm


def align(R, n):
    """step 5 of the surface constraint on arrays: R = (x, y, z, w), n = (x, y, z), float32 -> (R', took the half-turn branch)"""
    one, zero = np.ones_like(n[0]), np.zeros_like(n[0])
    with np.errstate(all="ignore"):
        zb = _qrot(R, (zero, zero, one))
        w = F(1) + ((zb[0] * n[0] + zb[1] * n[1]) + zb[2] * n[2])
        half = w < F(1e-6)
        xb = _qrot(R, (one, zero, zero))
        q = (np.where(half, xb[0], zb[1] * n[2] - zb[2] * n[1]), np.where(half, xb[1], zb[2] * n[0] - zb[0] * n[2]),
             np.where(half, xb[2], zb[0] * n[1] - zb[1] * n[0]), np.where(half, F(0), w))
        return _qnormalise(_qmul(_qnormalise(q), R)), half


class Sampler:
    def __init__(self, tris, n_faces, p):
        check_params(p)
        self.p = p
        self.tris = np.asarray(tris, np.uint32).reshape(-1, 16)
        self.n_faces = int(n_faces)
        self.tab = face_table(self.tris, self.n_faces, p)
        if self.tab["T"] == 0:
            raise ValueError("no face with a positive weight")

    def info(self):
        t = self.tab
        fin = t["eligible"] & np.isfinite(t["area"])
        total = np.float64(0.0)
        for a in t["area"][fin]:                       # sequential, in increasing face id
            total = total + a
        return dict(n_faces=self.n_faces, n_eligible=int(t["eligible"].sum()), n_weighted=int((t["w"] > 0).sum()),
                    area_eligible=float(total), weight_total=t["T"])

    def faces_of(self, A):
        """the face every block A [n, 4] uint32 selects: pos = hi64(r * T) with Python integers"""
        T = self.tab["T"]
        r = (A[:, 0].astype(object) << 32) | A[:, 1].astype(object)
        pos = np.array([(int(x) * T) >> 64 for x in r], np.uint64)
        return np.searchsorted(self.tab["C"], pos, side="right")          # the first f with C[f] > pos

    def draw(self, A, B):
        """poses (TRANSFORM [n]) and faces of the blocks A, B [n, 4] uint32"""
        p = self.p
        f = self.faces_of(A)
        r = self.tris[self.tab["rec"][f]].view(F)
        v0, e1, e2, nrm = (r[:, k:k + 3] for k in (0, 3, 6, 12))
        u = (A[:, 2].astype(np.float64) + 0.5) * (1.0 / TWO32)
        v = (A[:, 3].astype(np.float64) + 0.5) * (1.0 / TWO32)
        refl = u + v > 1.0
        u, v = np.where(refl, 1.0 - u, u), np.where(refl, 1.0 - v, v)
        pt = [((v0[:, d].astype(np.float64) - u * e1[:, d].astype(np.float64)) + v * e2[:, d].astype(np.float64)).astype(F) for d in range(3)]
        uy = (B[:, 0].astype(np.float64) + 0.5) * (1.0 / TWO32)
        yaw = (np.float64(p["yaw_min"]) + (np.float64(p["yaw_max"]) - np.float64(p["yaw_min"])) * uy).astype(F)
        flip = nrm[:, 2] < 0
        n = tuple(np.where(flip, -nrm[:, d], nrm[:, d]).astype(F) for d in range(3))
        zero = np.zeros(len(f), F)
        R = pir.euler_to_quat(zero, zero, yaw)
        a = (zero, zero, np.ones(len(f), F))
        self.last_half_turn = np.zeros(len(f), bool)
        if p["align"]:
            R, self.last_half_turn = align(R, n)
            a = n
        t = tuple((pt[d] + p["height"] * a[d]).astype(F) for d in range(3))
        return pir._poses(R, t), f


def _blocks(index, second, draw, stream, seed):
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    ctr = np.zeros((len(index), 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = index, np.uint32(second), draw, stream
    return pir.philox4x32_10(ctr, key)


def _indices(first, count):
    return (np.arange(count, dtype=np.uint64) + np.uint64(first)).astype(np.uint32)


def init_surface(sampler, first, count, seed, epoch=0, with_faces=False):
    """(poses, attrs) of global particles first .. first+count-1: blocks (i, epoch, 2, 1) and (i, epoch, 3, 1)"""
    i = _indices(first, count)
    poses, f = sampler.draw(_blocks(i, epoch, 2, 1, seed), _blocks(i, epoch, 3, 1, seed))
    return (poses, pir._attrs(count), f) if with_faces else (poses, pir._attrs(count))


def inject_threshold(p_inject):
    if not (p_inject >= 0.0 and p_inject <= 1.0):
        raise ValueError("p_inject")
    return int(math.floor(p_inject * TWO32))


def inject_mask(first, count, p_inject, seed, step):
    """slot first + k is replaced iff philox((j, step, 9, 0))[0] < floor(p * 2^32), compared in 64 bits"""
    thr = inject_threshold(p_inject)
    return _blocks(_indices(first, count), step, 9, 0, seed)[:, 0].astype(np.uint64) < np.uint64(thr) if thr < 2 ** 32 else np.ones(count, bool)


def inject(sampler, poses, attrs, first, p_inject, seed, step):
    """(poses', attrs', mask) of rmclhip_particles_inject_surface on elements first .. first+len-1 of a cloud; inputs untouched"""
    poses, attrs = poses.copy(), attrs.copy()
    mask = inject_mask(first, len(poses), p_inject, seed, step)
    if mask.any():
        j = _indices(first, len(poses))[mask]
        fresh, _ = sampler.draw(_blocks(j, step, 10, 0, seed), _blocks(j, step, 11, 0, seed))
        poses[mask] = fresh
        attrs[mask] = pir._attrs(int(mask.sum()))
    return poses, attrs, mask


def recovery_params(alpha_slow=0.001, alpha_fast=0.1, p_max=1.0):
    return dict(alpha_slow=float(alpha_slow), alpha_fast=float(alpha_fast), p_max=float(p_max))


def recovery_update(state, prm, likelihood_sum, n):
    """state: [w_slow, w_fast] (updated in place); returns p_inject; raises ValueError for a refusal (state untouched)"""
    a_s, a_f, p_max = prm["alpha_slow"], prm["alpha_fast"], prm["p_max"]
    if not (0.0 < a_s <= 1.0) or not (0.0 < a_f <= 1.0) or a_s > a_f or not (0.0 <= p_max <= 1.0) or n == 0:
        raise ValueError("recovery parameters")
    if not math.isfinite(likelihood_sum) or likelihood_sum < 0.0:
        raise ValueError("likelihood sum")
    avg = float(likelihood_sum) / float(n)
    state[0] = avg if state[0] == 0.0 else state[0] + a_s * (avg - state[0])
    state[1] = avg if state[1] == 0.0 else state[1] + a_f * (avg - state[1])
    p = 0.0
    if state[0] > 0.0:
        p = 1.0 - state[1] / state[0]
        if not p > 0.0:
            p = 0.0
        if p > p_max:
            p = p_max
    return p


def recovery_reset(state):
    state[0] = state[1] = 0.0


def pose_bytes(poses):
    return np.ascontiguousarray(poses, TRANSFORM).view(np.uint8).reshape(len(poses), 32)
