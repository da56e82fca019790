"""The Stein variational step on the distance field (include/rmclhip.h, STEIN STEP ON THE FIELD) restated in numpy: every operation in
the header's precision and order, vectorised over particles and pairs (element-wise numpy arithmetic rounds every operation to the
array's type, which is the header's "unfused").  The pass, the solve, the limit and the candidate are refine_ref's; the random word is
the resamplers' stream (adaptive_ref).  step(..., brute=True) sums over ALL pairs instead of the adjacent bins: with max_per_bin >= n
the two are the same bytes, which is the proof in numbers that the cell list covers the kernel's support.  The table of occupied bins
(mix64, bin_key, table_words, table_slots) is restated too: where a cloud's bins land decides which words and scan blocks a case
reaches (tests/stein_cases.py).  Not a test module.
"""
import numpy as np

import adaptive_ref as ar
import refine_ref as rr

F = np.float32
D = np.float64
I64 = np.int64
MAX_PARTICLES = 1 << 26
RESULT = np.dtype([("cost", np.float32), ("n_used", np.uint32), ("n_neighbours", np.uint32), ("kernel_weight", np.float32)])

# every parameter refusal: what rmclhip_pf_stein_step answers with RMCLHIP_ERR_INVALID and check() with ValueError
BAD_PARAMS = list(rr.BAD_PARAMS) + [dict(max_step_trans=16.5), dict(max_step_rot=17.0), dict(max_per_bin=0)] + \
    [{k: bad} for k in ("h_trans", "h_rot") for bad in (0.0, -1.0, float("nan"), float("inf"))] + \
    [dict(repulsion=bad) for bad in (-0.5, float("nan"), float("inf"))]


def params(iterations=1, dof_mask=0x3F, max_dist=0.5, max_step_trans=0.5, max_step_rot=0.25, lambda0=1e-3, h_trans=0.25, h_rot=0.2,
           repulsion=0.25, max_per_bin=256, seed=0, step=0):
    """rmclhip_stein_params with the defaults of rmclhip_stein_params_default"""
    p = rr.params(iterations, dof_mask, max_dist, max_step_trans, max_step_rot, lambda0)
    p.update(h_trans=F(h_trans), h_rot=F(h_rot), repulsion=F(repulsion), max_per_bin=int(max_per_bin), seed=int(seed), step=int(step))
    return p


def check(p, n_particles, n_beams):
    """the refusals of rmclhip_pf_stein_step that concern neither pointers nor the field: ValueError where the library returns
    RMCLHIP_ERR_INVALID"""
    rr.check(p, 0, 0)
    for k in ("max_step_trans", "max_step_rot"):
        if not p[k] <= 16:
            raise ValueError(k)
    for k in ("h_trans", "h_rot"):
        if not (np.isfinite(p[k]) and p[k] > 0):
            raise ValueError(k)
    if not (np.isfinite(p["repulsion"]) and p["repulsion"] >= 0):
        raise ValueError("repulsion")
    if not 1 <= p["max_per_bin"] <= 0xFFFFFFFF:
        raise ValueError("max_per_bin")
    if n_particles > MAX_PARTICLES:
        raise ValueError("n_particles")
    rr.check(p, n_particles, n_beams)


# ---- the cell list ---------------------------------------------------------------------------------------------------------------------
def bin_width(p):
    return F(F(1.001) * p["h_trans"])


def _coords(t, p):
    """raw bin coordinates [n, 3] float32: t_k / width on the free axes, 0 on a locked one"""
    mask, width = p["dof_mask"] & 0x3F, bin_width(p)
    c = np.zeros(t.shape, F)
    with np.errstate(all="ignore"):
        for k in range(3):
            if (mask >> k) & 1:
                c[:, k] = t[:, k] / width
    return c


def bins(t, p):
    """[n, 3] int64: the translation bin of BINS on the free axes (floor clamped to -8192 .. 8191), 0 on a locked one"""
    with np.errstate(all="ignore"):
        return np.minimum(np.maximum(np.floor(_coords(t, p)), F(-8192.0)), F(8191.0)).astype(I64)


def bin_margin(poses, p):
    """smallest distance, in bins, of a finite-pose particle's free coordinate to an edge that separates two bin indices"""
    R, t = rr.pose_arrays(poses)
    fin = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    c = _coords(t[fin], p).astype(D)
    frac = c - np.floor(c)
    inside = np.minimum(frac, 1.0 - frac)
    outside = np.where(c < -8192.0, -8192.0 - c, c - 8192.0)
    m = np.where((c >= -8192.0) & (c < 8192.0), inside, outside)
    free = np.array([bool((p["dof_mask"] >> k) & 1) for k in range(3)])
    return float(m[:, free].min()) if m[:, free].size else 1.0


def cell_list(t, finite, p, it):
    """(bin index [n, 3], count_B of every particle's bin [n], listed [n] bool, listed_B of every particle's bin [n], n_bins,
    n_thinned_bins); particles that are not finite are in no bin"""
    n = len(t)
    b = bins(np.where(finite[:, None], t, F(0)), p)
    count, listed_b = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    listed = np.zeros(n, bool)
    n_bins = n_thinned = 0
    if finite.any():
        uniq, inv, cnt = np.unique(b[finite], axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        count[finite] = cnt[inv]
        r = ar._words(np.arange(n, dtype=np.uint32), (p["step"] + it) & 0xFFFFFFFF, 8, p["seed"])[:, 0].astype(np.uint64)
        cap = np.uint64(p["max_per_bin"])
        listed = finite & ((count <= cap) | (r * count < (cap << np.uint64(32))))
        per_bin = np.bincount(inv, weights=listed[finite].astype(D), minlength=len(uniq)).astype(np.uint64)
        listed_b[finite] = per_bin[inv]
        n_bins, n_thinned = len(uniq), int((cnt > p["max_per_bin"]).sum())
    return b, count, listed, listed_b, n_bins, n_thinned


# ---- the table of occupied bins (kld_bins.hip.h, k_stein_insert): where bins land -------------------------------------------------------
_M64 = (1 << 64) - 1


def mix64(x):
    """splitmix64's finaliser on a Python int, as kld_bins.hip.h's mix64"""
    x &= _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def table_words(n):
    """kld_table_words: the power of two >= max(64, 2 n)"""
    words = 64
    while words < 2 * n:
        words <<= 1
    return words


def bin_key(b):
    """the 42-bit key of a bin index (bx, by, bz) as bins() gives it (0 on a locked axis): index + 8192 in 14 bits each, x | y << 14 |
    z << 28, so a locked axis holds 8192"""
    bx, by, bz = (int(v) + 8192 for v in b)
    assert 0 <= bx <= 16383 and 0 <= by <= 16383 and 0 <= bz <= 16383
    return bx | (by << 14) | (bz << 28)


def table_slots(keys, words):
    """linear probing from mix64(key) & (words - 1) over `words` words, the distinct keys inserted in the order given:
    (occupied slots (a set), {key: home slot}, {key: the slot it is stored at in THIS order}).  The occupied set -- and the sum of the
    displacements -- is the same for every insertion order; which key sits where inside a run is the order's (on the device: the
    atomics')."""
    assert words >= 64 and words & (words - 1) == 0
    stored, home, used = {}, {}, {}
    for key in keys:
        key = int(key)
        if key in stored:
            continue
        assert len(stored) < words
        home[key] = sl = mix64(key) & (words - 1)
        while sl in used:
            sl = (sl + 1) & (words - 1)
        used[sl] = key
        stored[key] = sl
    return set(used), home, stored


def table_of(poses, p):
    """table_slots of a cloud's finite-pose particles in index order, in the table of len(poses) particles: (words, occupied, home,
    stored)"""
    R, t = rr.pose_arrays(poses)
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    words = table_words(len(R))
    return (words,) + table_slots([bin_key(b) for b in bins(t[finite], p)], words)


# ---- the sums and the move ---------------------------------------------------------------------------------------------------------------
def quantise(x, counts):
    """Q(x) = int64(rint(double(x) * 2^32)) where `counts`, 0 elsewhere"""
    with np.errstate(all="ignore"):
        return np.rint(np.where(counts, x, F(0)).astype(D) * 4294967296.0).astype(I64)


def limit(delta, p):
    """refine's length limit of a step [n, 6] float64"""
    with np.errstate(all="ignore"):
        nv = np.sqrt((delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]) + delta[:, 2] * delta[:, 2])
        nw = np.sqrt((delta[:, 3] * delta[:, 3] + delta[:, 4] * delta[:, 4]) + delta[:, 5] * delta[:, 5])
        scale = np.ones(len(delta), D)
        q = np.where(nv > 0.0, D(p["max_step_trans"]) / nv, np.inf)
        scale = np.where(q < scale, q, scale)
        q = np.where(nw > 0.0, D(p["max_step_rot"]) / nw, np.inf)
        scale = np.where(q < scale, q, scale)
        return delta * scale[:, None]


def drives(info, lattice, R, t, finite, Tsb, beams, p):
    """(drive [n, 6] float32, C [n] float64, n_used [n]): refine's first candidate step of every particle"""
    mask = p["dof_mask"] & 0x3F
    C, A, b, n_used = rr.evaluate(info, lattice, R, t, Tsb, beams, p)
    delta, ok = rr.solve(A, b, mask, np.full(len(R), D(p["lambda0"]), D), p)
    with np.errstate(all="ignore"):
        drive = np.where((finite & (n_used != 0) & ok)[:, None], delta.astype(F), F(0)).astype(F)
    return drive, C, n_used


def pair_terms(R, t, finite, p, it, brute=False):
    """every pair (i, j) at the poses (R, t): (e [n, n, 6], counts [n, n] bool, a [n, n], wu [n, n], the cell list's tuple); row i is
    particle i, column j its candidate neighbour"""
    n = len(R)
    mask = p["dof_mask"] & 0x3F
    free = [k for k in range(6) if (mask >> k) & 1]
    cl = cell_list(t, finite, p, it)
    b, count, listed, listed_b = cl[:4]
    with np.errstate(all="ignore"):
        w_bin = (count.astype(F) / np.where(listed_b > 0, listed_b, 1).astype(F)).astype(F)       # of particle j's bin
        cand = finite[:, None] & listed[None, :] & ~np.eye(n, dtype=bool)
        if not brute:
            cand &= (np.abs(b[:, None, :] - b[None, :, :]) <= 1).all(axis=2)
        e = np.zeros((n, n, 6), F)
        s = np.zeros((n, n), F)
        for k in range(3):
            if (mask >> k) & 1:
                e[..., k] = (t[None, :, k] - t[:, None, k]) / p["h_trans"]
        if mask & 0x38:
            conj = R * np.array([-1, -1, -1, 1], F)
            dq = rr.qmul(np.broadcast_to(R[None, :, :], (n, n, 4)), np.broadcast_to(conj[:, None, :], (n, n, 4)))
            rho = F(2.0) * dq[..., :3]
            rho = np.where((dq[..., 3] < 0)[..., None], -rho, rho)
            for k in range(3, 6):
                if (mask >> k) & 1:
                    e[..., k] = rho[..., k - 3] / p["h_rot"]
        for k in free:
            s = s + e[..., k] * e[..., k]
        counts = cand & (s < F(1.0))
        u = F(1.0) - s
        kk = u * u
        a = w_bin[None, :] * kk
        wu = w_bin[None, :] * u
    return e, counts, a, wu, cl


def iteration(info, lattice, R, t, Tsb, beams, p, it, brute=False):
    """one iteration at the poses (R, t): (R', t', rows, counts dict)"""
    n = len(R)
    mask = p["dof_mask"] & 0x3F
    free = [k for k in range(6) if (mask >> k) & 1]
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    drive, C, n_used = drives(info, lattice, R, t, finite, Tsb, beams, p)
    e, counts, a, wu, (b, count, listed, listed_b, n_bins, n_thinned) = pair_terms(R, t, finite, p, it, brute)
    with np.errstate(all="ignore"):
        W = quantise(a, counts).sum(axis=1) + (finite.astype(I64) << 32)
        Dk, Rk = np.zeros((n, 6), I64), np.zeros((n, 6), I64)
        for k in free:
            Dk[:, k] = quantise(a * drive[None, :, k], counts).sum(axis=1) + quantise(drive[:, k], finite)
            Rk[:, k] = quantise(wu * e[..., k], counts).sum(axis=1)
        phi = np.zeros((n, 6), D)
        Wd = np.where(finite, W, 1).astype(D)
        for k in free:
            c = (D(p["repulsion"]) * 4.0) * D(p["h_trans"] if k < 3 else p["h_rot"])
            phi[:, k] = (Dk[:, k].astype(D) - c * Rk[:, k].astype(D)) / Wd
        phi = limit(phi, p)
        R2, t2 = rr.candidate(R, t, phi, mask)
        R2, t2 = np.where(finite[:, None], R2, R), np.where(finite[:, None], t2, t)
        rows = np.zeros(n, RESULT)
        rows["cost"], rows["n_used"] = C.astype(F), n_used
        rows["n_neighbours"] = counts.sum(axis=1)
        rows["kernel_weight"] = (W.astype(D) * (1.0 / 4294967296.0)).astype(F)
    st = dict(n_particles=n, n_not_finite=int((~finite).sum()), n_no_beams=int((finite & (n_used == 0)).sum()), n_bins=n_bins,
              n_thinned_bins=n_thinned, listed=listed)
    return R2, t2, rows, st


def step(info, lattice, poses, beams, Tsb, p=None, brute=False):
    """rmclhip_pf_stein_step: (poses', rows [n] of RESULT, stats dict) without touching its inputs"""
    p = params() if p is None else p
    poses = np.array(poses).reshape(-1)
    n = len(poses)
    check(p, n, len(np.asarray(beams).reshape(-1)))
    rows = np.zeros(n, RESULT)
    st = dict(n_particles=n, n_not_finite=0, n_no_beams=0, n_bins=0, n_thinned_bins=0, cost_sum=0.0)
    if n == 0 or p["iterations"] == 0:
        return poses, rows, st
    R, t = rr.pose_arrays(poses)
    for it in range(p["iterations"]):
        R, t, rows, st = iteration(info, lattice, R, t, Tsb, beams, p, it, brute)
    for i, k in enumerate("xyzw"):
        poses["R"][k] = R[:, i]
    for i, k in enumerate("xyz"):
        poses["t"][k] = t[:, i]
    st.pop("listed")
    st["cost_sum"] = float(np.cumsum(rows["cost"].astype(D))[-1])
    return poses, rows, st


def listed_of(poses, p, it=0):
    """which particles the iteration `it` lists, at these poses: [n] bool"""
    R, t = rr.pose_arrays(poses)
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    return cell_list(t, finite, p, it)[2]


def pairs_of(poses, p, it=0, brute=False):
    """pair_terms of the iteration `it` at these poses"""
    R, t = rr.pose_arrays(poses)
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    return pair_terms(R, t, finite, p, it, brute)


# ---- the clouds the CPU and the GPU tests share -----------------------------------------------------------------------------------------
THINNED_N, THINNED_MAX_PER_BIN, THINNED_SEED, THINNED_STEP = 1025, 64, 11, 3


def spread_cloud(truth, n, seed):
    """n particles over +-2 m and +-1 rad of yaw around `truth`: most bins hold one particle or none"""
    return rr.perturbed_starts(truth, n, seed, d_trans=2.0, d_yaw=1.0)


def thinned_cloud(truth, p, n=THINNED_N, seed=41):
    """n particles in ONE bin of params p: uniformly within 0.4 of a bin around the centre of truth's bin, yaw +- 0.15"""
    _, t0 = rr.pose_arrays(truth)
    width = D(bin_width(p))
    centre = (np.floor(t0[0].astype(D) / width) + 0.5) * width
    poses = rr.perturbed_starts(truth, n, seed, d_trans=0.0, d_yaw=0.15)
    off = np.random.RandomState(seed + 1).uniform(-0.4, 0.4, (n, 3)) * width
    for i, k in enumerate("xyz"):
        poses["t"][k] = (centre[i] + off[:, i]).astype(F)
    return poses


def covariance_trace(poses):
    """trace of the positions' covariance, float64"""
    _, t = rr.pose_arrays(poses)
    return float(t.astype(D).var(axis=0).sum())


def build_example(tmp_path):
    """examples/stein_step_cpp_example.cpp compiled with hipcc for gfx950 against the C ABI: the executable's path"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = "stein_step_cpp_example.cpp"
    exe = str(tmp_path / source.replace(".cpp", ""))
    libdir = os.path.join(root, "rmcl_amd")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(root, "include"), os.path.join(root, "examples", source), "-L" + libdir, "-lrmclhip",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe
