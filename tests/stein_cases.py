"""Every cloud of the Stein step's edge tests (tests/test_gpu_stein_edges.py), made deterministically from fixed seeds -- and proved
non-vacuous without a device by tests/test_stein_cases_cpu.py, which asserts each cloud's premise on the restatement
(tests/stein_ref.py) with a lattice of exact oracle distances.

The world is room30k at cell 0.4, margin 0.5 (the one of tests/test_gpu_stein.py) unless a case says otherwise; the bins are those of
the default h_trans (0.25 m, width 0.25025 m).

  tilted clouds      rotations that differ about all three world axes: e[3], e[4] and the repulsion sums R[3], R[4] are not zero
  flipped            the same cloud with some quaternions negated: the product's w < 0 in a pair's either direction
  clustered clouds   32 .. 64 occupied bins spread over every 1024-word block of the prefix sum over the table
  full clouds        the fullest tables there are: n = 32 in 64 words, n = 512 in 1024
  row cloud          six adjacent bins of 130, 70, 10, 64, 65 and 1 particles: thinned bins beside unthinned ones, caps at, below
                     and above a bin's count, the 130 contiguous in index (one wave's add crosses the cap from 0) or interleaved
  collision cloud    six bins whose keys start at words 62 and 63 of a 64-word table: the probe chain wraps to word 0
  hard maps          field_cases' floor (rank three) and degcube

Not a test module."""
import itertools

import numpy as np

import field_cases as fc
import refine_ref as rr
import stein_ref as sr

F = np.float32
D = np.float64
PLANAR = 0b100011
ROOM_CELL, ROOM_MARGIN = 0.4, 0.5
SEED64 = (0x9E3779B9 << 32) | 11         # a key whose high word is not zero


def room_truth():
    """[1] TRANSFORM: where room30k's scan is taken from (tests/test_gpu_stein.py's)"""
    from rmcl_amd import types as T
    return np.array([T.transform_from_rpy((1.0, -1.5, 1.2), (0.0, 0.0, 0.5))]).reshape(1)


def room_scan(mesh):
    """(truth [1], Tsb, the oracle's spherical scan from the truth): sample the beams from it with ra.sample_beams(cloud, n, seed=7)"""
    from rmcl_amd import synthetic as syn
    truth, Tsb = room_truth(), syn.tsb_offset()
    return truth, Tsb, mesh.simulate_spherical(syn.model_c1(), Tsb, truth[0], bvh=True)["points"]


# ---- small tools -------------------------------------------------------------------------------------------------------------------------
def set_rotations(poses, R):
    for i, k in enumerate("xyzw"):
        poses["R"][k] = R[:, i]
    return poses


def set_translations(poses, t):
    for i, k in enumerate("xyz"):
        poses["t"][k] = np.asarray(t)[:, i].astype(F)
    return poses


def rotvec_quat(v):
    """rotation vectors [n, 3] float64 -> quaternions [n, 4] (x, y, z, w) float32"""
    v = np.asarray(v, D)
    ang = np.sqrt((v * v).sum(axis=1))
    k = np.where(ang > 0, np.sin(0.5 * ang) / np.where(ang > 0, ang, 1.0), 0.5)
    return np.concatenate([v * k[:, None], np.cos(0.5 * ang)[:, None]], axis=1).astype(F)


def tilt(poses, seed, d_rot):
    """every rotation left-multiplied by the quaternion of a uniform rotation vector in +-d_rot per world axis, normalised"""
    R, _ = rr.pose_arrays(poses)
    v = np.random.RandomState(seed).uniform(-d_rot, d_rot, (len(R), 3))
    return set_rotations(poses, rr.qnormalise(rr.qmul(rotvec_quat(v), R)))


def bin_of(truth, p):
    """(bin index [3] of truth's translation as float64, the bins' width as float64)"""
    _, t0 = rr.pose_arrays(truth)
    width = D(sr.bin_width(p))
    return np.floor(t0[0].astype(D) / width), width


def negate_rotations(poses, idx):
    out = poses.copy()
    for k in "xyzw":
        out["R"][k][idx] = -out["R"][k][idx]
    return out


# ---- 1. tilted clouds ----------------------------------------------------------------------------------------------------------------------
N_TILTED = (1, 2, 64, 65, 257)
TILTED_DENSE = dict(seed=51, d_trans=0.3, d_rot=0.06)      # most pairs are in each other's reach
TILTED_SPREAD = dict(seed=52, d_trans=2.0, d_rot=0.5)      # loners, most bins hold one particle


def tilted_cloud(truth, n, seed, d_trans, d_rot):
    """refine_ref.perturbed_starts without yaw, then tilted about all three world axes.  A prefix of the cloud of n is the cloud of
    the prefix's length."""
    return tilt(rr.perturbed_starts(truth, n, seed, d_trans=d_trans, d_yaw=0.0), seed + 1000, d_rot)


def tilted(truth, kind, n=257):
    return tilted_cloud(truth, n, **(TILTED_DENSE if kind == "dense" else TILTED_SPREAD))


# 1b: every odd particle and two even ones: pairs of one negated and one plain quaternion in either direction, pairs of two negated
FLIP_EXTRA = (0, 100)


def flipped_indices(n):
    return np.array(sorted(set(range(1, n, 2)) | set(i for i in FLIP_EXTRA if i < n)))


def product_w(poses):
    """w of q_j * conj(q_i), [i, j] float32, as the pair sums compute it"""
    R, _ = rr.pose_arrays(poses)
    n = len(R)
    conj = R * np.array([-1, -1, -1, 1], F)
    return rr.qmul(np.broadcast_to(R[None, :, :], (n, n, 4)), np.broadcast_to(conj[:, None, :], (n, n, 4)))[..., 3]


# ---- 2. many bins across the blocks of the prefix sum -------------------------------------------------------------------------------------
N_CLUSTERED = (513, 1025)            # 2048 words: 2 blocks of 1024; 4096 words: 4 blocks
N_CLUSTERS = 64
N_FULL = (32, 512)                   # exactly 2 n words: 64 and 1024
FULL = dict(seed=53, d_trans=2.0, d_rot=0.5)


def clustered_cloud(truth, n, seed=54, n_clusters=N_CLUSTERS, span=3.0, d_rot=0.05):
    """n particles in n_clusters clusters over +-span metres around truth: every cluster in a bin of its own, its centre within 0.22 of
    a bin of the bin's centre and its members within 0.2 of a bin of that (0.08 of a bin from every edge), particle i in cluster
    i mod n_clusters; rotations tilted by +-d_rot"""
    p = sr.params()
    b0, width = bin_of(truth, p)
    rng = np.random.RandomState(seed)
    reach = int(span / width) - 1                  # the bin's far edge stays within span of truth's bin
    offs = []
    while len(offs) < n_clusters:
        o = tuple(rng.randint(-reach, reach + 1, 3))
        if o not in offs:
            offs.append(o)
    centre = np.array(offs, D) + 0.5 + rng.uniform(-0.22, 0.22, (n_clusters, 3))
    member = np.arange(n) % n_clusters
    t = (b0 + centre[member] + rng.uniform(-0.2, 0.2, (n, 3))) * width
    poses = set_translations(rr.perturbed_starts(truth, n, seed, d_trans=0.0, d_yaw=0.0), t)
    return tilt(poses, seed + 1000, d_rot)


def full_cloud(truth, n):
    """spread_cloud's placement (+-2 m), tilted: nearly every particle in a bin of its own, in a table of exactly 2 n words"""
    assert sr.table_words(n) == 2 * n
    return tilted_cloud(truth, n, **FULL)


def occupied_per_block(poses, p):
    """how many occupied words each 1024-word block of the cloud's table holds"""
    words, occupied, _, _ = sr.table_of(poses, p)
    per = np.zeros(max(1, words // 1024), np.int64)
    for s in occupied:
        per[s >> 10] += 1
    return per


# ---- 3. several thinned bins --------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (130, 70, 10, 64, 65, 1)
ROW_OFFSETS = (-2, -1, 0, 1, 2, 3)                 # along x; truth's own bin is the third
ROW_CAPS = (1, 2, 63, 64, 65, 0xFFFFFFFF)
ROW_THINNED = (5, 5, 4, 3, 2, 0)                   # the counts above each cap
# the step at which, in both orderings and for every cap, each thinned bin lists somebody (found by search over 0, 1, 2, ...;
# tests/test_stein_cases_cpu.py asserts it)
ROW_STEP = 3
ROW_PERM_SEED = 7


def row_cloud(truth, interleaved=False, seed=55):
    """sum(ROW_COUNTS) = 340 particles in six adjacent bins along x around truth's bin, uniformly within +-0.45 of a bin of each bin's
    centre, rotations tilted by +-0.05.  Bin after bin in index (the first wave of 64 lies in the bin of 130, so its one add takes the
    count from 0 past a cap below 64), or, interleaved, the same particles under a fixed permutation (a later wave crosses the cap)."""
    p = sr.params()
    b0, width = bin_of(truth, p)
    n = sum(ROW_COUNTS)
    rng = np.random.RandomState(seed)
    which = np.repeat(np.arange(6), ROW_COUNTS)
    centre = b0[None, :] + 0.5 + np.stack([np.array(ROW_OFFSETS, D)[which], np.zeros(n), np.zeros(n)], axis=1)
    t = (centre + rng.uniform(-0.45, 0.45, (n, 3))) * width
    poses = tilt(set_translations(rr.perturbed_starts(truth, n, seed, d_trans=0.0, d_yaw=0.0), t), seed + 1000, 0.05)
    return poses[row_permutation()] if interleaved else poses


def row_permutation():
    return np.random.RandomState(ROW_PERM_SEED).permutation(sum(ROW_COUNTS))


def row_params(cap, **kw):
    return sr.params(**dict(dict(max_per_bin=cap, seed=SEED64, step=ROW_STEP), **kw))


def row_bins(poses, p, it=0):
    """the row's bins in x order: (count, listed) of each, at these poses"""
    R, t = rr.pose_arrays(poses)
    finite = np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    b, count, listed, listed_b = sr.cell_list(t, finite, p, it)[:4]
    out = {}
    for i in range(len(t)):
        out[int(b[i, 0])] = (int(count[i]), int(listed_b[i]))
    return [out[k] for k in sorted(out)]


# ---- 5. masks ----------------------------------------------------------------------------------------------------------------------------
MASKS = (0x00, 0x38, 0x01, 0x04, 0x24, 0x1F)


def mask_params(mask):
    """two iterations at the default cap of 256 on tilted-dense's 257: with the translations locked everybody shares one bin, and under
    this key the thinning lists 256 of them in the first iteration and 253 in the second"""
    return sr.params(iterations=2, dof_mask=mask, seed=SEED64, step=0)


# ---- 6. chosen collisions ----------------------------------------------------------------------------------------------------------------
N_COLLIDING_BINS, N_LONERS = 6, 6


def colliding_bins(truth, words=64, reach=10):
    """six bins within +-reach of truth's whose keys' home slots are the table's last two words, nearest first, one of them with the
    last word but one as its home: [(bin index [3] int, home slot)]"""
    b0, _ = bin_of(truth, sr.params())
    found = []
    for d in itertools.product(range(-reach, reach + 1), repeat=3):
        b = tuple(int(b0[k]) + d[k] for k in range(3))
        home = sr.mix64(sr.bin_key(b)) & (words - 1)
        if home >= words - 2:
            found.append((max(abs(x) for x in d), sum(abs(x) for x in d), d, b, home))
    found.sort()
    first = next(f for f in found if f[4] == words - 2)
    rest = [f for f in found if f is not first][:N_COLLIDING_BINS - 1]
    return [(f[3], f[4]) for f in [first] + rest]


def collision_cloud(truth, seed=56):
    """three particles in each of colliding_bins (within 0.1 of a bin of its centre, tilted by +-0.02: mutual neighbours), bin after
    bin, then six loners 3.5 m and more away: 24 particles, a table of 64 words"""
    p = sr.params()
    _, width = bin_of(truth, p)
    _, t0 = rr.pose_arrays(truth)
    rng = np.random.RandomState(seed)
    centre = np.repeat(np.array([b for b, _ in colliding_bins(truth)], D) + 0.5, 3, axis=0)
    t = (centre + rng.uniform(-0.1, 0.1, centre.shape)) * width
    lone = t0[0].astype(D)[None, :] + np.array([(3.5 + 0.6 * i, -3.5 - 0.4 * i, 0.3) for i in range(N_LONERS)])
    t = np.concatenate([t, lone])
    poses = set_translations(rr.perturbed_starts(truth, len(t), seed, d_trans=0.0, d_yaw=0.0), t)
    return tilt(poses, seed + 1000, 0.02)


# ---- 8. hard maps --------------------------------------------------------------------------------------------------------------------------
HARD_MAPS = ("floor", "degcube")
HARD = dict(seed=57, d_trans=0.3, d_rot=0.06)
N_HARD = 65


def hard_case(ra, orc, name):
    """(truth [1], Tsb, beams, 65 tilted poses around the truth, the keywords of stein_ref.params): field_cases.refine_case's truth,
    beams and max_dist on the map's cell and margin (field_cases.cell_margin)"""
    truth, Tsb, beams, _, rp = fc.refine_case(ra, orc, name)
    return truth, Tsb, beams, tilted_cloud(truth, N_HARD, **HARD), dict(max_dist=rp["max_dist"])


# ---- what a test prints about a case ------------------------------------------------------------------------------------------------------
def describe(what, rows, st):
    nb = rows["n_neighbours"]
    return "[stein-edges] %s: n %d, %d bins (%d thinned), neighbours min %d median %d max %d" % (
        what, len(nb), st["n_bins"], st["n_thinned_bins"], nb.min(), np.median(nb), nb.max())
