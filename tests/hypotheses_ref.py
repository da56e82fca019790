"""Host restatement (numpy + Python ints) of the pose hypotheses -- what rmcl_amd/csrc/hypotheses.hip and capi_hypotheses.cpp compute
(include/rmclhip.h, POSE HYPOTHESES, states the rules):

    pack_keys            the 63-bit key of a bin tuple, as the kernel packs it
    last_index           the index the bin rule gives the angle pi_f
    adjacent             the adjacency rule on two bin tuples (what the components are defined by; the search below enumerates it)
    hypotheses           components by a plain union-find over a dict of keys, exact per-cluster sums in Python ints, the ranking,
                         the labels, and every hypothesis's estimate from pf_cycle_cases.estimate_ref on its members in index order
and the clouds the CPU and the GPU tests share (at_bins and the case builders).  Bin tuples, the counted mask, the integer weights and
the likelihood maximum are adaptive_ref's.
"""
import itertools
import math

import numpy as np

import adaptive_ref as ar
import pf_cycle_cases as pc
from particle_init_ref import euler_to_quat
from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM

f32 = np.float32
NONE = 0xFFFFFFFF
SHIFTS = (0, 14, 28, 42, 49, 56)
FIELD_MAX = (16383, 16383, 16383, 126, 126, 126)
WRAPS = (False, False, False, True, False, True)          # roll and yaw
DEFAULT_WIDTHS = (0.5, 0.5, 0.5, 0.17453292, 0.17453292, 0.17453292)
BASE = (3, -2, 1, 18, 17, 5)                              # a bin well inside every range (pitch index 17: -0.09 rad)


def pack_keys(tup):
    """[m, 6] int bin tuples -> list of Python ints"""
    t = np.asarray(tup, dtype=np.int64).reshape(-1, 6)
    return [((int(r[0]) + 8192) | ((int(r[1]) + 8192) << 14) | ((int(r[2]) + 8192) << 28) | (int(r[3]) << 42) | (int(r[4]) << 49) | (int(r[5]) << 56))
            for r in t]


def unpack_key(key):
    """key -> the six field values as the key stores them (x, y, z with their offset of 8192)"""
    return tuple((key >> s) & (0x3FFF if d < 3 else 0x7F) for d, s in enumerate(SHIFTS))


def last_index(width):
    """bin_ang(3.14159265f, width): floor((pi_f + pi_f) / width) in float32, clamped to [0, 126]; 0 for an ignored dimension"""
    width = f32(width)
    if width == 0:
        return 0
    return int(min(max(np.floor((f32(3.14159265) + ar.PI_F) / width), f32(0.0)), f32(126.0)))


def _widths(p):
    return [f32(w) for w in list(p.bin_xyz) + list(p.bin_rpy)]


def adjacent(a, b, p):
    """the rule itself, on two stored field tuples (unpack_key)"""
    for d, w in enumerate(_widths(p)):
        i, j = a[d], b[d]
        if abs(i - j) <= 1:
            continue
        if WRAPS[d] and w != 0 and min(i, j) == 0 and max(i, j) >= last_index(w) - 1:
            continue
        return False
    return True


def _field_candidates(i, d, width):
    if width == 0:
        return [i]
    c = {i - 1, i, i + 1}
    if WRAPS[d]:
        last = last_index(width)
        if i == 0:
            c |= {last - 1, last}
        if i >= last - 1:
            c.add(0)
    return sorted(v for v in c if 0 <= v <= FIELD_MAX[d])


def components(keys, p):
    """keys: iterable of distinct Python ints -> {key: key_min of its component}"""
    widths = _widths(p)
    parent = {k: k for k in keys}

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    for k in list(parent):
        f = unpack_key(k)
        cands = [[v << SHIFTS[d] for v in _field_candidates(f[d], d, widths[d])] for d in range(6)]
        for combo in itertools.product(*cands):
            nk = combo[0] | combo[1] | combo[2] | combo[3] | combo[4] | combo[5]
            if nk > k and nk in parent:
                a, b = find(k), find(nk)
                if a != b:
                    parent[max(a, b)] = min(a, b)          # the smaller key wins: a root is its component's key_min
    return {k: find(k) for k in parent}


def hypotheses(poses, attrs, p, max_hypotheses=8, estimates=True):
    """-> {"n_clusters", "hypotheses": [{key_min, weight, weight_share, n_bins, nparticles, members, + estimate_ref's fields}], "labels",
    "clusters": every cluster's (key_min, weight, n_bins, n_particles) in rank order, "total"}"""
    n = len(poses)
    labels = np.full(n, NONE, dtype=np.uint32)
    empty = {"n_clusters": 0, "hypotheses": [], "labels": labels, "clusters": [], "total": 0}
    if n == 0:
        return empty
    max_l = ar.likelihood_max(attrs)
    if not (max_l > 0 and math.isfinite(max_l)):
        return empty
    counted, tup = ar.bin_tuples(poses, attrs, p, max_l)
    if not counted.any():
        return empty
    members_idx = np.flatnonzero(counted)
    keys = pack_keys(tup[counted])
    w = ar.sys_weights(attrs["likelihood"]["mean"][counted], max_l)
    root_of = components(set(keys), p)
    clusters = {}
    for i, k, wi in zip(members_idx, keys, w):
        c = clusters.setdefault(root_of[k], {"weight": 0, "bins": set(), "members": []})
        c["weight"] += wi
        c["bins"].add(k)
        c["members"].append(int(i))
    total = sum(w)
    order = sorted(clusters, key=lambda r: (-clusters[r]["weight"], r))
    out = []
    for rank, r in enumerate(order[:max_hypotheses]):
        c = clusters[r]
        m = np.array(c["members"], dtype=np.int64)
        labels[m] = rank
        h = {"key_min": r, "weight": c["weight"], "weight_share": float(c["weight"]) / float(total), "n_bins": len(c["bins"]), "members": m}
        if estimates:
            h.update(pc.estimate_ref(poses[m], attrs[m]))
        else:
            h["nparticles"] = len(m)
        out.append(h)
    return {"n_clusters": len(order), "hypotheses": out, "labels": labels, "total": total,
            "clusters": [(r, clusters[r]["weight"], len(clusters[r]["bins"]), len(clusters[r]["members"])) for r in order]}


# ---- the clouds the tests share ---------------------------------------------------------------------------------------------------
def at_bins(idx, seed, widths=DEFAULT_WIDTHS):
    """particles at the centres of the bins idx [n, 6] plus a jitter of at most 0.3 bin per dimension; likelihoods 1"""
    idx = np.asarray(idx, dtype=np.float64).reshape(-1, 6)
    n = len(idx)
    jit = np.random.RandomState(seed).uniform(-0.3, 0.3, size=(n, 6))
    w = np.asarray(widths, dtype=np.float64)
    c = (idx + 0.5 + jit) * np.where(w == 0, 1.0, w)[None, :]
    c[:, 3:] -= math.pi
    c[:, w == 0] = 0.0                                      # an ignored dimension: any value would do
    assert n == 0 or np.abs(c[:, 4]).max() <= 1.2          # pitch stays away from the poles: it never reaches index 0 or `last`
    c = c.astype(f32)
    p = np.zeros(n, dtype=TRANSFORM)
    for k, q in zip("xyzw", euler_to_quat(c[:, 3], c[:, 4], c[:, 5])):
        p["R"][k] = q
    for d, k in enumerate("xyz"):
        p["t"][k] = c[:, d]
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = 1.0
    return p, a


def rep(n, rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    return rows[np.arange(n) % len(rows)]


def kld(widths=DEFAULT_WIDTHS, min_likelihood_rel=0.01):
    return ar.Kld(bin_xyz=widths[:3], bin_rpy=widths[3:], min_likelihood_rel=min_likelihood_rel)


def assert_margin(poses, attrs, p, exact=None):
    """no counted particle lies closer than 0.19 bin to an edge -- an ulp between the device's and numpy's atan2 cannot move it.
    exact: mask of particles left out: their quaternions are (0, 0, 1, 0) or (1, 0, 0, 0), whose Euler angles are atan2(0, +-1) and
    asin(0) -- exact on both sides, so their bins are the same float divisions wherever they are taken."""
    keep = np.ones(len(poses), bool) if exact is None else ~np.asarray(exact, bool)
    if keep.any():
        max_l = ar.likelihood_max(attrs)
        assert ar.bin_margin(poses[keep], attrs[keep], p, max_l) >= 0.19


def blob(lo, hi):
    """every bin tuple of the box lo .. hi (inclusive, six fields)"""
    return np.array(list(itertools.product(*[range(a, b + 1) for a, b in zip(lo, hi)])), dtype=np.int64)


def two_blobs(n, seed=40):
    """two 3 x 3 x 1 blobs over the same x, y with ONE empty bin between them along z; two thirds of the particles in the upper one.
    The weighted mean of all particles lies a third of the way from the heavy blob's centre to the light one's: 1/3 m in z, outside the
    half-bin (0.25 m) either blob extends from its centre.
    -> poses, attrs, params, (box of the light blob, box of the heavy blob) as (lo xyz, hi xyz) in metres"""
    a = blob((0, -3, 1, 18, 17, 5), (2, -1, 1, 18, 17, 5))
    b = blob((0, -3, 3, 18, 17, 5), (2, -1, 3, 18, 17, 5))
    heavy = (np.arange(n) % 3) != 0
    hi, li = np.cumsum(heavy) - 1, np.cumsum(~heavy) - 1
    rows = np.where(heavy[:, None], b[hi % len(b)], a[li % len(a)])
    poses, attrs = at_bins(rows, seed)
    boxes = (((0.0, -1.5, 0.5), (1.5, 0.0, 1.0)), ((0.0, -1.5, 1.5), (1.5, 0.0, 2.0)))
    return poses, attrs, kld(), boxes


def exact_pi_particle(field):
    """one particle whose roll (field 3) or yaw (field 5) is exactly +pi_f; everything else zero"""
    p = np.zeros(1, dtype=TRANSFORM)
    p["R"]["x" if field == 3 else "z"] = 1.0
    a = np.zeros(1, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = 1.0
    return p, a


def wrap_case(n, field, width, indices, with_pi, seed=50):
    """a blob over the given indices of the wrapping field (3: roll, 5: yaw), every other field in the bin the exact +pi particle falls
    into; with_pi appends that particle.  -> poses, attrs, params, exact mask"""
    widths = (0.5, 0.5, 0.5, width, width, width)
    p = kld(widths)
    ep, ea = exact_pi_particle(field)
    _, tup = ar.bin_tuples(ep, ea, p)
    base = [int(v) for v in tup[0]]
    assert base[field] == last_index(width) and base[4] not in (0, last_index(width))
    rows = rep(n, [base])
    rows[:, field] = np.asarray(indices)[np.arange(n) % len(indices)]
    poses, attrs = at_bins(rows, seed, widths)
    exact = np.zeros(n, bool)
    if with_pi:
        poses, attrs = np.concatenate([poses, ep]), np.concatenate([attrs, ea])
        exact = np.concatenate([exact, [True]])
    return poses, attrs, p, exact


def chain_rows(shape, n=2000):
    """n bins, one after the other: a line along x, or an L-shaped snake in x-y (half along x, then along y)"""
    rows = rep(n, [BASE])
    i = np.arange(n)
    if shape == "line":
        rows[:, 0] = i - n // 2
    else:
        h = n // 2
        rows[:, 0] = np.minimum(i, h - 1) - h // 2
        rows[:, 1] = np.maximum(i - (h - 1), 0) - 2
    return rows


def isolated_grid_rows(n=4096):
    """every bin on a stride-2 grid in x and y: no two are neighbours"""
    rows = rep(n, [BASE])
    i = np.arange(n)
    rows[:, 0], rows[:, 1] = 2 * (i % 64) - 64, 2 * (i // 64) - 64
    return rows


def five_clusters(n, seed=60):
    """five clusters along x, three bins apart, with 5 : 4 : 3 : 2 : 1 of the particles (n >= 15)"""
    rows = rep(n, [BASE])
    share = np.repeat(np.arange(5), [5, 4, 3, 2, 1])
    rows[:, 0] = 3 * share[np.arange(n) % 15] - 6
    return at_bins(rows, seed) + (kld(),)


def rnd_rows(n):
    """random bins as test_gpu_adaptive's `rnd`"""
    rs_ = np.random.RandomState(100 + n)
    return np.stack([rs_.randint(-6, 6, n), rs_.randint(-6, 6, n), rs_.randint(-2, 2, n), rs_.randint(14, 22, n), rs_.randint(14, 22, n),
                     rs_.randint(0, 36, n)], axis=1)


def rnd_cases(n):
    """name -> (poses, attrs, params): amcl_x_y_yaw and one zero bin size per dimension"""
    rnd = rnd_rows(n)
    out = {"amcl_x_y_yaw": at_bins(rnd, 11) + (ar.Kld(bin_xyz=(0.5, 0.5, 0.0), bin_rpy=(0.0, 0.0, 0.17453292)),)}
    for d in range(6):
        bx, br = [0.5] * 3, [0.17453292] * 3
        (bx if d < 3 else br)[d % 3] = 0.0
        out["zero_bin_dim_%d" % d] = at_bins(rnd, 12) + (ar.Kld(bin_xyz=bx, bin_rpy=br),)
    return out
