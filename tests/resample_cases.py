"""Every cloud, likelihood vector and parameter set of the resamplers' edge tests (tests/test_gpu_resample_edges.py), made
deterministically from fixed seeds -- and proved non-vacuous on the CPU oracle alone by tests/test_resample_cases_cpu.py.

Tournament clouds (tournament_case): what k_gladiator_resample's comparison `Le > Lc` and its perturbation can get wrong.
    ties          one likelihood everywhere: nobody wins, the new cloud is a byte copy
    two_level     likelihoods 0.25 / 0.75: champion k is replaced exactly when it holds 0.25 and its enemy holds 0.75
    signed_zero   +0 / -0 (and a few 1e-3): no zero beats a zero of either sign
    denormal      0, 1e-45 .. 1e-39: IEEE orders them; a comparison that flushes denormals calls them all equal
    nan_inf       NaN (three payloads), +inf, -inf among ordinary values: NaN neither wins nor loses, its record is copied bit for bit
    gimbal        pitch = +-pi/2, random roll and yaw, quaternions of both signs: both sides of the `fabsf(sinp) >= 1` branch; run with
                  all-zero noise widths and with the defaults
    unnormalised  |q| = 0.5 and |q| = 2
    n_meas_edges  the n_meas values at which uint32(float(n_meas) * rate) is exact, rounds, or leaves the uint32 range, under five
                  pairs of forget rates and both trans_dist_metric values
    n<N>          cloud sizes about the wave (64), the block (256) and 1023, and 300007 for large champion indices
Every tournament case runs at step 0 and step 2^32 - 1 with SEED, whose high word is not zero.

Statistics vectors (stats_vector / STATS_CASES), residual cases (residual_case / RESIDUAL) and refused configurations
(BAD_CONFIGS) follow further down.  Positions stay within +-9 m: the bar for perturbed poses (atol 1e-6 against the oracle) keeps its
meaning.
"""
import math

import numpy as np

import oracle as orc

f32 = np.float32
SEED = 0xDEADBEEF12345                     # high word 0xDEADB
STEPS = (0, 0xFFFFFFFF)
ZERO_NOISE = dict(min_noise_tx=0.0, min_noise_ty=0.0, min_noise_tz=0.0, min_noise_roll=0.0, min_noise_pitch=0.0, min_noise_yaw=0.0)
NOISY = dict(min_noise_tz=0.01, min_noise_roll=0.005, min_noise_pitch=0.005)          # every width non-zero (with the defaults)
N_MEAS_EDGES = (0, 1, 3, 9999, 10000, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1)
GLADIATOR_FORGET = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.3, 0.2), (1e-12, 0.0))
RESIDUAL_FORGET = ((1.0, 1.0), (0.0, 1.0), (0.5, 0.5))
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 300007)
N = 3001                                   # "a few thousand", not a multiple of the wave or the block
NAN_PAYLOADS = (0x7FC00000, 0xFFC12345, 0x7FA00001)     # quiet, negative quiet with a payload, signalling

TOURNAMENT = ("ties", "two_level", "signed_zero", "denormal", "nan_inf", "gimbal", "unnormalised", "n_meas_edges") + tuple("n%d" % n for n in SIZES)


def n_meas_scaled(n_meas, rate):
    """the pinned rule in three lines: saturate, NaN -> 0"""
    with np.errstate(all="ignore"):
        v = float(f32(f32(n_meas) * f32(rate)))
    if not v > 0.0:
        return 0
    return 0xFFFFFFFF if v >= 4294967296.0 else int(v)


def quat_from_rpy(roll, pitch, yaw):
    """float64 ZYX composition, rounded to float32 (x, y, z, w)"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return ((sr * cp * cy - cr * sp * sy).astype(f32), (cr * sp * cy + sr * cp * sy).astype(f32), (cr * cp * sy - sr * sp * cy).astype(f32),
            (cr * cp * cy + sr * sp * sy).astype(f32))


def sinp_of(poses):
    """the float32 expression the kernels branch on"""
    q = poses["R"]
    return f32(2.0) * (q["w"] * q["y"] - q["z"] * q["x"])


def cloud(n, seed, pitch=None):
    """the smooth cloud of tests/test_gpu_resample.py, every field filled so that a record copied from the wrong place shows"""
    rng = np.random.RandomState(seed)
    poses, attrs = np.zeros(n, orc.TRANSFORM), np.zeros(n, orc.PARTICLE_ATTRIBUTES)
    for k, (lo, hi) in zip("xyz", ((-9, 9), (-9, 9), (0.2, 3.0))):
        poses["t"][k] = rng.uniform(lo, hi, n)
    roll, p, yaw = rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-math.pi, math.pi, n)
    if pitch is not None:
        p = pitch
    for k, v in zip("xyzw", quat_from_rpy(roll, p, yaw)):
        poses["R"][k] = v
    poses["stamp"] = rng.randint(0, 1 << 30, n)
    attrs["likelihood"]["mean"] = rng.uniform(0, 1, n)
    attrs["likelihood"]["sigma"] = rng.uniform(0, 0.1, n)
    attrs["likelihood"]["n_meas"] = rng.randint(0, 10001, n)
    attrs["state_sigma"] = rng.uniform(0, 1, (n, 6))
    return poses, attrs


def gimbal_poses(n, seed):
    rng = np.random.RandomState(seed)
    pitch = np.where(rng.randint(0, 2, n) == 1, 1.0, -1.0) * (math.pi / 2.0)
    poses, attrs = cloud(n, seed + 1, pitch=pitch)
    flip = rng.randint(0, 2, n) == 1                       # q and -q are the same rotation
    for k in "xyzw":
        poses["R"][k] = np.where(flip, -poses["R"][k], poses["R"][k])
    return poses, attrs


def enemies(n, step, first=0, count=None, seed=SEED):
    """enemy index of champions first .. first+count-1: philox(champion, step, 0, 0)[0] % n, through the oracle's Philox"""
    count = n - first if count is None else count
    return (orc.philox_word0(first, count, step, 0, seed).astype(np.uint64) % np.uint64(n)).astype(np.int64)


def set_means_bits(attrs, bits):
    attrs["likelihood"]["mean"] = np.asarray(bits, dtype=np.uint32).view(f32)


_cases = {}


def tournament_case(name):
    """{"poses", "attrs", "configs": [keyword sets of gladiator_config]} -- every config runs at every step of STEPS"""
    if name in _cases:
        return _cases[name]
    configs = [dict(NOISY)]
    idx = TOURNAMENT.index(name)
    rng = np.random.RandomState(1000 + idx)
    if name.startswith("n") and name[1:].isdigit():
        poses, attrs = cloud(int(name[1:]), 40 + idx)
    elif name == "gimbal":
        poses, attrs = gimbal_poses(N, 50)
        configs = [dict(ZERO_NOISE), dict(NOISY), {}]
    elif name == "n_meas_edges":
        poses, attrs = cloud(N, 51)
        attrs["likelihood"]["n_meas"] = np.array(N_MEAS_EDGES, dtype=np.uint32)[rng.randint(0, len(N_MEAS_EDGES), N)]
        configs = [dict(NOISY, likelihood_forget_per_meter=fm, likelihood_forget_per_radian=fr, trans_dist_metric=m)
                   for (fm, fr) in GLADIATOR_FORGET for m in (0, 1)]
        configs.append(dict(ZERO_NOISE, likelihood_forget_per_meter=1.0, likelihood_forget_per_radian=0.0))   # pow(0, 0) = 1: nothing forgotten
    else:
        poses, attrs = cloud(N, 52 + idx)
        L = attrs["likelihood"]["mean"]
        if name == "ties":
            L[:] = 0.37
        elif name == "two_level":
            L[:] = np.where(rng.randint(0, 2, N) == 1, 0.75, 0.25)
        elif name == "signed_zero":
            set_means_bits(attrs, np.array([0x00000000, 0x80000000, 0x3A83126F], dtype=np.uint32)[rng.choice(3, N, p=(0.45, 0.45, 0.10))])
        elif name == "denormal":
            L[:] = np.array([0.0, 1e-45, 3e-45, 1e-42, 1e-40, 1e-39], dtype=f32)[rng.randint(0, 6, N)]
        elif name == "nan_inf":
            bits = L.view(np.uint32).copy()
            special = np.array(NAN_PAYLOADS + (0x7F800000, 0xFF800000), dtype=np.uint32)
            pick = rng.randint(0, 10, N)                   # half the cloud special, a tenth each
            bits[pick < 5] = special[pick[pick < 5]]
            set_means_bits(attrs, bits)
        elif name == "unnormalised":
            s = np.where(rng.randint(0, 2, N) == 1, f32(2.0), f32(0.5))
            for k in "xyzw":
                poses["R"][k] = poses["R"][k] * s
        else:
            raise KeyError(name)
    _cases[name] = {"name": name, "poses": poses, "attrs": attrs, "configs": configs}
    return _cases[name]


def tournament_reference(case, kw, step, first=0, count=None):
    return orc.gladiator_resample(case["poses"], case["attrs"], orc.gladiator_config(**kw), SEED, step, first, count)


def replaced_mask(case, attrs_new, first=0):
    """champions whose record is no longer their own: state_sigma is six random floats per particle and no resampler touches it"""
    own = case["attrs"]["state_sigma"][first:first + len(attrs_new)]
    return (attrs_new["state_sigma"].view(np.uint32) != own.view(np.uint32)).any(axis=1)


def shard_cuts(n):
    """a partition of [0, n) cut at {0, 1, 63, 64, 65, 257, n - 1, n}: shards that start and end off the wave boundary"""
    cuts = sorted({c for c in (0, 1, 63, 64, 65, 257, n - 1, n) if 0 <= c <= n})
    return list(zip(cuts[:-1], cuts[1:]))


# ---- statistics vectors ----------------------------------------------------------------------------------------------------------
STATS_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, 300007)
STATS_FILLS = ("uniform", "denormal", "zero", "negative", "nan_first", "nan_mid", "nan_last", "inf", "max_last", "max_255", "max_256",
               "max_last_trip", "one_big")
ONE_BIG_N = 65536


def stats_stride(n):
    """threads of k_likelihood_stats_partial's launch: min(256, ceil(n / 1024)) blocks (at least one) of 256"""
    return 256 * min(256, max(1, (n + 1023) // 1024))


def stats_vector(n, fill):
    """float32 likelihoods, or None where the fill needs an index the size does not have"""
    rng = np.random.RandomState(7000 + n % 9973 + 31 * STATS_FILLS.index(fill))
    if fill == "one_big":
        if n != ONE_BIG_N:
            return None
        v = np.ones(n, dtype=f32)
        v[0] = 16777216.0
        return v
    v = rng.uniform(0, 1, n).astype(f32)
    if n == 0:
        return v if fill == "uniform" else None
    if fill == "denormal":
        v = (rng.randint(1, 1 << 23, n).astype(np.uint32)).view(f32).copy()       # every positive denormal pattern
    elif fill == "zero":
        v[:] = 0.0
    elif fill == "negative":
        v = -v - f32(1e-3)
    elif fill.startswith("nan_"):
        v[{"nan_first": 0, "nan_mid": n // 2, "nan_last": n - 1}[fill]] = np.nan
    elif fill == "inf":
        v[(2 * n) // 3] = np.inf
    elif fill.startswith("max_"):
        trip = ((n - 1) // stats_stride(n)) * stats_stride(n)
        at = {"max_last": n - 1, "max_255": 255, "max_256": 256, "max_last_trip": trip}[fill]
        if at >= n or (fill == "max_last_trip" and trip == 0):
            return None
        v[at] = 1.5
    return v


STATS_CASES = [(n, fill) for fill in STATS_FILLS for n in STATS_SIZES + (ONE_BIG_N,) if stats_vector(n, fill) is not None]


def stats_attrs(v):
    """attributes holding v as likelihood.mean, the other eight floats of a record filled with values that would spoil the result"""
    a = np.zeros(len(v), orc.PARTICLE_ATTRIBUTES)
    a["likelihood"]["mean"] = v
    a["likelihood"]["sigma"] = 1e30
    a["likelihood"]["n_meas"] = 0x7FC00000                  # the bits of a NaN
    a["state_sigma"] = np.inf
    return a


def ulp32(x):
    """the spacing of float32 in the binade of |x| (a double)"""
    x = abs(float(x))
    if x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.frexp(x)[1] - 1 - 23)


def stats_sum_bound(v):
    """(fsum, bound): a double accumulator in ANY order is within n * 2^-53 * sum|L| of the exact sum; its rounding to float32 adds half
    an ulp of float32"""
    d = [float(x) for x in v]
    s = math.fsum(d)
    return s, 0.5 * ulp32(s) + len(d) * 2.0 ** -53 * math.fsum(abs(x) for x in d)


# ---- residual cases --------------------------------------------------------------------------------------------------------------
RESIDUAL_SEED = 77
RESIDUAL = ("retry_twice", "single_1", "single_5", "exact_shares_1", "exact_shares_2", "one_slot", "n_meas_edges", "gimbal")
RETRY_N, RETRY_N_NEW, RETRY_WINDOW = 2000, 1000, 40000


def latest_second_appearance(n, seed, step, window):
    """(particle, draw index of its second appearance): the particle whose SECOND appearance in the stream philox(k, step, 2, 0)[0] % n,
    k < window, comes latest"""
    idx = (orc.philox_word0(0, window, step, 2, seed).astype(np.uint64) % np.uint64(n)).astype(np.int64)
    seen, second = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for k, i in enumerate(idx.tolist()):
        seen[i] += 1
        if seen[i] == 2:
            second[i] = k
    assert (second >= 0).all(), "window too short: a particle appears fewer than twice"
    return int(second.argmax()), int(second.max())


def first_block(n, n_new, expect):
    """draws of the library's first block (capi_pf.cpp: residual_draws_enqueue): n_new / (expect / n) * 1.25 + 4096, truncated"""
    return int(float(n_new) / (float(expect) / float(n)) * 1.25 + 4096.0)


def residual_expect(L, n_new):
    """sum over the particles of the integer part of their share (k_residual_expect), shares in double from the double sum"""
    L = np.asarray(L, dtype=f32).astype(np.float64)
    share = L / math.fsum(L.tolist()) * float(n_new)
    return int(np.floor(np.clip(share, 0.0, float(n_new))).sum())


def residual_case(name):
    """{"poses", "attrs", "n_new", "runs": [(config keywords, step)]}; seed RESIDUAL_SEED"""
    key = "residual:" + name
    if key in _cases:
        return _cases[key]
    runs = [(dict(NOISY), 0), (dict(NOISY), 0xFFFFFFFF)]
    extra = {}
    if name == "retry_twice":
        poses, attrs = cloud(RETRY_N, 60)
        heavy, second = latest_second_appearance(RETRY_N, RESIDUAL_SEED, 0, RETRY_WINDOW)
        attrs["likelihood"]["mean"] = 1e-12
        attrs["likelihood"]["mean"][heavy] = 1.0
        n_new, runs, extra = RETRY_N_NEW, [(dict(NOISY), 0)], {"heavy": heavy, "second": second}
    elif name in ("single_1", "single_5"):
        poses, attrs = cloud(1, 61)
        n_new = int(name[-1])
    elif name in ("exact_shares_1", "exact_shares_2"):
        poses, attrs = cloud(1024, 62)
        attrs["likelihood"]["mean"] = 0.125
        n_new = 1024 * int(name[-1])
    elif name == "one_slot":
        poses, attrs = cloud(300, 63)
        attrs["likelihood"]["mean"] = 0.0                         # with ONE slot a share below 1 truncates to 0 (refused: see
        attrs["likelihood"]["mean"][17] = 1.0                     # test_gpu_resample.py), so one particle holds all the weight: share 1.0
        n_new = 1
    elif name == "n_meas_edges":
        poses, attrs = cloud(N, 64)
        rng = np.random.RandomState(65)
        attrs["likelihood"]["mean"] = rng.uniform(0.5, 1.0, N)
        attrs["likelihood"]["n_meas"] = np.array(N_MEAS_EDGES, dtype=np.uint32)[rng.randint(0, len(N_MEAS_EDGES), N)]
        n_new = 2 * N + 1
        runs = [(dict(NOISY, likelihood_forget_per_meter=fm, likelihood_forget_per_radian=fr), 0) for fm, fr in RESIDUAL_FORGET]
        runs.append((dict(ZERO_NOISE, likelihood_forget_per_meter=0.0, likelihood_forget_per_radian=1.0), 0))   # pow(0, 0) * 1: rate 1
    elif name == "gimbal":
        poses, attrs = gimbal_poses(N, 66)
        attrs["likelihood"]["mean"] = np.random.RandomState(67).uniform(0.5, 1.0, N)
        n_new = 2 * N + 1
        runs = [(dict(ZERO_NOISE), 0), (dict(NOISY), 0xFFFFFFFF)]
    else:
        raise KeyError(name)
    _cases[key] = dict({"name": name, "poses": poses, "attrs": attrs, "n_new": n_new, "runs": runs}, **extra)
    return _cases[key]


def residual_reference(case, kw, step):
    """(poses_new, attrs_new, filled, draws) of the oracle's sequential loop"""
    return orc.residual_resample(case["poses"], case["attrs"], orc.gladiator_config(**kw), RESIDUAL_SEED, step, n_new=case["n_new"])


def residual_refused_clouds():
    """(label, likelihoods of 1000 particles, n_new, the word of the error) -- inputs rmclhip.h says the residual resampler refuses, and
    two it handles: negative and NaN likelihoods insert nothing (a non-positive or NaN share) while the sum stays positive"""
    rng = np.random.RandomState(68)
    base = rng.uniform(0.5, 1.0, 1000).astype(f32)
    neg, nan = base.copy(), base.copy()
    neg[::3] = -0.01
    nan[5] = np.nan
    allneg = -base
    return [("negatives", neg, 3000, None), ("one_nan", nan, 3000, "sum to zero"), ("all_negative", allneg, 3000, "sum to zero")]


# ---- refused configurations ------------------------------------------------------------------------------------------------------
BAD_RATES = (-1e-9, -1.0, 1.0 + 1e-6, 2.0, math.inf, -math.inf, math.nan)
NOISE_FIELDS = ("min_noise_tx", "min_noise_ty", "min_noise_tz", "min_noise_roll", "min_noise_pitch", "min_noise_yaw")
BAD_CONFIGS = [{f: r} for f in ("likelihood_forget_per_meter", "likelihood_forget_per_radian") for r in BAD_RATES] + \
              [{f: w} for f in NOISE_FIELDS for w in (math.nan, math.inf)]
GOOD_END_CONFIGS = [dict(likelihood_forget_per_meter=a, likelihood_forget_per_radian=b) for a in (0.0, 1.0) for b in (0.0, 1.0)]
