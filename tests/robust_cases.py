"""Every input of the robust-MICP tests (tests/test_robust_cpu.py, tests/test_gpu_robust.py), made from fixed seeds -- and proved fit
for their purpose without a device by tests/test_robust_cases_cpu.py.

LINE CASES.  D = 0, I = (0, 0, r), N = (0, 0, 1) under the identity pre-transform make spd == r exactly ((0 * 0 + 0 * 0) + r * 1), so
a test chooses the residuals bit by bit (r = -0 alone arrives as +0; both have the key 0 and the weight 1).

What the median cases are for: the selection (rmcl_amd/csrc/robust.hip) takes the f32 pattern of |r| in three digits, bits 31..21,
20..10 and 9..0, one histogram pass each, and picks the bucket that holds rank (m - 1) // 2.
"""
import math

import numpy as np

import pose_information_cases as pic
import robust_ref as rr

F = np.float32
MAX_DIST = F(1.0)


def _f(bits):
    return np.asarray(bits, np.uint32).view(F)


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


# ---- the weights' grid -----------------------------------------------------------------------------------------------------------------
GRID_C = tuple(F(c) for c in (1e-30, 1e-3, 0.05, 0.3, 0.99, 7.5))


def grid_r(c):
    """residuals around the scale c: +-0, |r| == c, one ulp either side of c, a denormal, small, large and random values, both signs"""
    c = F(c)
    rng = np.random.RandomState(int(_bits(c)) % 100003)
    pos = [F(0.0), c, np.nextafter(c, F(0.0)), np.nextafter(c, F(np.inf)), F(1e-40), F(1.1754944e-38), F(0.5) * c, F(2.0) * c, F(1e-3),
           F(0.25), F(0.999), F(3.0e19), F(1.0e30)]
    pos += list((c * rng.uniform(0.0, 3.0, 6)).astype(F)) + list(rng.uniform(0.0, 1.0, 6).astype(F))
    pos = np.array(pos, F)
    return np.concatenate([pos, -pos]).astype(F)


def line_case(r, dmask=None, mmask=None):
    """dict D, I, N, dmask, mmask of n elements whose residual under the identity is r[i]"""
    r = np.asarray(r, F)
    n = len(r)
    D = np.zeros((n, 3), F)
    I = np.zeros((n, 3), F)
    I[:, 2] = r
    N = np.zeros((n, 3), F)
    N[:, 2] = 1.0
    return dict(D=D, I=I, N=N, dmask=np.ones(n, np.uint8) if dmask is None else np.asarray(dmask, np.uint8),
                mmask=np.ones(n, np.uint8) if mmask is None else np.asarray(mmask, np.uint8))


def weights_case():
    """~300 elements: the grid's residuals at every c below MAX_DIST (gated in or out by their size), then masked elements and
    elements with NaN / inf points; `poison`: the indices of the latter"""
    r = np.concatenate([grid_r(c) for c in GRID_C])
    n0 = len(r)
    r = np.concatenate([r, np.full(12, F(0.1))])
    c = line_case(r)
    c["dmask"][n0:n0 + 3] = 0
    c["mmask"][n0 + 3:n0 + 6] = 0
    c["D"][n0 + 6, 0] = np.nan
    c["I"][n0 + 7, 1] = np.inf
    c["I"][n0 + 8, 2] = -np.inf
    c["N"][n0 + 9, 2] = np.nan
    c["D"][n0 + 10, 2] = np.inf
    c["poison"] = list(range(n0, n0 + 11))
    return c


# ---- the median's cases ----------------------------------------------------------------------------------------------------------------
MEDIAN_COUNTS = (1, 2, 3, 256, 257, 4097)
LOW_DIGIT_BASE = 0x3DCCC800          # 0.1 and a bit; bits 9..0 are zero: the last pass's digit alone tells these keys apart
STRADDLE_LAST = 0x3E0003FF           # ... bits 9..0 all ones: + 1 is the next bucket of the second pass
STRADDLE_FIRST = 0x3DFFFFFF          # + 1 = 0x3E000000 is the next bucket of the FIRST pass


def median_cases():
    """{name: (residuals float32 with signs, expected m)}; every |r| is below MAX_DIST"""
    rng = np.random.RandomState(77)
    cases = {}
    for m in MEDIAN_COUNTS:
        r = rng.uniform(-0.9, 0.9, m).astype(F)
        cases["m%d" % m] = (r, m)
    cases["all_equal"] = (np.full(300, F(-0.125)), 300)
    z = np.concatenate([np.zeros(260, F), rng.uniform(0.01, 0.9, 240).astype(F)])
    cases["mostly_zero"] = (rng.permutation(z).astype(F), 500)
    pz = np.concatenate([np.zeros(150, F), -np.zeros(150, F), rng.uniform(0.01, 0.9, 200).astype(F) * F(-1.0)])
    cases["signed_zeros"] = (rng.permutation(pz).astype(F), 500)
    low = _f(LOW_DIGIT_BASE + rng.permutation(1024)[:777].astype(np.uint32))
    cases["low_digit"] = ((low * np.where(rng.uniform(size=777) < 0.5, -1, 1)).astype(F), 777)
    # the median is the LAST copy of the value below a bucket boundary (rank 400 of 0..400 | 401..800), then the first above it
    for name, key in (("straddle_last_pass", STRADDLE_LAST), ("straddle_first_pass", STRADDLE_FIRST)):
        below, above = _f(np.full(401, key, np.uint32)), _f(np.full(400, key + 1, np.uint32))
        cases[name + "_below"] = (rng.permutation(np.concatenate([below, above])).astype(F), 801)
        below, above = _f(np.full(400, key, np.uint32)), _f(np.full(403, key + 1, np.uint32))
        cases[name + "_above"] = (rng.permutation(np.concatenate([below, above])).astype(F), 803)
    multi = rng.uniform(-0.9, 0.9, 3001).astype(F)
    multi[::7] = multi[3]                  # ties
    cases["order_a"] = (multi, 3001)
    cases["order_b"] = (multi[::-1].copy(), 3001)
    cases["empty"] = (np.full(64, F(2.0)), 0)          # every |r| beyond the gate
    return cases


# ---- the reduction's edges ----------------------------------------------------------------------------------------------------------------
SUM_SIZES = pic.FREE_SIZES
SUM_FAR = tuple(n for n, rows in zip(pic.FREE_SIZES, pic.FREE_ROWS) if rows in pic.FAR_ROWS)
SUM_MAX_DIST = pic.MAX_DIST
SUM_PARAMS = (("huber_mad", lambda: rr.params(rr.HUBER)), ("tukey_fixed", lambda: rr.params(rr.TUKEY, scale=0.25)),
              ("cauchy_mad", lambda: rr.params(rr.CAUCHY)))


def sum_case(n, far=False):
    return pic.free_case(n, pic.free_seed(n, far), far)


def sum_reference(c, Tpre, p, max_dist=SUM_MAX_DIST):
    return rr.robust_statistics(Tpre, c["D"], c["dmask"], c["I_nan"], c["N_nan"], c["mmask"], max_dist, p)


# ---- on a map: the contaminated scan ---------------------------------------------------------------------------------------------------
SCAN_MAX_DIST = 1.0
SCAN_ITER = 10
POSE_BAR = 1e-5          # the README's bar for pose deltas


def contaminated_scan(orc):
    """cube_room(10, grid 9) seen through model_c1() from pose_c2_truth(); a contiguous azimuth sector of about a fifth of the rays
    (columns 5..11 of 32) is shortened by 0.3 - 0.8 m: a pallet in front of the wall.  The estimate starts 0.2 m / 2 degrees off.
    dict: map (v, f), mesh, model, Tsb, truth, estimate, dataset (points, mask), short (bool per ray), and the model buffers the find at
    the estimate gives (points, normals, hits -- the oracle's)"""
    from rmcl_amd import synthetic as syn, types as T
    v, f = syn.cube_room(10.0, 9)
    mesh = orc.Mesh(v, f)
    model = syn.model_c1()
    Tsb = syn.tsb_offset()
    truth = syn.pose_c2_truth()
    estimate = T.mult(truth, T.transform_from_rpy((0.2, 0.0, 0.0), (0.0, 0.0, 2.0 * math.pi / 180)))
    meas = mesh.simulate_spherical(model, Tsb, truth, bvh=False)
    H, W = 32, 32
    rng = np.random.RandomState(5)
    short = np.zeros((H, W), bool)
    short[:, 5:12] = True
    short = short.reshape(-1) & (meas["hits"] > 0)
    ranges = meas["ranges"].astype(F).copy()
    ranges[short] = (ranges[short] - rng.uniform(0.3, 0.8, int(short.sum())).astype(F)).astype(F)
    pts = (orc.spherical_directions(model) * ranges[:, None]).astype(F)
    sim = mesh.simulate_spherical(model, Tsb, estimate, bvh=False)
    return dict(map=(v, f), mesh=mesh, model=model, Tsb=Tsb, truth=truth, estimate=estimate, dataset=(pts, meas["hits"].astype(np.uint8)),
                short=short, points=sim["points"], normals=sim["normals"], hits=sim["hits"].astype(np.uint8))


def pose_error(orc, T_onew_oold, s):
    """(metres, radians) between estimate corrected by T_onew_oold (Tom = identity: odometry frame = map frame, Tbo = the estimate) and
    the truth"""
    corrected = orc.tmult(T_onew_oold, s["estimate"])
    d = orc.tmult(orc.tinv(s["truth"]), corrected)
    t = math.sqrt(sum(float(d["t"][k]) ** 2 for k in "xyz"))
    ang = 2.0 * math.asin(min(1.0, math.sqrt(sum(float(d["R"][k]) ** 2 for k in "xyz"))))
    return t, ang


def restated_loop(orc, s, p, n_iter=SCAN_ITER):
    """robust_ref.correct_once on the scan's buffers: Tom the identity, Tbo the estimate"""
    pts, mask = s["dataset"]
    return rr.correct_once(orc, p, n_iter, s["Tsb"], s["estimate"], pts, mask, s["points"], s["normals"], s["hits"], SCAN_MAX_DIST)
