"""Hand-built PointCloud2 clouds on small spherical models: the inputs of tests/test_scan_edge_cases_cpu.py (which pins, on the
restatement tests/pc2scan_ref.py alone, what every named point is there for) and of tests/test_gpu_pc2scan_edges.py (which compares the
device with that restatement byte for byte).  numpy only; the C library's cosf / sinf are reached through ctypes for the one table the
library builds with them (capi_rcc.cpp: rmclhip_rcc_set_model_spherical).

A model is the tuple of pc2scan_ref.model_tuple: (phi_min, phi_inc, H, theta_min, theta_inc, W, range_min, range_max).
A case point is (name, (x, y, z), expect): expect maps a flag word to what the point, binned ALONE, must be:
    a cell number >= 0   stored in that cell            IMG   inside the image, outside the range interval
    OUT                  finite, outside the image      NF    skipped by the finite test
Flag words that `expect` does not name are not pinned on the CPU; the GPU comparison covers every flag word for every point.
"""
import ctypes
import ctypes.util
import math

import numpy as np

import pc2scan_ref as pr

f32 = np.float32
IMG, OUT, NF = -1, -2, -3
FLAGS = (0, 2, 4, 7, 8, 15)
PI = math.pi
RMIN, RMAX = f32(0.5), f32(10.0)
ULPS = 4    # the condition of ulp_condition(): twice the 2 ulp the device math library is said to keep for atan2 (see there)


def _m(phi_min, phi_inc, H, th_min, th_inc, W, rmin=RMIN, rmax=RMAX):
    return (f32(phi_min), f32(phi_inc), int(H), f32(th_min), f32(th_inc), int(W), f32(rmin), f32(rmax))


MODELS = {
    "tiny": _m(-0.8, 0.4, 5, -PI, 2 * PI / 8, 8),             # 40 cells: fewer than a wave
    "odd": _m(-0.9, 0.3, 7, -PI, 2 * PI / 37, 37),            # 259 cells: a workgroup plus three; period 37
    "half": _m(-0.3, 0.2, 4, -PI / 2, PI / 16, 16),           # period 32 != W: a wrapped id lands outside the image
    "nowrap": _m(-0.3, 0.2, 4, -1.0, 0.1, 20),                # 2 pi / inc = 62.83: the wrap flag must change nothing
    "poles": _m(-PI / 2, PI / 8, 9, -PI, 2 * PI / 8, 8),      # rows that true elevation reaches at +-pi/2
    "row": _m(0.0, 0.0, 1, -PI, 2 * PI / 360, 360),           # the 2-D scanner
    "col": _m(-0.4, 0.05, 16, 0.0, 0.0, 1),
    "one": _m(0.0, 0.0, 1, 0.0, 0.0, 1),
    "down": _m(0.5, -0.2, 6, -PI, 2 * PI / 12, 12),           # rows from top to bottom: phi.min > 0, phi.inc < 0
    "zero_min": _m(-0.8, 0.4, 5, -PI, 2 * PI / 8, 8, rmin=0.0),
    # a full circle that starts 2 rad after -pi: theta_est in [-pi, -pi + 2) has a NEGATIVE id, which WRAP_THETA moves INTO the image
    # (columns 9 to 11) -- the one model here on which the flag's `theta_id < 0` branch decides a cell
    "turned": _m(-0.3, 0.2, 4, -PI + 2.0, 2 * PI / 12, 12),
}
MODEL_ORDER = ("odd", "row", "poles", "down", "nowrap", "half", "turned", "tiny", "zero_min", "col", "one")   # cells: largest first


def model_struct(name_or_tuple):
    """the SphericalModel struct the library takes (float32 fields, rmcl_amd.types.spherical_model)"""
    from rmcl_amd import types as T
    m = MODELS[name_or_tuple] if isinstance(name_or_tuple, str) else name_or_tuple
    return T.spherical_model(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7])


def period(m):
    """the whole-number wrap period WRAP_THETA uses for this model, or 0 (capi_pc2scan.cpp: pc2scan_check)"""
    if m[4] == 0:
        return 0
    P = 2.0 * PI / float(m[4])
    return int(round(P)) if abs(P - round(P)) < 1e-3 else 0


# ---- points aimed at cells ------------------------------------------------------------------------------------------------------------
def aim(phi, theta, r, true_elevation=False):
    """a point whose angle estimates are (phi, theta): by the reference's rule phi_est = atan2(z, range) = atan(sin(elevation)); with
    TRUE_ELEVATION phi_est is the elevation.  None where the reference's rule cannot reach phi (|tan(phi)| > 1)."""
    if true_elevation:
        el = phi
    else:
        t = math.tan(phi)
        if abs(t) > 1.0 + 1e-6:
            return None
        el = math.asin(min(max(t, -1.0), 1.0))
    return (r * math.cos(el) * math.cos(theta), r * math.cos(el) * math.sin(theta), r * math.sin(el))


def _axis_angles(mn, inc, size, q):
    """the angle at bin coordinate q (cells from the minimum) of an axis; a zero increment has one cell and any angle reaches it"""
    return float(mn) + q * float(inc) if inc != 0 else float(mn) + 0.1 * q


def own_cell_points(name):
    """for every cell one point along its own direction and one a quarter cell inside each of its four edges, aimed by the reference's
    rule (pinned under the flag words without TRUE_ELEVATION) and by true elevation (pinned under 7 and 15)"""
    m = MODELS[name]
    pmin, pinc, H, tmin, tinc, W = m[:6]
    out = []
    for true_el, flag_words in ((False, (0, 2, 4, 8)), (True, (7, 15))):
        for v in range(H):
            for h in range(W):
                for dv, dh in ((0, 0), (-0.25, 0), (0.25, 0), (0, -0.25), (0, 0.25)):
                    if (pinc == 0 and dv) or (tinc == 0 and dh):
                        continue
                    phi, th = _axis_angles(pmin, pinc, H, v + dv), _axis_angles(tmin, tinc, W, h + dh)
                    words = flag_words
                    if th > PI + 1e-6 and period(m) == W and float(tmin) > -PI + 1e-3:
                        # a full circle that does not start at -pi: this direction's theta_est is th - 2 pi, its id is negative.
                        # floor + wrap bring it home; truncation toward zero does not (trunc(h - W + 0.5) + W = h + 1)
                        th, words = th - 2 * PI, ((6,) if not true_el else flag_words)
                    if abs(phi) > PI / 2 + 1e-6 or abs(th) > PI + 1e-6:
                        continue    # no point has such angles (beyond the first column of a model from -pi, beyond a pole row)
                    phi, th = min(max(phi, -PI / 2), PI / 2), min(max(th, -PI), PI)    # (float(f32(-pi)) is a little below -pi)
                    p = aim(phi, th, 2.0 + 0.01 * ((v * W + h) % 50), true_el)
                    if p is None:
                        continue
                    out.append(("own%s[%d,%d]%+.2f%+.2f" % ("_el" if true_el else "", v, h, dv, dh), p, {fw: v * W + h for fw in words}))
    return out


def trunc_floor_points(name):
    """ids where truncation and floor differ: q + 0.5 in (-1, 0) is cell 0 by truncation and outside by floor; q in (size - 0.5, size)
    is outside either way.  Only where an angle below the minimum exists (theta.min > -pi, |phi| < pi/4 by the reference's rule)."""
    m = MODELS[name]
    pmin, pinc, H, tmin, tinc, W = m[:6]
    P = period(m)
    out = []
    mid_phi, mid_th = _axis_angles(pmin, pinc, H, (H - 1) // 2), _axis_angles(tmin, tinc, W, (W - 1) // 2)
    mid_v, mid_h = (H - 1) // 2, (W - 1) // 2
    if pinc != 0:
        for q, label in ((-0.8, "below"), (H - 0.25, "above")):
            p = aim(_axis_angles(pmin, pinc, H, q), mid_th, 3.0)
            if p is not None:
                exp = {0: mid_h, 4: mid_h, 8: mid_h, 2: OUT} if label == "below" else {0: OUT, 2: OUT, 4: OUT, 8: OUT}
                out.append(("phi_%s" % label, p, exp))
    if tinc != 0:
        for q, label in ((-0.8, "below"), (W - 0.25, "above")):
            th = _axis_angles(tmin, tinc, W, q)
            if th <= -PI or th >= PI:
                continue
            p = aim(mid_phi, th, 3.0)
            if label == "below":
                # floor gives -1; with the wrap flag -1 + period: outside unless period == W
                exp = {0: mid_v * W, 8: mid_v * W, 4: mid_v * W, 2: OUT}
                exp[7] = exp[15] = None
            else:
                exp = {0: OUT, 2: OUT, 8: OUT, 4: (mid_v * W if P == W else OUT)}
            out.append(("theta_%s" % label, p, {k: v for k, v in exp.items() if v is not None}))
    return out


def _ids(m, phi, th, wrap=False):
    """(phi id, theta id) of exact angle estimates by truncation; wrap: WRAP_THETA's one period"""
    pmin, pinc, H, tmin, tinc, W = m[:6]
    pi_ = 0 if pinc == 0 else math.trunc(float(f32((f32(phi) - pmin) / pinc)) + 0.5)
    ti = 0 if tinc == 0 else math.trunc(float(f32((f32(th) - tmin) / tinc)) + 0.5)
    P = period(m)
    if wrap and P:
        ti = ti - P if ti >= W else (ti + P if ti < 0 else ti)
    return pi_, ti


def _expect(m, phi, th, r, wrap=False):
    """what a point with these exact estimates must be: its cell, IMG or OUT"""
    pi_, ti = _ids(m, phi, th, wrap)
    if not (0 <= pi_ < m[2] and 0 <= ti < m[5]):
        return OUT
    return pi_ * m[5] + ti if float(m[6]) <= r <= float(m[7]) else IMG


def _cell_of(m, phi, th):
    return _expect(m, phi, th, 1.0)


def seam_points(name):
    """the +-pi seam, the signed zeros, the axes, the poles and the origin -- each with z = 1 and with z = 0.  The angle estimates of these
    points are exact (atan2 of zeros, ones and twos, correctly rounded by any libm), so the expectation is computed from the angles:
    on a model from -pi, theta = +pi has id W -- lost without WRAP_THETA, column 0 with it when the period is W ("half": lost either way)"""
    m = MODELS[name]
    nz = -0.0
    out = []
    seam = [("-1,+0", (-1.0, 0.0), PI), ("-1,-0", (-1.0, nz), -PI), ("-0,-0", (nz, nz), -PI), ("-0,+0", (nz, 0.0), PI),
            ("+0,-0", (0.0, nz), -0.0), ("0,+1", (0.0, 1.0), PI / 2), ("0,-1", (0.0, -1.0), -PI / 2)]
    for label, (x, y), th in seam:
        for z in (1.0, 0.0):
            r = math.sqrt(x * x + y * y + z * z)
            phi = math.atan2(z, r)
            out.append(("seam(%s,%g)" % (label, z), (x, y, z), {0: _expect(m, phi, th, r), 4: _expect(m, phi, th, r, wrap=True)}))
    for z in (2.0, -2.0):
        # phi is +-pi/4 by the reference's rule, +-pi/2 by true elevation; theta = atan2(+0, +0) = 0
        exp = {0: _expect(m, math.copysign(PI / 4, z), 0.0, 2.0)}
        if name == "poles":
            exp[7] = exp[15] = (8 if z > 0 else 0) * m[5] + 4
        out.append(("pole(%g)" % z, (0.0, 0.0, z), exp))
    return out


def origin_points(name):
    """range 0: stored (as bytes 00 00 00 00) only where range.min is 0"""
    m = MODELS[name]
    e0, e1 = _expect(m, 0.0, 0.0, 0.0), _expect(m, -0.0, -PI, 0.0)
    return [("origin(+0)", (0.0, 0.0, 0.0), {0: e0, 8: e0}), ("origin(-0)", (-0.0, -0.0, -0.0), {0: e1, 8: e1})]


def bound_values(m):
    """range.min, range.max and the float on either side of each -> [(label, r, inside)]"""
    lo, hi = m[6], m[7]
    v = [("rmin", lo, True), ("rmin+", np.nextafter(lo, f32(np.inf)), True), ("rmax-", np.nextafter(hi, f32(0)), True), ("rmax", hi, True),
         ("rmax+", np.nextafter(hi, f32(np.inf)), False)]
    if lo > 0:
        v.append(("rmin-", np.nextafter(lo, f32(0)), False))
    return v


def range_points(name):
    """along +x: the range bounds, a coordinate whose square overflows, and coordinates whose square is subnormal or zero"""
    m = MODELS[name]
    c = _cell_of(m, 0.0, 0.0)
    hit = lambda inside: c if (inside or c == OUT) else IMG
    out = [("bound(%s)" % label, (float(r), 0.0, 0.0), {0: hit(inside), 8: hit(inside)}) for label, r, inside in bound_values(m)]
    c45 = _cell_of(m, 0.0, PI / 4)
    out.append(("overflow", (3e38, 3e38, 0.0), {0: IMG if c45 != OUT else OUT}))
    stored = m[6] == 0
    out.append(("square_subnormal", (1e-20, 0.0, 0.0), {0: hit(stored)}))
    out.append(("square_zero", (1e-42, 0.0, 0.0), {0: hit(stored)}))
    return out


def nonfinite_points():
    out = []
    for k, axis in enumerate("xyz"):
        for label, bad in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            p = [1.0, 0.5, 0.25]
            p[k] = bad
            out.append(("%s(%s)" % (label, axis), tuple(p), {fw: NF for fw in FLAGS}))
    return out


def case_points(name):
    """every named point of a model, the origin first (buffer index 0: the default key (0 + 1) << 32 | 0, the nearest key 0)"""
    return origin_points(name) + seam_points(name) + range_points(name) + nonfinite_points() + trunc_floor_points(name) + own_cell_points(name)


def padding(name, n, seed=0):
    """n random points inside the image and the range interval of the model (by the reference's rule)"""
    m = MODELS[name]
    pmin, pinc, H, tmin, tinc, W = m[:6]
    rs = np.random.RandomState(seed + 17 * len(name))
    out = np.zeros((n, 3), f32)
    for i in range(n):
        while True:
            phi = _axis_angles(pmin, pinc, H, rs.uniform(-0.4, H - 0.6))
            th = _axis_angles(tmin, tinc, W, rs.uniform(-0.4, W - 0.6))
            p = aim(phi, th, rs.uniform(1.0, 9.0)) if abs(phi) < PI / 2 and -PI < th < PI else None
            if p is not None:
                out[i] = p
                break
    return out


def edge_cloud(name, n=None, seed=0):
    """(n, 3) float32: the named points of the model in order, cut to n or padded to n with random in-image points"""
    pts = np.array([p for _, p, _ in case_points(name)], np.float64).astype(f32)
    if n is None or n == len(pts):
        return pts
    if n < len(pts):
        return pts[:n].copy()
    return np.concatenate([pts, padding(name, n - len(pts), seed)])


# ---- FLOAT64 records ------------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(f32).max)
_TIE = FLT_MAX + 2.0 ** 103     # FLT_MAX + 1/2 ulp, exact in double: the tie, which rounds to the even neighbour 2^128 = inf
F64_VALUES = [
    ("1e300", 1e300, np.inf),
    ("below_tie", float(np.nextafter(_TIE, 0.0)), FLT_MAX),
    ("tie", _TIE, np.inf),
    ("above_tie", float(np.nextafter(_TIE, np.inf)), np.inf),
    ("1e-40", 1e-40, float(f32(1e-40))),
    ("half_even_down", 1.0 + 2.0 ** -24, 1.0),                      # between 1 and 1 + 2^-23: to the even 1
    ("half_even_up", 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -22),       # between 1 + 2^-23 and 1 + 2^-22: to the even 1 + 2^-22
    ("just_above_half", float(np.nextafter(1.0 + 2.0 ** -24, 2.0)), 1.0 + 2.0 ** -23),
]


def f64_cloud(name):
    """(n, 3) float64 for a FLOAT64 record: the values of F64_VALUES as x (y = z = 0), then the model's named points widened and moved
    off the float grid by a relative 1e-9 (so the cast has to round) -> (xyz float64, expected float32 x of the first len(F64_VALUES))"""
    special = np.array([[v, 0.0, 0.0] for _, v, _ in F64_VALUES], np.float64)
    pts = np.array([p for _, p, _ in case_points(name)], np.float64).astype(f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pts = pts * (1.0 + 1e-9 * np.arange(1, 4)[None, :])
    return np.concatenate([special, pts]), np.array([c for _, _, c in F64_VALUES], np.float64)


# ---- the winner rule ------------------------------------------------------------------------------------------------------------------
RIVAL_SLOTS = (0, 63, 64, 255, 256, -1)     # different waves (64 lanes) and workgroups (256 lanes) of one launch


def winner_cloud(name, order, n=300, two_cells=False):
    """six rivals of one cell at buffer indices 0, 63, 64, 255, 256 and n - 1 (a second cell's six at 1, 62, 65, 254, 257, n - 2 with
    the opposite order when two_cells), everything else in other cells.  order: "asc" / "desc" ranges by index, or "tail": ascending
    with the last rival beyond range.max and the one before it NaN.
    -> (xyz float32, [(cell, winner index by the default rule, winner index by NEAREST)])"""
    m = MODELS[name]
    pmin, pinc, H, tmin, tinc, W = m[:6]
    cells = [(H // 2, W // 2)] + ([(H // 2 - 1, W // 2 + 1)] if two_cells else [])
    taken = {v * W + h for v, h in cells}
    rs = np.random.RandomState(3)
    xyz = np.zeros((n, 3), f32)
    i = 0
    while i < n:      # filler: centres of the other cells, in range
        v, h = rs.randint(0, H), rs.randint(0, W)
        p = aim(_axis_angles(pmin, pinc, H, v), _axis_angles(tmin, tinc, W, h), rs.uniform(1.0, 9.0))
        if v * W + h in taken or p is None or (h == 0 and float(tmin) == float(f32(-PI))):
            continue
        xyz[i] = p
        i += 1
    winners = []
    for k, (v, h) in enumerate(cells):
        slots = [(s + k if s in (0, 64, 256) else s - k) % n for s in RIVAL_SLOTS]
        ranges = [2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
        if (order == "desc") != (k == 1):
            ranges = ranges[::-1]
        if order == "tail":
            ranges = sorted(ranges)
            ranges[5] = 50.0
        for s, r in zip(slots, ranges):
            xyz[s] = aim(_axis_angles(pmin, pinc, H, v), _axis_angles(tmin, tinc, W, h), r)
        valid = list(zip(slots, ranges))
        if order == "tail":
            by_index = sorted(slots)
            xyz[by_index[4], 1] = np.nan                    # the rival before the last one
            valid = [(s, r) for s, r in valid if s != by_index[4] and r <= float(m[7])]
        last = max(s for s, _ in valid)
        near = min(valid, key=lambda sr: (sr[1], sr[0]))[0]
        winners.append((v * W + h, last, near))
    return xyz, winners


# ---- record layouts -------------------------------------------------------------------------------------------------------------------
REC13 = np.dtype({"names": ["z", "y", "x", "tag"], "formats": ["<f4", "<f4", "<f4", "u1"], "offsets": [0, 4, 8, 12], "itemsize": 13})
REC29 = np.dtype({"names": ["a", "x", "y", "z", "b"], "formats": ["u1", "<f8", "<f8", "<f8", "<u2"], "offsets": [0, 3, 11, 19, 27],
                  "itemsize": 29})
REC12 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])


def cut_to_last_coordinate(data, lay):
    """the shortest byte count the layout allows: up to the end of the last point's last coordinate"""
    size = 8 if lay["datatype"] == pr.FLOAT64 else 4
    last = (lay["height"] - 1) * lay["row_step"] + (lay["width"] - 1) * lay["point_step"] + max(lay["offset_x"], lay["offset_y"], lay["offset_z"]) + size
    return data[:last] if lay["width"] * lay["height"] else data[:0]


# ---- the condition byte parity rests on -----------------------------------------------------------------------------------------------
def ids_with_moved_angles(xyz, m, flags, k_theta, k_phi):
    """pc2scan_ref.bin_points' steps 3 and 4 with both double atan2 results moved by k double ulps before the cast to float
    -> (phi ids, theta ids) as float64 (NaN where an angle is NaN)"""
    pmin, pinc, H, tmin, tinc, W = m[:6]
    p = np.asarray(xyz, f32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z).astype(f32)
        den = np.sqrt(x * x + y * y).astype(f32) if flags & pr.TRUE_ELEVATION else r
        th64 = np.arctan2(y.astype(np.float64), x.astype(np.float64))
        ph64 = np.arctan2(z.astype(np.float64), den.astype(np.float64))
        th = (th64 + k_theta * np.spacing(th64)).astype(f32)
        ph = (ph64 + k_phi * np.spacing(ph64)).astype(f32)
        cp = ((ph - pmin) / pinc).astype(f32).astype(np.float64) + 0.5 if pinc != 0 else np.full(len(r), 0.5)
        ct = ((th - tmin) / tinc).astype(f32).astype(np.float64) + 0.5 if tinc != 0 else np.full(len(r), 0.5)
        rnd = np.floor if flags & pr.FLOOR else np.trunc
        return rnd(cp), rnd(ct)


def ulp_condition(xyz, m, flags, ulps=ULPS):
    """bool (n,): the point keeps both ids when the double results of both atan2 calls are moved by +-ulps double ulps before the cast
    to float.  The device evaluates atan2 in double; ROCm's device-library documentation gives 2 ulp for it, and no copy of that table
    is part of the repository or found under the ROCm installation the tests were written on -- so 4 is twice an UNVERIFIED 2."""
    fin = np.isfinite(np.asarray(xyz, f32).reshape(-1, 3)).all(1)
    p0, t0 = ids_with_moved_angles(xyz, m, flags, 0, 0)
    ok = np.ones(len(p0), bool)
    for kt in (-ulps, ulps):
        for kp in (-ulps, ulps):
            p1, t1 = ids_with_moved_angles(xyz, m, flags, kt, kp)
            ok &= ((p1 == p0) | (np.isnan(p1) & np.isnan(p0))) & ((t1 == t0) | (np.isnan(t1) & np.isnan(t0)))
    return ok | ~fin


# ---- the spherical model's direction table ---------------------------------------------------------------------------------------------
_libm = None


def _cfun(name):
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    fn = getattr(_libm, name)
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return fn


def spherical_table(m):
    """(cos phi, sin phi (H,), cos theta, sin theta (W,)) float32 as rmclhip_rcc_set_model_spherical fills them: angle = min +
    float(id) * inc in float, then the C library's cosf / sinf -- the same libm the library's host code calls on this machine"""
    cosf, sinf = _cfun("cosf"), _cfun("sinf")
    phi = (f32(m[0]) + np.arange(m[2], dtype=f32) * f32(m[1])).astype(f32)
    th = (f32(m[3]) + np.arange(m[5], dtype=f32) * f32(m[4])).astype(f32)
    tab = lambda fn, a: np.array([fn(float(v)) for v in a], f32)
    return tab(cosf, phi), tab(sinf, phi), tab(cosf, th), tab(sinf, th)


def spherical_dirs(m):
    """(H*W, 3) float32: mk3(cp * ct, cp * st, sp) of segment.hip seg_ray / pc2scan.hip k_pc2scan_resolve"""
    cp, sp, ct, st = spherical_table(m)
    H, W = m[2], m[5]
    d = np.empty((H, W, 3), f32)
    d[..., 0] = cp[:, None] * ct[None, :]
    d[..., 1] = cp[:, None] * st[None, :]
    d[..., 2] = np.broadcast_to(sp[:, None], (H, W))
    return d.reshape(-1, 3)


def dataset_of(ranges, m):
    """k_pc2scan_resolve's dataset: points = scale3(dir, r) in float32, mask = !(r < min || r > max)"""
    r = np.asarray(ranges, f32).reshape(-1)
    with np.errstate(all="ignore"):
        pts = (spherical_dirs(m) * r[:, None]).astype(f32)
    return pts, (~((r < m[6]) | (r > m[7]))).astype(np.uint8)
