"""numpy restatement of ROBUST MICP (include/rmclhip.h): the gate and the residual of rmclhip_statistics_p2l in float32
(pose_information_ref.gate), the M-estimator weights in float32 with IEEE division and no fused operation, the exact lower median of
|r| and the scale, the weighted sums in float64 with math.fsum -- each with the sum of its terms' magnitudes, so that
n * 2^-52 * sum |terms| bounds the error of ANY summation order in double (pose_information_ref.assert_matches' idea) -- and the IRLS
loop of rmclhip_rcc_correct_once_robust with the oracle's transform algebra and Umeyama solve.

Per-element quantities (r, w, keys) are float32 / uint32 and must match the device byte for byte; the median, the count and c are
exact."""
import math

import numpy as np

import pose_information_ref as pir

F = np.float32
EPS64 = 2.0 ** -52
EPS32 = 2.0 ** -24          # half an ulp of a float32 in [1, 2)

NONE, HUBER, CAUCHY, TUKEY, GEMAN_MCCLURE = 0, 1, 2, 3, 4
KERNELS = (NONE, HUBER, CAUCHY, TUKEY, GEMAN_MCCLURE)
NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy", TUKEY: "tukey", GEMAN_MCCLURE: "geman_mcclure"}
TUNING = {NONE: F(1.0), HUBER: F(1.345), CAUCHY: F(2.385), TUKEY: F(4.685), GEMAN_MCCLURE: F(1.0)}
FIXED, MAD = 0, 1
NO_KEY = np.uint32(0xFFFFFFFF)


def params(kernel, scale=None, tuning=None, scale_min=1e-3):
    """dict twin of rmclhip_robust_params: the defaults of rmclhip_robust_params_default, scale=c switches to FIXED"""
    return dict(kernel=kernel, scale_mode=FIXED if scale is not None else MAD, scale=F(1.0 if scale is None else scale),
                tuning=F(TUNING[kernel] if tuning is None else tuning), scale_min=F(scale_min))


def weight(kernel, c, r):
    """w(r) at scale c, float32 in and out, one rounding per operation"""
    r = np.asarray(r, dtype=F)
    c = F(c)
    a = np.abs(r)
    one = F(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if kernel == NONE:
            return np.ones_like(r)
        if kernel == HUBER:
            safe = np.where(a <= c, one, a)          # never c / 0: the quotient is only used where |r| > c > 0
            return np.where(a <= c, one, (c / safe).astype(F)).astype(F)
        u = (r / c).astype(F)
        uu = (u * u).astype(F)
        if kernel == CAUCHY:
            return (one / (one + uu).astype(F)).astype(F)
        if kernel == TUKEY:
            t = (one - uu).astype(F)
            return np.where(a < c, (t * t).astype(F), F(0.0)).astype(F)
        assert kernel == GEMAN_MCCLURE
        t = (one + uu).astype(F)
        return (one / (t * t).astype(F)).astype(F)


def keys_of(r, kept):
    """the selection's key of every element: the bit pattern of |r| where gated in, NO_KEY elsewhere"""
    k = np.abs(np.asarray(r, dtype=F)).view(np.uint32).copy()
    k[~kept] = NO_KEY
    return k


def lower_median(abs_r):
    """(median, rank): element (m - 1) // 2 of the sorted float32 values; (0, 0) for none"""
    a = np.sort(np.asarray(abs_r, dtype=F))
    if len(a) == 0:
        return F(0.0), 0
    return a[(len(a) - 1) // 2], (len(a) - 1) // 2


def mad_scale(tuning, median, scale_min):
    """max((float)(tuning * 1.4826 * (double)median), scale_min): double arithmetic, one rounding"""
    c = F(float(F(tuning)) * 1.4826 * float(F(median)))
    return c if c > F(scale_min) else F(scale_min)


def scale_of(p, r, kept):
    """(c, median reported, m) of the gated-in residuals r[kept] under the parameters p"""
    m = int(kept.sum())
    if p["scale_mode"] == FIXED:
        return F(p["scale"]), F(0.0), m
    if m == 0:
        return F(p["scale_min"]), F(0.0), 0
    med, _ = lower_median(np.abs(r[kept]))
    return mad_scale(p["tuning"], med, p["scale_min"]), med, m


def _fsum(x):
    return math.fsum(np.asarray(x, np.float64).tolist())


def robust_statistics(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist, p, scale=None):
    """the record rmclhip_statistics_p2l_robust returns, and what it is made of:
    kept, r, w (float32 per element, 0 where masked or gated out), keys, m, median, c; sums[19] = the 16 weighted sums | sum w (again,
    index 15) ... laid out as the device's row: sd[3] sm[3] smd[9] sum_w | count | wrss | rss, with sums_abs the terms' magnitudes;
    dataset_mean, model_mean, covariance (float32, as finalize_pose forms them with sum w for n), n_meas.
    scale=(c, median, m): use this scale instead of selecting one (the loop holds the first iteration's)"""
    kept, D, r = pir.gate(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist)
    N = np.ascontiguousarray(model_normals, dtype=F).reshape(-1, 3)
    c, med, m = scale_of(p, r, kept) if scale is None else scale
    w = np.zeros(len(r), F)
    w[kept] = weight(p["kernel"], c, r[kept])
    Dk, Nk, rk = D[kept], N[kept], r[kept]
    with np.errstate(over="ignore", invalid="ignore"):
        Mk = (Dk + (Nk * rk[:, None]).astype(F)).astype(F)        # Mi = Di + Ni * spd in float32
    wd, d, mm, rd = w[kept].astype(np.float64), Dk.astype(np.float64), Mk.astype(np.float64), rk.astype(np.float64)
    terms = [wd * d[:, k] for k in range(3)] + [wd * mm[:, k] for k in range(3)]
    terms += [wd * (mm[:, a] * d[:, b]) for a in range(3) for b in range(3)]
    terms += [wd, np.ones(len(wd)), wd * (rd * rd), rd * rd]
    sums = np.array([_fsum(t) for t in terms])
    sums_abs = np.array([_fsum(np.abs(t)) for t in terms])
    out = dict(kept=kept, r=r, w=w, keys=keys_of(r, kept), m=int(kept.sum()), median=med, c=c, sums=sums, sums_abs=sums_abs,
               weight_sum=sums[15], wrss=sums[17], rss=sums[18], n_meas=int(kept.sum()),
               dataset_mean=np.zeros(3, F), model_mean=np.zeros(3, F), covariance=np.zeros(9, F))
    W = sums[15]
    if W > 0.0:
        md, mo = sums[0:3] / W, sums[3:6] / W
        out["dataset_mean"], out["model_mean"] = md.astype(F), mo.astype(F)
        cov = np.array([sums[6 + 3 * a + b] / W - mo[a] * md[b] for a in range(3) for b in range(3)])
        out["covariance"] = np.zeros(9, F) if out["n_meas"] == 1 else cov.astype(F)
    return out


def as_cross_statistics(T, ref):
    rec = np.zeros((), dtype=T.CROSS_STATISTICS)
    for k, name in enumerate("xyz"):
        rec["dataset_mean"][name], rec["model_mean"][name] = ref["dataset_mean"][k], ref["model_mean"][k]
    rec["covariance"], rec["n_meas"] = ref["covariance"], ref["n_meas"]
    return rec


def assert_matches(got, ref, what=""):
    """a ROBUST_STATISTICS record against robust_statistics(): n_meas, scale and median exact; weight_sum, wrss, rss within the
    any-order bound n * 2^-52 * sum |terms|; the means and the covariance within what that bound on their sums allows after the
    division by sum w -- e(S) / W + |S| e(W) / W^2 per quotient, the product of the means likewise -- plus some roundings in double of
    the entries' own size and the final rounding to float32."""
    n = ref["n_meas"]
    assert int(got["stats"]["n_meas"]) == n, "%s: n_meas %d != %d" % (what, int(got["stats"]["n_meas"]), n)
    assert F(got["scale"]).tobytes() == F(ref["c"]).tobytes(), "%s: scale %r != %r" % (what, got["scale"], ref["c"])
    want_med = ref["median"]
    assert F(got["median_abs_residual"]).tobytes() == F(want_med).tobytes(), "%s: median %r != %r" % (what, got["median_abs_residual"], want_med)
    bound = n * EPS64 * ref["sums_abs"]
    for key, k in (("weight_sum", 15), ("wrss", 17), ("rss", 18)):
        err = abs(float(got[key]) - ref["sums"][k])
        assert err <= bound[k], "%s: %s off by %.3g, bound %.3g" % (what, key, err, bound[k])
    W = ref["sums"][15]
    if not W > 0.0:
        assert not np.any(np.frombuffer(got["stats"].tobytes(), np.uint8)[:60]), "%s: means / covariance not zero without weight" % what
        return
    S, eW = ref["sums"], bound[15]

    def quot_err(k):
        return bound[k] / W + abs(S[k]) * eW / (W * W)

    def close(g, r, e, name):
        tol = 1.0001 * e + EPS32 * abs(r) * 1.0001 + 1e-45
        assert abs(float(g) - float(r)) <= tol, "%s: %s %r != %r (tolerance %.3g)" % (what, name, g, r, tol)

    md, mo = S[0:3] / W, S[3:6] / W
    for k, name in enumerate("xyz"):
        close(got["stats"]["dataset_mean"][name], F(md[k]), quot_err(k), "dataset_mean." + name)
        close(got["stats"]["model_mean"][name], F(mo[k]), quot_err(3 + k), "model_mean." + name)
    cov = np.asarray(got["stats"]["covariance"], np.float64).reshape(9)
    for a in range(3):
        for b in range(3):
            k = 6 + 3 * a + b
            e = quot_err(k) + abs(mo[a]) * quot_err(b) + abs(md[b]) * quot_err(3 + a) + 4.0 * EPS64 * (abs(S[k] / W) + abs(mo[a] * md[b]))
            want = 0.0 if n == 1 else S[k] / W - mo[a] * md[b]
            close(cov[3 * a + b], F(want), 0.0 if n == 1 else e, "covariance[%d]" % (3 * a + b))


def correct_once(orc, p, n_iter, Tsb, Tbo, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist):
    """rmclhip_rcc_correct_once_robust after its find: the scale once at the identity, then n_iter x {weighted statistics at
    T_snew_sold, Umeyama, T_snew_sold *= U}; an iteration without weight moves nothing.  Returns (T_onew_oold, T_snew_sold, last
    statistics, scale)"""
    T_s = orc.transform()
    kept, _, r = pir.gate(T_s, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist)
    scale = scale_of(p, r, kept)
    last = None
    for _ in range(n_iter):
        last = robust_statistics(T_s, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist, p, scale=scale)
        if last["weight_sum"] > 0.0:
            cs = np.zeros((), dtype=orc.CROSS_STATISTICS)
            for k, name in enumerate("xyz"):
                cs["dataset_mean"][name], cs["model_mean"][name] = last["dataset_mean"][k], last["model_mean"][k]
            cs["covariance"], cs["n_meas"] = last["covariance"], last["n_meas"]
            T_s = orc.tmult(T_s, orc.umeyama(cs))
    Tso = orc.tmult(Tbo, Tsb)
    return orc.tmult(orc.tmult(Tso, T_s), orc.tinv(Tso)), T_s, last, scale
