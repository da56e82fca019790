"""numpy restatement of ROBUST MICP FOR SENSOR RIGS (include/rmclhip.h): the weighted merge of CrossStatistics in
float32, operation for operation; the rig loop on robust_ref.robust_statistics, the oracle's cs_transform and umeyama; the weighted pose
information with math.fsum sums and the sums of their terms' magnitudes (n * 2^-52 * sum |terms| bounds any summation order in double).
"""
import math

import numpy as np

import pose_information_ref as pir
import robust_ref as rr

F = np.float32


def _v(rec, name):
    return np.array([rec[name][k] for k in "xyz"], F)


def merge_weighted(orc, a, wa, b, wb):
    """(merged, W) of rmclhip_cross_statistics_merge_weighted: W = wa + wb in double, the two fractions float32 divisions of the
    weights rounded to float32, then cs_merge's float32 expressions; the counts add (mod 2^32) whatever the weights are"""
    W = float(wa) + float(wb)
    out = np.zeros((), dtype=orc.CROSS_STATISTICS)
    out["n_meas"] = np.uint32((int(a["n_meas"]) + int(b["n_meas"])) & 0xFFFFFFFF)
    if not W > 0.0:
        return out, W
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w1, w2 = F(F(wa) / F(W)), F(F(wb) / F(W))
        ad, am, bd, bm = _v(a, "dataset_mean"), _v(a, "model_mean"), _v(b, "dataset_mean"), _v(b, "model_mean")
        rd = ((ad * w1).astype(F) + (bd * w2).astype(F)).astype(F)
        rm = ((am * w1).astype(F) + (bm * w2).astype(F)).astype(F)
        m1, d1, m2, d2 = (am - rm).astype(F), (ad - rd).astype(F), (bm - rm).astype(F), (bd - rd).astype(F)
        ca, cb = np.asarray(a["covariance"], F).reshape(3, 3), np.asarray(b["covariance"], F).reshape(3, 3)
        P1 = ((ca * w1).astype(F) + (cb * w2).astype(F)).astype(F)
        P2 = ((np.outer(m1, d1).astype(F) * w1).astype(F) + (np.outer(m2, d2).astype(F) * w2).astype(F)).astype(F)
        cov = (P1 + P2).astype(F)
    for k, name in enumerate("xyz"):
        out["dataset_mean"][name], out["model_mean"][name] = rd[k], rm[k]
    out["covariance"] = cov.reshape(9)
    return out, W


def sensor_scale(orc, s, max_dist):
    """the scale a rig's sensor holds: selected at the identity pre-transform under its max_dist'"""
    kept, _, r = pir.gate(orc.transform(), s["ds"], s["mask"], s["points"], s["normals"], s["hits"], max_dist)
    return rr.scale_of(s["p"], r, kept)


def rig_loop(orc, sensors, n_iter, max_dists=None):
    """rmclhip_micp_correct_once_robust after its finds.  sensors: dicts p (robust_ref.params), Tsb, Tbo, ds, mask (or None), points,
    normals, hits (the find's buffers, cut to the dataset's length by the caller where that is shorter), max_dist, w (the multiplier).
    Returns dict T (T_onew_oold), merged, merged_weight, stats (the last iteration's robust_statistics per sensor), scales, traj."""
    n = len(sensors)
    md = [s["max_dist"] for s in sensors] if max_dists is None else max_dists
    scales = [sensor_scale(orc, s, md[k]) for k, s in enumerate(sensors)]
    T_o = orc.transform()
    T_s = [orc.transform() for _ in range(n)]
    merged, W, stats, traj = orc.cs_identity(), 0.0, [None] * n, []
    for _ in range(n_iter):
        merged, W = orc.cs_identity(), 0.0
        merged_w, Ww = orc.cs_identity(), 0.0
        for k, s in enumerate(sensors):
            st = rr.robust_statistics(T_s[k], s["ds"], s["mask"], s["points"], s["normals"], s["hits"], md[k], s["p"], scale=scales[k])
            stats[k] = st
            Cs_o = orc.cs_transform(s["Tbo"], orc.cs_transform(s["Tsb"], rr.as_cross_statistics(orc, st)))
            merged, W = merge_weighted(orc, merged, W, Cs_o, st["weight_sum"])
            merged_w, Ww = merge_weighted(orc, merged_w, Ww, Cs_o, st["weight_sum"] * float(s["w"]))      # no truncation
        if Ww > 0.0:
            T_o = orc.tmult(T_o, orc.umeyama(merged_w))
        traj.append(T_o.copy())
        for k, s in enumerate(sensors):
            T_b = orc.tmult(orc.tmult(orc.tinv(s["Tbo"]), T_o), s["Tbo"])
            T_s[k] = orc.tmult(orc.tmult(orc.tinv(s["Tsb"]), T_b), s["Tsb"])
    return dict(T=T_o, merged=merged, merged_weight=W, stats=stats, scales=scales, traj=traj)


def _fsum(x):
    return math.fsum(np.asarray(x, np.float64).tolist())


def pose_information_weighted(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist, p):
    """rmclhip_rcc_pose_information_robust: A = sum w u u^T (6 x 6), g, rss = sum w r^2, every term (double)w * (u[a] * u[b]); the
    scale selected at Tpre.  dict A, g, rss, weight_sum, rss_unweighted, each with its '_abs', n_meas, c, median, w (float32, kept)"""
    kept, D, r = pir.gate(Tpre, dataset_points, dataset_mask, model_points, model_normals, model_mask, max_dist)
    N = np.ascontiguousarray(model_normals, dtype=F).reshape(-1, 3)
    c, med, _ = rr.scale_of(p, r, kept)
    w = rr.weight(p["kernel"], c, r[kept])
    wd = w.astype(np.float64)
    U = pir.u_vectors(D[kept], N[kept], r[kept])
    S, Sa = np.zeros((7, 7)), np.zeros((7, 7))
    for a in range(7):
        for b in range(a, 7):
            terms = wd * (U[:, a] * U[:, b])
            S[a, b] = S[b, a] = _fsum(terms)
            Sa[a, b] = Sa[b, a] = _fsum(np.abs(terms))
    plain = U[:, 6] * U[:, 6]
    return dict(A=S[:6, :6].copy(), g=S[:6, 6].copy(), rss=float(S[6, 6]), A_abs=Sa[:6, :6].copy(), g_abs=Sa[:6, 6].copy(),
                rss_abs=float(Sa[6, 6]), weight_sum=_fsum(wd), weight_sum_abs=_fsum(wd), rss_unweighted=_fsum(plain),
                rss_unweighted_abs=_fsum(plain), n_meas=int(kept.sum()), c=c, median=med, w=w, kept=kept)
