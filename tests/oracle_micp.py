"""Oracle-side (CPU) restatement of the callers of the hot path, used only by tests and the golden
generator: dataset construction (MICPSphericalSensorCPU.cpp:181-233), the MICP-L inner loop
(micp_localization.cpp:900-964 + MICPSensor.hpp:146-184) and the v1 batch corrector loop
(lidar_corrector_embree_benchmark.cpp:127-135).  Built from oracle primitives only.
"""
import numpy as np

import oracle as orc


def directions(model):
    """rmagine SphericalModel::getDirection for every (vid, hid), from the C oracle (libm cosf/sinf)."""
    return orc.spherical_directions(model)


def dataset_from_ranges(model, ranges):
    """unpackMessage: point = dir * range; mask = 0 iff range < range.min or range > range.max."""
    r = np.asarray(ranges, dtype=np.float32).reshape(-1)
    pts = (directions(model) * r[:, None]).astype(np.float32)
    mask = np.where((r < np.float32(model.range.min)) | (r > np.float32(model.range.max)), 0, 1).astype(np.uint8)
    return pts, mask


def compute_cross_statistics_b(sim, ds_points, ds_mask, Tsb, T_bnew_bold, max_dist):
    """MICPSensor_::computeCrossStatistics (MICPSensor.hpp:159-184), stats in the base frame."""
    T_snew_sold = orc.tmult(orc.tmult(orc.tinv(Tsb), T_bnew_bold), Tsb)
    stats_s = orc.statistics_p2l_exact(T_snew_sold, ds_points, ds_mask, sim["points"], sim["normals"], sim["hits"], max_dist)
    return orc.cs_transform(Tsb, stats_s)


def correct_once(mesh, model, Tsb, Tbo, Tom, ds_points, ds_mask, n_iter, max_dist, adaptive_min=None,
                 convergence_progress=0.0, refind=False, nthreads=1):
    """Returns (T_onew_oold, merged stats in odom frame, list of T_onew_oold after each iteration)."""
    if adaptive_min is None:
        adaptive_min = max_dist
    md = orc.adaptive_max_dist(max_dist, adaptive_min, convergence_progress)
    ident = orc.transform()
    T_onew_oold = ident
    traj = []
    merged = orc.cs_identity()
    sim = None
    for i in range(n_iter):
        if sim is None or refind:
            Tom_cur = orc.tmult(Tom, T_onew_oold) if refind else Tom
            sim = mesh.simulate_spherical(model, Tsb, orc.tmult(Tom_cur, Tbo), bvh=True, nthreads=nthreads)
        T_delta = ident if refind else T_onew_oold
        T_bnew_bold = orc.tmult(orc.tmult(orc.tinv(Tbo), T_delta), Tbo)
        Cs_b = compute_cross_statistics_b(sim, ds_points, ds_mask, Tsb, T_bnew_bold, md)
        Cs_o = orc.cs_transform(Tbo, Cs_b)
        merged = orc.cs_merge(orc.cs_identity(), Cs_o)
        T_inner = orc.umeyama(merged)
        T_onew_oold = orc.tmult(T_onew_oold, T_inner)
        traj.append(T_onew_oold.copy())
    return T_onew_oold, merged, traj


def simulate_model(mesh, model, Tsb, Tbm):
    """one scan of any of the four sensor models.  `model`: an rmagine SphericalModel, or a dict with "kind" in spherical
    ("model"), o1dn ("width", "height", "range_min", "range_max", "orig", "dirs"), ondn (the same with "origs") and pinhole
    ("width", "height", "range_min", "range_max", "f", "c")."""
    if not isinstance(model, dict):
        return mesh.simulate_spherical(model, Tsb, Tbm, bvh=True)
    k = model["kind"]
    if k == "spherical":
        return mesh.simulate_spherical(model["model"], Tsb, Tbm, bvh=True)
    size = (model["width"], model["height"], model["range_min"], model["range_max"])
    if k == "o1dn":
        return mesh.simulate_o1dn(*size, model["orig"], model["dirs"], Tsb, Tbm, bvh=True)
    if k == "ondn":
        return mesh.simulate_ondn(*size, model["origs"], model["dirs"], Tsb, Tbm, bvh=True)
    if k == "pinhole":
        return mesh.simulate_pinhole(*size, model["f"], model["c"], Tsb, Tbm, bvh=True)
    raise ValueError("unknown sensor model kind %r" % (k,))


def reduced(sim, ds_points, ds_mask):
    """the correspondences the statistics run over: the first nred = min(n_dataset, n_model) of both sides"""
    ds_points = np.asarray(ds_points, np.float32).reshape(-1, 3)
    nred = min(len(ds_points), len(sim["hits"]))
    cut = {k: sim[k][:nred] for k in ("points", "normals", "hits")}
    return cut, ds_points[:nred], None if ds_mask is None else np.asarray(ds_mask, np.uint8).reshape(-1)[:nred]


def correct_once_multi(mesh, sensors, Tom, n_iter, convergence_progress=0.0, want_traj=False):
    """MICPLocalizationNode::correctOnce with several sensors (micp_localization.cpp:921-963): sensors = [(model, Tsb, Tbo,
    ds_points, ds_mask, max_dist, adaptive_min, merge_weight_multiplier)], `model` as simulate_model takes it (a bare
    SphericalModel: spherical); ds_mask may be None and the dataset shorter than the model.  Returns (T_onew_oold, merged unweighted
    stats, the weighted merged stats every iteration solved) and, with want_traj, T_onew_oold after every iteration as a fourth."""
    ident = orc.transform()
    T_onew_oold = ident
    merged = orc.cs_identity()
    sims = [reduced(simulate_model(mesh, model, Tsb, orc.tmult(Tom, Tbo)), ds_points, ds_mask)
            for model, Tsb, Tbo, ds_points, ds_mask, *_ in sensors]
    solved, traj = [], []
    for _ in range(n_iter):
        merged, merged_w = orc.cs_identity(), orc.cs_identity()
        for (sim, ds_points, ds_mask), (model, Tsb, Tbo, _p, _m, max_dist, adaptive_min, w) in zip(sims, sensors):
            md = orc.adaptive_max_dist(max_dist, adaptive_min, convergence_progress)
            T_bnew_bold = orc.tmult(orc.tmult(orc.tinv(Tbo), T_onew_oold), Tbo)
            Cs_o = orc.cs_transform(Tbo, compute_cross_statistics_b(sim, ds_points, ds_mask, Tsb, T_bnew_bold, md))
            Cs_w = Cs_o.copy()
            Cs_w["n_meas"] = np.uint32(int(float(Cs_w["n_meas"]) * w))   # :934 truncates
            merged = orc.cs_merge(merged, Cs_o)
            merged_w = orc.cs_merge(merged_w, Cs_w)
        solved.append(merged_w)
        T_onew_oold = orc.tmult(T_onew_oold, orc.umeyama(merged_w))
        traj.append(T_onew_oold.copy())
    if want_traj:
        return T_onew_oold, merged, solved, traj
    return T_onew_oold, merged, solved


def correct_batch(mesh, model, Tsb, Tbm, ds_points, ds_mask, max_dist, nthreads=1):
    """v1 SphereCorrector::correct: per pose raycast + reduce (Tpre = I) + Umeyama;
    Tdelta_b = Tsb * T_s * ~Tsb.  `model`: a SphericalModel, or any model simulate_model takes."""
    Tbm = np.asarray(Tbm, dtype=orc.TRANSFORM).reshape(-1)
    out = np.zeros(len(Tbm), dtype=orc.TRANSFORM)
    stats = np.zeros(len(Tbm), dtype=orc.CROSS_STATISTICS)
    ident = orc.transform()
    for i in range(len(Tbm)):
        if isinstance(model, dict):
            sim = simulate_model(mesh, model, Tsb, Tbm[i])
        else:
            sim = mesh.simulate_spherical(model, Tsb, Tbm[i], bvh=True, nthreads=nthreads)
        s = orc.statistics_p2l_exact(ident, ds_points, ds_mask, sim["points"], sim["normals"], sim["hits"], max_dist)
        Ts = orc.umeyama(s)
        out[i] = orc.tmult(orc.tmult(Tsb, Ts), orc.tinv(Tsb))
        stats[i] = s
    return out, stats
