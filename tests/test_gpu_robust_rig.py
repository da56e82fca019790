"""ROBUST MICP FOR SENSOR RIGS on the device (rmcl_amd/csrc/robust.hip, pose_information.hip; include/rmclhip.h) against
the numpy restatement tests/robust_rig_ref.py on the rigs of tests/robust_rig_cases.py, whose premise tests/test_robust_rig_cpu.py asserts
without a device.  The restatement runs on the buffers the device's own finds left (modelView()).

Scales, medians and counts exact; poses within the README's 1e-5; the double sums within the any-order bound n * 2^-52 * sum |terms|."""
import numpy as np
import pytest

import micp_multi_cases as mmc
import pose_information_cases as pic
import robust_cases as rc
import robust_ref as rr
import robust_rig_cases as rgc
import robust_rig_ref as rgr

pytestmark = pytest.mark.gpu

F = np.float32
EPS64 = 2.0 ** -52


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def _operators(ra, hm, sensors):
    ops = []
    for s in sensors:
        op = mmc.make_operator(ra, hm, s)
        op.setTsb(s["Tsb"])
        ops.append(op)
    return ops


def _run(ra, ops, sensors, params, n_iter, Tom=None, progress=0.0, multipliers="own"):
    """the module function on a rig: params one restatement dict for all sensors or one per sensor"""
    T = ra.types
    per = params if isinstance(params, (list, tuple)) else [params] * len(ops)
    w = [s["w"] for s in sensors] if multipliers == "own" else multipliers
    return ra.micp_correct_once_robust(ops, T.identity() if Tom is None else Tom, np.array([s["Tbo"] for s in sensors], dtype=T.TRANSFORM), w,
                                       [rgc.params_of(ra, p) for p in per], n_iter, progress)


def _restate(orc, ops, sensors, params, n_iter, progress=0.0, multipliers=None):
    """the restatement on the buffers the operators' last finds left"""
    ref = rgc.ref_sensors(sensors, params, buffers=[op.modelView() for op in ops], multipliers=multipliers)
    md = [float(orc.adaptive_max_dist(s["max_dist"], s["adaptive_min"], progress)) for s in sensors]
    return rgr.rig_loop(orc, ref, n_iter, max_dists=md), ref, md


def _pre_transform(T, s, T_onew_oold):
    T_b = T.mult(T.mult(T.inv(s["Tbo"]), T_onew_oold), s["Tbo"])
    return T.mult(T.mult(T.inv(s["Tsb"]), T_b), s["Tsb"])


def _plain(ra, ops, sensors, Tom, n_iter, progress=0.0, multipliers=None):
    """rmclhip_micp_correct_once in its per-iteration form (set_micp_fast(0)) on the same handles -> (T_onew_oold, merged)"""
    ms = [ra.MICPSensor(s["name"], op, Tsb=s["Tsb"], Tbo=s["Tbo"], merge_weight_multiplier=s["w"] if multipliers is None else multipliers[k])
          for k, (op, s) in enumerate(zip(ops, sensors))]
    loc = ra.MICPLocalization(ms, optimization_iterations=n_iter)
    loc.convergence_progress_ = progress
    for op in ops:
        op.set_micp_fast(0)
    try:
        return loc._device_loop(Tom)
    finally:
        for op in ops:
            op.set_micp_fast(1)


@pytest.fixture(scope="module")
def maps(ra, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            v, f, _ = mmc.mesh_arrays(name)
            cache[name] = ra.import_hip_map(ctx, v, f)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def rig(ra, orc, ctx):
    r = rgc.rig(orc)
    hm = ra.import_hip_map(ctx, *r["scan"]["map"])
    return dict(r, ops=_operators(ra, hm, r["sensors"]))


@pytest.fixture(scope="module")
def edge(ra, maps):
    cache = {}

    def get(name):
        if name not in cache:
            case = mmc.cases()[name]
            cache[name] = (case, _operators(ra, maps(case.mesh_name), case.sensors))
        return cache[name]
    return get


# ---- 1. NONE is the plain loop ------------------------------------------------------------------------------------------------------------
def test_none_equals_the_plain_loop(ra, orc, edge):
    T = ra.types
    case, ops = edge("mixed4")
    w = list(rgc.NONE_MULTIPLIERS)
    p = rr.params(rr.NONE)
    want_T, want_merged = _plain(ra, ops, case.sensors, case.Tom, 1, multipliers=w)
    got_T, got_merged, W, stats = _run(ra, ops, case.sensors, p, 1, Tom=case.Tom, multipliers=w)
    assert got_T.tobytes() == want_T.tobytes() and got_merged.tobytes() == want_merged.tobytes()
    assert W == float(int(want_merged["n_meas"])) == sum(float(st["weight_sum"]) for st in stats)
    # five iterations: the plain loop's fifth reduction runs at the pre-transforms its first four leave
    T4, _ = _plain(ra, ops, case.sensors, case.Tom, 4, multipliers=w)
    T5, merged5 = _plain(ra, ops, case.sensors, case.Tom, 5, multipliers=w)
    plain_n = [int(op.computeCrossStatistics(_pre_transform(T, s, T4), 0.0)["n_meas"]) for op, s in zip(ops, case.sensors)]
    got_T, got_merged, _, stats = _run(ra, ops, case.sensors, p, 5, Tom=case.Tom, multipliers=w)
    assert [int(st["stats"]["n_meas"]) for st in stats] == plain_n and min(plain_n) > 0
    assert rgc.delta(orc, T5, got_T) <= rc.POSE_BAR, rgc.delta(orc, T5, got_T)
    print("NONE, 5 iterations: T bytes equal %s, merged bytes equal %s, pose delta %.3g" %
          (got_T.tobytes() == T5.tobytes(), got_merged.tobytes() == merged5.tobytes(), rgc.delta(orc, T5, got_T)))


# ---- 2. the contaminated rig --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", rgc.KERNELS)
def test_contaminated_rig_against_the_restatement(ra, orc, rig, kernel):
    T = ra.types
    s, sensors, ops = rig["scan"], rig["sensors"], rig["ops"]
    p = rr.params(kernel)
    got_T, merged, W, stats = _run(ra, ops, sensors, p, rc.SCAN_ITER)
    res, ref, md = _restate(orc, ops, sensors, p, rc.SCAN_ITER)
    for k in range(2):
        c, med, _ = res["scales"][k]
        assert F(stats[k]["scale"]).tobytes() == F(c).tobytes() and F(stats[k]["median_abs_residual"]).tobytes() == F(med).tobytes(), k
        assert int(stats[k]["stats"]["n_meas"]) == res["stats"][k]["n_meas"] > 0, k
    assert rgc.delta(orc, res["T"], got_T) <= rc.POSE_BAR, rgc.delta(orc, res["T"], got_T)
    assert int(merged["n_meas"]) == sum(int(st["stats"]["n_meas"]) for st in stats)
    assert abs(W - sum(float(st["weight_sum"]) for st in stats)) <= 1e-9 * W
    # merged_out is the fold of the sensors' own statistics, carried to the odometry frame, with weight_sum_s and NOT with the
    # multiplier: the host's merge and frame change are the device's definitions (devmath.h), so the bytes are the same
    hand, hand_W = T.cross_statistics_identity(), 0.0
    for sn, st in zip(sensors, stats):
        Cs_o = T.cross_statistics_transform(sn["Tbo"], T.cross_statistics_transform(sn["Tsb"], st["stats"]))
        hand, hand_W = T.cross_statistics_merge_weighted(hand, hand_W, Cs_o, float(st["weight_sum"]))
    assert merged.tobytes() == hand.tobytes() and W == hand_W
    with_multiplier, _ = T.cross_statistics_merge_weighted(
        T.cross_statistics_transform(sensors[0]["Tbo"], T.cross_statistics_transform(sensors[0]["Tsb"], stats[0]["stats"])),
        float(stats[0]["weight_sum"]) * sensors[0]["w"],
        T.cross_statistics_transform(sensors[1]["Tbo"], T.cross_statistics_transform(sensors[1]["Tsb"], stats[1]["stats"])),
        float(stats[1]["weight_sum"]) * sensors[1]["w"])
    assert with_multiplier.tobytes() != merged.tobytes()          # the premise: the two merges of this rig differ
    # ... and it is the restatement's merged: float32 means of coordinates below 8 m and covariances below 16 m^2, a few ulps of
    # those (2^-21, 2^-20) for the merge's roundings plus the pose bar for the pre-transforms the two loops reduce at
    for name in ("dataset_mean", "model_mean"):
        for k in "xyz":
            assert abs(float(merged[name][k]) - float(res["merged"][name][k])) <= 8 * 2.0 ** -21 + 10 * rc.POSE_BAR, (name, k)
    assert np.all(np.abs(merged["covariance"].astype(np.float64) - res["merged"]["covariance"].astype(np.float64)) <= 8 * 2.0 ** -20 + 160 * rc.POSE_BAR)
    assert abs(W - res["merged_weight"]) <= 1e-3 * W
    # the last iteration's statistics, each against the restatement at the pre-transform the DEVICE reduced at (its n_iter - 1 result)
    T_prev = _run(ra, ops, sensors, p, rc.SCAN_ITER - 1)[0]
    for k, (sn, rs) in enumerate(zip(sensors, ref)):
        at = rr.robust_statistics(_pre_transform(T, sn, T_prev), rs["ds"], rs["mask"], rs["points"], rs["normals"], rs["hits"], md[k], p,
                                  scale=res["scales"][k])
        rr.assert_matches(stats[k], at, "%s sensor %d" % (rr.NAMES[kernel], k))
    # closer to the truth than the plain rig call
    plain_T, _ = _plain(ra, ops, sensors, T.identity(), rc.SCAN_ITER)
    e_rob, e_plain = rc.pose_error(orc, got_T, s), rc.pose_error(orc, plain_T, s)
    print("%s: device robust rig %.6f m %.6f rad | device plain rig %.6f m %.6f rad | restatement %.6f m" %
          (rr.NAMES[kernel], e_rob[0], e_rob[1], e_plain[0], e_plain[1], rc.pose_error(orc, res["T"], s)[0]))
    assert e_rob[0] < e_plain[0]
    # two runs, the same bytes
    again = _run(ra, ops, sensors, p, rc.SCAN_ITER)
    assert again[0].tobytes() == got_T.tobytes() and again[1].tobytes() == merged.tobytes() and again[2] == W
    assert again[3].tobytes() == stats.tobytes()
    # the sensors in the other order: another order of the merge's float32 additions, the same pose within the bar
    swapped = _run(ra, ops[::-1], sensors[::-1], p, rc.SCAN_ITER)
    assert rgc.delta(orc, got_T, swapped[0]) <= rc.POSE_BAR, rgc.delta(orc, got_T, swapped[0])
    assert [int(st["stats"]["n_meas"]) for st in swapped[3]] == [int(st["stats"]["n_meas"]) for st in stats][::-1]


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------------
def test_one_sensor_is_the_single_sensor_loop(ra, edge):
    case, ops = edge("one")
    p = rr.params(rr.TUKEY)
    s = case.sensors[0]
    got_T, merged, W, stats = _run(ra, ops, case.sensors, p, case.n_iter, Tom=case.Tom)
    want_T, want_st = ops[0].correct_once_robust(case.Tom, s["Tbo"], case.n_iter, 0.0, rgc.params_of(ra, p))
    assert got_T.tobytes() == want_T.tobytes() and stats[0].tobytes() == want_st.tobytes()
    assert int(merged["n_meas"]) == int(want_st["stats"]["n_meas"]) > 0 and W == float(want_st["weight_sum"]) > 0.0


def test_empty_member_and_rigs_that_say_nothing(ra, orc, edge):
    T = ra.types
    p = rr.params(rr.HUBER)
    case, ops = edge("empty_member")
    got_T, merged, W, stats = _run(ra, ops, case.sensors, p, case.n_iter, Tom=case.Tom)
    assert [int(st["stats"]["n_meas"]) for st in stats][0] == 0 and int(stats[2]["stats"]["n_meas"]) == 0
    assert int(stats[1]["stats"]["n_meas"]) > 0 and int(merged["n_meas"]) == int(stats[1]["stats"]["n_meas"])
    alone = _run(ra, ops[1:2], case.sensors[1:2], p, case.n_iter, Tom=case.Tom)
    assert rgc.delta(orc, alone[0], got_T) <= rc.POSE_BAR, rgc.delta(orc, alone[0], got_T)
    assert rgc.delta(orc, T.identity(), got_T) > 10 * rc.POSE_BAR          # and it did move
    for name in ("all_empty", "all_weight_zero"):
        case, ops = edge(name)
        got_T, merged, W, stats = _run(ra, ops, case.sensors, p, case.n_iter, Tom=case.Tom)
        assert got_T.tobytes() == T.identity().tobytes(), name
        if name == "all_empty":
            assert W == 0.0 and int(merged["n_meas"]) == 0 and all(int(st["stats"]["n_meas"]) == 0 for st in stats)
        else:
            # the sensors see, their multipliers say nothing: the unweighted merge still reports them
            assert W > 0.0 and int(merged["n_meas"]) == sum(int(st["stats"]["n_meas"]) for st in stats) > 0


def test_a_sensor_without_weight_still_counts(ra, orc, rig):
    sensors, ops = rig["sensors"], rig["ops"]
    per = [rr.params(rr.TUKEY, scale=1e-30), rr.params(rr.TUKEY)]
    got_T, merged, W, stats = _run(ra, ops, sensors, per, 3)
    res, _, _ = _restate(orc, ops, sensors, per, 3)
    assert res["stats"][0]["weight_sum"] == 0.0 and res["stats"][0]["n_meas"] > 0          # the premise, on the restatement
    assert float(stats[0]["weight_sum"]) == 0.0 and int(stats[0]["stats"]["n_meas"]) == res["stats"][0]["n_meas"]
    assert int(merged["n_meas"]) == int(stats[0]["stats"]["n_meas"]) + int(stats[1]["stats"]["n_meas"])
    assert W == float(stats[1]["weight_sum"]) > 0.0
    assert rgc.delta(orc, res["T"], got_T) <= rc.POSE_BAR


@pytest.mark.parametrize("name,n_iter,progress", [("short_dataset", 5, 0.0), ("mixed4", 0, 0.0), ("mixed4", 1, 0.0), ("mixed4", 5, 0.5)])
def test_edge_rigs_against_the_restatement(ra, orc, edge, name, n_iter, progress):
    T = ra.types
    case, ops = edge(name)
    p = [rr.params(rr.TUKEY), rr.params(rr.HUBER), rr.params(rr.CAUCHY), rr.params(rr.HUBER, scale=0.05)][:len(ops)]
    got_T, merged, W, stats = _run(ra, ops, case.sensors, p, n_iter, Tom=case.Tom, progress=progress)
    if n_iter == 0:
        assert got_T.tobytes() == T.identity().tobytes() and W == 0.0 and not np.any(np.frombuffer(merged.tobytes(), np.uint8))
        for k, st in enumerate(stats):
            assert int(st["stats"]["n_meas"]) == 0 and float(st["weight_sum"]) == 0.0
            assert F(st["scale"]) == (F(p[k]["scale"]) if p[k]["scale_mode"] == rr.FIXED else F(p[k]["scale_min"]))
        return
    res, _, md = _restate(orc, ops, case.sensors, p, n_iter, progress)
    got_n = [int(st["stats"]["n_meas"]) for st in stats]
    assert got_n == [st["n_meas"] for st in res["stats"]] and sum(got_n) == int(merged["n_meas"]) > 0
    for k, st in enumerate(stats):
        assert F(st["scale"]).tobytes() == F(res["scales"][k][0]).tobytes(), k
    assert rgc.delta(orc, res["T"], got_T) <= rc.POSE_BAR, rgc.delta(orc, res["T"], got_T)
    if progress > 0.0:
        # the tighter gate is every sensor's: the counts are not the ones of the open gate
        assert all(abs(m - 0.5) < 1e-6 for m in md)
        open_n = [int(st["stats"]["n_meas"]) for st in _run(ra, ops, case.sensors, p, n_iter, Tom=case.Tom)[3]]
        assert all(a <= b for a, b in zip(got_n, open_n)) and got_n != open_n


def test_eight_sensors_run_nine_are_refused(ra, orc, edge):
    T = ra.types
    case, ops = edge("eight")
    p = rr.params(rr.CAUCHY)
    got_T, merged, W, stats = _run(ra, ops, case.sensors, p, case.n_iter, Tom=case.Tom)
    res, _, _ = _restate(orc, ops, case.sensors, p, case.n_iter)
    assert [int(st["stats"]["n_meas"]) for st in stats] == [st["n_meas"] for st in res["stats"]]
    assert rgc.delta(orc, res["T"], got_T) <= rc.POSE_BAR, rgc.delta(orc, res["T"], got_T)
    with pytest.raises(ra.RmclHipError, match="at most 8 sensors"):
        _run(ra, ops + ops[:1], case.sensors + case.sensors[:1], p, case.n_iter, Tom=case.Tom)
    again = _run(ra, ops, case.sensors, p, case.n_iter, Tom=case.Tom)
    assert again[0].tobytes() == got_T.tobytes() and again[3].tobytes() == stats.tobytes()


def test_bad_parameters_name_their_sensor_and_change_nothing(ra, edge):
    case, ops = edge("mixed4")
    p = rr.params(rr.TUKEY)
    before = _run(ra, ops, case.sensors, p, 3, Tom=case.Tom)
    bad = [rr.params(rr.TUKEY) for _ in ops]
    bad[2] = dict(bad[2], tuning=F("nan"))
    with pytest.raises(ra.RmclHipError, match=r"sensor 2: tuning"):
        _run(ra, ops, case.sensors, bad, 3, Tom=case.Tom)
    with pytest.raises(ra.RmclHipError, match=r"sensor 1: merge_weight_multiplier"):
        _run(ra, ops, case.sensors, p, 3, Tom=case.Tom, multipliers=[1.0, -0.5, 1.0, 1.0])
    with pytest.raises(ra.RmclHipError, match=r"sensor 3: the same operator as sensor 0"):
        _run(ra, ops[:3] + ops[:1], case.sensors, p, 3, Tom=case.Tom)
    after = _run(ra, ops, case.sensors, p, 3, Tom=case.Tom)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes() and after[3].tobytes() == before[3].tobytes()


# ---- 4. weighted pose information ----------------------------------------------------------------------------------------------------------
INFO_MODEL_H, INFO_MODEL_W = 130, 128          # 16 640 rays: every size of pose_information_cases.FREE_SIZES as min(dataset, model)


@pytest.fixture(scope="module")
def info_scan(ra, ctx):
    """one operator on the cube room whose dataset is its own scan at the truth with every eighth ray shortened; the find runs 5 cm off"""
    import math
    from rmcl_amd import synthetic as syn, types as T
    hm = ra.import_hip_map(ctx, *syn.cube_room())
    model = T.spherical_model(F(-0.6), F(1.2 / (INFO_MODEL_H - 1)), INFO_MODEL_H, F(-math.pi), F(2 * math.pi / INFO_MODEL_W), INFO_MODEL_W, F(0.1),
                              F(60.0))
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(syn.tsb_offset())
    rcc.setModel(model)
    rcc.params.max_dist = rcc.adaptive_max_dist_min = 0.3
    truth = syn.pose_c2_truth()
    rcc.find(truth)
    at = rcc.modelView()
    pts = at["points"].copy()
    rng = np.random.RandomState(12)
    short = (np.arange(len(pts)) % 8) == 5
    pts[short] = (pts[short] * (1.0 - rng.uniform(0.01, 0.08, (int(short.sum()), 1)))).astype(F)
    pts[at["hits"] == 0] = 0.0
    estimate = T.mult(truth, T.transform_from_rpy((0.05, -0.03, 0.02), (0.0, 0.0, 0.01)))
    return dict(rcc=rcc, pts=pts, mask=at["hits"].astype(np.uint8), estimate=estimate)


@pytest.mark.parametrize("n", pic.FREE_SIZES)
def test_weighted_information_at_every_row_count(ra, info_scan, n):
    T = ra.types
    rcc = info_scan["rcc"]
    pts, mask = info_scan["pts"][:n], info_scan["mask"][:n]
    rcc.set_dataset(pts, mask)
    rcc.find(info_scan["estimate"])
    mv = rcc.modelView()
    I, N, hits = mv["points"][:n], mv["normals"][:n], mv["hits"][:n]
    print("n = %d: rows = %d" % (n, pic.rows(n)))
    for Tpre in (T.identity(), T.transform_from_rpy((0.01, -0.02, 0.005), (0.001, 0.0, -0.003))):
        plain = rcc.computePoseInformation(Tpre, 0.0)
        none = rcc.pose_information_robust(Tpre, 0.0, "none")
        assert none["info"].tobytes() == plain.tobytes()
        assert float(none["weight_sum"]) == float(int(plain["n_meas"])) and 0.3 * n < int(plain["n_meas"])
        for kernel in rgc.KERNELS:
            p = rr.params(kernel)
            got = rcc.pose_information_robust(Tpre, 0.0, rgc.params_of(ra, p))
            ref = rgr.pose_information_weighted(Tpre, pts, mask, I, N, hits, 0.3, p)
            what = "n=%d %s" % (n, rr.NAMES[kernel])
            assert int(got["info"]["n_meas"]) == ref["n_meas"], what
            assert F(got["scale"]).tobytes() == F(ref["c"]).tobytes() and F(got["median_abs_residual"]).tobytes() == F(ref["median"]).tobytes(), what
            nm = ref["n_meas"]
            for key in ("A", "g", "rss"):
                err = np.abs(np.asarray(got["info"][key], np.float64) - np.asarray(ref[key]))
                assert np.all(err <= nm * EPS64 * np.asarray(ref[key + "_abs"])), (what, key, float(err.max()))
            for key in ("weight_sum", "rss_unweighted"):
                assert abs(float(got[key]) - ref[key]) <= nm * EPS64 * ref[key + "_abs"], (what, key)
            assert np.array_equal(got["info"]["A"], got["info"]["A"].T)
            st = rcc.compute_robust_statistics(Tpre, 0.0, rgc.params_of(ra, p))
            assert abs(float(got["weight_sum"]) - float(st["weight_sum"])) <= nm * EPS64 * ref["weight_sum_abs"], what
            assert abs(float(got["info"]["rss"]) - float(st["wrss"])) <= nm * EPS64 * ref["rss_abs"], what
            assert rcc.pose_information_robust(Tpre, 0.0, rgc.params_of(ra, p)).tobytes() == got.tobytes(), what


def test_weighted_information_discounts_the_pallet(ra, rig):
    """on the contaminated lidar the weighted A is smaller than the plain A along the normal of the wall behind the shortened sector;
    the call only reads: moment set and ccs_info stay"""
    T = ra.types
    s, sn, rcc = rig["scan"], rig["sensors"][0], rig["ops"][0]
    p = rgc.params_of(ra, rr.params(rr.TUKEY))
    Tc, _ = rcc.correct_once_robust(T.identity(), s["estimate"], rc.SCAN_ITER, 0.0, p)
    Ts = _pre_transform(T, sn, Tc)
    before = rcc.computeCrossStatistics(T.identity(), 0.0)
    i0 = rcc.ccs_info()
    plain = rcc.computePoseInformation(Ts, 0.0)
    rob = rcc.pose_information_robust(Ts, 0.0, p)
    assert rcc.ccs_info() == i0
    assert rcc.computeCrossStatistics(T.identity(), 0.0).tobytes() == before.tobytes()
    mv = rcc.modelView()
    valid = s["short"] & (mv["hits"] > 0)
    d = mv["normals"][valid].astype(np.float64).mean(axis=0)
    d /= np.linalg.norm(d)
    a_plain, a_rob = float(d @ plain["A"][:3, :3] @ d), float(d @ rob["info"]["A"][:3, :3] @ d)
    cov_plain, cov_rob = T.pose_covariance(plain), T.pose_covariance_robust(rob)
    print("along the pallet's wall normal %s: plain A %.3f, weighted A %.3f | covariance trace plain %.6g (s2 %.3g), robust %.6g (s2 %.3g) | "
          "weight_sum %.1f of n_meas %d" % (np.round(d, 3), a_plain, a_rob, float(np.trace(cov_plain["covariance"])), float(cov_plain["s2"]),
                                            float(np.trace(cov_rob["covariance"])), float(cov_rob["s2"]), float(rob["weight_sum"]),
                                            int(rob["info"]["n_meas"])))
    assert a_rob < a_plain
    assert int(rob["info"]["n_meas"]) == int(plain["n_meas"]) and float(rob["weight_sum"]) < int(plain["n_meas"])
    assert float(rob["rss_unweighted"]) > float(rob["info"]["rss"]) > 0.0


# ---- 5. MICPLocalization --------------------------------------------------------------------------------------------------------------
def test_micp_localization_runs_the_rig(ra, rig):
    T = ra.types
    s, sensors, ops = rig["scan"], rig["sensors"], rig["ops"]
    own = T.robust_params("huber")
    ms = [ra.MICPSensor(sn["name"], op, Tsb=sn["Tsb"], Tbo=sn["Tbo"], merge_weight_multiplier=sn["w"]) for op, sn in zip(ops, sensors)]
    ms[1].robust = own                                     # a sensor's own setting wins over the localization's
    loc = ra.MICPLocalization(ms, optimization_iterations=rc.SCAN_ITER, adaptive_max_dist=False, robust="tukey")
    got = loc.correctOnce(device_loop=True)
    want = ra.micp_correct_once_robust(ops, T.identity(), np.array([sn["Tbo"] for sn in sensors], dtype=T.TRANSFORM), [sn["w"] for sn in sensors],
                                       ["tukey", own], rc.SCAN_ITER, 0.0)
    assert got.tobytes() == want[0].tobytes()
    assert isinstance(loc.robust_statistics_latest_, list) and len(loc.robust_statistics_latest_) == 2
    assert all(a.tobytes() == b.tobytes() for a, b in zip(loc.robust_statistics_latest_, want[3]))
    assert loc.correction_stats_latest_["valid_matches"] == int(want[1]["n_meas"])
    all_tukey = ra.micp_correct_once_robust(ops, T.identity(), np.array([sn["Tbo"] for sn in sensors], dtype=T.TRANSFORM),
                                            [sn["w"] for sn in sensors], "tukey", rc.SCAN_ITER, 0.0)
    assert all_tukey[3][1].tobytes() != want[3][1].tobytes()
    # the host loop still refuses several sensors
    loc2 = ra.MICPLocalization(ms, optimization_iterations=3, robust="tukey")
    with pytest.raises(NotImplementedError, match="one sensor"):
        loc2.correctOnce()
    with pytest.raises(NotImplementedError, match="device_loop=True"):
        loc2.correctOnce(device_loop=False)
    # the weighted information of the rig = the per-sensor records carried to the odometry frame and merged by hand
    merged, cov = loc.poseInformation(got, robust=True)
    hand = T.pose_information_identity()
    wsum = 0.0
    for m, sn, setting in zip(ms, sensors, ("tukey", own)):
        rec = m.correspondences_.pose_information_robust(_pre_transform(T, sn, got), 0.0, setting)
        hand = T.pose_information_merge(hand, T.pose_information_transform(sn["Tbo"], T.pose_information_transform(sn["Tsb"], rec["info"])), sn["w"])
        wsum += sn["w"] * float(rec["weight_sum"])
    assert merged.tobytes() == hand.tobytes()
    assert float(cov["s2"]) == float(hand["rss"]) / (wsum - 6.0)
    plain_merged, _ = loc.poseInformation(got)
    assert int(plain_merged["n_meas"]) == int(merged["n_meas"]) and float(plain_merged["rss"]) > float(merged["rss"])
