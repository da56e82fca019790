"""ROBUST MICP on the device (rmcl_amd/csrc/robust.hip; include/rmclhip.h) against the numpy restatement
tests/robust_ref.py, on the cases of tests/robust_cases.py, whose premises tests/test_robust_cases_cpu.py asserts without a device.

Per-element weights byte for byte; the median, the count and the scale exact; the double sums within the any-order bound
n * 2^-52 * sum |terms|; poses within the README's 1e-5."""

import numpy as np
import pytest

import pose_batch_cases as pc
import pose_information_cases as pic
import robust_cases as rc
import robust_ref as rr

pytestmark = pytest.mark.gpu

F = np.float32


def _params(ra, p):
    """the ctypes twin of a restatement's parameter dict"""
    q = ra._capi.RobustParams()
    q.kernel, q.scale_mode, q.scale, q.tuning, q.scale_min, q.reserved = p["kernel"], p["scale_mode"], p["scale"], p["tuning"], p["scale_min"], 0
    return q


class _Dev:
    """device copies of a case's arrays, freed together"""

    def __init__(self, ra, ctx, case, keys=("D", "I", "N", "dmask", "mmask")):
        self.ra, self.ctx = ra, ctx
        self.n = len(case["D"])
        self.dev = {k: ra.DeviceArray.from_host(ctx, case[k]) for k in keys if len(case[k])}

    def args(self, max_dist, use_d=True, use_m=True, pts="I", nrm="N"):
        d = self.dev
        return (d["D"], d["dmask"] if use_d else None, d[pts], d[nrm], d["mmask"] if use_m else None, self.n, float(max_dist))

    def free(self):
        for d in self.dev.values():
            d.free()


def _run(ra, ctx, dev, Tpre, max_dist, p, weights=False, **kw):
    w = ra.DeviceArray(ctx, np.float32, max(dev.n, 1)) if weights else None
    try:
        got = ra.statistics_p2l_robust(ctx, Tpre, *dev.args(max_dist, **kw), robust=_params(ra, p), weights_out=w)
        return (got, w.download()[:dev.n].copy()) if weights else got
    finally:
        if w is not None:
            w.free()


# ---- 1. weights ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", rr.KERNELS)
def test_weights_byte_for_byte(ra, ctx, kernel):
    T = ra.types
    case = rc.weights_case()
    dev = _Dev(ra, ctx, case)
    try:
        for c in rc.GRID_C:
            p = rr.params(kernel, scale=c)
            ref = rr.robust_statistics(T.identity(), case["D"], case["dmask"], case["I"], case["N"], case["mmask"], rc.MAX_DIST, p)
            got, w = _run(ra, ctx, dev, T.identity(), rc.MAX_DIST, p, weights=True)
            assert w.tobytes() == ref["w"].tobytes(), (rr.NAMES[kernel], c, np.flatnonzero(w.view(np.uint32) != ref["w"].view(np.uint32))[:8])
            assert not w[case["poison"]].any() and not w[~ref["kept"]].any()
            rr.assert_matches(got, ref, "%s c=%g" % (rr.NAMES[kernel], c))
        # the MAD scale of the same elements
        p = rr.params(kernel)
        ref = rr.robust_statistics(T.identity(), case["D"], case["dmask"], case["I"], case["N"], case["mmask"], rc.MAX_DIST, p)
        got, w = _run(ra, ctx, dev, T.identity(), rc.MAX_DIST, p, weights=True)
        assert w.tobytes() == ref["w"].tobytes()
        rr.assert_matches(got, ref, "%s MAD" % rr.NAMES[kernel])
    finally:
        dev.free()


# ---- 2. sums at the reduction's edges ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sums(ra, ctx):
    cache = {}

    def get(n, far=False):
        if (n, far) not in cache:
            case = rc.sum_case(n, far)
            cache[(n, far)] = (case, _Dev(ra, ctx, case, ("D", "I", "N", "I_nan", "N_nan", "dmask", "mmask")))
        return cache[(n, far)]
    yield get
    for _, d in cache.values():
        d.free()


SUMS = [(n, False) for n in rc.SUM_SIZES] + [(n, True) for n in rc.SUM_FAR] + [(1, False)]


@pytest.mark.parametrize("n,far", SUMS)
def test_sums_at_every_row_count(ra, ctx, sums, n, far):
    T = ra.types
    case, dev = sums(n, far)
    print("n = %d, far = %s: rows = %d" % (n, far, pic.rows(n)))
    for which in ("identity", "general"):
        Tpre = T.identity() if which == "identity" else pic.tpre_general(far)
        for name, make in rc.SUM_PARAMS:
            p = make()
            what = "n=%d far=%s Tpre=%s %s" % (n, far, which, name)
            ref = rc.sum_reference(case, Tpre, p)
            got, w = _run(ra, ctx, dev, Tpre, rc.SUM_MAX_DIST, p, weights=True, pts="I_nan", nrm="N_nan")
            rr.assert_matches(got, ref, what)
            assert w.tobytes() == ref["w"].tobytes(), what
            assert _run(ra, ctx, dev, Tpre, rc.SUM_MAX_DIST, p, pts="I_nan", nrm="N_nan").tobytes() == got.tobytes(), what
            if n > 1:
                assert 0.3 * n <= ref["n_meas"] <= 0.7 * n, what


def test_sums_at_the_row_cap(ra, ctx):
    T = ra.types
    n = pic.CAP_SIZE
    case = rc.sum_case(n)
    dev = _Dev(ra, ctx, case, ("D", "I_nan", "N_nan", "dmask", "mmask"))
    try:
        p = rr.params(rr.HUBER)
        ref = rc.sum_reference(case, T.identity(), p)
        got = _run(ra, ctx, dev, T.identity(), rc.SUM_MAX_DIST, p, pts="I_nan", nrm="N_nan")
        rr.assert_matches(got, ref, "cap")
        assert _run(ra, ctx, dev, T.identity(), rc.SUM_MAX_DIST, p, pts="I_nan", nrm="N_nan").tobytes() == got.tobytes()
        assert pic.rows(n) == 1024 and 0.3 * n <= ref["n_meas"] <= 0.7 * n
        # 1024 rows take the fold's longest loop: weight one still gives the plain reduction's bytes
        plain = ra.statistics_p2l(ctx, T.identity(), *dev.args(rc.SUM_MAX_DIST, pts="I_nan", nrm="N_nan"))
        none = _run(ra, ctx, dev, T.identity(), rc.SUM_MAX_DIST, rr.params(rr.NONE), pts="I_nan", nrm="N_nan")
        assert none["stats"].tobytes() == plain.tobytes() and float(none["weight_sum"]) == float(int(plain["n_meas"]))
    finally:
        dev.free()


def test_no_element(ra, ctx):
    T = ra.types
    for p, c in ((rr.params(rr.TUKEY), F(1e-3)), (rr.params(rr.TUKEY, scale_min=0.02), F(0.02)), (rr.params(rr.HUBER, scale=0.3), F(0.3))):
        got = ra.statistics_p2l_robust(ctx, T.identity(), None, None, None, None, None, 0, 1.0, robust=_params(ra, p))
        assert int(got["stats"]["n_meas"]) == 0 and float(got["weight_sum"]) == 0.0 and float(got["rss"]) == 0.0
        assert F(got["scale"]) == c and float(got["median_abs_residual"]) == 0.0
        assert not np.frombuffer(got["stats"].tobytes(), np.uint8).any()


def test_one_element(ra, ctx):
    """n = 1: the median is the element, one correspondence has no covariance"""
    T = ra.types
    case = rc.line_case(np.array([-0.2], F))
    dev = _Dev(ra, ctx, case)
    try:
        for kernel in rr.KERNELS:
            p = rr.params(kernel)
            ref = rr.robust_statistics(T.identity(), case["D"], None, case["I"], case["N"], None, rc.MAX_DIST, p)
            got, w = _run(ra, ctx, dev, T.identity(), rc.MAX_DIST, p, weights=True, use_d=False, use_m=False)
            rr.assert_matches(got, ref, rr.NAMES[kernel])
            assert ref["n_meas"] == 1 and F(got["median_abs_residual"]) == F(0.2) and w.tobytes() == ref["w"].tobytes()
            assert not np.asarray(got["stats"]["covariance"]).any()
    finally:
        dev.free()


# ---- 3. weight one is the plain reduction --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,far", [(513, False), (8193, False), (8193, True), (16385, False), (1, False)])
def test_weight_one_gives_the_plain_reduction_bytes(ra, ctx, sums, n, far):
    T = ra.types
    case, dev = sums(n, far)
    for which in ("identity", "general"):
        Tpre = T.identity() if which == "identity" else pic.tpre_general(far)
        plain = ra.statistics_p2l(ctx, Tpre, *dev.args(rc.SUM_MAX_DIST, pts="I_nan", nrm="N_nan"))
        for p in (rr.params(rr.NONE), rr.params(rr.NONE, scale=0.01), rr.params(rr.HUBER, scale=float(rc.SUM_MAX_DIST)),
                  rr.params(rr.HUBER, scale=5.0)):
            got = _run(ra, ctx, dev, Tpre, rc.SUM_MAX_DIST, p, pts="I_nan", nrm="N_nan")
            assert got["stats"].tobytes() == plain.tobytes(), (n, far, which, p)
            assert float(got["weight_sum"]) == float(int(plain["n_meas"]))
    if n > 1:
        assert int(plain["n_meas"]) > 0.3 * n


# ---- 4. the median -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recompute", (0, 1))
def test_median_is_exact(ra, ctx, recompute):
    T = ra.types
    cases = rc.median_cases()
    L = ra._capi.lib()
    ra._capi.check(L.rmclhip_debug_robust_select_recompute(recompute))
    try:
        seen = {}
        for name, (r, m) in cases.items():
            case = rc.line_case(r)
            dev = _Dev(ra, ctx, case)
            try:
                for kernel, tuning in ((rr.HUBER, None), (rr.TUKEY, 2.5)):
                    p = rr.params(kernel, tuning=tuning)
                    ref = rr.robust_statistics(T.identity(), case["D"], None, case["I"], case["N"], None, rc.MAX_DIST, p)
                    got = _run(ra, ctx, dev, T.identity(), rc.MAX_DIST, p, use_d=False, use_m=False)
                    assert ref["m"] == m, name
                    rr.assert_matches(got, ref, "%s %s" % (name, rr.NAMES[kernel]))
                    seen[(name, kernel)] = got
            finally:
                dev.free()
        assert F(seen[("mostly_zero", rr.HUBER)]["scale"]) == F(1e-3) and float(seen[("empty", rr.HUBER)]["weight_sum"]) == 0.0
        assert F(seen[("empty", rr.TUKEY)]["scale"]) == F(1e-3) and int(seen[("empty", rr.TUKEY)]["stats"]["n_meas"]) == 0
        for kernel in (rr.HUBER, rr.TUKEY):
            a, b = seen[("order_a", kernel)], seen[("order_b", kernel)]
            assert F(a["scale"]).tobytes() == F(b["scale"]).tobytes() and F(a["median_abs_residual"]).tobytes() == F(b["median_abs_residual"]).tobytes()
            assert int(a["stats"]["n_meas"]) == int(b["stats"]["n_meas"])
    finally:
        ra._capi.check(L.rmclhip_debug_robust_select_recompute(0))


# ---- 5. on a map ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan(ra, orc, ctx):
    s = rc.contaminated_scan(orc)
    hm = ra.import_hip_map(ctx, *s["map"])
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(s["Tsb"])
    rcc.setModel(s["model"])
    rcc.set_dataset(*s["dataset"])
    rcc.params.max_dist = rc.SCAN_MAX_DIST
    rcc.adaptive_max_dist_min = rc.SCAN_MAX_DIST
    s["rcc"] = rcc
    return s


def _delta(orc, a, b):
    d = orc.tmult(orc.tinv(a), b)
    return max(max(abs(float(d["t"][k])) for k in "xyz"), max(abs(float(d["R"][k])) for k in "xyz"))


@pytest.mark.parametrize("kernel", (rr.TUKEY, rr.HUBER))
def test_correct_once_robust_on_the_contaminated_scan(ra, orc, scan, kernel):
    T = ra.types
    s, rcc = scan, scan["rcc"]
    p = rr.params(kernel)
    rcc.find(s["estimate"])
    before = rcc.computeCrossStatistics(T.identity(), 0.0)
    i0 = rcc.ccs_info()
    assert rcc.computeCrossStatistics(T.identity(), 0.0).tobytes() == before.tobytes()
    i1 = rcc.ccs_info()
    steady = {k: i1[k] - i0[k] for k in i0}            # what one more call costs while the find's moment set stands
    assert steady["calls"] == 1 and steady["passes"] == 0
    # the forms that only read the find's buffers: the moment set and ccs_info stay, the next call is served as the one before
    rcc.compute_robust_statistics(T.identity(), 0.0, _params(ra, p))
    rcc.robust_weights(T.identity(), 0.0, _params(ra, p))
    rcc.residual_scale(T.identity(), 0.0, _params(ra, p))
    assert rcc.ccs_info() == i1
    assert rcc.computeCrossStatistics(T.identity(), 0.0).tobytes() == before.tobytes()
    i2 = rcc.ccs_info()
    assert {k: i2[k] - i1[k] for k in i1} == steady
    # the correction: its find rewrites the model buffers and drops the moment set, as every find does; ccs_info itself is not touched,
    # the next call pays ONE moment pass (no speculation ran) and returns the same bytes, the find having run at the same pose
    Tc, st = rcc.correct_once_robust(T.identity(), s["estimate"], rc.SCAN_ITER, 0.0, _params(ra, p))
    assert rcc.ccs_info() == i2
    after = rcc.computeCrossStatistics(T.identity(), 0.0)
    assert after.tobytes() == before.tobytes()
    i3 = rcc.ccs_info()
    print("ccs_info: steady %s | after the robust correction %s" % (steady, {k: i3[k] - i2[k] for k in i2}))
    assert i3["calls"] == i2["calls"] + 1 and i3["passes"] == i2["passes"] + 1 and i3["speculative_finds"] == i2["speculative_finds"]
    assert i3["from_moments"] - i2["from_moments"] == steady["from_moments"]
    assert rcc.computeCrossStatistics(T.identity(), 0.0).tobytes() == before.tobytes()
    i4 = rcc.ccs_info()
    assert {k: i4[k] - i3[k] for k in i3} == steady     # the new set stands
    # the restatement on the buffers the device's own find left
    mv = rcc.modelView()
    pts, mask = s["dataset"]
    want_T, want_Ts, want_st, want_scale = rr.correct_once(orc, p, rc.SCAN_ITER, s["Tsb"], s["estimate"], pts, mask, mv["points"], mv["normals"],
                                                           mv["hits"], rc.SCAN_MAX_DIST)
    assert F(st["scale"]).tobytes() == F(want_scale[0]).tobytes() and F(st["median_abs_residual"]).tobytes() == F(want_scale[1]).tobytes()
    assert int(st["stats"]["n_meas"]) == want_st["n_meas"]
    assert _delta(orc, want_T, Tc) <= rc.POSE_BAR, _delta(orc, want_T, Tc)
    # closer to the truth than the plain per-iteration loop on the same handle
    rcc.set_micp_fast(0)
    try:
        Tp, _ = rcc.correct_once(T.identity(), s["estimate"], rc.SCAN_ITER, 0.0)
    finally:
        rcc.set_micp_fast(1)
    e_rob, e_plain = rc.pose_error(orc, Tc, s), rc.pose_error(orc, Tp, s)
    print("%s: device robust %.6f m %.6f rad | device plain %.6f m %.6f rad | restatement robust %.6f m" %
          (rr.NAMES[kernel], e_rob[0], e_rob[1], e_plain[0], e_plain[1], rc.pose_error(orc, want_T, s)[0]))
    assert e_rob[0] < e_plain[0]
    # two runs, the same bytes
    Tc2, st2 = rcc.correct_once_robust(T.identity(), s["estimate"], rc.SCAN_ITER, 0.0, _params(ra, p))
    assert Tc2.tobytes() == Tc.tobytes() and st2.tobytes() == st.tobytes()
    # the weights at the result mark the shortened rays
    Ts = T.mult(T.mult(T.inv(T.mult(s["estimate"], s["Tsb"])), Tc), T.mult(s["estimate"], s["Tsb"]))
    w = rcc.robust_weights(Ts, 0.0, _params(ra, p))
    assert len(w) == len(s["short"])
    valid = mv["hits"] > 0
    low_short = float((w[s["short"] & valid] < 0.5).mean())
    low_clean = float((w[~s["short"] & valid] < 0.5).mean())
    print("weights below 0.5: %.3f of the shortened rays, %.3f of the untouched" % (low_short, low_clean))
    assert low_short > low_clean
    # the operator forms agree with the restatement at that pre-transform
    ref = rr.robust_statistics(Ts, pts, mask, mv["points"], mv["normals"], mv["hits"], rc.SCAN_MAX_DIST, p)
    assert w.tobytes() == ref["w"].tobytes()
    rr.assert_matches(rcc.compute_robust_statistics(Ts, 0.0, _params(ra, p)), ref, "operator form")
    c, med, m = rcc.residual_scale(Ts, 0.0, _params(ra, p))
    assert (F(c).tobytes(), F(med).tobytes(), m) == (F(ref["c"]).tobytes(), F(ref["median"]).tobytes(), ref["m"])
    # no iteration: the identity
    T0, st0 = rcc.correct_once_robust(T.identity(), s["estimate"], 0, 0.0, _params(ra, p))
    assert T0.tobytes() == T.identity().tobytes() and int(st0["stats"]["n_meas"]) == 0 and float(st0["weight_sum"]) == 0.0


def test_invalid_parameters_are_refused_before_any_launch(ra, scan):
    T = ra.types
    rcc = scan["rcc"]
    rcc.find(scan["estimate"])
    bad = ra._capi.RobustParams()
    ra._capi.lib().rmclhip_robust_params_default(rr.TUKEY, bad)
    bad.tuning = float("nan")
    for call in (lambda: rcc.correct_once_robust(T.identity(), scan["estimate"], 3, 0.0, bad),
                 lambda: rcc.compute_robust_statistics(T.identity(), 0.0, bad), lambda: rcc.robust_weights(T.identity(), 0.0, bad),
                 lambda: rcc.residual_scale(T.identity(), 0.0, bad)):
        with pytest.raises(ra.RmclHipError, match="tuning"):
            call()


def test_micp_localization_option(ra, orc, scan):
    """robust= on MICPLocalization / MICPSensor: one sensor runs the robust correction, several refuse"""
    T = ra.types
    s, rcc = scan, scan["rcc"]
    sensor = ra.MICPSensor("lidar", rcc, Tsb=s["Tsb"], Tbo=s["estimate"])
    loc = ra.MICPLocalization([sensor], optimization_iterations=rc.SCAN_ITER, adaptive_max_dist=False, robust="tukey")
    got = loc.correctOnce()
    want, st = rcc.correct_once_robust(T.identity(), s["estimate"], rc.SCAN_ITER, 0.0, "tukey")
    assert got.tobytes() == want.tobytes()
    assert loc.robust_statistics_latest_.tobytes() == st.tobytes() and loc.correction_stats_latest_["valid_matches"] == int(st["stats"]["n_meas"])
    # the sensor's own setting serves when the localization has none
    sensor.robust = T.robust_params("tukey")
    loc2 = ra.MICPLocalization([sensor], optimization_iterations=rc.SCAN_ITER, adaptive_max_dist=False)
    assert loc2.correctOnce().tobytes() == want.tobytes()
    two = ra.MICPLocalization([sensor, sensor], optimization_iterations=3, robust="huber")
    with pytest.raises(NotImplementedError, match="one sensor"):
        two.correctOnce()


@pytest.mark.parametrize("kind", ("spherical", "o1dn", "ondn", "pinhole"))
def test_every_sensor_model_class(ra, orc, ctx, kind):
    from rmcl_amd import synthetic as syn, types as T
    hm = ra.import_hip_map(ctx, *pc.map_arrays("cube"))
    rcc = pc.operator(ra, hm, pc.model(kind))            # the 21 x 150 models of tests/pose_batch_cases.py, the smallest the suite keeps for
    Tsb = pc.tsb()                                       # all four classes (O1Dn / OnDn with their NaN direction rows)
    truth = syn.pose_c2_truth()
    estimate = T.mult(truth, T.transform_from_rpy((0.05, -0.04, 0.02), (0.0, 0.0, 0.01)))
    rcc.find(truth)
    at_truth = rcc.modelView()
    pts = at_truth["points"].copy()
    n = len(pts)
    sector = (np.arange(n) % 8) == 3
    rng = np.random.RandomState(9)
    pts[sector] = (pts[sector] * (1.0 - rng.uniform(0.05, 0.15, (int(sector.sum()), 1)))).astype(F)   # shortened towards the sensor's origin
    pts[at_truth["hits"] == 0] = 0.0
    rcc.set_dataset(pts, at_truth["hits"])
    rcc.params.max_dist = rcc.adaptive_max_dist_min = 1.0
    p = rr.params(rr.CAUCHY)
    Tc, st = rcc.correct_once_robust(T.identity(), estimate, 5, 0.0, _params(ra, p))
    mv = rcc.modelView()
    want_T, _, want_st, want_scale = rr.correct_once(orc, p, 5, Tsb, estimate, pts, at_truth["hits"], mv["points"], mv["normals"], mv["hits"], 1.0)
    assert int(st["stats"]["n_meas"]) == want_st["n_meas"] > 0.5 * n
    assert F(st["scale"]).tobytes() == F(want_scale[0]).tobytes()
    assert _delta(orc, want_T, Tc) <= rc.POSE_BAR, (kind, _delta(orc, want_T, Tc))
