"""GPU: rmclhip_micp_correct_once -- the N-sensor MICP correction -- in each of its three loop forms, on rigs of mixed sensor models
and at its edges, against the oracle's loop (tests/oracle_micp.py::correct_once_multi).  The rigs: tests/micp_multi_cases.py;
tests/test_micp_multi_cases_cpu.py shows that they are what they claim and that no correspondence sits on a gate.

One answer, three pieces of code (rmcl_amd/csrc/capi_micp.cpp):
    host            set_micp_fast(1) on every sensor: moments + at most 1024 undecided correspondences per sensor, iterations on the host
    device          k_micp_multi_fast_loop: modes 3 / 4, or the hand-over when the host form reports code 2; at most 4096 undecided
    per-iteration   k_micp_multi_init / k_micp_multi_step: mode 0 on any sensor, n_iter < 2, or both moment forms gave up
EVERY test here proves from rmclhip_rcc_micp_fast_info, read on every sensor before and after the call, which form served it
(prove_form): a call that quietly lands in another form fails.

The refusal for sensors of two contexts on different devices is not tested: the suite runs with one visible device.
"""
import ctypes as C

import numpy as np
import pytest

import micp_multi_cases as mc
import umeyama_cases as uc
from test_gpu_reduce import _transform_close

pytestmark = pytest.mark.gpu

FORM_CASES = ("mixed4", "eight", "one", "empty_member", "all_empty", "all_weight_zero", "short_dataset", "cube6", "near")
FORM_MODE = {"per-iteration": 0, "host": 1, "device": 4}
KEYS = ("attempts", "done", "cap_exits", "overflows", "host_loops")


@pytest.fixture(scope="module")
def maps(ra, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            v, f, _ = mc.mesh_arrays(name)
            cache[name] = ra.import_hip_map(ctx, v, f)
        return cache[name]
    return get


def deltas(before, after):
    return [{k: a[k] - b[k] for k in KEYS} for b, a in zip(before, after)]


def prove_form(form, before, after, what=""):
    """the form one call ended in, from the fast_info of every sensor before and after it"""
    for d, a in zip(deltas(before, after), after):
        tag = (what, form, d, a)
        if form == "per-iteration":             # the moment forms were not tried
            assert d["attempts"] == 0, tag
        elif form == "host":
            assert d["attempts"] == 1 and d["host_loops"] == 1 and d["done"] == 1 and a["last_code"] == 0, tag
        elif form == "device":                  # also the hand-over: the host form records nothing when it reports code 2
            assert d["attempts"] == 1 and d["done"] == 1 and d["host_loops"] == 0 and a["last_code"] == 0, tag
        elif form == "overflow":                # a moment form gave up on the count, the per-iteration form served the call
            assert d["attempts"] == 1 and d["overflows"] == 1 and d["done"] == 0 and d["host_loops"] == 0 and a["last_code"] == 2, tag
        elif form == "cap-exit":
            assert d["attempts"] == 1 and d["cap_exits"] == 1 and d["done"] == 0 and d["host_loops"] == 0 and a["last_code"] == 1, tag
        else:
            raise AssertionError(form)


def proven_call(loc, case, form, what=""):
    before = mc.infos(loc)
    T, merged = mc.call(loc, case)
    after = mc.infos(loc)
    prove_form(form, before, after, what or case.name)
    return T, merged, after


def model_views_hold_the_scan(loc, case):
    """after the call every sensor's buffers equal a plain find(Tom * Tbo[s]) bit for bit (rmclhip.h: "every sensor's model
    buffers hold its scan")"""
    for s in loc.sensors_vec_:
        rcc = s.correspondences_
        left = rcc.modelView()
        rcc.find(mc.orc.tmult(case.Tom, s.Tbo))
        plain = rcc.modelView()
        for k in ("hits", "ranges", "points", "normals", "face_ids"):
            assert left[k].tobytes() == plain[k].tobytes(), (case.name, s.name, k)


def run_form(ra, hm, case, form, mode=None, check_views=True):
    """the case's call in one loop form on fresh operators, the form proven.  The moment forms are called three times -- identical
    calls; the first ones learn the sensors' caps -- and the third is the one that is checked."""
    loc = mc.make_localization(ra, hm, case, FORM_MODE[form] if mode is None else mode)
    if form != "per-iteration":
        for _ in range(2):
            mc.call(loc, case)
    T, merged, after = proven_call(loc, case, form)
    if check_views:
        model_views_hold_the_scan(loc, case)
    mc.close(loc)
    return {"T": T, "merged": merged, "last_uncertain": after[0]["last_uncertain"], "form": form}


def deviation(a, b):
    """(metres, radians) between two transforms"""
    qa, qb = uc.quat_of(a), uc.quat_of(b)
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    vec = qa[3] * qb[:3] - qb[3] * qa[:3] - np.cross(qa[:3], qb[:3])
    return float(np.linalg.norm(uc.trans_of(a) - uc.trans_of(b))), 2.0 * float(np.arctan2(np.linalg.norm(vec), abs(np.dot(qa, qb))))


def against_oracle(case, T, merged, order=None):
    """the issue's bars: T_onew_oold within _transform_close(..., 1e-5) of the oracle's loop, n_meas equal, means and covariance
    within rtol 1e-5, atol 1e-5"""
    To, so = mc.oracle(case, order)[:2]
    assert int(merged["n_meas"]) == int(so["n_meas"]), (case.name, int(merged["n_meas"]), int(so["n_meas"]))
    _transform_close(T, To, 1e-5)
    for f in ("dataset_mean", "model_mean"):
        assert np.allclose([merged[f][k] for k in "xyz"], [so[f][k] for k in "xyz"], rtol=1e-5, atol=1e-5), (case.name, f)
    assert np.allclose(merged["covariance"], so["covariance"], rtol=1e-5, atol=1e-5), case.name
    if case.identity:
        assert T.tobytes() == mc.orc.transform().tobytes(), (case.name, T)


@pytest.fixture(scope="module")
def form_results(ra, ctx, maps):
    """(case, form) -> the proven result, computed once"""
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            case = mc.cases()[name]
            cache[(name, form)] = run_form(ra, maps(case.mesh_name), case, form)
        return cache[(name, form)]
    return get


@pytest.mark.parametrize("form", ["per-iteration", "host", "device"])
@pytest.mark.parametrize("name", FORM_CASES)
def test_every_case_in_every_form_against_the_oracle(form_results, name, form):
    """mixed models, eight sensors (two per wave of the device loop), one sensor, empty members, an empty rig, weights of zero, a
    short and an unmasked dataset, six sensors with nothing undecided (the device loop's one-sensor-per-wave sums with sensors w
    and w + 4 on one wave) and the bracket rig with undecided correspondences in several sensors (its sensor-by-sensor sums)"""
    case = mc.cases()[name]
    r = form_results(name, form)
    against_oracle(case, r["T"], r["merged"])
    if name == "all_empty":
        assert int(r["merged"]["n_meas"]) == 0
    if name == "cube6" and form != "per-iteration":
        assert r["last_uncertain"] == 0, r["last_uncertain"]
    if name == "near" and form != "per-iteration":
        assert 1 <= r["last_uncertain"] <= 1024, r["last_uncertain"]


@pytest.mark.parametrize("name", FORM_CASES)
def test_the_three_forms_agree(form_results, name):
    res = [form_results(name, f) for f in ("per-iteration", "host", "device")]
    for a in res:
        for b in res:
            _transform_close(a["T"], b["T"], 1e-5)
            assert int(a["merged"]["n_meas"]) == int(b["merged"]["n_meas"])


@pytest.mark.parametrize("mode", [3, (1, 4, 1, 4), (1, 1, 0, 1)], ids=["all-3", "mixed-1-4", "one-sensor-0"])
def test_other_mode_mixtures_take_the_form_they_must(ra, ctx, maps, mode):
    """mode 3 on every sensor and a mixture of 1 and 4 end in the device loop (the host form needs mode 1 everywhere); mode 0 on one
    sensor alone sends the whole rig to the per-iteration form"""
    case = mc.cases()["mixed4"]
    form = "per-iteration" if mode == (1, 1, 0, 1) else "device"
    r = run_form(ra, maps(case.mesh_name), case, form, mode=mode)
    against_oracle(case, r["T"], r["merged"])


# ---- undecided brackets ------------------------------------------------------------------------------------------------
def test_near_has_undecided_correspondences_in_at_least_two_sensors(ra, ctx, maps):
    """near: 1 ... 1024 undecided on the third call, spread over the sensors, so that the device loop's list has more than one
    segment.  A sensor's share: its own single-sensor call through the same entry point (the rig's info carries the sum)."""
    case = mc.cases()["near"]
    hm = maps(case.mesh_name)
    shares = []
    for s in case.sensors:
        single = mc.Case("near-%s" % s["name"], case.mesh_name, [s], case.truth, mc.orc.transform(), n_iter=case.n_iter)
        single.Tom = case.Tom
        shares.append(run_form(ra, hm, single, "host", check_views=False)["last_uncertain"])
    assert sum(1 for n in shares if n >= 1) >= 2, shares
    for form in ("host", "device"):
        r = run_form(ra, hm, case, form, check_views=False)
        assert 1 <= r["last_uncertain"] <= 1024, (form, r["last_uncertain"], shares)
        against_oracle(case, r["T"], r["merged"])


def test_mid_is_handed_from_the_host_form_to_the_device_loop(ra, ctx, maps):
    """mid: a sensor above the host form's 1024, the rig within the device loop's 4096: in the default mode the host form reports
    code 2 and the device loop completes -- inside one call"""
    case = mc.cases()["mid"]
    assert case.form == "device"
    loc = mc.make_localization(ra, maps(case.mesh_name), case, 1)
    for _ in range(2):
        mc.call(loc, case)
    T, merged, after = proven_call(loc, case, "device")
    assert all(1024 < a["last_uncertain"] <= 4096 for a in after), after
    against_oracle(case, T, merged)
    model_views_hold_the_scan(loc, case)
    mc.close(loc)


@pytest.mark.parametrize("mode", [1, 4])
def test_far_overflows_into_the_per_iteration_form(ra, ctx, maps, mode):
    """far: more than 4096 undecided; both moment forms give up (code 2) and the per-iteration form serves the call"""
    case = mc.cases()["far"]
    assert case.form == "per-iteration"
    loc = mc.make_localization(ra, maps(case.mesh_name), case, mode)
    T, merged, after = proven_call(loc, case, "overflow")
    assert all(a["last_uncertain"] > 4096 for a in after), after
    against_oracle(case, T, merged)
    model_views_hold_the_scan(loc, case)
    mc.close(loc)


def test_cap_exit_after_the_caps_were_learnt_small(ra, ctx, maps):
    """near's calls, then thirty at an error of 4 mm: every completed call lets the caps shrink by a tenth, down to twice what it
    met.  Under small caps few correspondences are undecided even at far's pose (some 600 against more than 4096
    under fresh caps), so the moment form starts there -- and the second iteration's pre-transform leaves the caps: code 1, and
    the per-iteration form serves the call"""
    cap_exit_after_small_caps(ra, maps, 1, "host")


def test_cap_exit_in_the_device_loop(ra, ctx, maps):
    """the same calls with every sensor in mode 4: the caps are learnt by the device's moment loop, and it is that loop which
    reports code 1 at far's pose; the per-iteration form serves the call and learns the caps from the loop's status"""
    cap_exit_after_small_caps(ra, maps, 4, "device")


def cap_exit_after_small_caps(ra, maps, mode, form):
    near, far = mc.cases()["near"], mc.cases()["far"]
    tiny = near.with_state(Tom=mc.orc.tmult(near.truth, mc.bracket_pert(mc.TINY_SCALE)))
    loc = mc.make_localization(ra, maps(near.mesh_name), near, mode)
    for _ in range(2):
        mc.call(loc, near)
    proven_call(loc, near, form)
    for _ in range(30):
        proven_call(loc, tiny, form)
    caps = [(a["rho_cap"], a["tau_cap"]) for a in mc.infos(loc)]
    assert all(r < 0.005 and t < 0.03 for r, t in caps), caps
    T, merged, after = proven_call(loc, far, "cap-exit")
    assert all(a["last_uncertain"] <= 4096 for a in after), after
    against_oracle(far, T, merged)
    mc.close(loc)


def test_hold_off_after_two_overflows(ra, ctx, maps):
    """two overflows in a row: the next 32 calls do not try the moment forms at all, the 33rd does; every result is the
    per-iteration form's"""
    case = mc.cases()["far"]
    hm = maps(case.mesh_name)
    ref = run_form(ra, hm, case, "per-iteration", check_views=False)
    loc = mc.make_localization(ra, hm, case, 1)
    for k in range(2):
        T, merged, _ = proven_call(loc, case, "overflow", "overflow %d" % k)
        _transform_close(T, ref["T"], 1e-5)
    moved = []
    for k in range(34):
        before = mc.infos(loc)
        T, merged = mc.call(loc, case)
        after = mc.infos(loc)
        d = deltas(before, after)
        assert len({x["attempts"] for x in d}) == 1, d
        moved.append(d[0]["attempts"])
        if d[0]["attempts"] == 0:
            prove_form("per-iteration", before, after, "held off %d" % k)
        else:
            assert all(x["done"] == 0 and x["host_loops"] == 0 for x in d), d      # ... and it was served per iteration again
        _transform_close(T, ref["T"], 1e-5)
        assert int(merged["n_meas"]) == int(ref["merged"]["n_meas"])
    assert moved == [0] * 32 + [1, 1], moved
    mc.close(loc)


# ---- state that lives with sensor 0 --------------------------------------------------------------------------------------
def test_orders_and_subsets_of_one_set_of_operators(ra, ctx, maps):
    """the call block, the join flags and the sequence number belong to whichever sensor comes first: six calls in a row on ONE set of
    six operators in the device loop, each with another first sensor or another subset and at another state, each against the
    per-iteration form (and the oracle) of the same order and state.  A lost or stale join shows as a different result -- the
    rows of the call before belong to another pose -- or as another form."""
    calls = mc.order_calls()
    hm = maps(calls[0][1].mesh_name)
    dev, per = mc.make_localization(ra, hm, calls[0][1], 4), mc.make_localization(ra, hm, calls[0][1], 0)
    got = []
    for order, case in calls:        # (no other call between the six)
        loc = ra.MICPLocalization([dev.sensors_vec_[i] for i in order], optimization_iterations=case.n_iter)
        got.append(proven_call(loc, case, "device", "order %s" % (order,))[:2])
    model_views_hold_the_scan(loc, case)        # the sixth call's scans
    for (order, case), (T, merged) in zip(calls, got):
        loc = ra.MICPLocalization([per.sensors_vec_[i] for i in order], optimization_iterations=case.n_iter)
        Tp, mp, _ = proven_call(loc, case, "per-iteration")
        _transform_close(T, Tp, 1e-5)
        assert int(merged["n_meas"]) == int(mp["n_meas"])
        against_oracle(case, T, merged, order)
    assert not np.array_equal(uc.trans_of(got[0][0]), uc.trans_of(got[5][0]))      # the same six sensors, another state
    mc.close(dev)
    mc.close(per)


# ---- n_iter, convergence_progress ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 4])
def test_zero_and_one_iteration(ra, ctx, maps, mode):
    """n_iter < 2 is not eligible for the moment forms, in mode 0 nothing is: 0 gives the identity and empty statistics, 1 one
    oracle iteration"""
    base = mc.cases()["mixed4"]
    loc = mc.make_localization(ra, maps(base.mesh_name), base, mode)
    zero = base.with_state(n_iter=0)
    T, merged, _ = proven_call(loc, zero, "per-iteration")
    assert T.tobytes() == mc.orc.transform().tobytes() and int(merged["n_meas"]) == 0
    one = base.with_state(n_iter=1)
    T, merged, _ = proven_call(loc, one, "per-iteration")
    against_oracle(one, T, merged)
    mc.close(loc)


@pytest.mark.parametrize("mode", [0, 1, 4])
@pytest.mark.parametrize("progress", [0.0, 0.4, 1.0])
def test_convergence_progress_sets_every_sensors_gate(ra, ctx, maps, progress, mode):
    """max_dist 0.8, adaptive_min 0.2: the gate is adaptive_max_dist per sensor, 0.8, 0.56 and 0.2 m.  At 0.2 m the gate is as
    narrow as the band the caps leave undecided around it (0.016 |D| + 0.08 m on the third call): one sensor has more than the
    host form's 1024 undecided, and the default mode ends in the device loop by hand-over (1024 < undecided <= 4096)."""
    case = mc.cases()["mixed4"].with_state(convergence_progress=progress)
    assert all(s["max_dist"] != s["adaptive_min"] for s in case.sensors)
    form = {0: "per-iteration", 1: "host", 4: "device"}[mode]
    if (progress, mode) == (1.0, 1):
        form = "device"
    r = run_form(ra, maps(case.mesh_name), case, form, mode=mode, check_views=False)
    if (progress, mode) == (1.0, 1):
        assert 1024 < r["last_uncertain"] <= 4096, r["last_uncertain"]
    against_oracle(case, r["T"], r["merged"])


# ---- refusals ----------------------------------------------------------------------------------------------------------
def raw_call(ra, handles, Tom, Tbo, weights, n_iter=5):
    from rmcl_amd import _capi
    from rmcl_amd.types import CROSS_STATISTICS, TRANSFORM, _ptr
    n = len(handles)
    arr = (C.c_void_p * n)(*handles)
    Tin = np.ascontiguousarray(Tom, dtype=TRANSFORM).reshape(1)
    Tb = np.array(Tbo, dtype=TRANSFORM)
    w = None if weights is None else np.array(weights, dtype=np.float64)
    Tout, merged = np.zeros(1, TRANSFORM), np.zeros(1, CROSS_STATISTICS)
    _capi.check(_capi.lib().rmclhip_micp_correct_once(arr, n, _ptr(Tin), _ptr(Tb), _ptr(w) if w is not None else None, n_iter, 0.0,
                                                      _ptr(Tout), _ptr(merged)))
    return Tout[0].copy(), merged[0].copy()


def test_refusals_leave_the_next_call_intact(ra, ctx, maps):
    """what the entry point refuses, each followed by a valid call that must give the oracle's result in the host form"""
    from rmcl_amd import _capi
    case = mc.cases()["mixed4"]
    hm = maps(case.mesh_name)
    loc = mc.make_localization(ra, hm, case, 1)
    for _ in range(2):
        mc.call(loc, case)
    ops = [s.correspondences_ for s in loc.sensors_vec_]
    h = [o._h for o in ops]
    Tbo = [s.Tbo for s in loc.sensors_vec_]
    w = [s["w"] for s in case.sensors]
    no_model = ra.RCCHipSpherical(hm)
    no_model.set_dataset(case.sensors[0]["ds"], case.sensors[0]["mask"])
    no_dataset = ra.RCCHipSpherical(hm)
    no_dataset.setModel(case.sensors[0]["model"]["model"])
    deselected = mc.make_operator(ra, hm, case.sensors[0])
    deselected.set_outputs(("ranges", "normals"))
    ident = mc.orc.transform()
    bad = [("nine sensors", (h * 3)[:9], (Tbo * 3)[:9], None, _capi.ERR_UNSUPPORTED, "8"),
           ("null entry", [h[0], None, h[2]], Tbo[:3], None, _capi.ERR_INVALID, "null"),
           ("no model", [h[0], no_model._h], [Tbo[0], ident], None, _capi.ERR_INVALID, "model"),
           ("no dataset", [h[0], no_dataset._h], [Tbo[0], ident], None, _capi.ERR_INVALID, "dataset"),
           ("deselected outputs", [h[0], deselected._h], [Tbo[0], ident], None, _capi.ERR_INVALID, "deselected"),
           ("weight -1", h, Tbo, [1.0, -1.0, 2.0, 0.0], _capi.ERR_INVALID, "sensor 1"),
           ("weight NaN", h, Tbo, [1.0, 0.37, float("nan"), 0.0], _capi.ERR_INVALID, "sensor 2"),
           ("weight inf", h, Tbo, [float("inf"), 0.37, 2.0, 0.0], _capi.ERR_INVALID, "sensor 0")]
    for what, handles, tbo, weights, status, word in bad:
        before = mc.infos(loc)
        with pytest.raises(ra.RmclHipError) as e:
            raw_call(ra, handles, case.Tom, tbo, weights, case.n_iter)
        assert e.value.status == status and word in str(e.value), (what, e.value.status, str(e.value))
        assert deltas(before, mc.infos(loc)) == deltas(before, before), what          # refused before anything ran
        T, merged, _ = proven_call(loc, case, "host", "after " + what)
        against_oracle(case, T, merged)
    # ... and the weights as given reach the call unchanged (a weight of zero is valid)
    T, merged = raw_call(ra, h, case.Tom, Tbo, w, case.n_iter)
    against_oracle(case, T, merged)
    for o in (no_model, no_dataset, deselected):
        o.close()
    mc.close(loc)
