"""CPU checks of tests/micp_multi_cases.py with the oracle alone: the rigs are what they claim to be, the extended
oracle_micp.correct_once_multi is the single-sensor loop for one sensor, and no correspondence of any case sits on a gate -- so that
tests/test_gpu_micp_multi.py may assert n_meas exactly.
"""
import numpy as np
import pytest

import micp_multi_cases as mc
import oracle_micp as om
import umeyama_cases as uc

NAMES = ("mixed4", "eight", "one", "empty_member", "all_empty", "all_weight_zero", "short_dataset", "cube6", "near", "mid", "far")
IDENTITY = ("all_empty", "all_weight_zero")
GATE_MARGIN = 1e-4       # of max_dist


@pytest.fixture(scope="module")
def cases(orc):
    return mc.cases()


def _is_identity(T):
    return np.array_equal(uc.quat_of(T), [0, 0, 0, 1]) and np.array_equal(uc.trans_of(T), [0, 0, 0])


def test_cases_are_the_rigs_they_claim(cases):
    assert set(cases) == set(NAMES)
    for name, c in cases.items():
        assert c.form in mc.FORMS and (name in IDENTITY) == c.identity
        for s in c.sensors:
            H, W = mc.model_shape(s["model"])
            assert H * W <= 14400 and s["ds"].dtype == np.float32
    m4 = cases["mixed4"]
    assert [s["model"]["kind"] for s in m4.sensors] == ["spherical", "o1dn", "ondn", "pinhole"]
    assert [s["w"] for s in m4.sensors] == [1.0, 0.37, 2.0, 0.0]
    assert any(m4.sensors[1]["model"]["orig"]) and len(np.unique(m4.sensors[2]["model"]["origs"], axis=0)) == 480
    assert mc.model_shape(m4.sensors[3]["model"]) == (48, 64)
    for key in ("Tsb", "Tbo"):
        assert len({s[key].tobytes() for s in m4.sensors}) == 4
    assert all(s["max_dist"] != s["adaptive_min"] for s in m4.sensors)
    assert len(cases["eight"].sensors) == 8 and len(cases["one"].sensors) == 1 and len(cases["cube6"].sensors) == 6
    assert {s["model"]["kind"] for s in cases["eight"].sensors} == {"spherical", "o1dn", "ondn", "pinhole"}
    short, unmasked = cases["short_dataset"].sensors
    assert len(short["ds"]) == 519 < 1024 and short["mask"] is not None
    assert unmasked["mask"] is None and np.isnan(unmasked["ds"]).any() and np.isfinite(unmasked["ds"]).any()
    assert all(s["w"] == 0.0 for s in cases["all_weight_zero"].sensors)
    rig = [s["name"] for s in cases["near"].sensors]
    assert all([s["name"] for s in cases[k].sensors] == rig for k in ("mid", "far"))      # one rig, three perturbations
    assert cases["near"].sensors is cases["far"].sensors
    assert (cases["near"].form, cases["mid"].form, cases["far"].form) == ("host", "device", "per-iteration")


def test_empty_members_are_empty_for_the_reason_given(cases):
    """`masked`: a dataset mask of zeros over finite points; `blind`: a valid dataset, but every ray of its find misses"""
    for name in ("empty_member", "all_empty"):
        c = cases[name]
        mesh = mc.mesh_arrays(c.mesh_name)[2]
        for s in c.sensors:
            sim = om.simulate_model(mesh, s["model"], s["Tsb"], mc.orc.tmult(c.Tom, s["Tbo"]))
            if s["name"] == "masked":
                assert not s["mask"].any() and np.isfinite(s["ds"]).all() and sim["hits"].sum() > 500
            elif s["name"] == "blind":
                assert s["mask"].sum() > 200 and not sim["hits"].any()
            else:
                assert s["mask"].sum() > 100 and sim["hits"].sum() > 100
            single = om.correct_once_multi(mesh, [c.spec()[c.sensors.index(s)]], c.Tom, 1)[1]
            assert (int(single["n_meas"]) == 0) == (s["name"] in ("masked", "blind")), (name, s["name"])


def test_one_spherical_sensor_is_the_single_sensor_loop(cases):
    """correct_once_multi of one spherical sensor at weight 1 == correct_once, iteration by iteration, to the bit"""
    c = cases["one"]
    model, Tsb, Tbo, ds, mask, max_dist, adaptive_min, _ = c.spec()[0]
    mesh = mc.mesh_arrays(c.mesh_name)[2]
    for progress in (0.0, 0.4):
        T1, s1, traj1 = om.correct_once(mesh, model["model"], Tsb, Tbo, c.Tom, ds, mask, c.n_iter, max_dist, adaptive_min, progress)
        for m in (model, model["model"]):       # the dict and the bare SphericalModel of the earlier call sites
            Tn, sn, solved, trajn = om.correct_once_multi(mesh, [(m, Tsb, Tbo, ds, mask, max_dist, adaptive_min, 1.0)], c.Tom, c.n_iter,
                                                          progress, want_traj=True)
            assert Tn.tobytes() == T1.tobytes() and sn.tobytes() == s1.tobytes() and solved[-1].tobytes() == s1.tobytes()
            assert len(trajn) == c.n_iter and all(a.tobytes() == b.tobytes() for a, b in zip(trajn, traj1))
    assert len(om.correct_once_multi(mesh, c.spec(), c.Tom, 2)) == 3        # without want_traj: the three values it always returned


@pytest.mark.parametrize("name", NAMES)
def test_case_moves_toward_the_truth_or_is_the_identity(cases, name):
    c = cases[name]
    T, merged, solved, traj = mc.oracle(c)
    assert len(traj) == c.n_iter and traj[-1].tobytes() == T.tobytes()
    if c.identity:
        assert _is_identity(T) and int(solved[-1]["n_meas"]) == 0
        assert (int(merged["n_meas"]) == 0) == (name == "all_empty")       # weights of zero: the unweighted merge is not empty
        return
    assert int(merged["n_meas"]) > 200 and int(solved[-1]["n_meas"]) > 200
    before = np.linalg.norm(uc.trans_of(c.Tom) - uc.trans_of(c.truth))
    after = np.linalg.norm(uc.trans_of(mc.orc.tmult(c.Tom, T)) - uc.trans_of(c.truth))
    assert after < 0.5 * before, (name, before, after)


def test_empty_member_changes_nothing(cases):
    """identity statistics of the empty members: the merge is the seeing sensor's alone"""
    c = cases["empty_member"]
    alone = om.correct_once_multi(mc.mesh_arrays(c.mesh_name)[2], c.spec([1]), c.Tom, c.n_iter)
    T, merged = mc.oracle(c)[:2]
    assert int(merged["n_meas"]) == int(alone[1]["n_meas"]) and T.tobytes() == alone[0].tobytes()


def _variants(cases, name):
    c = cases[name]
    out = [(c, None)]
    if name == "cube6":         # the six calls of the order-and-subset test
        out += [(case, order) for order, case in mc.order_calls()]
    if name == "mixed4":        # the states test_gpu_micp_multi.py also runs it at
        out += [(c.with_state(convergence_progress=p), None) for p in (0.4, 1.0)] + [(c.with_state(n_iter=1), None)]
    return out


@pytest.mark.parametrize("name", [n for n in NAMES if n not in IDENTITY])
def test_gate_margin(cases, name):
    """THE condition of the exact n_meas assertions on the device: at every iteration's pre-transform, no masked, hit correspondence of
    any sensor lies within 1e-4 max_dist of its gate (float64 numpy).  A case that fails this gets another pose, not a wider margin."""
    for c, order in _variants(cases, name):
        margin = mc.gate_margins(c, order)
        assert margin >= GATE_MARGIN, (name, order, c.convergence_progress, c.n_iter, margin)
