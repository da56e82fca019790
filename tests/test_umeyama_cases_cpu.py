"""CPU checks of tests/umeyama_cases.py: the crafted covariances and the degenerate scenes are what they claim to be, so the GPU tests
built on them (tests/test_gpu_umeyama.py) cannot pass vacuously; the oracle's solve equals the float64 definition on all of them.
"""
import collections

import numpy as np
import pytest

import umeyama_cases as uc


@pytest.fixture(scope="module")
def crafted():
    return uc.crafted_cases()


def _ratios(stats):
    s = uc.singular_values(stats)
    return (s[1] / s[0], s[2] / s[0]) if s[0] > 0 else (0.0, 0.0)


def test_families_are_populated_and_of_the_rank_they_claim(crafted):
    count = collections.Counter(fam for fam, _, _ in crafted)
    assert set(count) == {"general", "rank1", "rank1_half", "near_rank1", "rank2", "zero", "empty"}
    assert min(count.values()) >= 10, count
    assert len({(fam, name) for fam, name, _ in crafted}) == len(crafted)
    for fam, name, s in crafted:
        r2, r3 = _ratios(s)
        sv = uc.singular_values(s)
        if fam in ("rank1", "rank1_half"):
            assert sv[0] > 0 and r2 <= uc.BAND[0], (name, r2)
            C = uc.cov64(s)
            v = np.linalg.svd(C)[2][0]
            d = float(np.dot(C @ v / np.linalg.norm(C @ v), v))
            assert (d <= -1.0 + 1e-12) == (fam == "rank1_half"), (name, d)
            assert d <= -1.0 + 1e-12 or d > -1.0 + 1e-6, (name, d)     # nothing near the switch to the half turn
        elif fam == "near_rank1":
            assert uc.BAND[1] <= r2 <= 2e-3, (name, r2)
        elif fam == "rank2":
            assert r2 > 1e-3 and r3 < 1e-7, (name, r2, r3)
        elif fam == "zero":
            assert sv[0] == 0.0 and int(s["n_meas"]) == 1
        elif fam == "empty":
            assert sv[0] > 0.0 and int(s["n_meas"]) == 0
    # the general list keeps what test_abi checked before: most of it of full rank, reflections among them
    dets = [np.linalg.det(uc.cov64(s)) for fam, _, s in crafted if fam == "general"]
    assert sum(d < 0 for d in dets) >= 10


def test_no_case_sits_in_the_classification_band(crafted):
    """solver and reference classify rank <= 1 from the same float32 numbers at s2 = 1e-6 s1; no case may come near that"""
    for fam, name, s in crafted:
        r2, _ = _ratios(s)
        assert not (uc.BAND[0] < r2 < uc.BAND[1]), (fam, name, r2)


def test_reference_is_a_rotation_that_attains_the_optimum(crafted):
    """umeyama_ref itself: unit quaternion, and trace(R C^T)... = the sum of the singular values (with the reflection's sign): the
    Kabsch optimum, which every member of the rank-one family attains -- so the shortest arc is a valid instance of the definition"""
    for fam, name, s in crafted:
        if fam in ("zero", "empty"):
            continue
        q, _ = uc.umeyama_ref(s)
        assert abs(np.linalg.norm(q) - 1.0) < 1e-12
        C = uc.cov64(s)
        U, S, Vt = np.linalg.svd(C)
        best = S[0] + S[1] + S[2] * (1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0)
        got = np.trace(uc._matrix_from_quat(q).T @ C)
        # at rank <= 1 the rule ignores s2 and s3 (noise by classification): the optimum is attained up to them
        slack = 2.0 * (S[1] + S[2]) if fam in ("rank1", "rank1_half") or S[1] <= uc.RANK1_RATIO * S[0] else 0.0
        assert abs(got - best) <= 1e-9 * S[0] + slack, (fam, name, got, best)


def test_rank_one_reference_is_the_shortest_member_of_its_family(crafted):
    """no rotation taking v1 to u1 turns by less than the angle between them"""
    for fam, name, s in crafted:
        if fam != "rank1":
            continue
        C = uc.cov64(s)
        v = np.linalg.svd(C)[2][0]
        u = C @ v / np.linalg.norm(C @ v)
        q, _ = uc.umeyama_ref(s)
        assert abs(uc.rotation_angle(q) - np.arccos(np.clip(np.dot(u, v), -1, 1))) < 1e-7, name


def test_oracle_equals_the_reference_on_every_case(orc, crafted):
    for fam, name, s in crafted:
        uc.assert_matches_ref(orc.umeyama(s), s, "%s/%s" % (fam, name))


@pytest.fixture(scope="module")
def scene_stats(orc):
    """scene -> (oracle correction after one iteration, its float32 statistics)"""
    out = {}
    for name, sc in uc.scenes().items():
        To, so, _ = sc.oracle_correct_once(1)
        out[name] = (To, so)
    return out


def test_scenes_are_what_they_claim(scene_stats):
    S = uc.scenes()
    assert set(S) == {"floor", "corridor2d", "wall_line", "wall_line_tilt", "cube_0", "cube_1", "cube_2", "cube_3", "nothing"}
    for name, sc in S.items():
        assert 2 <= len(sc.f) <= 12 and sc.model.phi.size * sc.model.theta.size <= 14400, name
        _, so = scene_stats[name]
        r2, r3 = _ratios(so)
        n = int(so["n_meas"])
        if name.startswith("wall_line"):
            assert r2 < 1e-12 and n > 300, (name, r2, n)
        elif name == "floor":
            assert r2 > 0.9 and r3 < 1e-12 and n > 1000, (name, r2, r3, n)
        elif name == "corridor2d":
            assert uc.singular_values(so)[2] == 0.0 and r2 > 0.05 and n > 300, (name, r2, n)
        elif name.startswith("cube_"):
            assert n == int(name[-1]), (name, n)
        else:
            assert n == 0, (name, n)
        assert not (uc.BAND[0] < r2 < uc.BAND[1]), (name, r2)
    for name in ("corridor2d", "wall_line", "wall_line_tilt", "nothing"):
        assert S[name].model.phi.size == 1 and S[name].model.theta.size == 900      # one-row images


def test_oracle_equals_the_reference_on_every_scene(scene_stats):
    for name, (To, so) in scene_stats.items():
        import oracle as orc
        uc.assert_matches_ref(orc.umeyama(so), so, name)


def test_wall_scenes_get_a_small_correction_from_the_oracle(scene_stats):
    """a 2-D lidar facing one wall, estimate off by 5 cm and about one degree: the correction is that, not a quarter turn"""
    for name in ("wall_line", "wall_line_tilt"):
        for n_iter in (1, 4):
            To, _, _ = uc.scenes()[name].oracle_correct_once(n_iter)
            assert np.degrees(uc.rotation_angle(uc.quat_of(To))) < 2.0, (name, n_iter)
            assert np.linalg.norm(uc.trans_of(To)) < 0.2, (name, n_iter)
    To, _ = scene_stats["wall_line"]
    assert abs(np.degrees(uc.rotation_angle(uc.quat_of(To))) - np.degrees(0.02)) < 1e-3     # the yaw error of the estimate
    for name in ("cube_0", "nothing"):
        To, so = scene_stats[name]
        assert To.tobytes() == uc.orc.transform().tobytes() and int(so["n_meas"]) == 0


def test_listed_floors_are_four_times_the_measured_sensitivity():
    """a scene's widened floor is the reference's own sensitivity to one ulp of one covariance entry, times four -- recomputed here"""
    import oracle_micp as om
    assert set(uc.TWO_SENSOR_FLOORS) == {"cube_3"}
    for name, (rad, metres) in uc.TWO_SENSOR_SENSITIVITY.items():
        sc = uc.scenes()[name]
        _, _, solved = om.correct_once_multi(sc.mesh, uc.two_sensor_spec(sc), sc.Tom, 1)
        d_ang, _, d_t = uc.ulp_sensitivity(solved[0])
        assert abs(d_ang - rad) < 0.01 * rad and abs(d_t - metres) < 0.01 * metres, (name, d_ang, d_t)
        assert uc.TWO_SENSOR_FLOORS[name] == (4.0 * rad, 4.0 * metres)
