"""Host side of ROBUST MICP FOR SENSOR RIGS (include/rmclhip.h), no GPU: the weighted merge against its numpy
restatement byte for byte and against the count-weighted merge at the counts, its refusals, the robust covariance against the plain one,
the new struct's layout against a compiled probe -- and the premise of the rig of tests/robust_rig_cases.py on the oracle's buffers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_micp as om
import robust_cases as rc
import robust_ref as rr
import robust_rig_cases as rgc
import robust_rig_ref as rgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _random_cs(orc, rng, n_meas):
    s = np.zeros((), dtype=orc.CROSS_STATISTICS)
    for name in "xyz":
        s["dataset_mean"][name], s["model_mean"][name] = F(rng.uniform(-20, 20)), F(rng.uniform(-20, 20))
    s["covariance"] = rng.uniform(-3, 3, 9).astype(F)
    s["n_meas"] = n_meas
    return s


def test_weighted_merge_equals_the_restatement_byte_for_byte(ra, orc):
    T = ra.types
    rng = np.random.RandomState(21)
    weights = [(0.25, 1e-3), (1234.567, 0.37 * 891.25), (1e-12, 5.0), (7.0, 0.0), (0.0, 3.5), (2.0 ** 40, 1.0), (16777217.0, 3.0)] + [tuple(rng.uniform(0.0, 5000.0, 2)) for _ in range(40)]
    for wa, wb in weights:
        a, b = _random_cs(orc, rng, int(rng.randint(0, 5000))), _random_cs(orc, rng, int(rng.randint(0, 5000)))
        want, W = rgr.merge_weighted(orc, a, wa, b, wb)
        got, gW = T.cross_statistics_merge_weighted(a, wa, b, wb)
        assert got.tobytes() == want.tobytes(), (wa, wb, got, want)
        assert gW == W == float(wa) + float(wb)
        assert int(got["n_meas"]) == int(a["n_meas"]) + int(b["n_meas"])


@pytest.mark.parametrize("na,nb", [(0, 0), (0, 5), (1, 1), (2 ** 24 + 1, 3), (2 ** 31 - 1, 2 ** 31)])
def test_weighted_merge_with_the_counts_is_the_count_weighted_merge(ra, orc, na, nb):
    T = ra.types
    rng = np.random.RandomState(na % 1000 + nb)
    for _ in range(8):
        a, b = _random_cs(orc, rng, na), _random_cs(orc, rng, nb)
        want = T.cross_statistics_merge(a, b)
        got, W = T.cross_statistics_merge_weighted(a, float(na), b, float(nb))
        assert got.tobytes() == want.tobytes(), (na, nb)
        assert W == float(na + nb)
        assert rgr.merge_weighted(orc, a, float(na), b, float(nb))[0].tobytes() == want.tobytes()
        # ... and the oracle's own operator+= says the same
        assert orc.cs_merge(a, b).tobytes() == want.tobytes()


def test_weighted_merge_without_weight_and_refusals(ra, orc):
    T = ra.types
    L = ra._capi.lib()
    rng = np.random.RandomState(4)
    a, b = _random_cs(orc, rng, 17), _random_cs(orc, rng, 25)
    got, W = T.cross_statistics_merge_weighted(a, 0.0, b, 0.0)
    assert W == 0.0 and int(got["n_meas"]) == 42                      # the counts still add
    assert not np.any(np.frombuffer(got.tobytes(), np.uint8)[:60])    # means and covariance are zero
    # w_out is optional
    one = lambda x: np.ascontiguousarray(x, dtype=T.CROSS_STATISTICS).reshape(1)
    out = np.zeros(1, dtype=T.CROSS_STATISTICS)
    assert L.rmclhip_cross_statistics_merge_weighted(T._ptr(one(a)), 1.0, T._ptr(one(b)), 2.0, T._ptr(out), None) == 0
    assert out[0].tobytes() == T.cross_statistics_merge_weighted(a, 1.0, b, 2.0)[0].tobytes()
    for wa, wb in ((-1.0, 1.0), (1.0, -1e-300), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf"))):
        with pytest.raises(ra.RmclHipError, match="finite and >= 0"):
            T.cross_statistics_merge_weighted(a, wa, b, wb)
    assert L.rmclhip_cross_statistics_merge_weighted(None, 1.0, T._ptr(one(b)), 1.0, T._ptr(out), None) == 1


def _information(ra, rng, n_meas):
    T = ra.types
    J = rng.normal(size=(max(n_meas, 8), 6))
    r = rng.normal(scale=0.02, size=len(J))
    info = np.zeros((), dtype=T.POSE_INFORMATION)
    info["A"], info["g"], info["rss"], info["n_meas"] = J.T @ J, J.T @ r, float(r @ r), n_meas
    return info


def test_robust_covariance_with_the_count_as_weight_is_the_plain_covariance(ra):
    T = ra.types
    rng = np.random.RandomState(8)
    for n_meas in (7, 8, 500):
        info = _information(ra, rng, n_meas)
        rec = np.zeros((), dtype=T.POSE_INFORMATION_ROBUST)
        rec["info"], rec["weight_sum"], rec["rss_unweighted"] = info, float(n_meas), 2.0 * float(info["rss"])
        for kw in ({}, {"sigma": 0.03}, {"rcond": 1e-3, "degenerate_variance": 7.0}):
            assert T.pose_covariance_robust(rec, **kw).tobytes() == T.pose_covariance(info, **kw).tobytes(), (n_meas, kw)
        # a real weight: the estimated noise divides by weight_sum - 6
        rec["weight_sum"] = n_meas - 0.5
        cov = T.pose_covariance_robust(rec)
        assert float(cov["s2"]) == float(info["rss"]) / (n_meas - 0.5 - 6.0)
    # the estimate is refused unless weight_sum > 6, whatever n_meas says; a given sigma needs no weight
    info = _information(ra, rng, 500)
    rec = np.zeros((), dtype=T.POSE_INFORMATION_ROBUST)
    rec["info"] = info
    for w in (0.0, 5.9, 6.0):
        rec["weight_sum"] = w
        with pytest.raises(ra.RmclHipError, match="weight_sum > 6"):
            T.pose_covariance_robust(rec)
        assert float(T.pose_covariance_robust(rec, sigma=0.1)["s2"]) == 0.1 * 0.1
    for w in (-1.0, float("nan"), float("inf")):
        rec["weight_sum"] = w
        with pytest.raises(ra.RmclHipError, match="weight_sum"):
            T.pose_covariance_robust(rec, sigma=0.1)


def test_struct_layout_matches_the_c_header(ra, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rmclhip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rmclhip_pose_information_robust),\n'
                   '  offsetof(rmclhip_pose_information_robust, info), offsetof(rmclhip_pose_information_robust, weight_sum),\n'
                   '  offsetof(rmclhip_pose_information_robust, rss_unweighted), offsetof(rmclhip_pose_information_robust, scale),\n'
                   '  offsetof(rmclhip_pose_information_robust, median_abs_residual)); return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    D = ra.types.POSE_INFORMATION_ROBUST
    assert got == [D.itemsize] + [D.fields[k][1] for k in ("info", "weight_sum", "rss_unweighted", "scale", "median_abs_residual")]
    assert got == [376, 0, 352, 360, 368, 372]


def test_premise_of_the_rig(orc):
    """on the oracle's buffers the restated Tukey loop ends closer to the truth in translation than the plain N-sensor loop
    (oracle_micp.correct_once_multi) on the same rig -- and the clean sensor alone would not have hidden the pallet from the plain loop"""
    rig = rgc.rig(orc)
    s, sensors = rig["scan"], rig["sensors"]
    assert [x["w"] for x in sensors] == [1.0, 0.37]
    assert len(sensors[0]["ds"]) == 1024 and len(sensors[1]["ds"]) == 256
    assert int(s["short"].sum()) >= 0.15 * 1024 and int(np.asarray(sensors[1]["mask"]).sum()) >= 200
    plain_T, _, _ = om.correct_once_multi(s["mesh"], rgc.spec(sensors), orc.transform(), rc.SCAN_ITER)
    e_plain = rc.pose_error(orc, plain_T, s)
    errs = {}
    for kernel in rgc.KERNELS:
        res = rgr.rig_loop(orc, rgc.ref_sensors(sensors, rr.params(kernel)), rc.SCAN_ITER)
        errs[kernel] = rc.pose_error(orc, res["T"], s)
        print("%s: restated rig loop %.6f m %.6f rad | plain rig loop (oracle) %.6f m %.6f rad | start %.6f m" %
              (rr.NAMES[kernel], errs[kernel][0], errs[kernel][1], e_plain[0], e_plain[1], rc.pose_error(orc, orc.transform(), s)[0]))
        assert all(st["n_meas"] > 0 and st["weight_sum"] > 0.0 for st in res["stats"])
    assert errs[rr.TUKEY][0] < e_plain[0]
    # NONE on the restatement is the plain loop wherever the multiplier's product needs no truncation
    none = rgr.rig_loop(orc, rgc.ref_sensors(sensors, rr.params(rr.NONE), multipliers=(1.0, 2.0)), 3)
    want, _, _ = om.correct_once_multi(s["mesh"], rgc.spec([dict(sensors[0], w=1.0), dict(sensors[1], w=2.0)]), orc.transform(), 3)
    assert rgc.delta(orc, want, none["T"]) <= rc.POSE_BAR
