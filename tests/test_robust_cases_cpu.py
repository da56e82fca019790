"""Premises of the robust-MICP GPU cases (tests/robust_cases.py), asserted on the numpy restatement alone, no device: every median case
has the m, the rank, the ties and the digits it claims; every size reaches the row count it claims; the weights' case holds the grid,
masked, gated-out and poisoned elements; on the contaminated scan the restatement's plain loop ends far from the truth and its robust
loops end closer."""
import numpy as np
import pytest

import pose_information_cases as pic
import pose_information_ref as pir
import robust_cases as rc
import robust_ref as rr

F = np.float32


def _ident(orc):
    return orc.transform()


def _plus_zero(r):
    """(0 * 0 + 0 * 0) + (-0) * 1 is +0: the only residual the line cases do not hand through bit for bit"""
    return np.where(r == 0, F(0.0), r).astype(F)


def test_line_cases_give_the_residual_exactly(orc):
    c = rc.weights_case()
    kept, _, r = pir.gate(_ident(orc), c["D"], c["dmask"], c["I"], c["N"], c["mmask"], rc.MAX_DIST)
    n0 = c["poison"][0]
    assert 280 <= len(r) <= 340
    assert r[:n0].tobytes() == _plus_zero(c["I"][:n0, 2]).tobytes()     # spd == r bit for bit (a -0 arrives as +0: 0 + -0)
    assert not kept[c["poison"]].any() and kept[n0 + 11]
    inside = np.abs(c["I"][:n0, 2]) < rc.MAX_DIST
    assert np.array_equal(kept[:n0], inside) and 100 < inside.sum() < n0 - 30      # both gated in and gated out
    for cc in rc.GRID_C:
        g = rc.grid_r(cc)
        assert np.isin(g.view(np.uint32), c["I"][:n0, 2].view(np.uint32)).all()


def test_median_cases_are_what_they_claim(orc):
    cases = rc.median_cases()
    for m in rc.MEDIAN_COUNTS:
        assert cases["m%d" % m][1] == m
    for name, (r, m) in cases.items():
        c = rc.line_case(r)
        kept, _, rr_ = pir.gate(_ident(orc), c["D"], None, c["I"], c["N"], None, rc.MAX_DIST)
        assert int(kept.sum()) == m, name
        assert rr_.tobytes() == _plus_zero(r).tobytes(), name
    a = np.abs(cases["all_equal"][0])
    assert len(np.unique(a)) == 1
    r, m = cases["mostly_zero"]
    assert (r == 0).sum() > m // 2 and rr.lower_median(np.abs(r))[0] == 0
    p = rr.params(rr.HUBER)
    assert rr.scale_of(p, r, np.ones(m, bool))[0] == F(1e-3)                        # the floor
    r, m = cases["signed_zeros"]
    bits = r.view(np.uint32)
    assert (bits == 0).sum() == 150 and (bits == 0x80000000).sum() == 150 and rr.lower_median(np.abs(r))[0] == 0
    r, m = cases["low_digit"]
    k = np.abs(r).view(np.uint32)
    assert len(np.unique(k >> 10)) == 1 and len(np.unique(k)) == m                  # one bucket of the first two passes, all distinct
    for name, key in (("straddle_last_pass", rc.STRADDLE_LAST), ("straddle_first_pass", rc.STRADDLE_FIRST)):
        shift = 10 if name == "straddle_last_pass" else 21
        assert (key >> shift) != ((key + 1) >> shift)
        r, m = cases[name + "_below"]
        med, rank = rr.lower_median(np.abs(r))
        assert med.view(np.uint32) == key and rank == 400 and (np.abs(r).view(np.uint32) == key).sum() == 401      # the last copy below
        r, m = cases[name + "_above"]
        med, rank = rr.lower_median(np.abs(r))
        assert med.view(np.uint32) == key + 1 and rank == 401 and (np.abs(r).view(np.uint32) == key).sum() == 400  # the first copy above
    a, b = cases["order_a"][0], cases["order_b"][0]
    assert a.tobytes() != b.tobytes() and np.array_equal(np.sort(a), np.sort(b))
    assert len(np.unique(np.abs(a))) < len(a) - 300                                 # ties
    assert cases["empty"][1] == 0


def test_sum_sizes_reach_their_rows():
    assert tuple(pic.rows(n) for n in rc.SUM_SIZES) == pic.FREE_ROWS and {1, 2, 15, 16, 17, 31, 32, 33} <= set(pic.FREE_ROWS)
    assert pic.rows(pic.CAP_SIZE) == 1024 and pic.rows(1) == 1
    assert tuple(pic.rows(n) for n in rc.SUM_FAR) == pic.FAR_ROWS == (15, 17, 33)


def test_restatement_with_weight_one_is_the_plain_reduction(orc):
    """NONE, and HUBER with c >= max_dist, give the oracle's statistics_p2l in double: the restatement's sums are the plain ones"""
    n = 513
    c = rc.sum_case(n)
    T = pic.tpre_general()
    want = orc.statistics_p2l_f64(T, c["D"], c["dmask"], c["I_nan"], c["N_nan"], c["mmask"], float(rc.SUM_MAX_DIST))
    for p in (rr.params(rr.NONE), rr.params(rr.HUBER, scale=float(rc.SUM_MAX_DIST))):
        ref = rc.sum_reference(c, T, p)
        assert ref["n_meas"] == want["n_meas"] and ref["weight_sum"] == ref["n_meas"] and np.all(ref["w"][ref["kept"]] == 1)
        assert np.allclose(ref["covariance"].reshape(3, 3), want["covariance"], rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def scan(orc):
    return rc.contaminated_scan(orc)


def test_contaminated_scan_premises(orc, scan):
    s = scan
    n = len(s["short"])
    assert 0.15 * n <= s["short"].sum() <= 0.25 * n
    kept, _, r = pir.gate(_ident(orc), s["dataset"][0], s["dataset"][1], s["points"], s["normals"], s["hits"], rc.SCAN_MAX_DIST)
    assert kept.sum() > 0.9 * n                                  # the shortened rays lie INSIDE the gate a 0.2 m error needs
    assert kept[s["short"]].mean() > 0.8
    t0, a0 = rc.pose_error(orc, orc.transform(), s)
    assert 0.19 < t0 < 0.21 and abs(a0 - np.deg2rad(2.0)) < 1e-3


def test_plain_loop_is_pulled_away_and_the_robust_loops_are_not(orc, scan):
    plain = rc.restated_loop(orc, scan, rr.params(rr.NONE))
    t_plain, a_plain = rc.pose_error(orc, plain[0], scan)
    print("restatement, plain  : %.6f m %.6f rad" % (t_plain, a_plain))
    assert t_plain >= 10 * rc.POSE_BAR
    for kernel in (rr.TUKEY, rr.HUBER):
        rob = rc.restated_loop(orc, scan, rr.params(kernel))
        t_rob, a_rob = rc.pose_error(orc, rob[0], scan)
        print("restatement, %-7s: %.6f m %.6f rad (c = %.6f, median %.6f)" % (rr.NAMES[kernel], t_rob, a_rob, rob[3][0], rob[3][1]))
        assert t_rob < t_plain
