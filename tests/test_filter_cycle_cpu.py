"""The scenario of tests/filter_cycle_cases.py is not vacuous: its stages chained on the restatements alone, over the oracle's lattice,
shrink and regrow the cloud, reach both kinds of brick, kill particles, split and join clusters, keep away from the bin edges and
localise.  Every assertion here is a condition on the scenario, met by its steps, seeds and parameters -- not a tolerance.  No GPU."""
import numpy as np
import pytest

import adaptive_ref as ar
import field_ref as fr
import filter_cycle_cases as fc
import hypotheses_ref as hr


@pytest.fixture(scope="module")
def run(ra, orc):
    w = fc.World(ra, orc)
    w.set_fields(fr.oracle_lattice(w.mesh, w.logical))
    rows, est, state = fc.chain(w)
    for r in rows:
        print("[filter-cycle-cpu] " + fc.line(r) + ", estimate %.3f m from the truth" % r["error"])
    return w, rows, est, state


def test_the_fields_are_the_band_field_tests(run):
    w = run[0]
    table = w.banded["table"]
    assert w.logical["n"] == (81, 81, 81) and table.size == 1000 and int((table == 0xFFFFFFFF).sum()) == 216


def test_the_cloud_shrinks_below_a_wave_multiple_and_grows_again(run):
    rows = run[1]
    n = [r["n"] for r in rows] + [rows[-1]["n_new"]]
    assert n[0] == fc.N0 and all(fc.KLD.n_min <= v <= fc.CAPACITY for v in n)
    small = [i for i, v in enumerate(n) if v < 512]
    assert small and any(n[j] > n[j - 1] for j in range(small[0] + 1, len(n))), n
    assert not any(n[i] % 64 == 0 and n[i + 1] % 64 == 0 for i in range(len(n) - 1)), n
    assert all(r["n_new"] == fc.n_new_of(r["k"]) for r in rows)


def test_every_cycle_reaches_far_and_stored_bricks(run):
    for r in run[1]:
        assert r["far"] >= 20 and r["stored"] >= 500, fc.line(r)
        assert r["far"] + r["stored"] == r["n"] * fc.N_BEAMS


def test_the_motion_update_kills_and_the_probe_misses(run):
    rows = run[1]
    assert max(r["killed"] for r in rows) >= 5
    assert any(r["surface"]["n_missed"] > 0 or r["surface"]["n_steep"] > 0 for r in rows)
    assert all(r["surface"]["n_snapped"] > 0 and r["surface"]["n_particles"] == r["n"] for r in rows)


def test_the_third_stage_moves_and_the_stein_step_thins(run):
    rows = run[1]
    assert all(rows[c]["moved"]["n_moved"] >= rows[c]["n"] // 4 for c in (0, 2))
    assert all(rows[c]["moved"]["n_bins"] > 1 for c in (1, 3)) and any(rows[c]["moved"]["n_thinned_bins"] > 0 for c in (1, 3))


def test_clusters_split_join_and_split_again_after_the_kidnap(run):
    rows = run[1]
    assert rows[0]["n_clusters"] >= 2 and rows[-1]["n_clusters"] == 1 and rows[fc.KIDNAP_AFTER + 1]["n_clusters"] > 1
    assert all(r["n_clusters"] <= fc.MAX_HYPOTHESES for r in rows)          # every cluster gets its estimate checked


def test_few_particles_lie_on_a_bin_edge(run):
    rows = run[1]
    assert all(r["undecided"] <= 0.005 * r["counted"] for r in rows)
    assert sum(r["undecided"] == 0 for r in rows) >= 3


def test_the_chain_localises(run):
    w, rows, est, _ = run
    assert fc.position_error(est["pose"], w.truth[fc.N_CYCLES][0]) < 0.1
    assert rows[-1]["error"] < rows[0]["error"]


def test_undecided_flags_the_particles_at_an_edge_and_nobody_else():
    idx = hr.rep(6, [hr.BASE])
    widths = tuple(fc.KLD.bin_xyz) + tuple(fc.KLD.bin_rpy)
    poses, attrs = hr.at_bins(idx, 3, widths)
    assert not fc.undecided(poses, attrs, fc.KLD).any()                         # 0.2 bin and more from every edge
    assert fc.undecided(poses, attrs, fc.KLD, tol=0.5001).all() and not fc.undecided(poses, attrs, fc.KLD, tol=0.0).any()
    # yaw 0: (0 + pi_f) / 0.17453292 is 18 to within an ulp -- on the edge; a particle that is not counted is never flagged
    from particle_init_ref import euler_to_quat
    edge = poses.copy()
    q = euler_to_quat(np.float32([0.05]), np.float32([0.05]), np.float32([0.0]))
    for k, v in zip("xyzw", q):
        edge["R"][k][2] = v[0]
    c = ar._coords(edge[2:3], fc.KLD)[0, 5]
    assert abs(float(c) - 18.0) < 1e-5
    assert fc.undecided(edge, attrs, fc.KLD).tolist() == [False, False, True, False, False, False]
    dead = attrs.copy()
    dead["likelihood"]["mean"][2] = 0.0
    assert not fc.undecided(edge, dead, fc.KLD).any()


def test_the_vectorised_end_points_are_the_oracles_bytes(run):
    """filter_cycle_cases.end_points (refine_ref's arithmetic) against field_ref.end_points (the oracle's, a Python loop): the first 48
    particles of the start with every cycle's beams"""
    w = run[0]
    poses = np.concatenate([s[2] for s in fc.init_slices()])[fc.N_UNIFORM - 24:fc.N_UNIFORM + 24]
    for c in range(fc.N_CYCLES):
        assert fc.end_points(w, c, poses).tobytes() == fr.end_points(poses, w.Tsb[0], w.beams[c]).tobytes(), c
