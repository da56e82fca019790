"""The cases of tests/pf_cycle_cases.py are what they claim to be -- checked on the CPU oracle alone, so that the GPU test
(tests/test_gpu_pf_cycle.py) cannot pass vacuously: brute force and the oracle's BVH walk agree on every motion case, the deep
maps are deep and kill some particles and spare others, the gate cases sit on both sides of the gate, the vectorised float64
estimate reference is the oracle's, every estimate cloud has a defined mean, and the residual cloud needs more draws than one
trip of the scan of the block totals covers."""
import numpy as np
import pytest

import pf_cycle_cases as pc


@pytest.mark.parametrize("name", pc.MOTION_CASES)
def test_motion_case_brute_force_and_bvh_agree(orc, meshes, name):
    c = pc.motion_case(name, meshes)
    for collision in (False, True):
        p, a = pc.motion_reference(c, orc, collision, bvh=False)
        p2, a2 = pc.motion_reference(c, orc, collision, bvh=True)
        assert pc.first_difference(name, "poses (brute force, BVH walk)", p, p2) is None
        assert pc.first_difference(name, "attributes (brute force, BVH walk)", a, a2) is None
    k = pc.killed(pc.motion_reference(c, orc, True)[1])
    assert not pc.killed(pc.motion_reference(c, orc, False)[1]).any() or name.startswith("forget")    # (forget_1: n_meas -> 0, never MAX)
    print("[pf-cycle] %-18s map %-9s n %4d killed %4d" % (name, c["map"], len(k), k.sum()))
    if name in pc.DEEP_CASES + pc.WALL_CASES:
        assert k.any() and not k.all(), "%s: %d of %d particles killed" % (name, k.sum(), k.size)


def test_wall_case_holds_the_constructed_steps(orc, meshes):
    """the steps the wall case is made for are in it, and the oracle decides them as the closed interval [0, tfar] says"""
    c = pc.motion_case("wall_x", meshes)
    p, a = pc.motion_reference(c, orc, True)
    x, y, z, w = (c["poses"]["t"]["x"], c["poses"]["t"]["y"], c["poses"]["t"]["z"], c["poses"]["R"]["w"])
    k = pc.killed(a)
    fwd = (w == 1) & (y == np.float32(0.25)) & (z == np.float32(0.5))
    assert (fwd & (x < 0.75) & (x > 0.7)).sum() == 4 and not k[fwd & (x < 0.75)].any()        # ends short by ulps: survives
    assert k[fwd & (x > 0.75) & (x < 1.0)].all()                                                 # crosses
    on_end, on_start = fwd & (x == 0.75), fwd & (x == 1.0)
    assert on_end.sum() == 1 and on_start.sum() == 1
    print("[pf-cycle] wall_x: a step ending exactly on the wall is %s, one starting exactly on it %s" % (
        "killed" if k[on_end][0] else "spared", "killed" if k[on_start][0] else "spared"))
    assert not k[fwd & (x > 1.0)].any()                                                          # behind it, moving away
    diag = (w == 1) & (z == y + 1) & (x == np.float32(0.875))
    assert diag.sum() >= 4 and k[diag].all()                                                     # the diagonal and the corners A, C: watertight
    cp, ca = pc.motion_reference(pc.motion_case("wall_inplane", meshes), orc, True)
    assert (pc.step_lengths(pc.motion_case("wall_inplane", meshes), cp)[:100] == np.float32(0.25)).all()


def test_gate_cases_sit_on_both_sides_of_the_gate(orc, meshes):
    assert pc.GATE_STEPS[3] < 0.00001 < pc.GATE_STEPS[4] and np.float32(pc.GATE_STEPS[3]) == np.float32(1e-5)
    killed_above = 0
    for name in pc.GATE_CASES:
        c = pc.motion_case(name, meshes)
        p, a = pc.motion_reference(c, orc, True)
        k, below = pc.killed(a), pc.step_lengths(c, p).astype(np.float64) < 0.00001
        on_wall = c["poses"]["t"]["x"] == 0
        print("[pf-cycle] %s step %.9g: %d of %d steps below the gate, %d killed, %d particles on the wall" % (
            name, c["T_delta"]["t"]["x"], below.sum(), below.size, k.sum(), on_wall.sum()))
        assert on_wall.sum() >= 8
        assert not k[below].any(), "%s: particles %s are killed by a step below the gate" % (name, np.flatnonzero(k & below)[:8].tolist())
        if pc.GATE_STEPS[int(name[5:])] < 0.9e-5 + 1e-9:
            assert below.all()
        killed_above += int(k[~below].sum())
        if name in ("gate_4", "gate_5"):
            assert k[~below].any(), name
            near = (np.abs(c["poses"]["t"]["x"]) < 1e-5) & ~on_wall
            assert k[near & ~below].any() and (~k[near & ~below]).any(), name       # within one step of the wall: towards it, away from it
    assert killed_above > 0


def test_deep_maps_are_deep(meshes):
    """the particle filter's own tree (leaves of at most two triangles, the one k_pf_motion walks), built on the host"""
    from rmcl_amd import registration as reg
    for name in ("chain200", "nested200"):
        info = reg.build_bvh_host_pf(*meshes(name))[0]
        print("[pf-cycle] %s: n_faces %d n_nodes %d max_depth %d stack_need %d" % (name, info["n_faces"], info["n_nodes"], info["max_depth"], info["stack_need"]))
        assert 16 + 16 < info["stack_need"] <= 64, name         # (k_pf_motion: 16 LDS rows; deeper rows live in private memory)
    assert reg.build_bvh_host_pf(*meshes("fan20k"))[0]["stack_need"] <= 64


def _quat_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# covariance, vectorised float64 against the oracle: the oracle multiplies ~Tbm * T_i in float32 and extracts the Euler angles through
# its float32 orc_quat_to_euler, so each d carries ~1e-7 x (|t| + pi) and an entry 2 sigma x that.  Measured gap, relative to the
# largest entry: 2.7e-9 .. 3.4e-8 on the wide clouds (so 1e-6 holds there), 1.36e-5 .. 2.08e-5 on converged_pi and its flipped twin
# (sigma 0.01 against |t| = 3.7: 1e-6 cannot hold); one particle with all the weight: a covariance of rounding errors alone, at most
# 3.5e-18 absolute, left to the absolute bar.  Bar = 4 x the largest measured gap, 2.1e-5.
COV_BAR_REL = 4 * 2.1e-5
COV_BAR_ABS = 1e-11


@pytest.mark.parametrize("name", pc.ESTIMATE_CASES)
def test_estimate_reference_is_the_oracle_and_the_mean_is_defined(orc, name):
    c = pc.estimate_case(name)
    n = len(c["poses"])
    for n_ind in c["n_inductions"]:
        ref = pc.estimate_ref(c["poses"], c["attrs"], n_ind)
        ev = ref["eigenvalues"]
        assert ev[-1] - ev[-2] >= 1e-3, "%s n_induction %d: eigenvalues %s" % (name, n_ind, ev)
        assert ref["nparticles"] == min(n, n_ind)
        if min(n, n_ind) > 5000:
            continue
        o = orc.estimate_stats(c["poses"], c["attrs"], n_ind)
        assert o["nparticles"] == ref["nparticles"]
        for k in ("mean", "sigma", "min", "max"):
            assert abs(ref["likelihood"][k] - o["likelihood"][k]) <= 1e-12 * abs(o["likelihood"][k]), (name, n_ind, k)
        assert np.array_equal(ref["trans_bb_min"], o["trans_bb_min"]) and np.array_equal(ref["trans_bb_max"], o["trans_bb_max"])
        # the oracle hands its mean pose back ROUNDED to float32, so 1e-12 / 1e-9 cannot be asked of that record: the reference's mean
        # must round to the same floats (one ulp where the two float64 sums straddle a rounding boundary); the float64 values before
        # the rounding are held to 1e-12 / 1e-9 in test_estimate_reference_in_float64_against_the_oracles_own_formulas
        to, qo = np.array([o["pose"]["t"][k] for k in "xyz"]), np.array([o["pose"]["R"][k] for k in "xyzw"])
        assert (np.abs(ref["t"].astype(np.float32) - to) <= np.spacing(np.abs(to))).all(), (name, n_ind, ref["t"], to)
        assert _quat_dist(ref["q"], qo) <= 1.2e-7, (name, n_ind, ref["q"], qo)       # four components, half an ulp of 1 each
        gap = np.abs(ref["covariance"] - o["covariance"]).max()
        scale = np.abs(o["covariance"]).max()
        print("[pf-cycle] %-20s n_induction %6d eigen gap %.3g covariance gap %.3g absolute, %.3g of the largest entry %.3g" % (
            name, n_ind, ev[-1] - ev[-2], gap, gap / max(scale, 1e-300), scale))
        bar = COV_BAR_REL if name.startswith("converged_pi") else 1e-6
        assert gap <= bar * scale + COV_BAR_ABS, (name, n_ind, gap, scale)


def test_estimate_reference_in_float64_against_the_oracles_own_formulas(orc):
    """the bars of the issue on what float32 does not touch: the oracle's float64 statistics, mean translation and mean quaternion
    BEFORE it rounds them (recomputed here as oracle.estimate_stats states them), 1e-12 / 1e-12 / 1e-9"""
    for name in pc.ESTIMATE_CASES:
        c = pc.estimate_case(name)
        if len(c["poses"]) > 5000:
            continue
        P, A = c["poses"], c["attrs"]
        L = A["likelihood"]["mean"].astype(np.float64)
        w = L / L.sum()
        t = np.stack([P["t"][k] for k in "xyz"], 1).astype(np.float64)
        q = np.stack([P["R"][k] for k in "xyzw"], 1).astype(np.float64)
        ref = pc.estimate_ref(P, A)
        assert _rel(ref["t"], (t * w[:, None]).sum(0)) <= 1e-12
        evec = np.linalg.eigh((q * w[:, None]).T @ q)[1][:, -1]
        assert _quat_dist(ref["q"], evec) <= 1e-9 and ref["q"][3] >= 0
        # the covariance pass around a GIVEN mean: the same d d^T with the oracle's float32 transform algebra, one particle at a time
        Tbm = orc.transform((0.1, -0.05, 0.7, 0.7), (1.0, 2.0, 0.5))
        idx = np.sort(np.argsort(-L, kind="stable")[:64])                   # (the 64 heaviest: single_weight has one particle with weight)
        ref2 = pc.estimate_ref(P[idx], A[idx], mean_pose=Tbm)
        Tmb = orc.tinv(Tbm)
        d = np.zeros((len(idx), 6))
        for i, j in enumerate(idx):
            Td = orc.tmult(Tmb, P[j])
            d[i, :3] = [Td["t"][k] for k in "xyz"]
            d[i, 3:] = orc.quat_to_euler(Td["R"])
        w64 = L[idx] / L[idx].sum()
        cov = (d * w64[:, None]).T @ d
        assert np.abs(ref2["covariance"] - cov).max() <= 1e-5 * np.abs(cov).max(), name


def test_flipped_cloud_is_the_same_cloud():
    a, b = pc.estimate_case("converged_pi"), pc.estimate_case("converged_pi_flipped")
    qa = np.stack([a["poses"]["R"][k] for k in "xyzw"], 1)
    qb = np.stack([b["poses"]["R"][k] for k in "xyzw"], 1)
    assert np.array_equal(qa[0::2], qb[0::2]) and np.array_equal(qa[1::2], -qb[1::2]) and (qb[:, 3] < 0).sum() > 1000
    ra_, rb = pc.estimate_ref(a["poses"], a["attrs"]), pc.estimate_ref(b["poses"], b["attrs"])
    assert np.array_equal(ra_["covariance"], rb["covariance"]) and np.array_equal(ra_["q"], rb["q"])
    yaw = pc.euler_zyx(qa.astype(np.float64))[:, 2]
    assert (yaw > 3.0).sum() > 500 and (yaw < -3.0).sum() > 500             # the cloud straddles the wrap
    assert abs(abs(pc.euler_zyx(ra_["q"][None, :])[0, 2]) - (np.pi - 0.005)) < 2e-3


def test_residual_case_needs_more_draws_than_one_scan_trip(orc):
    poses, attrs = pc.residual_case()
    pn, an, filled, draws = orc.residual_resample(poses, attrs, orc.gladiator_config(**pc.RESIDUAL_NOISE), seed=pc.RESIDUAL_SEED, step=0)
    print("[pf-cycle] residual: n = n_new = %d, %d draws (%.2f trips of %d)" % (pc.RESIDUAL_N, draws, draws / pc.SCAN_TRIP, pc.SCAN_TRIP))
    assert draws > 262144 and filled == pc.RESIDUAL_N == len(pn)
