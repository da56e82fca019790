"""GPU: the rotation solve of the MICP correction on degenerate input -- half turns, reflections, planar sets and covariances of rank
<= 1 -- in every place it runs on the device: umeyama() and umeyama_fast() on crafted statistics (rmclhip_debug_solve), and the loop
forms of rmclhip_rcc_correct_once, the v1 batch corrector and the N-sensor loop on degenerate scenes (a floor, a 2-D corridor, a 2-D
lidar facing one wall, zero to three correspondences, a map out of range).  Cases, scenes and the float64 definition:
tests/umeyama_cases.py; tests/test_umeyama_cases_cpu.py shows they are what they claim to be.
"""
import numpy as np
import pytest

import oracle_micp as om
import umeyama_cases as uc
from test_gpu_reduce import _transform_close

pytestmark = pytest.mark.gpu

SCENES = ("floor", "corridor2d", "wall_line", "wall_line_tilt", "cube_0", "cube_1", "cube_2", "cube_3", "nothing")
EMPTY = ("cube_0", "nothing")


@pytest.fixture(scope="module")
def crafted():
    cases = uc.crafted_cases()
    return cases, np.array([s for _, _, s in cases], dtype=uc.orc.CROSS_STATISTICS)


@pytest.fixture(scope="module")
def solved(ra, ctx, crafted):
    """solver -> transforms of every crafted case; 258 cases = five blocks of 64 threads, the last one partly filled"""
    _, stats = crafted
    return {k: ra.types.debug_solve(ctx if k else None, stats, k) for k in (0, 1, 2)}


@pytest.mark.parametrize("solver", [1, 2], ids=["umeyama", "umeyama_fast"])
def test_device_solvers_match_the_definition_on_crafted_cases(crafted, solved, solver):
    cases, stats = crafted
    assert len(cases) > 256
    for (fam, name, _), s, T in zip(cases, stats, solved[solver]):
        uc.assert_matches_ref(T, s, "solver %d %s/%s" % (solver, fam, name))


def test_device_umeyama_is_bit_identical_to_the_host(crafted, solved):
    """devmath.h's promise: one source, explicit operation order, no contraction -- the same bits on the host and on gfx950"""
    cases, _ = crafted
    diff = [(fam, name) for (fam, name, _), a, b in zip(cases, solved[0], solved[1]) if a.tobytes() != b.tobytes()]
    assert not diff, diff


def test_debug_solve_refuses_other_solvers_and_accepts_nothing(ra, ctx, crafted):
    _, stats = crafted
    for bad in (-1, 3, 7):
        with pytest.raises(ra.RmclHipError) as e:
            ra.types.debug_solve(ctx, stats[:3], bad)
        assert e.value.status == ra._capi.ERR_INVALID
    assert len(ra.types.debug_solve(ctx, stats[:0], 1)) == 0
    one = ra.types.debug_solve(ctx, stats[100:101], 2)       # a single element: one block, one live thread
    uc.assert_matches_ref(one[0], stats[100], "single")


# ---- scenes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps(ra, ctx):
    cache = {}

    def get(sc):
        key = sc.v.tobytes() + sc.f.tobytes()
        if key not in cache:
            cache[key] = ra.import_hip_map(ctx, sc.v, sc.f)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def oracle_once():
    """(scene, refind) -> the oracle's correction of four iterations, computed once"""
    cache = {}

    def get(name, refind=False):
        if (name, refind) not in cache:
            cache[(name, refind)] = uc.scenes()[name].oracle_correct_once(4, refind=refind)[:2]
        return cache[(name, refind)]
    return get


def _operator(ra, hm, sc):
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(sc.Tsb)
    rcc.setModel(sc.model)
    rcc.set_dataset(sc.ds, sc.mask)
    rcc.params.max_dist = rcc.adaptive_max_dist_min = sc.max_dist
    return rcc


def _check(name, Tg, sg, To, so, floors=None):
    assert int(sg["n_meas"]) == int(so["n_meas"]), name
    atol_r, atol_t = floors if floors else (2e-7, 1e-6)
    _transform_close(Tg, To, 1e-5, atol_t=atol_t, atol_r=atol_r)
    if name in EMPTY:
        # the identity -- behind a mount that is not the identity the device forms (and the oracle's batch corrector) return
        # Tso I Tso^-1: the identity to f32 rounding
        assert int(sg["n_meas"]) == 0
        _transform_close(Tg, uc.orc.transform(), 1e-5)
    if name.startswith("wall_line"):
        assert np.degrees(uc.rotation_angle(uc.quat_of(Tg))) < 2.0 and np.linalg.norm(uc.trans_of(Tg)) < 0.2, (name, Tg)


FORMS = [(0, 0), (0, 1 << 9), (1, 0), (3, 0), (4, 0)]


@pytest.mark.parametrize("fast,variant_bits", FORMS, ids=["per-iteration", "per-iteration-direct", "moments-host", "moments-pass", "moments-epilogue"])
@pytest.mark.parametrize("name", SCENES)
def test_correct_once_on_degenerate_scenes(ra, ctx, maps, oracle_once, name, fast, variant_bits):
    """schedule (R) in every loop form: the per-iteration chain replayed from a hipGraph and enqueued directly, the moment form
    with the iterations on the host, and the two device loops (which solve with umeyama_fast).  Called three times: the moment
    forms learn their bounds on the first call.  The one-row scans also put an H = 1 image through the find's moment epilogue."""
    sc = uc.scenes()[name]
    rcc = _operator(ra, maps(sc), sc)
    rcc.set_variant(15 | variant_bits)
    rcc.set_micp_fast(fast)
    To, so = oracle_once(name)
    for _ in range(3):
        Tg, sg = rcc.correct_once(sc.Tom, sc.Tbo, 4, 0.0, False)
        _check(name, Tg, sg, To, so)
    rcc.close()


@pytest.mark.parametrize("name", SCENES)
def test_correct_once_refind_on_degenerate_scenes(ra, ctx, maps, oracle_once, name):
    """schedule (B): a find per iteration"""
    sc = uc.scenes()[name]
    rcc = _operator(ra, maps(sc), sc)
    To, so = oracle_once(name, True)
    Tg, sg = rcc.correct_once(sc.Tom, sc.Tbo, 4, 0.0, True)
    _check(name, Tg, sg, To, so)
    rcc.close()


@pytest.mark.parametrize("name", SCENES)
def test_correct_batch_on_degenerate_scenes(ra, ctx, maps, name):
    """the v1 corrector (k_batch_solve) on three perturbed poses of the scene"""
    sc = uc.scenes()[name]
    rcc = _operator(ra, maps(sc), sc)
    est = uc.orc.tmult(sc.Tom, sc.Tbo)
    rpy = uc.orc.transform_from_rpy
    poses = np.array([est, uc.orc.tmult(est, rpy((0.02, -0.03, 0.0), (0, 0, -0.03))), uc.orc.tmult(est, rpy((-0.04, 0.01, 0.0), (0, 0, 0.01)))],
                     dtype=uc.orc.TRANSFORM)
    Td, st = rcc.correct_batch(poses)
    Tr, sr = om.correct_batch(sc.mesh, sc.model, sc.Tsb, poses, sc.ds, sc.mask, sc.max_dist)
    for i in range(len(poses)):
        _check(name, Td[i], st[i], Tr[i], sr[i])
    rcc.close()


@pytest.mark.parametrize("name", SCENES)
def test_two_sensors_on_degenerate_scenes(ra, ctx, maps, name):
    """MICPLocalization.correctOnce with two sensors of the scene's model, the second mounted 1.5 m beside the first and merged
    at half weight: rmclhip_micp_correct_once (device_loop=True) and the Python host loop, against the oracle's loop.  The sensors
    are in the default mode, so every scene's three calls end in the HOST form of that entry point -- moments published by the
    finds, iterations and umeyama() on the host --, unless a call gives up and takes the per-iteration form (k_micp_multi_step); the
    device's moment loop (k_micp_multi_fast_loop, umeyama_fast) is not reached from here: tests/test_gpu_micp_multi.py.
    Both 2-D lidars see the one wall: the merged statistics are still of rank one.  cube_1 becomes two points."""
    sc = uc.scenes()[name]
    spec = uc.two_sensor_spec(sc)
    To, so, _ = om.correct_once_multi(sc.mesh, spec, sc.Tom, 4)
    if name.startswith("wall_line"):
        sv = uc.singular_values(so)
        assert int(so["n_meas"]) > 600 and sv[1] <= uc.BAND[0] * sv[0]      # merged: of rank one, clear of the band
    hm = maps(sc)

    def build():
        sensors = []
        for i, (model, Tsb, Tbo, ds, mask, md, _, w) in enumerate(spec):
            rcc = ra.RCCHipSpherical(hm)
            rcc.setModel(model)
            rcc.set_dataset(ds, mask)
            rcc.params.max_dist = rcc.adaptive_max_dist_min = md
            s = ra.MICPSensor("s%d" % i, rcc, Tsb=Tsb, Tbo=Tbo, merge_weight_multiplier=w)
            s.valid_dataset_measurements = int(mask.sum())
            sensors.append(s)
        return sensors

    for device_loop, calls in ((False, 1), (True, 3)):       # the device loop's moment form learns its bounds on the first call
        loc = ra.MICPLocalization(build(), optimization_iterations=4)
        for _ in range(calls):
            loc.Tom_, loc.convergence_progress_ = sc.Tom, 0.0
            Tg = loc.correctOnce(device_loop=device_loop)
            assert loc.correction_stats_latest_["valid_matches"] == int(so["n_meas"]), (name, device_loop)
            _check(name, Tg, so, To, so, uc.TWO_SENSOR_FLOORS.get(name))
        for s in loc.sensors_vec_:
            s.correspondences_.close()


@pytest.mark.parametrize("fast", [0, 1], ids=["streaming", "from-moments"])
def test_one_correspondence_has_no_covariance(ra, ctx, maps, fast):
    """computeCrossStatistics with ONE valid correspondence: n_meas 1 and a covariance of exact zeros, from the streaming reduction
    and from the moments the find published (whose sums carry their own rounding, ~1e-15: noise the solve would turn into a rotation)"""
    sc = uc.scenes()["cube_1"]
    rcc = _operator(ra, maps(sc), sc)
    rcc.set_micp_fast(fast)
    rcc.find(uc.orc.tmult(sc.Tom, sc.Tbo))
    for Tpre in (uc.orc.transform(), uc.orc.transform_from_rpy((0.0, 0.0, 0.17), (0, 0, 0)), uc.orc.transform_from_rpy((0.01, 0.0, 0.1), (0.01, 0, 0.02))):
        s = rcc.computeCrossStatistics(Tpre, 0.0)
        assert int(s["n_meas"]) == 1
        assert not np.any(s["covariance"]), s["covariance"]
    if fast:
        assert rcc.ccs_info()["from_moments"] >= 1      # the path this is about was taken
    rcc.close()
