"""Pose batches at their edges (find_batch, correct_batch, simulate with several poses, ShardedCorrectorHip): the world-order launch
(k_batch_tile_keys, k_batch_cell_scan, k_batch_tile_scatter, the slot -> (pose, tile) mapping at the top of k_find), its fall-back to
the pose-major launch, the four sensor models, k_reduce_partials with blockIdx.y = pose on both sides of its block-size switch at four
poses, and k_batch_solve -- against the CPU oracle, whose own fitness for these cases tests/test_pose_batch_cases_cpu.py shows.

The order is read back through rmclhip_debug_batch_order (include/rmclhip_lab.h): what a wrong slot mapping, cell start or last turn
of the XCDs would do -- a slot skipped, a slot computed twice -- shows in caller-owned buffers full of 0xA5 bytes; what a wrong key
would do shows against the restated keys of tests/pose_batch_cases.py.
"""
import numpy as np
import pytest

import oracle_micp as om
import pose_batch_cases as pc
from conftest import find_kinds
from test_gpu_find import _compare, _brute_force_sample
from test_gpu_reduce import _stats_close, _transform_close

pytestmark = pytest.mark.gpu

ATTRS = ("hits", "ranges", "points", "normals", "face_ids")
_DTYPE = dict(hits=np.uint8, ranges=np.float32, points=np.float32, normals=np.float32, face_ids=np.uint32)
_WIDTH = dict(hits=1, ranges=1, points=3, normals=3, face_ids=1)
GUARD = 256          # elements behind the bundle: one workgroup's worth of rays

_CACHE = {}


def _maps(ra, orc, ctx, name):
    """(oracle mesh, device map) of a map of the cases, made once"""
    if ("map", name) not in _CACHE:
        v, f = pc.map_arrays(name)
        hm = ra.import_hip_map(ctx, v, f)
        info = hm.info()
        lo, hi = pc.map_bbox(name)
        assert np.array_equal(np.array(info["bbox_min"], np.float32), lo) and np.array_equal(np.array(info["bbox_max"], np.float32), hi)
        _CACHE[("map", name)] = (orc.Mesh(v, f), hm)
    return _CACHE[("map", name)]


def _lists():
    if "lists" not in _CACHE:
        _CACHE["lists"] = {"spread": pc.spread(), "edges": pc.edges(), "one_cell": pc.one_cell()}
    return _CACHE["lists"]


def _ref(ra, orc, ctx, map_name, kind, list_name):
    """the oracle's scans of a map x model x pose list: computed once, shared, never written to"""
    key = ("ref", map_name, kind, list_name)
    if key not in _CACHE:
        ref = pc.simulate(_maps(ra, orc, ctx, map_name)[0], pc.model(kind), _lists()[list_name], bvh=True, nthreads=8)
        for a in ref.values():
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _slice(out, i, n=pc.N_RAYS):
    return {k: out[k][i * n:(i + 1) * n] for k in ATTRS if k in out}


def _same_bits(a, b, what):
    for k in ATTRS:
        if k in a:
            assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def _assert_all_misses(out, what):
    assert not out["hits"].any(), what
    assert np.all(out["ranges"] == np.float32(pc.RANGE_MAX + 1.0)), what
    assert np.all(out["face_ids"] == 0xFFFFFFFF), what
    assert np.isnan(out["points"]).all() and np.isnan(out["normals"]).all(), what


def _rule_twl(variant):
    """log2 of the tile width the library's rule gives a 21-row model: 8 x 8 for the wave-packet kind, 16 wide x 4 tall otherwise"""
    return 3 if variant == 0 else 4


def _check_order(op, nposes, ngroups, on):
    """the read-back of the last batch launch: every (pose, workgroup) exactly once, in non-decreasing key order"""
    keys, order, ng = op.debug_batch_order()
    if not on:
        assert len(keys) == len(order) == 0 and ng == 0
        return keys
    assert ng == ngroups and len(keys) == len(order) == nposes * ngroups
    want = ((np.arange(nposes, dtype=np.uint32)[:, None] << 16) | np.arange(ngroups, dtype=np.uint32)[None, :]).reshape(-1)
    assert np.array_equal(np.sort(order), want), "the order is not a permutation of every (pose, workgroup)"
    along = keys[(order >> 16).astype(np.int64) * ngroups + (order & 0xFFFF)]
    assert np.all(np.diff(along.astype(np.int64)) >= 0), "keys read along the order decrease"
    assert keys.max() < pc.N_ORDER_CELLS
    return keys


# ---- a. every slot computed exactly once ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_kind", ["spherical", "pinhole"])
@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32))
def test_world_order_computes_every_slot_exactly_once(ra, orc, ctx, variant, model_kind):
    """37 poses x 21 x 150 rays into a caller-owned bundle pre-filled with 0xA5 bytes and one workgroup's worth of elements longer
    than the batch, for tile widths 4 / 8 / 16 / 32 and the pose-major launch, the default granule, granules 2, 3, 7 and one larger
    than the whole list: the bundle equals the oracle (a miss writes its miss values: no sentinel survives in range), every byte
    behind it is still 0xA5, every setting gives the same bits; the order read back is a permutation of every (pose, workgroup)
    sorted by key, its keys are the restated ones and occupy the cells the CPU test promises."""
    mesh, hm = _maps(ra, orc, ctx, "room30k")
    m = pc.model(model_kind)
    poses = _lists()["spread"]
    ref = _ref(ra, orc, ctx, "room30k", model_kind, "spread")
    n = len(poses) * pc.N_RAYS
    bundle = {a: ra.DeviceArray(ctx, _DTYPE[a], (n + GUARD) * _WIDTH[a]) for a in ATTRS}
    fill = {a: np.full((n + GUARD) * _WIDTH[a] * np.dtype(_DTYPE[a]).itemsize, 0xA5, np.uint8).view(_DTYPE[a]) for a in ATTRS}
    group = pc.group_of(variant)
    for tile_bits in pc.TILE_BITS:
        twl = tile_bits - 1
        op = pc.operator(ra, hm, m, variant, tile_bits)
        ngroups = pc.n_groups(twl, group)
        restated, ng = pc.restated_keys(m, poses, pc.map_bbox("room30k"), twl, group)
        assert ng == ngroups
        first = None
        for on in pc.ORDER_SETTINGS:
            op.set_batch_order(on)
            for a in ATTRS:
                bundle[a].upload(fill[a])
            op.simulate(poses, attributes=ATTRS, into=bundle)
            op.sync()
            keys = _check_order(op, len(poses), ngroups, on)
            raw = {a: bundle[a].download() for a in ATTRS}
            what = "kind %d, %s, tile width %d, order %d" % (variant, model_kind, 1 << twl, on)
            for a in ATTRS:
                assert raw[a][n * _WIDTH[a]:].tobytes() == fill[a][n * _WIDTH[a]:].tobytes(), what + ": bytes behind the bundle changed (" + a + ")"
            out = {a: (raw[a][:n * 3].reshape(-1, 3) if _WIDTH[a] == 3 else raw[a][:n]) for a in ATTRS}
            if first is None:
                first = out
                _compare(out, ref, what)
            else:
                _same_bits(first, out, what)
            if on:
                cells, runs = pc.cells_and_runs(keys)
                assert cells >= pc.MIN_DISTINCT_CELLS and runs >= pc.MIN_SCAN_RUNS, (what, cells, runs)
                assert np.array_equal(keys, restated), "%s: %d of %d keys differ from the restated ones" % (what, (keys != restated).sum(), len(keys))
        op.close()
    for d in bundle.values():
        d.free()


# ---- b. the operator's own buffers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_name", pc.MAP_NAMES)
@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32))
def test_edge_poses_in_the_operators_own_buffers(ra, orc, ctx, variant, map_name):
    """find_batch of `edges` (inside, outside, 500 m away, NaN translation, NaN quaternion, on a bounding-box face, one pose three
    times) for the four models on the room, the cube and the flat two-triangle map, each call behind a find_batch of as many far
    poses -- stale contents are misses and cannot pass for the answer: equal to the oracle pose by pose, the three copies of one pose
    bit-identical to each other and to a single find of it."""
    mesh, hm = _maps(ra, orc, ctx, map_name)
    poses = _lists()["edges"]
    for model_kind in pc.MODEL_KINDS:
        what = "%s, %s, kind %d" % (map_name, model_kind, variant)
        op = pc.operator(ra, hm, pc.model(model_kind), variant)
        op.find_batch(pc.far_poses(len(poses)))
        _assert_all_misses(op.modelView(), what + ": far poses")
        op.find_batch(poses)
        _check_order(op, len(poses), pc.n_groups(_rule_twl(variant), pc.group_of(variant)), 1)
        out = op.modelView()
        ref = _ref(ra, orc, ctx, map_name, model_kind, "edges")
        for i in range(len(poses)):
            _compare(_slice(out, i), _slice(ref, i), "%s, pose %d (%s)" % (what, i, pc.EDGE_NAMES[i]))
        for i in pc.EDGE_NO_HIT:
            _assert_all_misses(_slice(out, i), "%s, pose %d" % (what, i))
        a0 = _slice(out, pc.EDGE_COPIES_OF_A[0])
        for i in pc.EDGE_COPIES_OF_A[1:]:
            _same_bits(a0, _slice(out, i), "%s, copies of interior A" % what)
        op.find_batch(pc.far_poses(1))
        op.find(poses[0])
        _same_bits(a0, op.modelView(), what + ", a single find of interior A")
        op.close()


# ---- c. one cell --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", find_kinds(0, 2, 23, 24, 32, 17, 25))
def test_a_batch_whose_entries_share_one_cell(ra, orc, ctx, variant):
    """40 poses with NaN translations: one key, the order still a permutation, every output a miss with the miss values; then
    `spread` on the same operator (its buffers and sort scratch go from the largest cell population to the smallest) equals the
    oracle."""
    mesh, hm = _maps(ra, orc, ctx, "room30k")
    op = pc.operator(ra, hm, pc.model("spherical"), variant)
    ngroups = pc.n_groups(_rule_twl(variant), pc.group_of(variant))
    poses = _lists()["one_cell"]
    op.find_batch(poses)
    keys = _check_order(op, len(poses), ngroups, 1)
    assert not keys.any()
    _assert_all_misses(op.modelView(), "one cell, kind %d" % variant)
    op.find_batch(_lists()["spread"])
    keys = _check_order(op, 37, ngroups, 1)
    assert pc.cells_and_runs(keys)[0] >= pc.MIN_DISTINCT_CELLS
    _compare(op.modelView(), _ref(ra, orc, ctx, "room30k", "spherical", "spread"), "spread after one cell, kind %d" % variant)
    op.close()


# ---- d. the fall-back ---------------------------------------------------------------------------------------------------------------
def test_more_workgroups_than_an_order_word_holds_falls_back_to_pose_major(ra, orc, ctx):
    """kind 2 runs one tile per workgroup: 1024 x 4096 rays are 65 536 of them per pose, one more than the 16 bits of an order word
    hold, and the batch goes pose-major -- the read-back says so, each pose's slice is bit-identical to a single find of it, and 2000
    rays of each agree with the exhaustive oracle."""
    import math
    from rmcl_amd import types as T
    mesh, hm = _maps(ra, orc, ctx, "cube")
    f32 = np.float32
    Hb, Wb = 1024, 4096
    model = T.spherical_model(f32(-1.0), f32(2.0 / (Hb - 1)), Hb, f32(-math.pi), f32(2 * math.pi / Wb), Wb, f32(0.1), f32(40.0))
    poses = np.array([T.transform_from_rpy((1.0, -2.0, 1.2), (0.02, -0.03, 0.4)), T.transform_from_rpy((-3.0, 2.5, -1.0), (0.1, 0.2, -2.0))],
                     dtype=T.TRANSFORM)
    names = ("hits", "ranges", "face_ids")
    op = ra.RCCHipSpherical(hm)
    op.setTsb(T.identity())
    op.setModel(model)
    op.set_traversal(2)
    op.set_outputs(names)
    n = Hb * Wb
    op.find_batch(pc.far_poses(2))
    op.find_batch(poses)
    keys, order, ng = op.debug_batch_order()
    assert len(keys) == 0 and len(order) == 0 and ng == 0
    out = op.modelView(names)
    assert out["hits"].size == 2 * n
    for i in range(2):
        op.find(poses[i])
        single = op.modelView(names)
        sl = {k: out[k][i * n:(i + 1) * n] for k in names}
        for k in names:
            assert sl[k].tobytes() == single[k].tobytes(), (i, k)
        _brute_force_sample(orc, mesh, model, poses[i], sl, 2000, seed=i)
    op.close()


# ---- e. batched reduction and solve -------------------------------------------------------------------------------------------------
def _exact_as_dict(s):
    return dict(dataset_mean=np.array([s["dataset_mean"][k] for k in "xyz"], np.float64), model_mean=np.array([s["model_mean"][k] for k in "xyz"], np.float64),
                covariance=s["covariance"].astype(np.float64).reshape(3, 3), n_meas=int(s["n_meas"]))


def _corrector(ra, hm, m, ranges, max_dist=0.5):
    op = pc.operator(ra, hm, m)
    op.set_dataset_from_ranges(ranges)
    op.params.max_dist = op.adaptive_max_dist_min = max_dist
    return op


@pytest.mark.parametrize("case", ["spherical", "pinhole", "o1dn", "ondn", "spherical 1x63", "spherical 1x1"])
def test_batched_reduction_on_both_sides_of_its_block_size_switch(ra, orc, ctx, case):
    """correct_batch of 1, 2, 3, 4, 5 and 9 poses (k_reduce_partials works in blocks of 512 elements below four poses and of 4096
    from four on) over 3150 elements -- a multiple of neither, nor of a wave -- for the four models, and over 63 and 1 element:
    n_meas exact, statistics against the oracle's exact ones, Tdelta against the oracle's correct_batch, pose by pose."""
    mesh, hm = _maps(ra, orc, ctx, "room30k")
    kind, _, shape = case.partition(" ")
    h, w = (int(x) for x in shape.split("x")) if shape else (pc.H, pc.W)
    m = pc.model(kind, h, w)
    truth, est9 = pc.truth_and_estimates(9)
    ranges, ds, mask = pc.measure(mesh, m, truth)
    op = _corrector(ra, hm, m, ranges)
    Tr, sr = om.correct_batch(mesh, m, pc.tsb(), est9, ds, mask, 0.5)
    if h * w == pc.N_RAYS:
        assert int(sr["n_meas"].min()) > 1000
    for n in pc.REDUCE_COUNTS:
        Td, st = op.correct_batch(est9[:n])
        assert len(Td) == len(st) == n
        for i in range(n):
            print("%s, %d poses, pose %d: n_meas %d (oracle %d)" % (case, n, i, int(st[i]["n_meas"]), int(sr[i]["n_meas"])))
            assert int(st[i]["n_meas"]) == int(sr[i]["n_meas"]), (case, n, i)
            _stats_close(st[i], _exact_as_dict(sr[i]))
            _transform_close(Td[i], Tr[i], 1e-5)
    op.close()


def test_empty_poses_in_a_batch_leave_their_neighbours_alone(ra, orc, ctx):
    """correct_batch of `edges`: the far pose and the two NaN poses have no correspondence -- n_meas 0 and the oracle's Tdelta, no NaN
    in it --, and every other pose returns the bytes it returns in a batch without those three (the partial rows of a pose are its
    own); the copies of interior A, which the dataset was measured next to, agree with the oracle."""
    mesh, hm = _maps(ra, orc, ctx, "room30k")
    m = pc.model("spherical")
    truth, _ = pc.truth_and_estimates(1)
    ranges, ds, mask = pc.measure(mesh, m, truth)
    op = _corrector(ra, hm, m, ranges)
    poses = _lists()["edges"]
    kept, where = pc.edges_without_the_empty_ones()
    Td9, st9 = op.correct_batch(poses)
    Td6, st6 = op.correct_batch(kept)
    Tr, sr = om.correct_batch(mesh, m, pc.tsb(), poses, ds, mask, 0.5)
    for i in range(len(poses)):
        assert int(st9[i]["n_meas"]) == int(sr[i]["n_meas"]), i
    for i in pc.EDGE_NO_HIT:
        assert int(st9[i]["n_meas"]) == 0
        assert not np.isnan(np.frombuffer(Td9[i].tobytes()[:28], np.float32)).any()
        _transform_close(Td9[i], Tr[i], 1e-5)
    for j, i in enumerate(where):
        assert Td9[i].tobytes() == Td6[j].tobytes() and st9[i].tobytes() == st6[j].tobytes(), "pose %d (%s)" % (i, pc.EDGE_NAMES[i])
    for i in pc.EDGE_COPIES_OF_A:
        assert int(st9[i]["n_meas"]) > 1000
        _stats_close(st9[i], _exact_as_dict(sr[i]))
        _transform_close(Td9[i], Tr[i], 1e-5)
        assert Td9[i].tobytes() == Td9[0].tobytes() and st9[i].tobytes() == st9[0].tobytes()
    op.close()


@pytest.mark.parametrize("devices", [(0,), (0, 0), (0, 0, 0)])
def test_sharded_edges_batch_equals_the_single_operator(ra, orc, ctx, devices):
    """ShardedCorrectorHip on the `edges` batch, one to three replicas on device 0 (shards of 9, 5 + 4 and 3 + 3 + 3 poses: the last
    on the other side of the reduction's switch than the unsharded batch): byte-identical to one operator's correct_batch."""
    mesh, hm = _maps(ra, orc, ctx, "room30k")
    v, f = pc.map_arrays("room30k")
    m = pc.model("spherical")
    truth, _ = pc.truth_and_estimates(1)
    ranges, _, _ = pc.measure(mesh, m, truth)
    one = _corrector(ra, hm, m, ranges)
    Td1, st1 = one.correct_batch(_lists()["edges"])
    sh = ra.ShardedCorrectorHip(devices, v, f)

    def configure(r):
        r.setTsb(pc.tsb())
        r.setModel(m["model"])
        r.set_dataset_from_ranges(ranges)
        r.params.max_dist = r.adaptive_max_dist_min = 0.5

    sh.for_each(configure)
    Td, st = sh.correct_batch(_lists()["edges"])
    diff = [i for i in range(9) if Td[i].tobytes() != Td1[i].tobytes() or st[i].tobytes() != st1[i].tobytes()]
    print("devices %r: poses that differ from the single operator: %r" % (devices, diff))
    assert Td.tobytes() == Td1.tobytes() and st.tobytes() == st1.tobytes(), diff
    sh.close()
    one.close()


# ---- f. refusals and state ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_operator_working(ra, orc, ctx):
    """32 769 poses are refused by find_batch, correct_batch and simulate with RMCLHIP_ERR_UNSUPPORTED, a dataset shorter than the
    model by correct_batch; computeCrossStatistics refuses after a batch and works again after a single find; the operator computes
    the same as before all of it, and a batch of 9 gives the same bytes before and after a batch of 2."""
    from rmcl_amd import types as T, _capi
    mesh, hm = _maps(ra, orc, ctx, "room30k")
    m = pc.model("spherical")
    truth, est9 = pc.truth_and_estimates(9)
    ranges, ds, mask = pc.measure(mesh, m, truth)
    op = _corrector(ra, hm, m, ranges)
    op.find_batch(est9)
    before = op.modelView()
    Tb, sb = op.correct_batch(est9)
    many = np.zeros(32769, dtype=T.TRANSFORM)
    many[:] = est9[0]
    big = ra.DeviceArray(ctx, np.float32, len(many) * pc.N_RAYS)      # (what the call would write, were it not refused)
    for call in (lambda: op.find_batch(many), lambda: op.correct_batch(many), lambda: op.simulate(many, attributes=("ranges",), into={"ranges": big})):
        with pytest.raises(ra.RmclHipError) as e:
            call()
        assert e.value.status == _capi.ERR_UNSUPPORTED and "32768" in str(e.value)
    big.free()
    _same_bits(before, op.modelView(), "model buffers after the refusals")
    op.set_dataset(ds[:100], mask[:100])
    with pytest.raises(ra.RmclHipError) as e:
        op.correct_batch(est9)
    assert e.value.status == _capi.ERR_INVALID and "dataset size" in str(e.value)
    op.set_dataset_from_ranges(ranges)
    op.find_batch(est9)
    with pytest.raises(ra.RmclHipError) as e:
        op.computeCrossStatistics(T.identity())
    assert "last find was a batch" in str(e.value)
    op.find(est9[0])
    s = op.computeCrossStatistics(T.identity())
    assert int(s["n_meas"]) == int(sb[0]["n_meas"]) > 1000
    # 9, 2, 9
    op.find_batch(est9[:2])
    two = op.modelView()
    _same_bits(_slice(before, 1), _slice(two, 1), "pose 1 of two")
    op.find_batch(est9)
    _same_bits(before, op.modelView(), "a batch of 9 after a batch of 2")
    op.correct_batch(est9[:2])
    Ta, sa = op.correct_batch(est9)
    assert Ta.tobytes() == Tb.tobytes() and sa.tobytes() == sb.tobytes()
    op.close()
