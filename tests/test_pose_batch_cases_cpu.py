"""The case generator of the pose-batch tests (tests/pose_batch_cases.py) through the CPU oracle alone: these are the conditions the
GPU tests (tests/test_gpu_pose_batch.py) rely on, shown of the reference before any kernel runs.

* the oracle's BVH walk, which the GPU tests take as their authority, equals its exhaustive walk on every ray of every map x model x
  pose list used there;
* every pose of `edges` does what its name says;
* the restated sort keys of `spread` spread: many cells, and many of the runs of sixteen cells one thread of the cell scan owns;
  those of `one_cell` are one cell; NaN, infinite and far poses still get a cell, on the flat map too."""
import numpy as np
import pytest

import pose_batch_cases as pc


@pytest.fixture(scope="module")
def lists():
    return {"spread": pc.spread(), "edges": pc.edges(), "one_cell": pc.one_cell()}


def test_shapes_and_tables():
    assert pc.N_RAYS == 3150 and all(pc.N_RAYS % b for b in (64, 256, 512, 4096))
    for twl, tiles in ((2, 76), (3, 57), (4, 60), (5, 55)):
        tx, ty = pc.tiling(twl)
        assert tx * ty == tiles and pc.W % (1 << twl) and pc.H % (64 >> twl)          # ragged right and bottom tiles
    assert pc.n_groups(3, 4) * 4 > 57 and pc.n_groups(5, 4) * 4 > 55                  # a last workgroup of fewer than four tiles
    rows = pc.nan_rows()
    for kind in ("o1dn", "ondn"):
        m = pc.model(kind)
        nan = np.isnan(m["dirs"]).any(axis=1)
        assert np.array_equal(np.nonzero(nan)[0], rows) and 20 <= nan.sum() < 60
        for twl in (2, 3, 4, 5):                                                       # for EVERY forced width some workgroup's central ray is NaN
            for group in (1, 4):
                hit = [g for g in range(pc.n_groups(twl, group)) if nan[np.ravel_multi_index(pc.central_ray(twl, group, g), (pc.H, pc.W))]]
                assert hit and len(hit) < pc.n_groups(twl, group)
    origs = pc.model("ondn")["origs"]
    assert np.abs(origs).max() <= 0.2 and np.abs(origs).max() > 0.19 and any(pc.O1DN_ORIG)
    assert pc.variant_word(32, 4) == (1 << 14) | (4 << 4) and pc.variant_word(2, 6) == 2 | (6 << 4)
    v, f = pc.quad_map()
    assert len(f) == 2 and np.ptp(v[:, 2]) == 0 and np.ptp(v[:, 0]) == np.ptp(v[:, 1]) == 16.0
    lo, hi = pc.map_bbox("quad")
    assert lo[2] == hi[2]                                                              # the axis without extent reaches the key kernel as such


def test_pose_lists(lists):
    assert [len(lists[k]) for k in ("spread", "edges", "one_cell")] == [37, 9, 40]
    assert lists["spread"].tobytes() == pc.spread().tobytes() and lists["edges"].tobytes() == pc.edges().tobytes()
    z = lists["spread"]["t"]["z"]
    assert z.min() >= 0.3 and z.max() <= 5.5 and z.min() < 1.0 and z.max() > 4.5
    e = lists["edges"]
    a, b, c = (e[i].tobytes() for i in pc.EDGE_COPIES_OF_A)
    assert a == b == c
    assert np.isnan(e[4]["t"]["x"]) and np.isnan(e[6]["R"]["x"]) and not np.isnan(e[6]["t"]["x"])
    assert all(np.isnan(lists["one_cell"]["t"][k]).all() for k in "xyz")
    kept, where = pc.edges_without_the_empty_ones()
    assert where == [0, 1, 2, 5, 7, 8] and kept.tobytes() == e[where].tobytes()
    import oracle as orc
    sensor = orc.tmult(e[7], pc.tsb())
    assert abs(float(sensor["t"]["x"]) - float(pc.map_bbox("room30k")[1][0])) < 2e-6   # on the face, to the rounding of two compositions


@pytest.mark.parametrize("map_name", pc.MAP_NAMES)
def test_bvh_walk_equals_the_exhaustive_walk_on_every_ray(orc, lists, map_name):
    mesh = orc.Mesh(*pc.map_arrays(map_name))
    n_disagree = 0
    for kind in pc.MODEL_KINDS:
        m = pc.model(kind)
        for name in ("spread", "edges") + (("one_cell",) if (map_name, kind) == ("room30k", "spherical") else ()):
            P = lists[name]
            fast, full = pc.simulate(mesh, m, P, bvh=True), pc.simulate(mesh, m, P, bvh=False)
            assert fast["hits"].size == len(P) * pc.N_RAYS
            n_disagree += int((fast["hits"] != full["hits"]).sum()) + int((fast["face_ids"] != full["face_ids"]).sum())
            if name == "one_cell":
                assert not full["hits"].any()
    print("%s: %d disagreements between the BVH walk and the exhaustive walk" % (map_name, n_disagree))
    assert n_disagree == 0


def test_every_edge_pose_does_what_it_is_named_for(orc, lists):
    mesh = orc.Mesh(*pc.map_arrays("room30k"))
    for kind in pc.MODEL_KINDS:
        ref = pc.simulate(mesh, pc.model(kind), lists["edges"], bvh=True)
        hits = ref["hits"].reshape(9, pc.N_RAYS)
        per = hits.sum(axis=1)
        print(kind, per.tolist())
        for i in pc.EDGE_INTERIOR:
            assert per[i] > pc.N_RAYS // 2, (kind, i)
        assert 0 < per[1] < pc.N_RAYS and 0 < per[7] < pc.N_RAYS, kind                 # outside looking in; on the face: hits and misses
        for i in pc.EDGE_NO_HIT:
            assert per[i] == 0, (kind, i)
        for k in ref:
            rows = ref[k].reshape((9, pc.N_RAYS) + ref[k].shape[1:])
            assert rows[0].tobytes() == rows[5].tobytes() == rows[8].tobytes(), (kind, k)
        if kind in ("o1dn", "ondn"):                                                   # NaN rows are misses at every pose
            assert not hits[:, pc.nan_rows()].any()


def test_restated_keys_spread_and_collapse(lists):
    bb = pc.map_bbox("room30k")
    for kind in pc.MODEL_KINDS:
        m = pc.model(kind)
        for twl in (2, 3, 4, 5):
            for group in (4, 1):
                keys, ng = pc.restated_keys(m, lists["spread"], bb, twl, group)
                assert len(keys) == 37 * ng and ng == pc.n_groups(twl, group) and keys.max() < pc.N_ORDER_CELLS
                assert group == 1 or ng == {2: 19, 3: 15, 4: 15, 5: 14}[twl]
                cells, runs = pc.cells_and_runs(keys)
                print("spread, %s, tile width %d, %d per workgroup: %d distinct cells in %d runs of sixteen" % (kind, 1 << twl, group, cells, runs))
                assert cells >= pc.MIN_DISTINCT_CELLS and runs >= pc.MIN_SCAN_RUNS
    for map_name in pc.MAP_NAMES:
        bb = pc.map_bbox(map_name)
        for kind in pc.MODEL_KINDS:
            m = pc.model(kind)
            for twl in (2, 3, 4, 5):
                for group in (1, 4):
                    keys, ng = pc.restated_keys(m, lists["one_cell"], bb, twl, group)
                    assert len(keys) == 40 * ng and not keys.any(), (map_name, kind, twl, group)
                    keys, ng = pc.restated_keys(m, lists["edges"], bb, twl, group)
                    rows = keys.reshape(9, ng).astype(np.int64)
                    assert rows.min() >= 0 and rows.max() < pc.N_ORDER_CELLS
                    assert np.array_equal(rows[0], rows[5]) and np.array_equal(rows[0], rows[8])


def test_restated_keys_of_special_values():
    """infinite coordinates, a ray without direction and a NaN central ray all end in a cell"""
    from rmcl_amd import types as T
    inf = float("inf")
    poses = np.array([T.transform_from_rpy((inf, 0.0, 1.0), (0.0, 0.0, 0.0)), T.transform_from_rpy((-inf, inf, -inf), (0.0, 0.0, 0.0)),
                      T.transform((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), T.transform_from_rpy((1.0e30, 0.0, 0.0), (0.0, 0.0, 0.0))], dtype=T.TRANSFORM)
    for map_name in pc.MAP_NAMES:
        for kind in pc.MODEL_KINDS:
            keys, ng = pc.restated_keys(pc.model(kind), poses, pc.map_bbox(map_name), 4, 4)
            assert keys.dtype == np.uint32 and len(keys) == 4 * ng and keys.max() < pc.N_ORDER_CELLS
            zero_q = keys.reshape(4, ng)[2]                                            # a zero quaternion: no direction, the origin's cell ...
            assert len(np.unique(zero_q[zero_q != 0])) == 1                            # ... or cell 0 where the central ray is a NaN row (0 * NaN)
            assert (zero_q == 0).any() == (kind in ("o1dn", "ondn"))
