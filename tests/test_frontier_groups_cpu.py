"""The group boxes of the frontier tables (bvh_build.h frontier_groups_of; exported by rmclhip_bvh_build_host_frontier): find kind 32
skips a block of its cull when the boxes of the block's four groups lie outside the tile's pyramid, so a group box that does not
contain one of its entries' boxes loses hits silently.  Host only: every group box contains the stored boxes of table entries
16 g ... 16 g + 15 and is their exact union, a short last group counts its entries, groups past the table's end hold the far point,
and both trees (the map's and the particle filter's) are covered."""
import numpy as np
import pytest

import descent_cases as dc

FAR = np.array([1.0e30, 2.0e30, 3.0e30], np.float32)


def _maps():
    from rmcl_amd import synthetic as syn
    return {
        "four_triangles": dc.tiny_map(4),               # one entry
        "one_triangle": dc.tiny_map(1),
        "chain200": syn.exp_chain(200, 1.5),            # leaves above the frontier's depth
        "nested200": syn.nested_triangles(200, 1.2, 1e-3),
        "cube4": syn.cube_room(grid=4),                 # <= 64 entries: one block of the cull
        "cube5": syn.cube_room(grid=5),                 # 65 - 128 entries, a short last group
        "cube": syn.cube_room(),                        # nearly full, a short last group
        "sphere20k": syn.uv_sphere(20000),              # a full table
        "room": syn.noisy_room(20000),
        "soup": dc.soup(21, 2500),
    }


def _boxes(rows):
    f = rows.view(np.float32)
    return f[:, 0:3], f[:, 3:6]


@pytest.mark.parametrize("pf_tree", [False, True], ids=["map_tree", "filter_tree"])
def test_group_boxes_are_the_unions_of_their_entries(ra, pf_tree):
    sizes = {}
    for name, (v, f) in _maps().items():
        table, groups = ra.build_bvh_host_frontier(v, f, pf_tree)
        n = len(table)
        sizes[name] = n
        assert 0 < n <= 256, name
        assert groups.shape == (16, 8), name
        lo, hi = _boxes(table)
        glo, ghi = _boxes(groups)
        assert (lo <= hi).all() and np.isfinite(lo).all() and np.isfinite(hi).all(), name
        for g in range(16):
            mine = slice(16 * g, min(16 * g + 16, n))
            count = max(0, min(16 * g + 16, n) - 16 * g)
            assert int(groups[g, 6]) == count, "%s group %d: covers %d entries, says %d" % (name, g, count, int(groups[g, 6]))
            assert int(groups[g, 7]) == 0
            if count == 0:
                assert np.array_equal(glo[g], FAR) and np.array_equal(ghi[g], FAR), "%s group %d: an empty group is the far point" % (name, g)
                continue
            assert (glo[g] <= lo[mine]).all() and (ghi[g] >= hi[mine]).all(), "%s group %d does not contain its entries" % (name, g)
            assert np.array_equal(glo[g], lo[mine].min(axis=0)) and np.array_equal(ghi[g], hi[mine].max(axis=0)), \
                "%s group %d is not the union of its entries" % (name, g)
    print("entries per table (%s): %s" % ("filter's tree" if pf_tree else "map's tree", sizes))
    if not pf_tree:     # the cases the GPU tests rely on (tests/test_gpu_find_cull_groups.py)
        assert sizes["cube4"] <= 64 < sizes["cube5"] <= 128 and sizes["cube5"] % 16 != 0
        assert sizes["cube"] > 128 and sizes["cube"] % 16 != 0
        assert sizes["sphere20k"] == 256 and sizes["four_triangles"] == 1


def test_the_two_trees_have_their_own_tables(ra):
    """the filter's tree cuts the same binary tree at smaller leaves: other entries, other groups"""
    from rmcl_amd import synthetic as syn
    v, f = syn.cube_room(grid=5)
    t0, g0 = ra.build_bvh_host_frontier(v, f, False)
    t1, g1 = ra.build_bvh_host_frontier(v, f, True)
    assert len(t0) != len(t1) and not np.array_equal(g0, g1)


def test_a_depth_two_subtree_is_one_group_on_a_full_table(ra):
    """what the skip relies on for its effect (not for its correctness): on a full table 16 consecutive entries are one depth-2 subtree, so
    the group boxes are far smaller than the map -- their volumes sum to less than four times the volume of their union"""
    from rmcl_amd import synthetic as syn
    table, groups = ra.build_bvh_host_frontier(*syn.uv_sphere(20000))
    assert len(table) == 256
    glo, ghi = _boxes(groups)
    vol = np.prod((ghi - glo).astype(np.float64), axis=1)
    whole = np.prod((ghi.max(axis=0) - glo.min(axis=0)).astype(np.float64))
    print("group volumes / map volume: %s" % np.round(vol / whole, 3).tolist())
    assert vol.sum() < 4.0 * whole and vol.max() < 0.5 * whole
