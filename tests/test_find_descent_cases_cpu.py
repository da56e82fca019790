"""The case generator of the cooperative-descent tests (tests/descent_cases.py) through the CPU oracle alone: the randomised scans
really contain hits AND misses (so a kernel that loses or invents hits cannot hide in empty scans), and on every one of them the
oracle's BVH walk over all rays equals brute force on a sample of the scan's own rays -- which is what lets the GPU test take the
fast walk as its authority."""
import numpy as np
import pytest

import descent_cases as dc


def test_knob_sets_and_their_encoding():
    assert dc.KNOB_SETS[0] == dc.DEFAULT_KNOBS == (64, 24, 24, False)
    assert len(set(dc.KNOB_SETS)) == len(dc.KNOB_SETS) == 11
    for group in (dc.TILE_KNOBS, dc.RANDOM_KNOBS, dc.BATCH_KNOBS, dc.MOMENT_KNOBS):
        assert set(group) <= set(dc.KNOB_SETS)
    for cap, levels, leaf_cap, four_wide in dc.KNOB_SETS:
        assert 0 <= cap <= 64                                   # the library refuses more
        w = dc.descent_word(levels, leaf_cap, four_wide)
        assert w & 0xFF == levels and (w >> 8) & 0xFF == leaf_cap and (w >> 31) == int(four_wide)
        assert (w >> 16) & 0x7FFF == 0                           # the tile-mapping override (bits 29..30) stays off
    assert dc.descent_word(24, 24, False) == 24 | (24 << 8)
    assert dc.descent_word(24, 24, True) == 24 | (24 << 8) | (1 << 31)
    with pytest.raises(AssertionError):
        dc.descent_word(24, 0, False)                           # leaf-cap bits of 0 would keep the old cap: never a complete word
    assert dc.variant_word(32) == (1 << 14) and dc.variant_word(23, 3) == 7 | (1 << 13) | (3 << 4)
    assert len(set(k for k in map(dc.knob_name, dc.KNOB_SETS))) == 11


def test_generator_is_deterministic():
    v, _ = dc.random_map("tiny")
    a, b = dc.random_scans("tiny", v), dc.random_scans("tiny", v)
    assert [s.name for s in a] == [s.name for s in b] and len(a) == dc.N_RANDOM_SCANS
    for x, y in zip(a, b):
        assert x.pose.tobytes() == y.pose.tobytes() and x.Tsb.tobytes() == y.Tsb.tobytes() and x.n_rays == y.n_rays
    assert [s.name for s in dc.random_scans("tiny", v, 8)] == [s.name for s in a[:8]]       # a cut keeps the first cases


def test_randomised_scans_contain_hits_and_misses_and_the_bvh_walk_equals_brute_force(orc):
    per_map, kinds, sizes = {}, set(), set()
    for name in dc.RANDOM_MAPS:
        v, f = dc.random_map(name)
        m = orc.Mesh(v, f)
        per_map[name] = []
        scans = dc.random_scans(name, v)
        assert len(scans) == dc.N_RANDOM_SCANS
        for s in scans:
            ref = s.oracle(m, bvh=True)
            assert ref["hits"].size == s.n_rays
            idx, hits, face_ids = s.brute_force_sample(orc, m)
            assert len(idx) == min(2048, s.n_rays)
            assert np.array_equal(ref["hits"][idx], hits), "%s: BVH walk and brute force disagree on hits" % s.name
            bad = ref["face_ids"][idx] != face_ids
            assert not bad.any(), "%s: BVH walk and brute force disagree on %d of %d face ids" % (s.name, bad.sum(), bad.size)
            per_map[name].append(ref["hits"])
            kinds.add(s.kind)
            if s.kind == "spherical":
                sizes.add((s.model.phi.size, s.model.theta.size))
    n_hits, n_rays = dc.hit_share_conditions(per_map)
    for name, scans in per_map.items():
        print("%-10s %2d scans with a hit, %2d with hits and misses, hit share %.3f" % (
            name, sum(1 for h in scans if h.any()), sum(1 for h in scans if h.any() and not h.all()),
            sum(int(h.sum()) for h in scans) / float(sum(h.size for h in scans))))
    print("all: %d of %d rays hit (%.3f)" % (n_hits, n_rays, n_hits / float(n_rays)))
    assert kinds == {"spherical", "o1dn", "pinhole"}
    assert (1, 7) in sizes and (128, 1024) in sizes
    # ties: on the duplicated soup every hit has a twin, and the smaller id of a pair must be the one reported
    v, f = dc.random_map("duplicates")
    key = np.sort(f.astype(np.int64), axis=1)
    order = np.lexsort(key.T[::-1])
    twin = np.empty(len(f), np.int64)
    twin[order[0::2]], twin[order[1::2]] = order[1::2], order[0::2]
    assert np.array_equal(key[twin], key)
    m = orc.Mesh(v, f)
    n_ties = 0
    for s in dc.random_scans("duplicates", v):
        ref = s.oracle(m, bvh=True)
        ids = ref["face_ids"][ref["hits"] > 0].astype(np.int64)
        assert (ids < twin[ids]).all(), s.name
        n_ties += len(np.unique(ids))
    assert n_ties > 200


def test_smallest_maps_are_hit_and_missed(orc):
    from rmcl_amd import types as T
    for n in (1, 4):
        v, f = dc.tiny_map(n)
        assert len(f) == n
        ref = orc.Mesh(v, f).simulate_spherical(dc.tiny_model(), T.identity(), dc.tiny_pose(), bvh=False)
        assert ref["hits"].any() and not ref["hits"].all()
        assert len(np.unique(ref["face_ids"][ref["hits"] > 0])) == n
