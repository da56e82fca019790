"""The premises of the Stein step's edge cases (tests/stein_cases.py) without a device: the numpy restatement (tests/stein_ref.py) on
lattices of exact oracle distances -- room30k at cell 0.4, margin 0.5, and field_cases' floor and degcube.  Every cloud that
tests/test_gpu_stein_edges.py sends to the device is shown here to hold what it is there for (rotational spread about every axis, bins
in every block of the prefix sum, thinned bins beside unthinned ones, a wrapped probe chain, ...), so a device failure can never be
blamed on an empty case.  Every test prints its case's number of bins and the neighbours' minimum, median and maximum
(profiles/stein_edge_cases.txt records them)."""
import itertools

import numpy as np
import pytest

import field_cases as fc
import field_ref as fr
import refine_ref as rr
import stein_cases as sc
import stein_ref as sr

F = np.float32
D = np.float64
PLANAR = sc.PLANAR


@pytest.fixture(scope="module")
def room(ra, orc):
    """made once: (info, oracle lattice, 5 beams, Tsb, truth [1])"""
    v, f = fc.build_map("room30k")
    m = orc.Mesh(v, f)
    info = fr.layout(v.min(0), v.max(0), cell=sc.ROOM_CELL, margin=sc.ROOM_MARGIN)
    truth, Tsb, cloud = sc.room_scan(m)
    beams = ra.sample_beams(cloud, 5, seed=7)
    assert len(beams) == 5
    return info, fr.oracle_lattice(m, info), beams, Tsb, truth


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def _binned_is_brute(room, poses, p):
    """the cell list against the sum over all pairs, with nobody thinned away; the binned result"""
    info, lat, beams, Tsb, _ = room
    assert p["max_per_bin"] >= len(poses)
    binned = sr.step(info, lat, poses, beams, Tsb, p)
    assert _same(binned, sr.step(info, lat, poses, beams, Tsb, p, brute=True)) and binned[2]["n_thinned_bins"] == 0
    return binned


# ---- 1. tilted clouds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0x3F, 0x38, 0x1F])
def test_tilted_dense_premises(room, mask):
    truth = room[4]
    poses = sc.tilted(truth, "dense")
    assert len(poses) == 257
    p = sr.params(iterations=2, dof_mask=mask, max_per_bin=257)
    out, rows, st = _binned_is_brute(room, poses, dict(p, iterations=1))
    print(sc.describe("tilted-dense, mask %#x, the start" % mask, rows, st))
    e, counts, _, _, _ = sr.pairs_of(poses, p)
    nb = counts.sum(axis=1)
    assert (nb == rows["n_neighbours"]).all() and np.median(nb) >= 16 and nb.max() > 64
    out, rows, st = _binned_is_brute(room, poses, p)
    print(sc.describe("tilted-dense, mask %#x, the second iteration" % mask, rows, st))
    # the rotational spread is about every free axis: for EVERY particle (so for a fixed one) more than half of its counted pairs have
    # e[3] != 0 and more than half e[4] != 0
    for k in (3, 4) + ((5,) if mask & 0x20 else ()):
        assert (((e[..., k] != 0) & counts).sum(axis=1) * 2 > nb).all()
    if not mask & 0x20:
        assert (e[..., 5] == 0).all()
    # and the rotations move
    R, t = rr.pose_arrays(poses)
    Ro, to = rr.pose_arrays(out)
    assert ((Ro != R).any(axis=1)).sum() > 200
    # a prefix of the cloud is the cloud of that size
    for n in sc.N_TILTED:
        assert sc.tilted(truth, "dense", n).tobytes() == poses[:n].tobytes()


def test_tilted_spread_premises(room):
    poses = sc.tilted(room[4], "spread")
    out, rows, st = _binned_is_brute(room, poses, sr.params(iterations=2, max_per_bin=257))
    print(sc.describe("tilted-spread", rows, st))
    assert st["n_bins"] > 200 and rows["n_neighbours"].min() == 0
    # +-0.5 rad per axis: the rotations are far from each other (w of the pairs' products goes well below 1), never half a turn apart
    w = sc.product_w(poses)
    assert w.min() < 0.95 and (w > 0).all()


def test_flipped_quaternions_negate_exactly_their_outputs(room):
    info, lat, beams, Tsb, truth = room
    poses = sc.tilted(truth, "dense")
    idx = sc.flipped_indices(len(poses))
    assert len(idx) == 128 + 2 and all(i in idx for i in sc.FLIP_EXTRA)
    flipped = sc.negate_rotations(poses, idx)
    is_flipped = np.zeros(len(poses), bool)
    is_flipped[idx] = True
    p = sr.params(iterations=1)
    _, counts, _, _, _ = sr.pairs_of(flipped, p)
    w = sc.product_w(flipped)
    # pairs that count with w < 0, the negated quaternion on either side; pairs of two negated quaternions with w > 0
    i_side = counts & (w < 0) & is_flipped[:, None] & ~is_flipped[None, :]
    j_side = counts & (w < 0) & ~is_flipped[:, None] & is_flipped[None, :]
    both = counts & (w > 0) & is_flipped[:, None] & is_flipped[None, :]
    print("[stein-edges] flipped: %d counted pairs with w < 0 and particle i negated, %d with j negated, %d with both (w > 0)" %
          (i_side.sum(), j_side.sum(), both.sum()))
    assert i_side.sum() > 1000 and j_side.sum() > 1000 and both.sum() > 1000
    assert ((counts & (w < 0)) == (counts & (is_flipped[:, None] != is_flipped[None, :]))).all()
    for extra in sc.FLIP_EXTRA:          # the two even ones, both ways round
        assert i_side[extra].any() and j_side[:, extra].any()
    for iterations in (1, 3):
        p = sr.params(iterations=iterations)
        a = sr.step(info, lat, poses, beams, Tsb, p)
        b = sr.step(info, lat, flipped, beams, Tsb, p)
        assert b[0].tobytes() == sc.negate_rotations(a[0], idx).tobytes() and b[1].tobytes() == a[1].tobytes() and a[2] == b[2]
        assert b[0].tobytes() != a[0].tobytes()


# ---- 2. many bins across the blocks of the prefix sum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.N_CLUSTERED)
def test_clustered_premises(room, n):
    poses = sc.clustered_cloud(room[4], n)
    p = sr.params(iterations=2, max_per_bin=n)
    assert len(poses) == n and 32 <= sc.N_CLUSTERS <= 64 and sr.bin_margin(poses, p) >= 0.05
    _, t = rr.pose_arrays(poses)
    _, t0 = rr.pose_arrays(room[4])
    assert np.abs(t.astype(D) - t0.astype(D)).max() <= 3.0
    b = sr.bins(t, p)
    for c in range(sc.N_CLUSTERS):       # each cluster inside one bin, several members
        assert len(np.unique(b[c::sc.N_CLUSTERS], axis=0)) == 1 and len(b[c::sc.N_CLUSTERS]) >= 8
    assert len(np.unique(b, axis=0)) == sc.N_CLUSTERS
    words = sr.table_words(n)
    assert words == {513: 2048, 1025: 4096}[n]
    per = sc.occupied_per_block(poses, p)
    print("[stein-edges] clustered %d: %d words, occupied words per 1024-word block %s" % (n, words, [int(k) for k in per]))
    assert len(per) == words // 1024 and per.sum() == sc.N_CLUSTERS and per.min() >= 8
    out, rows, st = _binned_is_brute(room, poses, dict(p, iterations=1))
    print(sc.describe("clustered %d, the start" % n, rows, st))
    assert st["n_bins"] == sc.N_CLUSTERS and np.median(rows["n_neighbours"]) >= 4
    out, rows, st = _binned_is_brute(room, poses, p)       # the repulsion has spread the clusters over more bins
    print(sc.describe("clustered %d, the second iteration" % n, rows, st))
    assert st["n_bins"] >= sc.N_CLUSTERS and np.median(rows["n_neighbours"]) >= 4
    # the planar table (the device test's other mask) has words in every block too
    assert sc.occupied_per_block(poses, sr.params(dof_mask=PLANAR)).min() >= 8


@pytest.mark.parametrize("n", sc.N_FULL)
def test_full_table_premises(room, n):
    poses = sc.full_cloud(room[4], n)
    p = sr.params(max_per_bin=n)
    assert len(poses) == n and sr.table_words(n) == 2 * n
    _binned_is_brute(room, poses, dict(p, iterations=2))
    out, rows, st = _binned_is_brute(room, poses, p)
    words, occupied, home, stored = sr.table_of(poses, p)
    displaced = sum(1 for k in stored if stored[k] != home[k])
    print(sc.describe("full %d" % n, rows, st) + "; %d of %d words occupied, %d keys not at their home word" % (len(occupied), words, displaced))
    assert st["n_bins"] == len(occupied) and 4 * st["n_bins"] >= 3 * n and displaced >= 1


# ---- 3. several thinned bins --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [False, True])
def test_row_premises(room, interleaved):
    info, lat, beams, Tsb, truth = room
    poses = sc.row_cloud(truth, interleaved)
    n = len(poses)
    assert n == sum(sc.ROW_COUNTS) == 340 and sc.ROW_COUNTS == (130, 70, 10, 64, 65, 1)
    assert sc.ROW_CAPS == (1, 2, 63, 64, 65, 0xFFFFFFFF) and sc.SEED64 == (0x9E3779B9 << 32) | 11 and sc.SEED64 >> 32 != 0
    _, t = rr.pose_arrays(poses)
    bx = sr.bins(t, sr.params())
    assert len(np.unique(bx[:, 1:], axis=0)) == 1 and sr.bin_margin(poses, sr.params()) >= 0.049
    if not interleaved:                  # the first wave lies in the bin of 130: its single add crosses a cap below 64 from 0
        assert len(np.unique(bx[:130], axis=0)) == 1
        assert sc.row_cloud(truth, True).tobytes() == poses[sc.row_permutation()].tobytes()
    else:                                # every wave of 64 holds particles of the bin of 130, none holds more than 63 of them
        in130 = bx[:, 0] == bx[:, 0].min()
        assert all(0 < in130[w:w + 64].sum() < 64 for w in range(0, n, 64))
    for cap, n_thinned in zip(sc.ROW_CAPS, sc.ROW_THINNED):
        p = sc.row_params(cap)
        assert p["iterations"] == 1 and n_thinned == sum(c > cap for c in sc.ROW_COUNTS)
        out, rows, st = sr.step(info, lat, poses, beams, Tsb, p)
        row = sc.row_bins(poses, p)
        print(sc.describe("row, %s, cap %d" % ("interleaved" if interleaved else "contiguous", cap), rows, st) + "; (count, listed) %s" % row)
        assert st["n_bins"] == 6 and st["n_thinned_bins"] == n_thinned and tuple(c for c, _ in row) == sc.ROW_COUNTS
        thinned = [c > cap for c, _ in row]
        for (c, l), th in zip(row, thinned):
            assert (1 <= l <= c) if th else l == c      # a thinned bin lists somebody
        ratio = [F(c) / F(l) for c, l in row]
        beside_unthinned = [k for k in range(6) if thinned[k] and any(0 <= j < 6 and not thinned[j] for j in (k - 1, k + 1))]
        if cap in (1, 2, 63):
            assert n_thinned >= 4
            # at least two thinned bins with different count / listed; a thinned bin lies beside an unthinned one; and two thinned
            # bins of different ratios lie beside each other
            assert len(set(ratio[k] for k in range(6) if thinned[k])) >= 2 and len(beside_unthinned) >= 1
            assert any(thinned[k] and thinned[k + 1] and ratio[k] != ratio[k + 1] for k in range(5))
        if cap == 63:                    # two thinned bins of different ratios, each beside an unthinned bin
            assert len(set(ratio[k] for k in beside_unthinned)) >= 2
        e, counts, _, _, cl = sr.pairs_of(poses, p)
        in_bins = sum((counts & (cl[0][None, :, 0] == k)).any(axis=1).astype(int) for k in np.unique(cl[0][:, 0]))
        if cap >= 63:                    # some particle has counted neighbours in at least three bins
            assert in_bins.max() >= 3
        assert out.tobytes() != poses.tobytes()
    # nobody thinned away: the interleaved result is the permutation of the contiguous one
    if interleaved:
        p = sc.row_params(0xFFFFFFFF, iterations=2)
        a = sr.step(info, lat, sc.row_cloud(truth, False), beams, Tsb, p)
        b = sr.step(info, lat, poses, beams, Tsb, p)
        perm = sc.row_permutation()
        assert b[0].tobytes() == a[0][perm].tobytes() and b[1].tobytes() == a[1][perm].tobytes()


# ---- 4. the draw's edges ------------------------------------------------------------------------------------------------------------------
def test_draw_premises(room):
    info, lat, beams, Tsb, truth = room
    poses = sc.row_cloud(truth)
    p = sc.row_params(64, step=0xFFFFFFFF, iterations=3)
    first, second, third = (sr.listed_of(poses, p, it) for it in range(3))
    assert (first != second).any() and (second != third).any()                    # step + it wraps to 0 and 1 ...
    assert (second == sr.listed_of(poses, dict(p, step=0), 0)).all() and (third == sr.listed_of(poses, dict(p, step=1), 0)).all()
    low = dict(p, seed=sc.SEED64 & 0xFFFFFFFF)
    assert all((sr.listed_of(poses, p, it) != sr.listed_of(poses, low, it)).any() for it in range(3))      # ... and the high word matters
    out, rows, st = sr.step(info, lat, poses, beams, Tsb, p)
    print(sc.describe("draw edges: step 0xFFFFFFFF, 3 iterations", rows, st) + "; listed %d, %d, %d at the start poses" %
          (first.sum(), second.sum(), third.sum()))
    assert sr.step(info, lat, poses, beams, Tsb, dict(p, iterations=1))[2]["n_thinned_bins"] == 3
    assert out.tobytes() != sr.step(info, lat, poses, beams, Tsb, low)[0].tobytes()


# ---- 5. masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", sc.MASKS)
def test_mask_premises(room, mask):
    info, lat, beams, Tsb, truth = room
    poses = sc.tilted(truth, "dense")
    p = sc.mask_params(mask)
    assert sc.MASKS == (0x00, 0x38, 0x01, 0x04, 0x24, 0x1F) and p["max_per_bin"] == 256 and p["iterations"] == 2 and len(poses) == 257
    out, rows, st = sr.step(info, lat, poses, beams, Tsb, p)
    print(sc.describe("mask %#04x" % mask, rows, st))
    if mask in (0x00, 0x38):
        assert st["n_bins"] == 1 and st["n_thinned_bins"] == 1
        assert sr.listed_of(poses, p, 0).sum() == 256 and sr.listed_of(out if mask == 0 else poses, p, 1).sum() == 253
    else:
        assert st["n_bins"] > 1 and st["n_thinned_bins"] == 0
    R, t = rr.pose_arrays(poses)
    Ro, to = rr.pose_arrays(out)
    if mask == 0x00:                     # nothing moves, the rows are written: everybody counts everybody who is listed
        assert out.tobytes() == poses.tobytes()
        assert rows["n_neighbours"].min() >= 200 and (rows["kernel_weight"] > 200).all() and (rows["n_used"] > 0).any()
    else:
        for k in range(3):
            moved = (to[:, k] != t[:, k]).sum()
            assert moved > 200 if (mask >> k) & 1 else moved == 0
        assert ((Ro != R).any(axis=1).sum() > 200) if mask & 0x38 else (Ro.tobytes() == R.tobytes())
        assert rows["n_neighbours"].max() > 0


# ---- 6. chosen collisions ----------------------------------------------------------------------------------------------------------------
def test_collision_premises(room):
    truth = room[4]
    chosen = sc.colliding_bins(truth)
    b0, _ = sc.bin_of(truth, sr.params())
    assert len(chosen) == len(set(b for b, _ in chosen)) == 6 and all(home in (62, 63) for _, home in chosen) and chosen[0][1] == 62
    assert all(max(abs(b[k] - b0[k]) for k in range(3)) <= 10 for b, _ in chosen)
    poses = sc.collision_cloud(truth)
    p = sr.params(iterations=2, max_per_bin=len(poses))
    assert len(poses) == 24 and sr.table_words(24) == 64
    words, occupied, home, stored = sr.table_of(poses, p)
    keys = [sr.bin_key(b) for b, _ in chosen]
    assert words == 64 and len(stored) == 12 and all(home[k] == h for k, (_, h) in zip(keys, chosen))
    # six keys from words 62 and 63 on, one of them from 62: whatever the order of insertion they fill 62, 63, 0, 1, 2, 3 -- the chain
    # wraps --, the key in word 2 has passed at least three foreign keys and the one in word 3 at least four
    assert {62, 63, 0, 1, 2, 3} <= occupied
    wrapped = [k for k in keys if stored[k] in (0, 1)]
    passed = {k: (stored[k] - home[k]) % 64 for k in keys}
    print("[stein-edges] collisions: occupied words %s; the six keys' (home, stored in index order) %s" %
          (sorted(occupied), [(home[k], stored[k]) for k in keys]))
    assert len(wrapped) == 2 and max(passed[k] for k in wrapped) >= 3 and sum(passed.values()) >= 1 + 2 + 3 + 4
    # the probes for the EMPTY bins around a cluster walk the chain too: some neighbouring bin's key starts inside it
    around = [sr.bin_key(tuple(b[k] + d[k] for k in range(3))) for b, _ in chosen for d in itertools.product((-1, 0, 1), repeat=3)]
    assert any(k not in stored and (sr.mix64(k) & 63) in (62, 63, 0, 1, 2) for k in around)
    out, rows, st = _binned_is_brute(room, poses, dict(p, iterations=1))
    print(sc.describe("collisions", rows, st))
    assert (rows["n_neighbours"][:18] == 2).all() and (rows["n_neighbours"][18:] == 0).all() and st["n_bins"] == 12
    _binned_is_brute(room, poses, p)


# ---- 7. the clouds of the scratch-reuse case -----------------------------------------------------------------------------------------------
def test_scratch_reuse_sizes():
    """1025 particles, then 5, then 65: the tables shrink from 4096 words to 64 and grow to 256, the scan from four blocks to one"""
    assert [sr.table_words(n) for n in (1025, 5, 65)] == [4096, 64, 256]
    assert [sr.table_words(n) for n in (1, 32, 33, 512, 513)] == [64, 64, 128, 1024, 2048]
    # splitmix64's first output from the seed 0 (its published test vector) is the finaliser of the golden-ratio increment
    assert sr.mix64(0) == 0 and sr.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF and sr.bin_key((0, 0, 0)) == 8192 | 8192 << 14 | 8192 << 28
    assert sr.bin_key((-8192, 8191, 1)) == 0 | 16383 << 14 | 8193 << 28


# ---- 8. hard maps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.HARD_MAPS)
def test_hard_map_premises(ra, orc, name):
    """floor, rank three: with the smallest lambda0 the check accepts (0 is refused) NO solve is rejected -- every pivot carries the
    solve's own + 1e-9, and the lattice's gradient along the plane is exactly zero, so the drive along x, y and yaw is exactly zero
    and those moves are the neighbours' repulsion alone.  The `ok == false` path of the drive is unreachable on this map."""
    info, lat, _ = fc.oracle_lattice(orc, name)
    truth, Tsb, beams, poses, kw = sc.hard_case(ra, orc, name)
    assert len(poses) == 65 and len(beams) == fc.REFINE_CASES[name][0]
    tiny = np.nextafter(F(0), F(1))
    with pytest.raises(ValueError):
        sr.check(sr.params(lambda0=0.0, **kw), 65, len(beams))
    sr.check(sr.params(lambda0=tiny, **kw), 65, len(beams))
    for mask in (0x3F, PLANAR):
        for lambda0 in (1e-3, tiny):
            p = sr.params(iterations=2, dof_mask=mask, max_per_bin=65, lambda0=lambda0, **kw)
            binned = sr.step(info, lat, poses, beams, Tsb, p)
            assert _same(binned, sr.step(info, lat, poses, beams, Tsb, p, brute=True))
            out, rows, st = binned
            print(sc.describe("%s, mask %#x, lambda0 %g" % (name, mask, lambda0), rows, st))
            assert np.median(rows["n_neighbours"]) >= 4 and rows["n_used"].min() > 0 and out.tobytes() != poses.tobytes()
            R, t = rr.pose_arrays(poses)
            C, A, b, n_used = rr.evaluate(info, lat, R, t, Tsb, beams, p)
            delta, ok = rr.solve(A, b, mask, np.full(65, D(p["lambda0"]), D), p)
            assert ok.all()
            if name == "floor":          # nothing drives along the plane; the particles move there all the same
                assert (delta[:, 0] == 0).all() and (delta[:, 1] == 0).all() and ((delta[:, 2] != 0).sum() > 60 or not mask & 4)
                assert (out["t"]["x"] != poses["t"]["x"]).sum() > 60
