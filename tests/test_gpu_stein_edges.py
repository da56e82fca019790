"""The Stein variational step on the device at its edges (include/rmclhip.h, STEIN STEP ON THE FIELD; kernels: stein.hip): poses, rows
and stats against the numpy restatement (tests/stein_ref.py, fed with the device's downloaded lattice) byte for byte, on the clouds of
tests/stein_cases.py -- tests/test_stein_cases_cpu.py proves without a device that every one of them holds what it is there for:

  1. tilted clouds: rotations that differ about all three axes (e[3], e[4], R[3], R[4] are zero in tests/test_gpu_stein.py's clouds),
     and negated quaternions (the w < 0 flip of a pair's rotation);
  2. 64 and more occupied bins, at least eight in every 1024-word block of the prefix sum over the table (k_scan_totals, k_scan_add),
     and the fullest tables (n = 32 in 64 words, n = 512 in 1024);
  3. six adjacent bins thinned at different ratios beside unthinned ones, caps of 1, 2, a bin's count and its count +- 1, the cap
     crossed by a wave's first add or by a later wave;
  4. a 64-bit key with a high word, and step + it wrapping past 2^32;
  5. the masks 0x00, 0x38, single axes and mixed ones;
  6. a probe chain that wraps from the table's last word to word 0;
  7. a small call after a large one on the same handle, and stats without rows;
  8. field_cases' floor (rank three) and degcube.

Out of scope: k_scan_totals' loop over more than 256 blocks of the scan starts at n > 131072 particles, which the all-pairs
restatement cannot reach; the resampler tests (tests/test_gpu_resample_edges.py) own that kernel at such sizes.

The last test prints the module's wall time (recorded in profiles/stein_edge_cases.txt)."""
import ctypes as C
import time

import numpy as np
import pytest

import field_cases as fc
import stein_cases as sc
import stein_ref as sr
from test_gpu_stein import _assert_same, _capi_params, _device, _same_stats

pytestmark = pytest.mark.gpu
F = np.float32
PLANAR = sc.PLANAR
_T0 = [None]


def _updater(ra, hm, fd):
    from rmcl_amd import types as T
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.set_field(fd)
    return upd


@pytest.fixture(scope="module")
def world(ra, orc, ctx):
    """per map, made once: (device map, field, info, downloaded lattice, truth [1], Tsb, scan points or None, updater with the field set)"""
    if _T0[0] is None:
        _T0[0] = time.time()
    cache = {}

    def get(name):
        if name not in cache:
            v, f = fc.build_map(name)
            hm = ra.import_hip_map(ctx, v, f)
            if name == "room30k":
                cell, margin = sc.ROOM_CELL, sc.ROOM_MARGIN
                truth, Tsb, cloud = sc.room_scan(orc.Mesh(v, f))
            else:
                (cell, margin), truth, Tsb, cloud = fc.cell_margin(name), None, None, None
            fd = ra.DistanceFieldHip(hm, cell=cell, margin=margin)
            cache[name] = (hm, fd, fd.info(), fd.download(), truth, Tsb, cloud, _updater(ra, hm, fd))
        return cache[name]

    yield get
    for w in cache.values():
        w[7].close()
        w[1].close()


@pytest.fixture(scope="module")
def room(ra, world):
    """room30k with 5 beams set: (info, lattice, truth, Tsb, beams, updater, device map, field)"""
    hm, fd, info, lat, truth, Tsb, cloud, upd = world("room30k")
    beams = ra.sample_beams(cloud, 5, seed=7)
    assert len(beams) == 5

    def get():
        upd.setInput(beams, Tsb)      # (a test that sets other beams on this updater is followed by tests that call this again)
        return info, lat, truth, Tsb, beams, upd, hm, fd

    return get


def _check(ra, ctx, room, poses, p, what):
    """the device against the restatement at these poses and parameters; both results"""
    info, lat, truth, Tsb, beams, upd, _, _ = room()
    ref = sr.step(info, lat, poses, beams, Tsb, p)
    got = _device(ra, ctx, upd, poses, p)
    _assert_same(got, ref, what)
    return got, ref


# ---- 1. tilted clouds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "spread"])
@pytest.mark.parametrize("mask", [0x3F, 0x38, 0x1F])
@pytest.mark.parametrize("iterations", [1, 3])
def test_tilted_clouds_are_the_restatement_byte_for_byte(ra, ctx, world, room, iterations, mask, kind):
    info, lat, truth, Tsb, beams, upd, _, _ = room()
    poses = sc.tilted(truth, kind)
    p = sr.params(iterations=iterations, dof_mask=mask)
    for n in sc.N_TILTED:               # particles are NOT independent: every size is a cloud of its own
        if n == 257 and mask == 0x3F:   # 65 beams: more than a wave's lanes in the drive's pass
            many = ra.sample_beams(world("room30k")[6], 65, seed=7)
            assert len(many) == 65
            upd.setInput(many, Tsb)
            ref = sr.step(info, lat, poses, many, Tsb, p)
            _assert_same(_device(ra, ctx, upd, poses, p), ref, "n = 257, 65 beams")
            upd.setInput(beams, Tsb)
            if kind == "dense" and iterations == 1:
                nb = ref[1]["n_neighbours"]
                assert np.median(nb) >= 16 and nb.max() > 64
        else:
            _check(ra, ctx, room, poses[:n], p, "n = %d" % n)


@pytest.mark.parametrize("iterations", [1, 3])
def test_negated_quaternions_negate_exactly_their_outputs(ra, ctx, room, iterations):
    truth = room()[2]
    poses = sc.tilted(truth, "dense")
    idx = sc.flipped_indices(len(poses))
    flipped = sc.negate_rotations(poses, idx)
    p = sr.params(iterations=iterations)
    plain, _ = _check(ra, ctx, room, poses, p, "plain")
    got, _ = _check(ra, ctx, room, flipped, p, "negated")
    assert got[0].tobytes() == sc.negate_rotations(plain[0], idx).tobytes() and got[0].tobytes() != plain[0].tobytes()
    assert got[1].tobytes() == plain[1].tobytes() and _same_stats(got[2], plain[2])


# ---- 2. many bins across the blocks of the prefix sum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.N_CLUSTERED)
@pytest.mark.parametrize("mask", [0x3F, PLANAR])
@pytest.mark.parametrize("iterations", [1, 2])
def test_bins_in_every_block_of_the_prefix_sum(ra, ctx, room, iterations, mask, n):
    poses = sc.clustered_cloud(room()[2], n)
    p = sr.params(iterations=iterations, dof_mask=mask, max_per_bin=n)
    assert sc.occupied_per_block(poses, p).min() >= 8 and len(sc.occupied_per_block(poses, p)) == {513: 2, 1025: 4}[n]
    got, ref = _check(ra, ctx, room, poses, p, "clustered %d" % n)
    assert ref[2]["n_bins"] >= (sc.N_CLUSTERS if mask == 0x3F else 32) and np.median(ref[1]["n_neighbours"]) >= 4


@pytest.mark.parametrize("n", sc.N_FULL)
@pytest.mark.parametrize("mask", [0x3F, PLANAR])
@pytest.mark.parametrize("iterations", [1, 2])
def test_fullest_tables(ra, ctx, room, iterations, mask, n):
    poses = sc.full_cloud(room()[2], n)
    got, ref = _check(ra, ctx, room, poses, sr.params(iterations=iterations, dof_mask=mask, max_per_bin=n), "full %d" % n)
    if mask == 0x3F and iterations == 1:
        assert 4 * ref[2]["n_bins"] >= 3 * n


# ---- 3. several thinned bins --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("cap", sc.ROW_CAPS)
def test_thinned_bins_beside_unthinned_ones(ra, ctx, room, cap, interleaved):
    poses = sc.row_cloud(room()[2], interleaved)
    p = sc.row_params(cap)
    got, ref = _check(ra, ctx, room, poses, p, "row, cap %d, one iteration" % cap)
    assert ref[2]["n_bins"] == 6 and ref[2]["n_thinned_bins"] == sc.ROW_THINNED[sc.ROW_CAPS.index(cap)] == got[2]["n_thinned_bins"]
    row = sc.row_bins(poses, p)
    assert all(1 <= listed <= count for count, listed in row) and tuple(count for count, _ in row) == sc.ROW_COUNTS
    again = _device(ra, ctx, room()[5], poses, p)              # the same call twice: the same bytes
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and _same_stats(again[2], got[2])
    _check(ra, ctx, room, poses, sc.row_params(cap, iterations=2), "row, cap %d, two iterations" % cap)


def test_unthinned_row_does_not_depend_on_the_order(ra, ctx, room):
    truth = room()[2]
    p = sc.row_params(0xFFFFFFFF, iterations=2)
    a, _ = _check(ra, ctx, room, sc.row_cloud(truth, False), p, "contiguous")
    b, _ = _check(ra, ctx, room, sc.row_cloud(truth, True), p, "interleaved")
    perm = sc.row_permutation()
    assert b[0].tobytes() == a[0][perm].tobytes() and b[1].tobytes() == a[1][perm].tobytes()
    p = sc.row_params(sum(sc.ROW_COUNTS), iterations=2)        # cap = n: as unthinned
    c, _ = _check(ra, ctx, room, sc.row_cloud(truth, True), p, "interleaved, cap = n")
    assert c[0].tobytes() == b[0].tobytes() and c[1].tobytes() == b[1].tobytes()


# ---- 4. the draw's edges ------------------------------------------------------------------------------------------------------------------
def test_key_with_a_high_word_and_a_wrapping_step(ra, ctx, room):
    poses = sc.row_cloud(room()[2])
    p = sc.row_params(64, step=0xFFFFFFFF, iterations=3)
    assert p["seed"] >> 32 != 0
    high, _ = _check(ra, ctx, room, poses, p, "step 0xFFFFFFFF, 3 iterations")
    low, _ = _check(ra, ctx, room, poses, dict(p, seed=p["seed"] & 0xFFFFFFFF), "the key's low word alone")
    assert high[0].tobytes() != low[0].tobytes()
    for iterations, step in ((1, 0xFFFFFFFF), (2, 0xFFFFFFFF), (1, 0), (1, 0xFFFFFFFE)):
        _check(ra, ctx, room, poses, dict(p, iterations=iterations, step=step), "step %#x, %d iterations" % (step, iterations))


# ---- 5. masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", sc.MASKS)
def test_masks(ra, ctx, room, mask):
    poses = sc.tilted(room()[2], "dense")
    got, ref = _check(ra, ctx, room, poses, sc.mask_params(mask), "mask %#04x" % mask)
    if mask in (0x00, 0x38):
        assert got[2]["n_bins"] == 1 and got[2]["n_thinned_bins"] == 1
    if mask == 0x00:                    # nothing moves, the rows are written
        assert got[0].tobytes() == poses.tobytes() and got[1]["n_neighbours"].min() >= 200 and (got[1]["n_used"] > 0).any()


# ---- 6. chosen collisions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0x3F, 0x07])
def test_probe_chain_that_wraps_to_word_zero(ra, ctx, room, mask):
    poses = sc.collision_cloud(room()[2])
    p = sr.params(dof_mask=mask, max_per_bin=len(poses))
    assert {62, 63, 0, 1, 2, 3} <= sr.table_of(poses, p)[1]
    got, ref = _check(ra, ctx, room, poses, p, "collisions")
    # nobody misses its own bin: every clustered particle finds its two companions, every loner nobody
    assert (got[1]["n_neighbours"][:18] >= 2).all() and (got[1]["n_neighbours"][18:] == 0).all() and got[2]["n_bins"] == 12
    _check(ra, ctx, room, poses, dict(p, iterations=2), "collisions, two iterations")


# ---- 7. scratch reuse, stats without rows ----------------------------------------------------------------------------------------------------
def test_small_call_after_a_large_one_on_one_handle(ra, ctx, room):
    info, lat, truth, Tsb, beams, _, hm, fd = room()
    upd = _updater(ra, hm, fd)          # a handle of its own: its scratch is this test's
    upd.setInput(beams, Tsb)
    try:
        big = sc.clustered_cloud(truth, 1025)
        small = sc.tilted(truth, "dense")
        p_big, p = sr.params(iterations=2, max_per_bin=1025), sr.params(iterations=2)
        for poses, q, what in ((big, p_big, "1025"), (small[:5], p, "5 after 1025"), (small[:65], p, "65 after 5"), (big, p_big, "1025 again")):
            _assert_same(_device(ra, ctx, upd, poses, q), sr.step(info, lat, poses, beams, Tsb, q), what)
        # stats without rows (the handle's own rows) against the call with rows: the same stats, the same poses
        L = ra._capi.lib()
        b, tsb = np.ascontiguousarray(beams), np.ascontiguousarray(Tsb)
        for poses, q in ((small[:65], p), (big, p_big), (small[:5], p)):
            with_rows = _device(ra, ctx, upd, poses, q)
            d_poses = ra.DeviceArray.from_host(ctx, poses)
            st = ra._capi.SteinStats()
            params = _capi_params(ra, q)
            assert L.rmclhip_pf_stein_step(upd._h, C.c_void_p(d_poses.ptr), len(poses), b.ctypes.data_as(C.c_void_p), len(b),
                                           tsb.ctypes.data_as(C.c_void_p), C.byref(params), None, C.byref(st)) == ra._capi.OK
            assert _same_stats(st.as_dict(), with_rows[2]) and d_poses.download().tobytes() == with_rows[0].tobytes()
    finally:
        upd.close()


# ---- 8. hard maps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.HARD_MAPS)
@pytest.mark.parametrize("mask", [0x3F, PLANAR])
def test_hard_maps(ra, orc, ctx, world, name, mask):
    """floor: the smallest lambda0 the check accepts too (0 is refused) -- no solve is rejected even then
    (tests/test_stein_cases_cpu.py says why): the drive's `ok == false` path cannot be reached on this map"""
    hm, fd, info, lat, _, _, _, upd = world(name)
    truth, Tsb, beams, poses, kw = sc.hard_case(ra, orc, name)
    upd.setInput(beams, Tsb)
    for lambda0 in (1e-3,) + ((np.nextafter(F(0), F(1)),) if name == "floor" else ()):
        p = sr.params(iterations=2, dof_mask=mask, lambda0=lambda0, **kw)
        ref = sr.step(info, lat, poses, beams, Tsb, p)
        assert ref[2]["n_no_beams"] == 0 and np.median(ref[1]["n_neighbours"]) >= 4 and ref[0].tobytes() != poses.tobytes()
        _assert_same(_device(ra, ctx, upd, poses, p), ref, "%s, lambda0 %g" % (name, lambda0))


def test_zz_wall_time_of_this_module():
    """printed for the record"""
    if _T0[0] is not None:
        print("[stein-edges] wall time of tests/test_gpu_stein_edges.py: %.1f s" % (time.time() - _T0[0]))
