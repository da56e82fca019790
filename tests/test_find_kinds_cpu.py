"""CPU test of the one table of find traversal kinds (rmcl_amd/csrc/find_kinds.h, find_kernel.hip.h find_kind_dev) and of the launch
shape every launcher derives from it (kernels.hip find_launch_shape), through the pure read-out rmclhip_debug_find_launch_shape.

The expectations below RESTATE the formulas the launchers carried one copy each before the table existed -- launch_find,
launch_find_moments, lab_find_kind, rmclhip_debug_wave_clock -- from the constants of traverse.hip.h, so that the table cannot drift
from what those launchers did.  Two cases pin the corrected value where those copies disagreed (see the two comments marked DEFECT).
"""
import ctypes as C
import itertools

import pytest

from conftest import PRODUCT_FIND_KINDS

# traverse.hip.h / layout.h / find_kernel.hip.h
QUAD_STACK_ENTRIES = 1 + 64 + 4
TAIL_RAYS, TAIL_XFER_DWORDS = 16, 12
NODE_DWORDS = 32
DESCENT_WAVE_DWORDS = (64 + 2 * 32) * 8
BF_ROWS = 24

LDS_QUAD = QUAD_STACK_ENTRIES * 64
LDS_TAIL = QUAD_STACK_ENTRIES * 64 + 4 * TAIL_RAYS * TAIL_XFER_DWORDS
LDS_WW = 16 * 256
LDS_BF = BF_ROWS * 256
LDS_WW_TAIL = LDS_WW + LDS_TAIL
LDS_BF_TAIL = LDS_BF + LDS_TAIL
LDS_31 = LDS_BF + 4 * DESCENT_WAVE_DWORDS

# dynamic LDS in dwords, as the `case` lines of lab_find_kind and the branches of launch_find had it
LDS_DWORDS = {0: 0, 1: LDS_BF, 2: LDS_QUAD, 4: LDS_WW, 5: LDS_WW_TAIL, 6: LDS_WW_TAIL + 85 * NODE_DWORDS, 7: LDS_WW_TAIL + 341 * NODE_DWORDS,
              8: LDS_WW_TAIL, 9: LDS_WW_TAIL + 85 * NODE_DWORDS, 10: LDS_WW_TAIL + 341 * NODE_DWORDS, 11: LDS_WW, 12: LDS_BF, 13: LDS_BF,
              14: LDS_BF, 16: LDS_BF_TAIL, 17: LDS_BF_TAIL, 19: LDS_BF_TAIL, 20: LDS_BF_TAIL, 21: LDS_WW_TAIL, 22: LDS_WW, 23: LDS_BF_TAIL,
              24: LDS_WW, 25: LDS_QUAD, 26: LDS_BF_TAIL, 27: LDS_BF_TAIL, 28: LDS_BF_TAIL, 29: LDS_BF_TAIL, 30: LDS_BF_TAIL, 31: LDS_31,
              32: LDS_31}
# launch_find_moments: kinds 23 and 32 stage in their lane stacks, kind 2 appends 21 rows of 256 dwords
LDS_DWORDS_MOMENTS = {2: LDS_QUAD + 21 * 256, 23: LDS_BF_TAIL, 32: LDS_31}
KINDS = sorted(LDS_DWORDS)
QUAD_KINDS = (2, 25)

TILINGS = [(1, 1), (7, 1), (8, 1), (9, 1), (32, 1), (33, 1), (65536, 1), (5, 7)]
NPOSES = (1, 3)
GRANULES = (0, 1, 3, 64)   # 0: world order off


def _round8(n):
    return (n + 7) & ~7


def _shape(L, ra, kind, moments, tx, ty, nposes, n_order, granule):
    out = ra._capi.FindLaunchShape()
    assert L.rmclhip_debug_find_launch_shape(kind, moments, tx, ty, nposes, n_order, granule, C.byref(out)) == 0
    return out


def test_lds_byte_counts_per_kind():
    """dynamic LDS per workgroup in bytes, kind by kind, from the restated constants"""
    by_bytes = {}
    for k, dw in LDS_DWORDS.items():
        by_bytes.setdefault(4 * dw, []).append(k)
    assert by_bytes == {0: [0], 17664: [2, 25], 16384: [4, 11, 22, 24], 24576: [1, 12, 13, 14],
                        45312: [16, 17, 19, 20, 23, 26, 27, 28, 29, 30], 40960: [31, 32], 37120: [5, 8, 21], 48000: [6, 9], 80768: [7, 10]}
    assert 4 * LDS_DWORDS_MOMENTS[2] == 39168


def test_which_numbers_are_kinds_and_which_the_product_builds(ra):
    L = ra._capi.lib()
    exists = [k for k in range(34) if _shape(L, ra, k, 0, 8, 1, 1, 0, 0).exists]
    assert exists == KINDS
    for k in (3, 15, 18, 33, -1, 64):
        s = _shape(L, ra, k, 0, 8, 1, 1, 0, 0)
        assert [getattr(s, f) for f, _ in s._fields_] == [0] * 8, k
    # conftest's list carries the automatic rule's number 15 as well, which is a rule and no kind
    assert [k for k in KINDS if _shape(L, ra, k, 0, 8, 1, 1, 0, 0).in_product] == [k for k in PRODUCT_FIND_KINDS if k != 15]
    assert [k for k in KINDS if _shape(L, ra, k, 0, 8, 1, 1, 0, 0).has_moments] == sorted(LDS_DWORDS_MOMENTS)


@pytest.mark.parametrize("kind", KINDS)
def test_launch_shape_is_what_the_launchers_computed(ra, kind):
    L = ra._capi.lib()
    group = 1 if kind in QUAD_KINDS else 4
    words = 24 if kind in (31, 32) else 8
    for (tx, ty), nposes, granule, moments in itertools.product(TILINGS, NPOSES, GRANULES, (0, 1)):
        ntiles = tx * ty
        ngroups = (ntiles + group - 1) // group
        n_order = ngroups * nposes if granule else 0   # batch_order_enqueue: one entry per workgroup of the pose-major launch
        s = _shape(L, ra, kind, moments, tx, ty, nposes, n_order, granule)
        what = "kind %d moments %d tiles %dx%d poses %d granule %d" % (kind, moments, tx, ty, nposes, granule)
        assert s.exists == 1 and s.tiles_per_block == group, what
        with_epilogue = bool(moments) and kind in LDS_DWORDS_MOMENTS   # asked of a kind without the epilogue: the plain launch
        if with_epilogue:
            # launch_find_moments: dim3(find_moments_blocks(p, variant), 1, 1); k_find ignores the tile order under kMoments
            grid = (_round8(ngroups), 1)
            lds = LDS_DWORDS_MOMENTS[kind]
        else:
            # launch_find / lab_find_kind: dim3(nblocks, nposes, 1), nblocks % 8 == 0 ...
            grid = (_round8(ngroups), nposes)
            if granule:
                # ... and under a world order one row of whole turns of the eight XCDs.  DEFECT 1 (world order with lab kinds): only
                # launch_find made this grid, lab_find_kind kept (nblocks, nposes) and k_find's world-order branch then left most
                # (pose, tile) pairs unwritten -- every kind gets the one-row grid now
                turn = 8 * max(granule, 1)
                grid = ((n_order + turn - 1) // turn * turn, 1)
            lds = LDS_DWORDS[kind]
        assert (s.grid_x, s.grid_y) == grid, what
        assert s.grid_x % 8 == 0, what
        assert s.lds_bytes == 4 * lds, what
        # k_find writes word block [8 | 16 more for the descent kinds] of wave (blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave
        assert s.clock_dwords == s.grid_x * s.grid_y * 4 * words, what
        if nposes == 1 and not granule and not moments:
            # rmclhip_debug_wave_clock: nblocks * 4 * (24 or 8).  DEFECT 2 (clocked launch of kind 25): it took nblocks as ntiles / 4
            # for every kind but 2, while lab_find_kind launches kind 25 with one tile per workgroup and wrote four times the
            # buffer -- the size follows tiles_per_block now
            assert s.clock_dwords == _round8(ngroups) * 4 * words, what


def test_the_order_s_group_is_the_kind_s_tiles_per_block(ra):
    """tests/pose_batch_cases.group_of, the `group` of batch_order_enqueue and the table agree (DEFECT 1: kind 25 had group 4)"""
    import pose_batch_cases as pc
    L = ra._capi.lib()
    for k in KINDS:
        assert _shape(L, ra, k, 0, 8, 1, 1, 0, 0).tiles_per_block == pc.group_of(k), k
