"""The banded distance field without a device (include/rmclhip.h, BANDED DISTANCE FIELD): rmclhip_band_field_layout_host against
the numpy restatement (tests/band_field_ref.py) and its refusals, and the restatement itself against the dense restatement
(tests/field_ref.py) on lattices of the oracle's distances -- a lookup in a STORED brick is the dense lookup to the bit, a lookup in a
FAR brick exceeds the band and is within 4 sqrt(3) cell of the oracle's distance."""
import math

import numpy as np
import pytest

import band_field_ref as bfr
import field_ref as fr

F = np.float32


# ---- 1. the layout -------------------------------------------------------------------------------------------------------------------------
BOXES = {
    "multiple_of_8": ((-2, -2, -2), (2, 2, 2), 0.1, 0.0, 0.05),          # 40 cells per axis
    "ragged": ((-2, -2, -2), (2.25, 2, 1.7), 0.1, 0.0, 0.3),             # 43, 40 and 37 cells
    "thin_axis": ((-3, -3, 0), (3, 3, 0), 0.1, 0.0, 0.05),               # n_z = 2
    "margin": ((-2, -2, -2), (2, 2, 2), 0.1, 0.15, 0.5),
    "automatic_cell": ((0, 0, 0), (30, 20, 3), 0.0, 0.5, 0.5),
    "refused_dense": ((0, 0, 0), (100, 100, 3), 0.05, 0.0, 0.5),         # 2.4e8 logical nodes
}


@pytest.mark.parametrize("name", sorted(BOXES))
def test_layout_is_the_restatement(ra, name):
    lo, hi, cell, margin, band = BOXES[name]
    ref = bfr.layout(lo, hi, cell, margin, band)
    got = ra.band_field_layout(lo, hi, cell=cell, margin=margin, band=band)
    assert bfr.same_layout(ref, got), (ref, got)
    logical, bricks = got
    n, nb = logical["n"], bricks["nb"]
    assert bricks["brick_edge"] == 8 and all(8 * (nb[k] - 1) < n[k] - 1 <= 8 * nb[k] for k in range(3))
    assert bricks["n_stored"] == 0 and bricks["bytes"] == 0 and logical["bytes"] == 0
    assert bricks["reach"] > bricks["band"] + 6.928 * logical["cell"]
    if name == "multiple_of_8":
        assert n == (41, 41, 41) and nb == (5, 5, 5) and not bfr.is_ragged(logical)
    if name == "ragged":
        assert nb == (6, 5, 5) and bfr.is_ragged(logical)
    if name == "thin_axis":
        assert n[2] == 2 and nb[2] == 1
    if name == "automatic_cell":
        assert fr.same_layout(dict(fr.layout(lo, hi, 0.0, margin), bytes=0), logical)
    if name == "refused_dense":
        assert logical["n_nodes"] > 2.3e8
        with pytest.raises(ra.RmclHipError, match="max_nodes"):
            ra.field_layout(lo, hi, cell=cell, margin=margin)
    else:
        # the logical lattice is the dense field's
        assert fr.same_layout(dict(ra.field_layout(lo, hi, cell=cell, margin=margin), bytes=0), logical)


def test_layout_refusals(ra):
    lo, hi = (-2, -2, -2), (2, 2, 2)

    def refused(match, **kw):
        args = dict(cell=0.1, margin=0.0, band=0.5)
        args.update(kw)
        box = (args.pop("lo", lo), args.pop("hi", hi))
        with pytest.raises(ra.RmclHipError, match=match) as e:
            ra.band_field_layout(box[0], box[1], **args)
        assert e.value.status == ra._capi.ERR_INVALID

    for band in (0.0, -0.5, math.nan, math.inf):
        refused("band must be finite and > 0", band=band)
    for cell in (-0.1, math.nan, math.inf):
        refused("cell must be finite", cell=cell)
    for margin in (-0.1, math.nan, math.inf):
        refused("margin must be finite", margin=margin)
    refused("min > max", lo=(2, -2, -2), hi=(-2, 2, 2))
    refused("not finite", hi=(2, math.inf, 2))
    refused("2\\^20 cells on an axis", hi=(600, 2, 2), cell=0.0005)
    # exactly 2^20 cells pass, one more does not
    logical, _ = ra.band_field_layout((0, 0, 0), (2.0 ** 20, 1, 1), cell=1.0, max_nodes=1 << 40)
    assert logical["n"][0] == 2 ** 20 + 1
    refused("2\\^20 cells on an axis", lo=(0, 0, 0), hi=(2.0 ** 20 + 1, 1, 1), cell=1.0, max_nodes=1 << 40)
    # the coarse lattice alone is over the cap: 6^3 = 216 coarse nodes
    assert ra.band_field_layout(lo, hi, cell=0.1, max_nodes=216)[1]["n_coarse"] == 216
    refused("max_nodes", max_nodes=215)


def test_params_default(ra):
    import ctypes as C
    p = ra._capi.BandFieldParams()
    ra._capi.lib().rmclhip_band_field_params_default(C.byref(p))
    assert (p.cell, p.margin, p.max_nodes, p.band, p.reserved) == (0.0, 0.0, 1 << 26, 0.5, 0)


# ---- 2. the restatement against the dense restatement, on the oracle's distances ---------------------------------------------------------
@pytest.fixture(scope="module")
def built(orc):
    """per case, made once: (mesh, logical, bricks, dense lattice of the oracle's distances, the banded arrays cut out of it)"""
    cache = {}

    def get(name):
        if name not in cache:
            v, f, logical, bricks = bfr.case(name)
            mesh = orc.Mesh(v, f)
            lat = fr.oracle_lattice(mesh, logical)
            cache[name] = (mesh, logical, bricks, lat, bfr.build(logical, bricks, lat))
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(bfr.CASES))
def test_cases_have_far_stored_and_ragged_bricks(built, name):
    _, logical, bricks, lat, arrays = built(name)
    table = arrays["table"]
    n_far = int((table == bfr.FAR).sum())
    assert 0 < n_far < table.size and arrays["n_stored"] == table.size - n_far
    assert bfr.is_ragged(logical) == (name in bfr.RAGGED)
    # stored bricks are numbered in brick order
    assert np.array_equal(table.reshape(-1)[table.reshape(-1) != bfr.FAR], np.arange(arrays["n_stored"], dtype=np.uint32))
    if name in bfr.RAGGED:
        assert np.isnan(arrays["bricks"]).any() and not np.isnan(lat).any()       # the padding, and nothing else
    else:
        assert not np.isnan(arrays["bricks"]).any()
    if name == "quad":
        assert logical["n"][2] == 2
    print("[band-field] %-11s n = %s, %d bricks, %d stored, %d bytes banded against %d dense" % (
        name, logical["n"], table.size, arrays["n_stored"], arrays["bytes"], 4 * lat.size))


@pytest.mark.parametrize("name", sorted(bfr.CASES))
def test_stored_is_the_dense_lookup_and_far_exceeds_the_band(built, name):
    mesh, logical, bricks, lat, arrays = built(name)
    pts, kinds = bfr.query_points(logical)
    dense = fr.lookup(logical, lat, pts)
    banded = bfr.lookup(logical, bricks, arrays, pts)
    stored = bfr.stored_mask(logical, bricks, arrays["table"], pts)
    special = kinds == "special"
    assert np.isnan(banded[special]).all() and not np.isnan(banded[~special]).any()
    far = ~stored & ~special
    for kind in ("inside", "face1", "face2", "face3", "outside1", "outside2", "outside3"):
        # (beyond three faces lie the corner bricks of the box, and the quad's are all FAR)
        assert stored[kinds == kind].any() or (name == "quad" and kind == "outside3"), kind
    assert far[kinds == "inside"].any() and far[np.char.startswith(kinds, "face")].any()
    assert banded[stored].tobytes() == dense[stored].tobytes()
    band, cell = float(bricks["band"]), float(logical["cell"])
    assert (banded[far] > band).all() and (dense[far] > band).all()
    # inside the lattice the blend's error is at most sum_c w_c |c - P| <= (sqrt(3) / 2) * 8 cell; rounding: seven lerps and the
    # oracle's own distance, a few ulp of the largest corner value each
    inside = far & ~np.char.startswith(kinds, "outside")
    truth = fr.oracle_distances(mesh, pts[inside])
    tol = 4.0 * math.sqrt(3.0) * cell + 32 * float(np.finfo(F).eps) * float(np.nanmax(arrays["coarse"]))
    err = np.abs(banded[inside].astype(np.float64) - truth)
    print("[band-field] %-11s %d stored and %d far points; far: max |lookup - oracle| = %.4f m of %.4f allowed" % (
        name, stored.sum(), far.sum(), err.max(), tol))
    assert (err <= tol).all()
    # and the dense guarantee wherever the brick is stored
    inside_s = stored & ~np.char.startswith(kinds, "outside")
    err_s = np.abs(banded[inside_s].astype(np.float64) - fr.oracle_distances(mesh, pts[inside_s]))
    assert (err_s <= fr.SQRT3_2 * cell + 32 * float(np.finfo(F).eps) * float(np.nanmax(lat))).all()


def test_exact_brick_faces(built):
    """cube_pow2: u is exact, so a point on a brick face lies on it to the bit -- its cell is the first of the next brick (the last
    of the last brick at the top), and the lookup at a coarse node is that node's value in either kind of brick"""
    _, logical, bricks, lat, arrays = built("cube_pow2")
    n, nb = logical["n"], bricks["nb"]
    c = np.stack(np.meshgrid(*[8 * np.arange(nb[k] + 1) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
    pts = (np.array(logical["origin"], F) + c.astype(F) * logical["cell"]).astype(F)
    got = bfr.lookup(logical, bricks, arrays, pts)
    assert got.tobytes() == lat[c[:, 2], c[:, 1], c[:, 0]].tobytes()
    i = bfr.locate(logical, pts)[0]
    assert np.array_equal(i, np.minimum(c, np.array(n) - 2))
    assert (~bfr.stored_mask(logical, bricks, arrays["table"], pts)).any()
