"""The distance field without a device: rmclhip_field_layout_host against its numpy restatement (tests/field_ref.py), every refusal
the host can make, the lookup's error bounds on a lattice of exact oracle distances, the premise of the GPU ranking test, and the C++
example and adapter types."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpc_cases as cc
import field_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bbox(name):
    v, _ = cc.build_map(name)
    v = np.asarray(v, F).reshape(-1, 3)
    return v.min(0), v.max(0)


@pytest.mark.parametrize("cell", [0.0, 0.25])
@pytest.mark.parametrize("margin", [0.0, 0.7])
@pytest.mark.parametrize("name", ["cube", "floor", "farcube", "tri1"])
def test_layout_host_equals_the_numpy_restatement(ra, name, margin, cell):
    lo, hi = _bbox(name)
    got = ra.field_layout(lo, hi, cell=cell, margin=margin, max_nodes=1 << 40)
    ref = fr.layout(lo, hi, cell=cell, margin=margin)
    assert fr.same_layout(ref, got), (ref, got)
    assert all(n >= 2 for n in got["n"]) and got["n_nodes"] == got["n"][0] * got["n"][1] * got["n"][2] and got["bytes"] == 4 * got["n_nodes"]
    if name == "floor" and margin == 0.0:
        assert hi[2] == lo[2] and got["n"][2] == 2              # extent 0 on z
    if name == "farcube":
        assert abs(got["origin"][0]) > 4000.0                   # 5 km from the origin
    if cell:
        assert got["cell"] == F(cell) and got["inv_cell"] == F(1.0) / F(cell)
        # the lattice covers the box plus its margin
        top = np.array(got["origin"], np.float64) + (np.array(got["n"]) - 1) * float(got["cell"])
        assert np.all(top >= hi.astype(np.float64) + margin - 1e-3)


def test_defaults(ra):
    p = ra._capi.FieldParams(1.0, 2.0, 3)
    ra._capi.lib().rmclhip_field_params_default(C.byref(p))
    assert (p.cell, p.margin, p.max_nodes) == (0.0, 0.0, 1 << 26)
    assert C.sizeof(ra._capi.FieldParams) == 16 and C.sizeof(ra._capi.FieldInfo) == 48
    lo, hi = _bbox("cube")
    info = ra._capi.FieldInfo()
    three = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(C.c_void_p)
    assert ra._capi.lib().rmclhip_field_layout_host(three(lo), three(hi), None, C.byref(info)) == ra._capi.OK      # NULL: the defaults
    assert fr.same_layout(fr.layout(lo, hi), info.as_dict())


def test_refusals_on_the_host(ra):
    L, E = ra._capi.lib(), ra._capi.ERR_INVALID
    lo, hi = _bbox("cube")
    for bad in (dict(cell=-0.1), dict(cell=float("nan")), dict(cell=float("inf")), dict(margin=-1.0), dict(margin=float("nan")),
                dict(margin=float("inf"))):
        with pytest.raises(ra.RmclHipError) as e:
            ra.field_layout(lo, hi, **bad)
        assert e.value.status == E, bad
    # a lattice of more than max_nodes nodes: one node too few is refused, the exact count is accepted
    n_nodes = ra.field_layout(lo, hi, cell=0.25)["n_nodes"]
    assert ra.field_layout(lo, hi, cell=0.25, max_nodes=n_nodes)["n_nodes"] == n_nodes
    for kw in (dict(cell=0.25, max_nodes=n_nodes - 1), dict(cell=1e-6), dict(cell=1e-30), dict(cell=1e-30, max_nodes=(1 << 64) - 1),
               dict(cell=0.25, max_nodes=0)):
        with pytest.raises(ra.RmclHipError) as e:
            ra.field_layout(lo, hi, **kw)
        assert e.value.status == E and "max_nodes" in str(e.value), kw
    # a box that is no box
    for blo, bhi in ((hi, lo), ((0, 0, np.nan), (1, 1, 1)), ((0, 0, 0), (1, np.inf, 1)), ((-3e38, 0, 0), (3e38, 1, 1))):
        with pytest.raises(ra.RmclHipError) as e:
            ra.field_layout(blo, bhi, cell=0.25)
        assert e.value.status == E
    # null pointers; the info is zeroed by a refused call
    info = ra._capi.FieldInfo()
    info.n_nodes = 7
    three = np.zeros(3, F).ctypes.data_as(C.c_void_p)
    assert L.rmclhip_field_layout_host(None, three, None, C.byref(info)) == E
    assert L.rmclhip_field_layout_host(three, None, None, C.byref(info)) == E
    assert L.rmclhip_field_layout_host(three, three, None, None) == E
    p = ra._capi.FieldParams(-1.0, 0.0, 1 << 26)
    assert L.rmclhip_field_layout_host(three, three, C.byref(p), C.byref(info)) == E and info.n_nodes == 0
    out = C.c_void_p(1)
    assert L.rmclhip_field_create(None, None, None, C.byref(out)) == E and not out.value
    assert L.rmclhip_field_create(None, None, None, None) == E
    assert L.rmclhip_field_get_info(None, C.byref(info)) == E
    assert L.rmclhip_field_download(None, three, 3) == E
    assert L.rmclhip_field_device_view(None, C.byref(out)) == E
    assert L.rmclhip_field_query(None, three, 1, 0, three) == E
    assert L.rmclhip_pf_set_field(None, None) == E
    assert L.rmclhip_pf_sharded_set_field(None, None) == E
    L.rmclhip_field_destroy(None)                                   # a no-op


@pytest.fixture(scope="module")
def cube_lattice(orc):
    """the cube's lattice (cell 0.25, margin 0.5) of exact oracle distances, computed once"""
    v, f = cc.build_map("cube")
    m = orc.Mesh(v, f)
    info = fr.layout(v.min(0), v.max(0), cell=0.25, margin=0.5)
    return m, info, fr.oracle_lattice(m, info, bvh=True)


def test_lookup_at_the_nodes_is_the_node_value(cube_lattice):
    m, info, lat = cube_lattice
    pos = fr.node_positions(info).reshape(-1, 3)
    sel = np.random.RandomState(3).permutation(len(pos))[:4000]
    # a node's u is its index up to rounding: the blend's weight on the node is 1 to a few ulp
    assert np.allclose(fr.lookup(info, lat, pos[sel]), lat.reshape(-1)[sel], rtol=0, atol=float(info["cell"]) * 1e-4)


def test_bound_inside_the_lattice(cube_lattice):
    """|lookup - d(P)| <= (sqrt(3) / 2) cell at 2 000 seeded points inside the cube's lattice (+ the float32 rounding of distances of
    up to 9 m: 1e-5 relative)"""
    m, info, lat = cube_lattice
    rng = np.random.RandomState(11)
    lo = np.array(info["origin"], np.float64)
    hi = lo + (np.array(info["n"]) - 1) * float(info["cell"])
    pts = rng.uniform(lo + 1e-3, hi - 1e-3, (2000, 3)).astype(F)
    got = fr.lookup(info, lat, pts).astype(np.float64)
    exact = fr.oracle_distances(m, pts).astype(np.float64)
    err = np.abs(got - exact)
    assert np.all(err <= fr.SQRT3_2 * float(info["cell"]) + 1e-5 * exact + 1e-6), err.max()
    assert err.max() > 1e-3          # ... and the test is not vacuous: the blend does differ from the distance near the walls' edges


def test_lower_bound_outside_the_lattice(cube_lattice):
    """outside, the lookup never reports less than d(P) - (sqrt(3) / 2) cell, and at most twice the distance to the lattice's box more"""
    m, info, lat = cube_lattice
    rng = np.random.RandomState(12)
    lo = np.array(info["origin"], np.float64)
    hi = lo + (np.array(info["n"]) - 1) * float(info["cell"])
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pts = centre + rng.uniform(-3.0, 3.0, (4000, 3)) * half
    outside = ((pts < lo) | (pts > hi)).any(axis=1)
    pts = pts[outside][:500].astype(F)
    assert len(pts) == 500
    got = fr.lookup(info, lat, pts).astype(np.float64)
    exact = fr.oracle_distances(m, pts).astype(np.float64)
    slack = fr.SQRT3_2 * float(info["cell"]) + 1e-5 * exact + 1e-5
    assert np.all(got >= exact - slack), (exact - got).max()
    to_box = np.linalg.norm(np.maximum(np.maximum(lo - pts, pts - hi), 0.0), axis=1)
    assert np.all(got <= exact + 2.0 * to_box + slack), (got - exact - 2.0 * to_box).max()
    assert (to_box > 1.0).sum() > 100


def test_lookup_of_special_points(cube_lattice):
    m, info, lat = cube_lattice
    pts = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e38, 0, 0], [0, -1e38, 1e38], [1e6, 0, 0]], F)
    got = fr.lookup(info, lat, pts)
    assert np.isnan(got[:3]).all() and np.isinf(got[3]) and np.isinf(got[4]) and got[3] > 0
    assert abs(float(got[5]) - (1e6 - 5.0)) < 1.0


def test_premise_of_the_ranking_test(ra, orc):
    """tests/test_gpu_field.py ranks 400 particles in room30k by the likelihood of one update: the particle at the truth must come
    first with exact closest-point errors and with the lookup (cell 0.1) -- here with the oracle's errors and with field_ref.lookup on
    the oracle's distances at the nodes the beams' end points touch"""
    v, f = cc.build_map("room30k")
    m = orc.Mesh(v, f)
    poses, attrs, beams, Tsb = fr.ranking_case(m)
    assert len(poses) == 400 and len(beams) == 32
    exact_attrs = attrs.copy()
    e_exact = m.pf_update(poses, exact_attrs, beams, Tsb, orc.pf_params(correspondence_type=1), bvh=True, nthreads=8, want_errors=True)
    mean_exact = exact_attrs["likelihood"]["mean"]
    assert int(np.argmax(mean_exact)) == fr.RANKING_TRUTH_INDEX
    assert e_exact[fr.RANKING_TRUTH_INDEX].max() < 1e-3              # the truth's beams end on the surface
    info = fr.layout(v.min(0), v.max(0), cell=fr.RANKING_CELL)
    ends = fr.end_points(poses, Tsb, beams)
    lat = fr.sparse_oracle_lattice(m, info, ends.reshape(-1, 3))
    e_field = fr.lookup(info, lat, ends.reshape(-1, 3)).reshape(len(poses), len(beams))
    assert not np.isnan(e_field).any()
    inside = (np.abs(ends) < 9.9).all(axis=2) & (ends[:, :, 2] > 0.0) & (ends[:, :, 2] < 5.9)
    assert np.all(np.abs(e_field - e_exact)[inside] <= fr.SQRT3_2 * float(info["cell"]) + 1e-4)
    p = orc.pf_params(correspondence_type=1)
    mean_field, _, n_meas = fr.chain(attrs, e_field, p.dist_sigma, p.max_n_meas)
    assert int(np.argmax(mean_field)) == fr.RANKING_TRUTH_INDEX and np.all(n_meas == attrs["likelihood"]["n_meas"] + len(beams))
    # the truth leads by more than twice what the two modes differ by anywhere: the lookup's error cannot change who comes first
    second = np.sort(mean_field)[-2]
    assert mean_field[fr.RANKING_TRUTH_INDEX] - second > 2 * np.abs(mean_field - mean_exact).max()


def test_example_compiles_and_links_without_gpu(ra, tmp_path):
    r = subprocess.run([fr.build_example(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_adapter_types(tmp_path):
    src = tmp_path / "shape.cpp"
    src.write_text(r'''
#include <optional>
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
namespace rm = rmcl_hip;
static_assert(sizeof(rmclhip_field_params) == 16 && sizeof(rmclhip_field_info) == 48, "");
static_assert(std::is_base_of<rmclhip_field_params, rm::FieldParams>::value, "");
static_assert(!std::is_copy_constructible<rm::DistanceFieldHip>::value, "shared through DistanceFieldHipPtr");
static_assert(std::is_same<rm::DistanceFieldHipPtr, std::shared_ptr<rm::DistanceFieldHip>>::value, "");
static_assert(std::is_same<decltype(std::declval<const rm::DistanceFieldHip&>().info()), rmclhip_field_info>::value, "");
static_assert(std::is_same<decltype(std::declval<const rm::DistanceFieldHip&>().query(std::declval<const std::vector<rm::Vector>&>())),
                           std::vector<float>>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::PCDSensorUpdaterHip&>().setField(std::declval<rm::DistanceFieldHipPtr>())), void>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::PCDSensorUpdaterHipSharded&>().setField(std::declval<std::optional<rm::FieldParams>>())),
                           void>::value, "");
int main() { rm::FieldParams p; return (p.cell == 0.0f && p.margin == 0.0f && p.max_nodes == (1ull << 26)) ? 0 : 1; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
