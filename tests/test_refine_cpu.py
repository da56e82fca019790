"""The refinement on the distance field without a device: the numpy restatement (tests/refine_ref.py) on a lattice of exact oracle
distances (room30k, cell 0.25, margin 0.5) -- the gradient against finite differences of the lookup, monotone cost, the fixed point,
the parameter refusals, the locked degrees of freedom, convergence in the set-up of profiles/refine_convergence.txt -- and the C++
example and adapter types."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpc_cases as cc
import field_ref as fr
import refine_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CELL, MARGIN = 0.25, 0.5
PLANAR = 0b100011

# profiles/refine_convergence.txt: the restatement's median end error (m) in the two set-ups below, as recorded there
RECORDED_MEDIAN = {"six": 0.0345, "planar": 0.0242}


@pytest.fixture(scope="module")
def room(ra, orc):
    """made once: (info, oracle lattice, beams, Tsb, truth [1])"""
    v, f = cc.build_map("room30k")
    m = orc.Mesh(v, f)
    info = fr.layout(v.min(0), v.max(0), cell=CELL, margin=MARGIN)
    lat = fr.oracle_lattice(m, info)
    poses, _, beams, Tsb = fr.ranking_case(m, n_particles=fr.RANKING_TRUTH_INDEX + 1, n_beams=64)
    return info, lat, beams, Tsb, poses[fr.RANKING_TRUTH_INDEX:fr.RANKING_TRUTH_INDEX + 1].copy()


@pytest.fixture(scope="module")
def runs(room):
    """the two convergence runs, shared: name -> (starts, refined, rows, stats)"""
    info, lat, beams, Tsb, truth = room
    out = {}
    for name, mask, z in (("six", 0x3F, True), ("planar", PLANAR, False)):
        starts = rr.perturbed_starts(truth, 40, seed=5, z=z)
        out[name] = (starts,) + rr.refine(info, lat, starts, beams, Tsb, rr.params(dof_mask=mask))
    return out


def test_gradient_is_the_finite_difference_of_the_lookup(room):
    info, lat, _, _, _ = room
    i32 = fr.info_f32(info)
    cell, n = float(i32["cell"]), i32["n"]
    rng = np.random.RandomState(3)
    cells = np.stack([rng.randint(0, n[k] - 1, 4000) for k in range(3)], -1)
    frac = rng.uniform(0.3, 0.7, (4000, 3))
    P = (np.array(i32["origin"], np.float64) + (cells + frac) * cell).astype(F)
    d, g, valid = rr.lookup_grad(info, lat, P)
    assert valid.all() and d.tobytes() == fr.lookup(info, lat, P).tobytes()          # d is the existing lookup's value, bit for bit
    h = 0.25 * cell                                                                  # P +- h stays 0.05 cell inside the cell's faces
    # Inside a cell the blend is linear along each axis, so the central difference IS the gradient but for rounding:
    #   - each lookup is 7 lerps of 3 roundings on values <= vmax: <= 21 eps vmax; two of them over 2h: 21 eps vmax / h
    #   - the fractions come from u = (P - origin) * inv_cell <= umax, three roundings: the step 2h / cell is off by <= 6 eps umax,
    #     relative to its 0.5: the slope |g| <= gmax is off by 12 eps umax gmax
    #   - the gradient's own 3 lerps and its product, of corner differences <= 2 vmax: <= 22 eps vmax / cell
    eps, vmax, umax, gmax = 2.0 ** -24, float(np.nanmax(lat)), float(max(n)), float(np.abs(g).max())
    tol = 21 * eps * vmax / h + 12 * eps * umax * gmax + 22 * eps * vmax / cell
    worst = 0.0
    for k in range(3):
        e = np.zeros(3, F)
        e[k] = h
        hi, lo = (P + e).astype(F), (P - e).astype(F)
        step = hi[:, k].astype(np.float64) - lo[:, k].astype(np.float64)
        fd = (fr.lookup(info, lat, hi).astype(np.float64) - fr.lookup(info, lat, lo).astype(np.float64)) / step
        worst = max(worst, float(np.abs(fd - g[:, k]).max()))
    print("max |finite difference - gradient| = %.3g, tolerance %.3g" % (worst, tol))
    assert worst <= tol and gmax > 0.5


def test_invalid_beams(room):
    info, lat, _, _, _ = room
    i32 = fr.info_f32(info)
    inside = np.array(i32["origin"], F) + F(3.3) * i32["cell"]
    pts = np.array([inside, inside - F(10), [np.nan, 0, 0], [np.inf, 0, 0]], F)
    _, _, valid = rr.lookup_grad(info, lat, pts)
    assert valid.tolist() == [True, False, False, False]
    holed = np.array(lat, F)
    holed[3:5, 3:5, 3:5] = np.nan                                      # a NaN corner: d and the gradient are not finite
    assert not rr.lookup_grad(info, holed, pts[:1])[2][0]


def test_cost_never_rises_and_counts_add_up(runs):
    for name, (starts, out, rows, st) in runs.items():
        assert np.all(rows["cost_after"] <= rows["cost_before"]), name
        assert st["n_particles"] == 40 and st["n_moved"] == int((rows["accepted"] > 0).sum()) and st["n_no_beams"] == st["n_not_finite"] == 0
        assert np.all(rows["accepted"] <= 8) and np.all(rows["n_used"] <= 64)
        still = rows["accepted"] == 0
        assert out[still].tobytes() == starts[still].tobytes()


def test_a_start_at_the_truth_moves_less_than_a_cell(room):
    info, lat, beams, Tsb, truth = room
    out, rows, _ = rr.refine(info, lat, truth, beams, Tsb)
    moved = float(rr.position_error(out, truth)[0])
    print("a start at the truth moves %.4f m (cell %.2f)" % (moved, CELL))
    assert moved < CELL and rows["cost_after"][0] <= rows["cost_before"][0]


def test_convergence(room, runs):
    info, lat, beams, Tsb, truth = room
    for name, (starts, out, rows, st) in runs.items():
        e0, e1 = rr.position_error(starts, truth), rr.position_error(out, truth)
        print("%s: median position error %.4f -> %.4f m, worst end error %.4f m, cost fell for %d of %d" %
              (name, np.median(e0), np.median(e1), e1.max(), int((rows["cost_after"] < rows["cost_before"]).sum()), len(e0)))
        assert np.median(e1) <= 2.0 * RECORDED_MEDIAN[name]
        assert np.all(e1 <= e0), "a particle ended farther from the truth than it started"


def test_untouched_cases(room):
    info, lat, beams, Tsb, truth = room
    starts = rr.perturbed_starts(truth, 6, seed=9)
    starts[2]["t"]["y"] = np.nan
    starts[3]["R"]["w"] = np.inf
    starts[4]["t"]["x"] = 500.0                                        # every end point outside the lattice
    for p in (rr.params(iterations=0), rr.params(dof_mask=0)):
        out, rows, st = rr.refine(info, lat, starts, beams, Tsb, p)
        assert out.tobytes() == starts.tobytes() and np.all(rows["accepted"] == 0) and st["n_moved"] == 0
        assert rows["cost_before"].tobytes() == rows["cost_after"].tobytes()
    out, rows, st = rr.refine(info, lat, starts, beams, Tsb)
    assert out[2:5].tobytes() == starts[2:5].tobytes() and st["n_not_finite"] == 2 and st["n_no_beams"] == 1 and st["n_moved"] == 3
    assert np.all(rows["n_used"][2:5] == 0) and np.all(rows["cost_before"][2:5] == F(64 * 0.25))
    # a beam with a NaN range is not used: the count drops by one, the cost carries its max_dist^2
    bad = beams.copy()
    bad["range"][11] = np.nan
    r_good = rr.refine(info, lat, truth, beams, Tsb, rr.params(iterations=0))[1]
    r_bad = rr.refine(info, lat, truth, bad, Tsb, rr.params(iterations=0))[1]
    assert r_good["n_used"][0] == 64 and r_bad["n_used"][0] == 63 and r_bad["cost_before"][0] > r_good["cost_before"][0]


def test_locked_degrees_of_freedom(room):
    info, lat, beams, Tsb, truth = room
    starts = rr.perturbed_starts(truth, 12, seed=11, z=False)          # yaw-only orientations: q.x == q.y == 0
    assert np.all(starts["R"]["x"] == 0) and np.all(starts["R"]["y"] == 0)
    out, rows, _ = rr.refine(info, lat, starts, beams, Tsb, rr.params(dof_mask=PLANAR))
    assert (rows["accepted"] > 0).all()
    assert out["t"]["z"].tobytes() == starts["t"]["z"].tobytes() and np.all(out["R"]["x"] == 0) and np.all(out["R"]["y"] == 0)
    out, rows, _ = rr.refine(info, lat, starts, beams, Tsb, rr.params(dof_mask=0b000111))
    assert (rows["accepted"] > 0).any() and out["R"].tobytes() == starts["R"].tobytes() and out["t"].tobytes() != starts["t"].tobytes()
    out, rows, _ = rr.refine(info, lat, starts, beams, Tsb, rr.params(dof_mask=0b111000))
    assert (rows["accepted"] > 0).any() and out["t"].tobytes() == starts["t"].tobytes() and out["R"].tobytes() != starts["R"].tobytes()
    out, rows, _ = rr.refine(info, lat, starts, beams, Tsb, rr.params(dof_mask=0b000100))
    assert out["t"]["x"].tobytes() == starts["t"]["x"].tobytes() and out["t"]["y"].tobytes() == starts["t"]["y"].tobytes()


def test_step_limits_bind(room):
    info, lat, beams, Tsb, truth = room
    starts = rr.perturbed_starts(truth, 12, seed=13)
    p = rr.params(iterations=4, max_step_trans=1e-3, max_step_rot=1e-3)
    out, rows, _ = rr.refine(info, lat, starts, beams, Tsb, p)
    _, t0 = rr.pose_arrays(starts)
    _, t1 = rr.pose_arrays(out)
    moved = np.sqrt(((t1.astype(np.float64) - t0) ** 2).sum(axis=1))
    # every accepted step is at most max_step_trans long in double, rounded to float32 per axis at |t| < 16: 3 ulp(16) = 6e-6 each
    assert (rows["accepted"] > 0).any() and np.all(moved <= rows["accepted"] * (1e-3 * (1 + 1e-6) + 6e-6))


def test_defaults_and_refusals(ra):
    p = ra._capi.RefineParams(1, 2, 3.0, 4.0, 5.0, 6.0)
    ra._capi.lib().rmclhip_refine_params_default(C.byref(p))
    ref = rr.params()
    assert (p.iterations, p.dof_mask) == (ref["iterations"], ref["dof_mask"]) == (8, 0x3F)
    assert np.array([p.max_dist, p.max_step_trans, p.max_step_rot, p.lambda0], F).tobytes() == \
        np.array([ref["max_dist"], ref["max_step_trans"], ref["max_step_rot"], ref["lambda0"]], F).tobytes() == \
        np.array([0.5, 0.5, 0.25, 1e-3], F).tobytes()
    assert C.sizeof(ra._capi.RefineParams) == 24 and C.sizeof(ra._capi.RefineStats) == 32 and rr.RESULT.itemsize == 16
    assert ra.field.REFINE_RESULT == rr.RESULT
    q = ra.refine_params(iterations=3, max_dist=0.25)
    assert (q.iterations, q.dof_mask, q.max_dist, q.lambda0) == (3, 0x3F, 0.25, F(1e-3))
    rr.check(rr.params(), 5, 1)
    rr.check(rr.params(iterations=64, dof_mask=0), 5, rr.MAX_BEAMS)
    rr.check(rr.params(), 0, 0)                                        # no particles: nothing is asked of the beams
    for bad in rr.BAD_PARAMS:
        with pytest.raises(ValueError):
            rr.check(rr.params(**bad), 5, 8)
    for n_beams in (0, rr.MAX_BEAMS + 1):
        with pytest.raises(ValueError):
            rr.check(rr.params(), 5, n_beams)
    # without a handle the library refuses before it reads anything else
    L, E = ra._capi.lib(), ra._capi.ERR_INVALID
    assert L.rmclhip_field_refine(None, None, 0, None, 0, None, None, None, None) == E
    assert L.rmclhip_pf_refine(None, None, 0, None, 0, None, None, None, None) == E
    assert L.rmclhip_pf_sharded_refine(None, None, 0, None, None, None) == E


def test_example_compiles_and_links_without_gpu(ra, tmp_path):
    r = subprocess.run([rr.build_example(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_adapter_types(tmp_path):
    src = tmp_path / "shape.cpp"
    src.write_text(r'''
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
namespace rm = rmcl_hip;
static_assert(sizeof(rmclhip_refine_params) == 24 && sizeof(rmclhip_refine_result) == 16 && sizeof(rmclhip_refine_stats) == 32, "");
static_assert(std::is_base_of<rmclhip_refine_params, rm::RefineParams>::value, "");
static_assert(std::is_base_of<rm::DeviceView<rm::Transform>, rm::MemoryView<rm::Transform, rm::VRAM_HIP>>::value, "");
static_assert(std::is_same<decltype(std::declval<const rm::DistanceFieldHip&>().refine(std::declval<rm::MemoryView<rm::Transform, rm::VRAM_HIP>>(),
                                    std::declval<const std::vector<rm::RangeMeasurement>&>(), std::declval<const rm::Transform&>())),
                           rm::RefineStats>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::PCDSensorUpdaterHip&>().refine(std::declval<rm::MemoryView<rm::Transform, rm::VRAM_HIP>>())),
                           rm::RefineStats>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::PCDSensorUpdaterHipSharded&>().refine(std::declval<const std::vector<rm::RangeMeasurement>&>(),
                                    std::declval<const rm::Transform&>())), rm::RefineStats>::value, "");
int main() {
  rm::RefineParams p;
  return (p.iterations == 8u && p.dof_mask == 0x3Fu && p.max_dist == 0.5f && p.max_step_trans == 0.5f && p.max_step_rot == 0.25f) ? 0 : 1;
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
