"""The Stein variational step without a device: the numpy restatement (tests/stein_ref.py) on a lattice of exact oracle distances
(room30k, cell 0.25, margin 0.5) -- the cell list against the sum over all pairs, permutations, particles out of each other's reach,
locked degrees of freedom, identical particles, the parameter refusals, and the premises of the thinned case the device test uses."""
import numpy as np
import pytest

import cpc_cases as cc
import field_ref as fr
import refine_ref as rr
import stein_ref as sr

F = np.float32
D = np.float64
CELL, MARGIN = 0.25, 0.5
PLANAR = 0b100011


@pytest.fixture(scope="module")
def room(ra, orc):
    """made once: (info, oracle lattice, beams, Tsb, truth [1])"""
    v, f = cc.build_map("room30k")
    m = orc.Mesh(v, f)
    info = fr.layout(v.min(0), v.max(0), cell=CELL, margin=MARGIN)
    lat = fr.oracle_lattice(m, info)
    poses, _, beams, Tsb = fr.ranking_case(m, n_particles=fr.RANKING_TRUTH_INDEX + 1, n_beams=64)
    return info, lat, beams, Tsb, poses[fr.RANKING_TRUTH_INDEX:fr.RANKING_TRUTH_INDEX + 1].copy()


def _clouds(truth):
    return {"dense": rr.perturbed_starts(truth, 257, seed=17), "spread": sr.spread_cloud(truth, 257, seed=18)}


@pytest.mark.parametrize("cloud", ["dense", "spread"])
@pytest.mark.parametrize("mask", [0x3F, PLANAR])
def test_cell_list_equals_the_sum_over_all_pairs(room, cloud, mask):
    info, lat, beams, Tsb, truth = room
    poses = _clouds(truth)[cloud]
    p = sr.params(iterations=2, dof_mask=mask, max_per_bin=257)
    binned = sr.step(info, lat, poses, beams, Tsb, p)
    brute = sr.step(info, lat, poses, beams, Tsb, p, brute=True)
    assert binned[0].tobytes() == brute[0].tobytes() and binned[1].tobytes() == brute[1].tobytes()
    assert binned[2] == brute[2] and binned[2]["n_thinned_bins"] == 0
    nb = binned[1]["n_neighbours"]
    print("%s, mask %#x: %d bins, neighbours min %d median %d max %d" % (cloud, mask, binned[2]["n_bins"], nb.min(), np.median(nb), nb.max()))
    # the dense cloud has neighbours everywhere, the spread one has particles with none and particles with some
    assert (nb.min() >= 1 and np.median(nb) > 64 and binned[2]["n_bins"] > 1) if cloud == "dense" else (nb.min() == 0 and nb.max() > 0 and binned[2]["n_bins"] > 100)
    assert binned[0].tobytes() != poses.tobytes()


def test_permuting_the_cloud_permutes_the_result(room):
    info, lat, beams, Tsb, truth = room
    poses = _clouds(truth)["dense"]
    perm = np.random.RandomState(5).permutation(len(poses))
    p = sr.params(iterations=2, max_per_bin=257)
    a = sr.step(info, lat, poses, beams, Tsb, p)
    b = sr.step(info, lat, poses[perm], beams, Tsb, p)
    assert b[0].tobytes() == a[0][perm].tobytes() and b[1].tobytes() == a[1][perm].tobytes()


def test_particles_out_of_reach_move_by_their_own_quantised_drive(room):
    info, lat, beams, Tsb, truth = room
    poses = rr.perturbed_starts(truth, 27, seed=3, d_trans=0.05)
    grid = np.array([(x, y, z) for x in (-0.6, 0.0, 0.6) for y in (-0.6, 0.0, 0.6) for z in (-0.3, 0.0, 0.3)])       # > h_trans = 0.25 apart
    for i, k in enumerate("xyz"):
        poses["t"][k] = (poses["t"][k].astype(D) + grid[:, i]).astype(F)
    p = sr.params()
    out, rows, st = sr.step(info, lat, poses, beams, Tsb, p)
    assert np.all(rows["n_neighbours"] == 0) and np.all(rows["kernel_weight"] == 1.0) and st["n_bins"] == 27
    R, t = rr.pose_arrays(poses)
    drive, _, n_used = sr.drives(info, lat, R, t, np.ones(27, bool), Tsb, beams, p)
    assert (n_used > 0).sum() > 20 and np.abs(drive).max() > 1e-3
    phi = sr.quantise(drive, np.ones(drive.shape, bool)).astype(D) / 4294967296.0
    R2, t2 = rr.candidate(R, t, sr.limit(phi, p), 0x3F)
    Ro, to = rr.pose_arrays(out)
    assert Ro.tobytes() == R2.tobytes() and to.tobytes() == t2.tobytes()


def test_locked_degrees_of_freedom_do_not_move(room):
    info, lat, beams, Tsb, truth = room
    poses = rr.perturbed_starts(truth, 65, seed=19, z=False)        # yaw-only poses
    out, rows, _ = sr.step(info, lat, poses, beams, Tsb, sr.params(iterations=3, dof_mask=PLANAR))
    assert out["t"]["z"].tobytes() == poses["t"]["z"].tobytes() and np.all(out["R"]["x"] == 0) and np.all(out["R"]["y"] == 0)
    assert (out["t"]["x"] != poses["t"]["x"]).sum() > 50 and (out["R"]["z"] != poses["R"]["z"]).sum() > 50
    # dof_mask 0: nothing moves
    out, rows, _ = sr.step(info, lat, poses, beams, Tsb, sr.params(dof_mask=0))
    assert out.tobytes() == poses.tobytes()


def test_identical_particles_stay_identical_without_repulsion(room):
    info, lat, beams, Tsb, truth = room
    poses = np.repeat(rr.perturbed_starts(truth, 1, seed=23), 33)
    out, rows, _ = sr.step(info, lat, poses, beams, Tsb, sr.params(iterations=3, repulsion=0.0))
    assert out.tobytes() == np.repeat(out[:1], 33).tobytes() and out[:1].tobytes() != poses[:1].tobytes()
    assert np.all(rows["n_neighbours"] == 32) and np.all(rows["kernel_weight"] == 33.0)


def test_every_refusal(room):
    for bad in sr.BAD_PARAMS:
        with pytest.raises(ValueError):
            sr.check(sr.params(**bad), 5, 9)
    for n, nb in ((sr.MAX_PARTICLES + 1, 9), (5, 0), (5, rr.MAX_BEAMS + 1)):
        with pytest.raises(ValueError):
            sr.check(sr.params(), n, nb)
    sr.check(sr.params(), sr.MAX_PARTICLES, rr.MAX_BEAMS)
    sr.check(sr.params(max_step_trans=16.0, max_step_rot=16.0, repulsion=0.0, max_per_bin=1), 0, 0)


def test_thinned_case_premises(room):
    """1025 particles in one bin, max_per_bin 64: the thinning lists between 32 and 128 of them, and no particle is close to a bin edge"""
    info, lat, beams, Tsb, truth = room
    p = sr.params(max_per_bin=sr.THINNED_MAX_PER_BIN, seed=sr.THINNED_SEED, step=sr.THINNED_STEP)
    poses = sr.thinned_cloud(truth, p)
    assert len(poses) == sr.THINNED_N == 1025
    assert sr.bin_margin(poses, p) >= 0.05
    R, t = rr.pose_arrays(poses)
    assert len(np.unique(sr.bins(t, p), axis=0)) == 1
    listed = int(sr.listed_of(poses, p).sum())
    print("listed %d of %d" % (listed, len(poses)))
    assert 32 <= listed <= 128
    out, rows, st = sr.step(info, lat, poses, beams, Tsb, p)
    assert st["n_bins"] == 1 and st["n_thinned_bins"] == 1 and out.tobytes() != poses.tobytes()


def test_params_structs_and_null_handle(ra):
    import ctypes as C
    p = ra.stein_params()
    ref = sr.params()
    assert (p.iterations, p.dof_mask, p.max_per_bin, p.seed, p.step) == (1, 0x3F, 256, 0, 0)
    assert np.array([p.max_dist, p.max_step_trans, p.max_step_rot, p.lambda0, p.h_trans, p.h_rot, p.repulsion], F).tobytes() == \
        np.array([ref[k] for k in ("max_dist", "max_step_trans", "max_step_rot", "lambda0", "h_trans", "h_rot", "repulsion")], F).tobytes() == \
        np.array([0.5, 0.5, 0.25, 1e-3, 0.25, 0.2, 0.25], F).tobytes()
    assert C.sizeof(ra._capi.SteinParams) == 56 and C.sizeof(ra._capi.SteinStats) == 32 and sr.RESULT.itemsize == 16
    assert ra.field.STEIN_RESULT == sr.RESULT
    q = ra.stein_params(iterations=3, h_trans=0.5, seed=(1 << 40) + 5, step=9)
    assert (q.iterations, q.h_trans, q.h_rot, q.seed, q.step) == (3, 0.5, F(0.2), (1 << 40) + 5, 9)
    # without a handle the library refuses before it reads anything else
    assert ra._capi.lib().rmclhip_pf_stein_step(None, None, 0, None, 0, None, None, None, None) == ra._capi.ERR_INVALID


def test_example_compiles_and_links_without_gpu(ra, tmp_path):
    import subprocess
    r = subprocess.run([sr.build_example(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_adapter_types(tmp_path):
    import os
    import subprocess
    src = tmp_path / "shape.cpp"
    src.write_text(r'''
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
namespace rm = rmcl_hip;
static_assert(sizeof(rmclhip_stein_params) == 56 && sizeof(rmclhip_stein_result) == 16 && sizeof(rmclhip_stein_stats) == 32, "");
static_assert(std::is_base_of<rmclhip_stein_params, rm::SteinParams>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::PCDSensorUpdaterHip&>().steinStep(std::declval<rm::MemoryView<rm::Transform, rm::VRAM_HIP>>())),
                           rm::SteinStats>::value, "");
int main() {
  rm::SteinParams p;
  return (p.iterations == 1u && p.dof_mask == 0x3Fu && p.h_trans == 0.25f && p.h_rot == 0.2f && p.repulsion == 0.25f && p.max_per_bin == 256u) ? 0 : 1;
}
''')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(root, "include"), str(src)])
