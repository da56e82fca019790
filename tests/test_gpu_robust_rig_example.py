"""examples/robust_rig_cpp_example.cpp -- a two-sensor rig corrected with M-estimator weights through the C++ adapters -- compiles with
plain g++ against the C ABI (CPU test) and, on a GPU, ends closer to the truth than the plain rig loop it runs beside and prints what
the Python binding computes for the same rig."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "robust_rig_cpp_example.cpp"


def _build(tmp_path):
    exe = str(tmp_path / SOURCE.replace(".cpp", ""))
    libdir = os.path.join(ROOT, "rmcl_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", SOURCE), "-L" + libdir, "-lrmclhip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_example_compiles_and_links_without_gpu(ra, tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_adapter_value_types_keep_the_abi_layout(tmp_path):
    src = tmp_path / "shape.cpp"
    src.write_text(r'''
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
namespace rm = rmcl_hip;
static_assert(std::is_same<rm::PoseInformationRobust, rmclhip_pose_information_robust>::value && sizeof(rm::PoseInformationRobust) == 376, "");
static_assert(std::is_same<decltype(std::declval<const rm::RCCHipSpherical&>().computePoseInformationRobust(std::declval<const rm::Transform&>(), 0.0,
                           std::declval<const rm::RobustParams&>())), rm::PoseInformationRobust>::value, "");
static_assert(std::is_same<decltype(rm::correctOnceRobust(std::declval<const std::vector<rm::CorrespondencesHIP*>&>(), std::declval<const rm::Transform&>(),
                           std::declval<const std::vector<rm::Transform>&>(), std::declval<const std::vector<double>&>(), 3u, 0.0,
                           std::declval<const std::vector<rm::RobustParams>&>())), rm::Transform>::value, "");
static_assert(std::is_same<decltype(rm::poseCovariance(std::declval<const rm::PoseInformationRobust&>())), rm::PoseCovariance>::value, "");
int main() { return 0; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def _write_scan(path, pts, mask):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(pts)))
        fh.write(np.ascontiguousarray(pts, np.float32).tobytes())
        fh.write(np.ascontiguousarray(mask, np.uint8).tobytes())


@pytest.mark.gpu
def test_example_beats_its_plain_loop_and_matches_the_python_binding(ra, orc, ctx, tmp_path):
    from rmcl_amd import synthetic as syn, types as T
    exe = _build(tmp_path)
    s = rc.contaminated_scan(orc)
    v, f = s["map"]
    # the example's own frames (float pi, its truth): the scans are re-made for them, the lidar's with robust_cases.contaminated_scan's recipe
    pi = float(np.float32(np.pi))
    Tsb = [T.transform_from_rpy((0.1, 0.0, 0.3), (0.0, 0.0, 10.0 * pi / 180)), T.transform_from_rpy((-0.2, 0.1, 0.5), (0.0, 0.1, -1.0))]
    truth = T.transform_from_rpy((0.5, -0.3, 0.2), (0.02, -0.03, 0.4))
    est = T.mult(truth, T.transform_from_rpy((0.2, 0.0, 0.0), (0.0, 0.0, 2.0 * pi / 180)))
    lidar = syn.model_c1()
    depth = T.spherical_model(np.float32(-pi / 8), np.float32((pi / 4) / 15), 16, np.float32(-pi / 4), np.float32((pi / 2) / 15), 16,
                              np.float32(0.1), np.float32(100.0))
    scans = []
    for model, mount in zip((lidar, depth), Tsb):
        meas = s["mesh"].simulate_spherical(model, mount, truth, bvh=False)
        scans.append((model, meas["ranges"].astype(np.float32).copy(), np.ascontiguousarray(meas["hits"], np.uint8)))
    short = np.zeros((32, 32), bool)
    short[:, 5:12] = True
    short = short.reshape(-1)
    scans[0][1][short] -= np.random.RandomState(5).uniform(0.3, 0.8, int(short.sum())).astype(np.float32)
    data = [((orc.spherical_directions(m) * r[:, None]).astype(np.float32), h) for m, r, h in scans]
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    _write_scan(tmp_path / "lidar.bin", *data[0])
    _write_scan(tmp_path / "depth.bin", *data[1])
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "lidar.bin"), str(tmp_path / "depth.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    e_plain, e_robust = float(out["plain_error"][0]), float(out["robust_error"][0])
    assert e_robust < e_plain < 0.2
    assert math.isfinite(float(out["plain_cov_trace"][0])) and math.isfinite(float(out["robust_cov_trace"][0]))
    assert 0.0 < float(out["robust_s2"][0]) < float(out["plain_s2"][0])

    hm = ra.import_hip_map(ctx, v, f)
    ops = []
    for (model, _, _), mount, (pts, mask) in zip(scans, Tsb, data):
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(mount)
        rcc.setModel(model)
        rcc.set_dataset(pts, mask)
        rcc.params.max_dist = rcc.adaptive_max_dist_min = 1.0
        ops.append(rcc)
    Tr, merged, _, st = ra.micp_correct_once_robust(ops, T.identity(), np.array([est, est], dtype=T.TRANSFORM), [1.0, 0.37], "tukey", 10, 0.0)
    want = [Tr["t"][k] for k in "xyz"] + [Tr["R"][k] for k in "xyzw"]
    assert [np.float32(x) for x in out["robust"]] == want
    for k in range(2):
        got = out["sensor%d" % k]
        assert int(got[0]) == int(st[k]["stats"]["n_meas"]) and float(got[1]) == float(st[k]["weight_sum"]) and np.float32(got[2]) == st[k]["scale"]
    assert int(out["merged_n_meas"][0]) == int(merged["n_meas"])
