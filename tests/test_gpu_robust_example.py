"""examples/robust_micp_cpp_example.cpp -- one sensor's correction with M-estimator weights through the C++ adapters -- compiles with
plain g++ against the C ABI (CPU test) and, on a GPU, prints what the Python binding computes for the same scan."""
import os
import struct
import subprocess

import numpy as np
import pytest

import robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "robust_micp_cpp_example.cpp"


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
static_assert(std::is_same<rm::RobustStatistics, rmclhip_robust_statistics>::value && sizeof(rm::RobustStatistics) == 96, "");
static_assert(std::is_base_of<rmclhip_robust_params, rm::RobustParams>::value && sizeof(rm::RobustParams) == 24, "");
static_assert(std::is_same<decltype(std::declval<const rm::RCCHipSpherical&>().computeRobustStatistics(std::declval<const rm::Transform&>(), 0.0,
                           std::declval<const rm::RobustParams&>())), rm::RobustStatistics>::value, "");
static_assert(std::is_same<decltype(std::declval<const rm::RCCHipO1Dn&>().robustWeights(std::declval<const rm::Transform&>(), 0.0,
                           std::declval<const rm::RobustParams&>())), std::vector<float>>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::RCCHipPinhole&>().correctOnceRobust(std::declval<const rm::Transform&>(),
                           std::declval<const rm::Transform&>(), 3u, 0.0, std::declval<const rm::RobustParams&>())), rm::Transform>::value, "");
int main() { return rm::RobustParams::fixed(RMCLHIP_ROBUST_CAUCHY, 0.5f).scale_mode == RMCLHIP_ROBUST_SCALE_FIXED ? 0 : 1; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_example_matches_the_python_binding(ra, orc, ctx, tmp_path):
    from rmcl_amd import synthetic as syn, types as T
    exe = _build(tmp_path)
    s = rc.contaminated_scan(orc)
    v, f = s["map"]
    # the example's own frames (float pi, its truth): the scan is re-made for them with the recipe of robust_cases.contaminated_scan
    pi = float(np.float32(np.pi))
    Tsb = T.transform_from_rpy((0.1, 0.0, 0.3), (0.0, 0.0, 10.0 * pi / 180))
    truth = T.transform_from_rpy((0.5, -0.3, 0.2), (0.02, -0.03, 0.4))
    est = T.mult(truth, T.transform_from_rpy((0.2, 0.0, 0.0), (0.0, 0.0, 2.0 * pi / 180)))
    model = syn.model_c1()
    meas = s["mesh"].simulate_spherical(model, Tsb, truth, bvh=False)
    ranges = meas["ranges"].astype(np.float32).copy()
    short = np.zeros((32, 32), bool)
    short[:, 5:12] = True
    short = short.reshape(-1)
    ranges[short] -= np.random.RandomState(5).uniform(0.3, 0.8, int(short.sum())).astype(np.float32)
    ds = (orc.spherical_directions(model) * ranges[:, None]).astype(np.float32)
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    with open(tmp_path / "dataset.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(ds)))
        fh.write(ds.tobytes())
        fh.write(np.ascontiguousarray(meas["hits"], np.uint8).tobytes())
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "dataset.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}

    rcc = ra.RCCHipSpherical(ra.import_hip_map(ctx, v, f))
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    rcc.set_dataset(ds, meas["hits"])
    rcc.params.max_dist = rcc.adaptive_max_dist_min = 1.0
    Tp, _ = rcc.correct_once(T.identity(), est, 10, 0.0)
    Tr, st = rcc.correct_once_robust(T.identity(), est, 10, 0.0, "tukey")
    assert np.allclose([float(x) for x in out["plain"]], [float(Tp["t"][k]) for k in "xyz"], rtol=0, atol=1e-5)
    assert [np.float32(x) for x in out["robust"]] == [Tr["t"][k] for k in "xyz"]
    assert [np.float32(x) for x in out["scale"]] == [st["scale"], st["median_abs_residual"]]
    assert int(out["n_meas"][0]) == int(st["stats"]["n_meas"]) and float(out["weight_sum"][0]) == float(st["weight_sum"])
    Tso = T.mult(est, Tsb)
    w = rcc.robust_weights(T.mult(T.mult(T.inv(Tso), Tr), Tso), 0.0, "tukey")
    assert [int(x) for x in out["weights"]] == [len(w), int((w < 0.5).sum())] and (w < 0.5).sum() > 100
    assert out["free_equals_operator"] == ["1"]
