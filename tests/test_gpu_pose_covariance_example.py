"""examples/pose_covariance_cpp_example.cpp -- publishPose() with the covariance computed from the correction's own correspondences,
through the C++ adapters -- compiles with plain g++ against the C ABI (CPU test) and, on a GPU, prints what the Python binding computes
for the same scene."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "pose_covariance_cpp_example.cpp"


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
static_assert(std::is_same<rm::PoseInformation, rmclhip_pose_information>::value && sizeof(rm::PoseInformation) == 352, "");
static_assert(std::is_same<rm::PoseCovariance, rmclhip_pose_covariance>::value && sizeof(rm::PoseCovariance) == 496, "");
static_assert(std::is_same<decltype(std::declval<const rm::RCCHipSpherical&>().computePoseInformation(std::declval<const rm::Transform&>(), 0.0)),
                           rm::PoseInformation>::value, "");
static_assert(std::is_same<decltype(std::declval<const rm::RCCHipO1Dn&>().computePoseInformationBatch(2u)), std::vector<rm::PoseInformation>>::value, "");
static_assert(std::is_same<decltype(rm::poseCovariance(std::declval<const rm::PoseInformation&>())), rm::PoseCovariance>::value, "");
static_assert(std::is_same<decltype(std::declval<const rm::Transform&>() * std::declval<const rm::PoseInformation&>()), rm::PoseInformation>::value, "");
int main() { return 0; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_example_matches_the_python_binding(ra, orc, ctx, meshes, tmp_path):
    from rmcl_amd import synthetic as syn, types as T
    exe = _build(tmp_path)
    v, f = meshes("cube")
    pi = float(np.float32(math.pi))                   # the example's float pi
    model = syn.model_c1()
    Tsb = T.transform_from_rpy((0.1, 0.0, 0.3), (0.0, 0.0, 10.0 * pi / 180))
    truth = T.transform_from_rpy((0.5, -0.3, 0.2), (0.02, -0.03, 0.4))
    est = T.mult(truth, T.transform_from_rpy((0.2, 0.1, 0.05), (0.0, 0.0, 2.0 * pi / 180)))
    meas = orc.Mesh(v, f).simulate_spherical(model, Tsb, truth, bvh=False)
    ds = (orc.spherical_directions(model) * meas["ranges"][:, None]).astype(np.float32)
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

    # the same steps through the Python binding
    rcc = ra.RCCHipSpherical(ra.import_hip_map(ctx, v, f))
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    rcc.set_dataset(ds, meas["hits"])
    rcc.params.max_dist = 1.0
    rcc.adaptive_max_dist_min = 0.15
    rcc.find(est)
    T_onew_oold = T.identity()
    for _ in range(5):
        T_snew_sold = T.mult(T.mult(T.inv(Tsb), T_onew_oold), Tsb)
        Cs_o = T.cross_statistics_transform(Tsb, rcc.computeCrossStatistics(T_snew_sold, 0.25))
        T_onew_oold = T.mult(T_onew_oold, T.umeyama_transform(T.cross_statistics_merge(T.cross_statistics_identity(), Cs_o)))
    T_final = T.mult(T.mult(T.inv(Tsb), T_onew_oold), Tsb)
    info = T.pose_information_transform(Tsb, rcc.computePoseInformation(T_final, 0.25))
    cov = T.pose_covariance(info, degenerate_variance=100.0)

    n_meas = int(info["n_meas"])
    assert [int(x) for x in out["n_meas"]] == [n_meas, n_meas] and n_meas > 500
    got = np.array([float(x) for x in out["covariance"]]).reshape(6, 6)
    assert np.max(np.abs(got - cov["covariance"])) <= 1e-6 * np.max(np.abs(cov["covariance"]))
    assert np.allclose([float(x) for x in out["information_diag"]], np.diag(info["A"]), rtol=1e-6)
    assert math.isclose(float(out["s2"][0]), float(cov["s2"]), rel_tol=1e-6) and math.isclose(float(out["rss"][0]), float(info["rss"]), rel_tol=1e-6)
    assert [int(x) for x in out["degenerate"]] == [0, 0]
    assert np.allclose([float(x) for x in out["eig_trans"]], cov["eig_trans"], rtol=1e-6) and abs(sum(float(x) for x in out["eig_trans"]) - 1.0) < 1e-6
    # the published covariance is a covariance, and it is not the reference's guess (1 - convergence_progress on the diagonal)
    np.linalg.cholesky(got)
    assert np.all(np.diag(got) < 1e-2)
    # five Umeyama iterations on fixed correspondences have covered more than half of the 0.2 m the estimate was off by: what is left of the
    # Gauss-Newton step is below 0.1
    assert np.max(np.abs([float(x) for x in out["remaining_step"]])) < 0.1
    assert out["free_equals_operator"] == ["1"]
    assert int(out["batch_n_meas"][1]) >= int(out["batch_n_meas"][0]) > 300 and float(out["batch_rss"][1]) < float(out["batch_rss"][0])
