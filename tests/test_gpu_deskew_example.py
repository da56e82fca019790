"""examples/deskew_cpp_example.cpp -- a cloud taken in motion -> knots from two odometry poses -> RCCHipOnDn::setInputPointCloud2Deskewed ->
correctOnce, through the C++ adapters -- compiles with plain g++ against the C ABI (CPU test) and, on a GPU, prints what the Python
binding computes for the same scene (the premise of tests/test_deskew_cpu.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import deskew_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "deskew_cpp_example.cpp"


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


def test_adapter_types(tmp_path):
    src = tmp_path / "shape.cpp"
    src.write_text(r'''
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
namespace rm = rmcl_hip;
static_assert(sizeof(rmclhip_pointcloud2_time) == 24 && sizeof(rmclhip_deskew_stats) == 20, "");
static_assert(std::is_same<decltype(std::declval<rm::RCCHipOnDn&>().setInputPointCloud2Deskewed(
                  nullptr, 0, std::declval<const rmclhip_pointcloud2_layout&>(), std::declval<const rmclhip_pointcloud2_time&>(),
                  std::declval<const rm::ScanMotion&>(), rm::Interval{0.f, 1.f})), rmclhip_deskew_stats>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::Pc2DeskewHip&>().convert(nullptr, 0, std::declval<const rmclhip_pointcloud2_layout&>(),
                  std::declval<const rm::ScanMotion&>())), rm::DeviceView<const float>>::value, "");
int main() { return 0; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    # the other operators refuse it at compile time: every ray needs its own origin
    bad = tmp_path / "bad.cpp"
    bad.write_text('#include "rmcl_hip/rmcl_hip.hpp"\nvoid f(rmcl_hip::RCCHipO1Dn& r, const rmclhip_pointcloud2_layout& l, const rmclhip_pointcloud2_time& t, '
                   'const rmcl_hip::ScanMotion& m) { r.setInputPointCloud2Deskewed(nullptr, 0, l, t, m, rmcl_hip::Interval{0.f, 1.f}); }\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "RCCHipOnDn only" in r.stderr


@pytest.mark.gpu
def test_example_matches_the_python_binding(ra, orc, ctx, meshes, tmp_path):
    from rmcl_amd import types as T
    exe = _build(tmp_path)
    v, f = meshes("cube")
    sc = dr.premise_scene(orc.Mesh(v, f))
    assert sc["layout"]["point_step"] == 16 and sc["time_field"] == (12, 7)
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    with open(tmp_path / "cloud.bin", "wb") as fh:
        fh.write(sc["cloud"].tobytes())
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "cloud.bin"), str(sc["W"])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}

    # the same steps through the Python binding
    yaw = lambda a, t: T.transform((0.0, 0.0, float(np.float32(np.sin(a / 2))), float(np.float32(np.cos(a / 2)))), t)
    last = yaw(0.4, (0.5, -0.3, 0.2))
    first = T.mult(last, T.inv(yaw(0.15, (0.4, 0.0, 0.0))))
    est = T.mult(last, yaw(0.05, (0.1, 0.1, 0.0)))
    motion = ra.wire.scan_motion(T.identity(), np.array([first, last], T.TRANSFORM), [0.0, 1.0], 1.0, 16)
    lay = sc["layout"]
    rcc = ra.RCCHipOnDn(ra.import_hip_map(ctx, v, f))
    rcc.params.max_dist = 1.0
    rcc.adaptive_max_dist_min = 1.0
    w, h, st = rcc.setInputPointCloud2Deskewed(sc["cloud"], *[lay[k] for k in ("width", "height", "point_step", "row_step", "offset_x", "offset_y",
                                                                               "offset_z")], sc["time_field"], motion, range_min=0.1, range_max=100.0)
    T_onew_oold, stats = rcc.correct_once(T.identity(), est, 40, 0.0, True)
    Tbm = T.mult(T_onew_oold, est)

    assert int(out["knots"][0]) == 17 == len(motion[0])
    assert np.allclose([float(x) for x in out["first_knot_t"]], [float(motion[0][0]["t"][c]) for c in "xyz"], atol=1e-7)
    assert [int(x) for x in out["stats"]] == [st[k] for k in ("n_points", "n_finite", "n_valid", "n_time_clamped", "n_time_nonfinite")]
    assert [int(x) for x in out["model"]] == [w, h] == [sc["W"], sc["H"]]
    assert np.allclose([float(x) for x in out["pose_t"]], [float(Tbm["t"][c]) for c in "xyz"], atol=1e-6)
    assert np.allclose([float(x) for x in out["pose_q"]], [float(Tbm["R"][c]) for c in "xyzw"], atol=1e-6)
    assert int(out["n_meas"][0]) == int(stats["n_meas"]) > w * h // 2
    # ... and the pose it ends at is the truth: the raw scan would end 0.25 m off (tests/test_gpu_deskew.py)
    assert np.linalg.norm(np.array([float(x) for x in out["pose_t"]]) - np.array([float(x) for x in out["truth_t"]])) < 1e-3
    assert [int(x) for x in out["cloud_form"]] == [w * h, st["n_valid"]]
