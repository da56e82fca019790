"""CPU tests of the map segmentation: the numpy restatement that serves as the GPU tests' yardstick (tests/segmentation_ref.py) is pinned
by hand-written rays and a committed fixture; the C ABI's new structs have the layout the Python binding assumes; the C++ adapters' new
members compile; the entry points reject null arguments before any HIP call.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import segmentation_ref as sr
from conftest import golden_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_hand_written_rays():
    """one ray per branch of the rule, values exact in binary: direction +x, the surface faces the sensor (normal -x, given unnormalised),
    range [0.5, 10], thresholds scan 0.25 / map 0.5"""
    nan = float("nan")
    rays = [
        # r_real, r_sim, label, expected point
        (1.0, 2.0, 2, (1.0, 0.0, 0.0)),       # in front of the surface by 1.0 > 0.25: scan outlier, preal_s
        (1.75, 2.0, 1, None),                 # plane_distance == threshold (0.25): strict >, not an outlier
        (1.875, 2.0, 1, None),                # in front by 0.125: inlier
        (2.0, 2.0, 1, None),                  # r_real == r_sim: the >= branch, distance 0
        (2.5, 2.0, 1, None),                  # behind by 0.5 == the map threshold: not an outlier
        (3.0, 2.0, 3, (2.0, 0.0, 0.0)),       # behind by 1.0 > 0.5: map outlier, pint_s
        (4.0, 11.0, 2, (4.0, 0.0, 0.0)),      # measured, simulated miss (range.max + 1): scan outlier
        (nan, 2.0, 3, (2.0, 0.0, 0.0)),       # NaN is not inside: the sim-only branch
        (0.25, 2.0, 3, (2.0, 0.0, 0.0)),      # below range.min: the same
        (0.0, 11.0, 0, None),                 # neither
        (nan, nan, 0, None),
    ]
    r_real = np.array([r[0] for r in rays], np.float32)
    r_sim = np.array([r[1] for r in rays], np.float32)
    n = len(rays)
    dirs = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1))
    normals = np.tile(np.array([-2.0, 0.0, 0.0], np.float32), (n, 1))
    out = sr.segment(r_real, r_sim, normals, dirs, np.zeros(3), 0.5, 10.0, 0.25, 0.5)
    assert list(out["labels"]) == [r[2] for r in rays]
    assert np.array_equal(out["outlier_scan"], np.array([r[3] for r in rays if r[2] == 2], np.float64))      # buffer order
    assert np.array_equal(out["outlier_map"], np.array([r[3] for r in rays if r[2] == 3], np.float64))
    # the two thresholds are not swapped
    swapped = sr.segment(r_real, r_sim, normals, dirs, np.zeros(3), 0.5, 10.0, 0.5, 0.25)
    assert list(swapped["labels"][:6]) == [2, 1, 1, 1, 3, 3]
    # a ray origin off the sensor frame's (O1Dn): preal_s carries it, the both-valid pint_s does not -- unless the flag says so -- and
    # the sim-only pint_s does.  r_real == r_sim then has plane distance |orig . n| = 0.375: the >= branch compares it with the MAP threshold
    orig = np.array([0.375, 0.5, 0.0], np.float32)
    o = sr.segment(r_real, r_sim, normals, dirs, orig, 0.5, 10.0, 0.25, 0.5)
    assert list(o["labels"]) == [2, 1, 1, 1, 3, 3, 2, 3, 3, 0, 0]     # every both-valid ray moved 0.375 towards "behind"
    assert np.array_equal(o["outlier_scan"], [[1.375, 0.5, 0.0], [4.375, 0.5, 0.0]])
    assert np.array_equal(o["outlier_map"], [[2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.375, 0.5, 0.0], [2.375, 0.5, 0.0]])
    w = sr.segment(r_real, r_sim, normals, dirs, orig, 0.5, 10.0, 0.25, 0.5, pint_with_origin=True)
    assert list(w["labels"]) == [r[2] for r in rays]
    assert np.array_equal(w["outlier_map"], [[2.375, 0.5, 0.0]] * 3)
    # undecided: only the rays that sit on a threshold or on a range bound
    und = sr.undecided(r_real, r_sim, normals, dirs, np.zeros(3), 0.5, 10.0, min_dist_outlier_scan=0.25, min_dist_outlier_map=0.5)
    assert list(np.nonzero(und)[0]) == [1, 4]


def test_fixture_is_reproduced_by_the_restatement():
    """tests/golden/g8_segmentation_cube.npz (written by tests/golden/make_g8_segmentation.py): real ranges, labels and both clouds on
    pose 0 of the committed cube simulation"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_g8_segmentation", golden_path("make_g8_segmentation.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(golden_path("g8_segmentation_cube.npz"))
    got = gen.build()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k], equal_nan=True), k
    L = want["labels"]
    hist = np.bincount(L, minlength=4)
    assert hist.sum() == 1024 and hist[2] > 30 and hist[3] > 30 and hist[1] > 500 and hist[0] == 0
    assert want["outlier_scan"].shape == (hist[2], 3) and want["outlier_map"].shape == (hist[3], 3)
    # the doctored blocks land where they must: the shortened block in outlier_scan, the two zero rows and the four beams beyond
    # the range in outlier_map through the sim-only branch
    L2 = L.reshape(32, 32)
    assert (L2[4:9, 3:12] == 2).all() and (L2[12:14, :] == 3).all() and (L2[30, 5:9] == 3).all()
    assert os.path.getsize(golden_path("g8_segmentation_cube.npz")) < 32768


def test_struct_layouts_match_the_c_header(ra, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rmclhip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %u\\n", sizeof(rmclhip_segmentation_params), sizeof(rmclhip_segmentation_views),\n'
                   '  offsetof(rmclhip_segmentation_params, flags), offsetof(rmclhip_segmentation_views, outlier_map_xyz_dev),\n'
                   '  offsetof(rmclhip_segmentation_views, counts_dev), RMCLHIP_SEG_PINT_WITH_ORIGIN); return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    P, V = ra._capi.SegmentationParams, ra._capi.SegmentationViews
    assert got == [C.sizeof(P), C.sizeof(V), P.flags.offset, V.outlier_map_xyz_dev.offset, V.counts_dev.offset, ra._capi.SEG_PINT_WITH_ORIGIN]
    assert C.sizeof(P) == 12 and C.sizeof(V) == 32


def test_adapter_members_compile(tmp_path):
    """SimulatorHip<M>::segment for all four models over host and device ranges, the two node classes"""
    src = tmp_path / "seg.cpp"
    src.write_text(r'''
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
using namespace rmcl_hip;
template <typename SimT>
SegmentationCounts both(SimT& sim, const Transform& T, const Memory<float, RAM>& host, Memory<float, VRAM_HIP>& dev,
                        Memory<Vector, VRAM_HIP>& a, Memory<Vector, VRAM_HIP>& b, Memory<uint8_t, VRAM_HIP>& labels) {
  SegmentationParams p;
  p.min_dist_outlier_scan = 0.1f; p.min_dist_outlier_map = 0.3f; p.pint_with_origin = true;
  sim.segment(T, host, p, a, b);
  sim.segment(T, MemoryView<const float, RAM>(host.raw(), host.size()), p, a, b, &labels);
  MemoryView<const float, VRAM_HIP> view;
  view.ptr = dev.raw(); view.n = dev.size();
  return sim.segment(T, view, p, a, b, &labels);
}
template SegmentationCounts both(SphereSimulatorHip&, const Transform&, const Memory<float, RAM>&, Memory<float, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<uint8_t, VRAM_HIP>&);
template SegmentationCounts both(O1DnSimulatorHip&, const Transform&, const Memory<float, RAM>&, Memory<float, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<uint8_t, VRAM_HIP>&);
template SegmentationCounts both(PinholeSimulatorHip&, const Transform&, const Memory<float, RAM>&, Memory<float, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<uint8_t, VRAM_HIP>&);
template SegmentationCounts both(OnDnSimulatorHip&, const Transform&, const Memory<float, RAM>&, Memory<float, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<Vector, VRAM_HIP>&, Memory<uint8_t, VRAM_HIP>&);
static_assert(std::is_same<decltype(ScanMapSegmentationHipNode::min_dist_outlier_scan_), float>::value &&
              std::is_same<decltype(O1DnMapSegmentationHipNode::min_dist_outlier_map_), float>::value, "the nodes' thresholds are float members");
SegmentationCounts scan(ScanMapSegmentationHipNode& node, const SphericalModel& m, const Memory<float, RAM>& r, const Transform& T) {
  node.min_dist_outlier_scan_ = 0.2f;
  return node.scanCB(m, r, T);
}
SegmentationCounts scan(O1DnMapSegmentationHipNode& node, const O1DnModel& m, const Memory<float, VRAM_HIP>& r, const Transform& T) {
  const SegmentationCounts n = node.scanCB(m, DeviceView<const float>{r.raw(), r.size()}, T);
  return node.cloud_outlier_scan_.size() == n.outlier_scan ? n : SegmentationCounts{};
}
int main() { return 0; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_segmentation_example_compiles_and_links_without_gpu(ra, tmp_path):
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "segmentation_cpp_example.cpp")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_null_arguments_are_rejected_before_any_hip_call(ra):
    """runs without a device: a null handle, pose, scan or parameter block is RMCLHIP_ERR_INVALID with a message"""
    L = ra._capi.lib()
    params = ra._capi.SegmentationParams(0.15, 0.15, 0)
    views = ra._capi.SegmentationViews()
    counts = (C.c_uint32 * 2)(7, 7)
    buf = (C.c_float * 8)()
    assert L.rmclhip_rcc_segment(None, buf, buf, 0, C.byref(params), C.byref(views), counts) == ra._capi.ERR_INVALID
    assert b"rcc_segment" in L.rmclhip_last_error()
    assert tuple(counts) == (0, 0)
    assert L.rmclhip_rcc_segment(None, buf, buf, 0, None, C.byref(views), counts) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_segment_async(None, buf, buf, 0, C.byref(params), C.byref(views)) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_segment_async(None, None, None, 0, None, None) == ra._capi.ERR_INVALID
    assert hasattr(ra.CorrespondencesHIP, "segment") and all(hasattr(getattr(ra, c), "segment") for c in
                                                             ("RCCHipSpherical", "RCCHipO1Dn", "RCCHipPinhole", "RCCHipOnDn"))
