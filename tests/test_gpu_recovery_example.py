"""examples/recovery_cpp_example.cpp -- a two-storey map, the cloud initialised on its floors, filter cycles with the field sensor update,
the adaptive resampler and the recovery injection, the robot moved to the other floor -- through the C++ adapters.  It compiles with
plain g++ against the C ABI (CPU test) and, on a GPU, shows what its construction guarantees: after the kidnapping the recovery rule asks for an
injection within the cycles its averages need, and particles then stand on the upper floor.  No convergence claim beyond that."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "recovery_cpp_example.cpp"
N, BEFORE, AFTER = 4000, 20, 10


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
static_assert(sizeof(rmclhip_surface_sample_params) == 44 && sizeof(rmclhip_surface_sample_info) == 32, "");
static_assert(sizeof(rmclhip_recovery_state) == 16 && sizeof(rmclhip_recovery_params) == 24, "");
static_assert(std::is_same<decltype(rm::injectSurface(std::declval<rm::ParticleCloud<rm::VRAM_HIP>&>(), std::declval<const rm::SurfaceSamplerHip&>(),
                                                      0.5, 1ull, 2u)), uint32_t>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::Recovery&>().update(1.0, 1u)), double>::value, "");
static_assert(std::is_same<decltype(std::declval<rm::PCDSensorUpdaterHipSharded&>().injectSurface(0.5, 1ull, 2u)), uint32_t>::value, "");
static_assert(!std::is_copy_constructible<rm::SurfaceSamplerHip>::value, "");
void f(rm::ParticleCloud<rm::VRAM_HIP>& c, const rm::SurfaceSamplerHip& s, rm::PCDSensorUpdaterHipSharded& p) {
  rm::initSamplesSurface(c, s, 1ull, 0u);
  rm::initSamplesSurface(c.posesView(), c.attrsView(), s, 1ull, 0u, 5u);
  p.setSurfaceSampler(rm::SurfaceSampleParams());
  p.initSamplesSurface(100u, 1ull);
  p.dropSurfaceSampler();
}
int main() { return 0; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_example_recovers_from_the_kidnapping(ra, ctx, tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "run", str(N), str(BEFORE), str(AFTER), "42"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    head = lines[0].split()
    assert head[:2] == ["sampler", "faces"] and int(head[2]) == 16 and int(head[4]) == 4 and float(head[6]) == 200.0    # the two floors
    rows = []
    for ln in lines[1:]:
        w = ln.split()
        rows.append({w[k]: float(w[k + 1]) for k in range(0, len(w), 2)})
    assert len(rows) == BEFORE + AFTER and [int(x["cycle"]) for x in rows] == list(range(BEFORE + AFTER))
    assert all(x["floor"] == 0 for x in rows[:BEFORE]) and all(x["floor"] == 1 for x in rows[BEFORE:])
    assert all(abs(x["share0"] + x["share1"] - 1.0) < 1e-5 and 0.0 <= x["p_inject"] <= 1.0 for x in rows)
    # the kidnapping: the likelihood drops, the recovery rule asks for an injection within the cycles its averages need ...
    after = rows[BEFORE:]
    first = next((k for k, x in enumerate(after) if x["p_inject"] > 0.0), None)
    assert first is not None, after
    assert after[first]["injected"] > 0
    # ... and particles then stand on the upper floor
    assert after[first]["share1"] > 0.0
    # (informational, no assertion: where the cloud stood before the kidnapping)
    print("before the kidnapping: share0 %.4f, p_inject %g; first injection %d cycles after it" % (rows[BEFORE - 1]["share0"], rows[BEFORE - 1]["p_inject"], first))
