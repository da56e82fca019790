"""CPU tests of the sampled odometry model (include/rmclhip.h, MOTION NOISE): rmclhip_motion_noise_sigma_host against the restatement
(tests/motion_noise_ref.py), and the premises of tests/test_gpu_motion_noise.py on the restatement alone.  No device needed."""
import ctypes as C
import math

import numpy as np
import pytest

import motion_noise_ref as mn

F = np.float32
N_STAT = 65536
STAT_SIGMA = np.array([0.25, 0.1, 0.05, 0.02, 0.03, 0.15], dtype=F)


def _params(ra, d):
    return ra.motion_noise_params(**d)


def _step(ra, t=(0, 0, 0), rpy=(0, 0, 0), flip=False):
    T = ra.types.transform_from_rpy(t, rpy)
    if flip:
        for k in "xyzw":
            T["R"][k] = -T["R"][k]
    return T


def _within_one_ulp(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


PARAMS = {
    "default": mn.default_params(),
    "mixed": {"alpha_trans_trans": [0.1, 0.02, 0.0], "alpha_trans_rot": [0.05, 0.3, 0.01], "alpha_rot_trans": [0.0, 0.0, 0.4],
              "alpha_rot_rot": [0.01, 0.02, 0.25]},
    "zero": {k: [0.0, 0.0, 0.0] for k in mn.FIELDS},
}


def test_defaults_are_amcls(ra):
    p = ra.motion_noise_params()
    for k in mn.FIELDS:
        assert list(getattr(p, k)) == [F(0.2)] * 3
    assert C.sizeof(p) == 48
    q = ra.motion_noise_params(alpha_rot_rot=0.5, alpha_trans_trans=(1, 2, 3))
    assert list(q.alpha_rot_rot) == [0.5] * 3 and list(q.alpha_trans_trans) == [1, 2, 3] and list(q.alpha_trans_rot) == [F(0.2)] * 3
    with pytest.raises(TypeError):
        ra.motion_noise_params(alpha=1)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_sigma_host_matches_the_restatement(ra, name):
    d = PARAMS[name]
    p = _params(ra, d)
    # the identity step: six zeros, whatever the alphas -- a robot that stands does not diffuse
    assert ra.motion_noise_sigma(p, ra.types.identity()).tobytes() == np.zeros(6, F).tobytes()
    rng = np.random.RandomState(5)
    steps = [_step(ra, t=(0.3, 0, 0)), _step(ra, t=(-0.1, 0.2, 0.05)),                         # pure translation
             _step(ra, rpy=(0, 0, 0.4)), _step(ra, rpy=(0.1, -0.2, 3.0)),                      # pure rotation in place
             _step(ra, t=(0.3, 0.01, 0), rpy=(0, 0, 0.2)), _step(ra, t=(1e-4, 0, 0), rpy=(0, 0, 1e-4)),
             _step(ra, rpy=(0, 0, math.pi))]                                                   # a half turn: w ~ 0
    steps += [_step(ra, t=rng.uniform(-1, 1, 3), rpy=rng.uniform(-3, 3, 3)) for _ in range(20)]
    for T in steps:
        want = mn.sigma_host(d, T)
        got = ra.motion_noise_sigma(p, T)
        assert got.dtype == F and _within_one_ulp(got, want), (name, T, got, want)
        # w < 0: q and -q are the same rotation and give the same sigma
        neg = T.copy()
        for k in "xyzw":
            neg["R"][k] = -neg["R"][k]
        assert ra.motion_noise_sigma(p, neg).tobytes() == got.tobytes()
    if name == "default":
        s = ra.motion_noise_sigma(p, _step(ra, t=(0.5, 0, 0)))
        assert _within_one_ulp(s, np.full(6, 0.2 * 0.5))
        s = ra.motion_noise_sigma(p, _step(ra, rpy=(0, 0, 0.5)))       # in place: the translations still get alpha_trans_rot * s_r
        assert np.allclose(s, 0.2 * 0.5, rtol=1e-6) and np.all(s[:3] > 0)
    if name == "zero":
        assert not ra.motion_noise_sigma(p, steps[4]).any()


def test_sigma_host_refusals(ra):
    L = ra._capi.lib()
    T = np.ascontiguousarray(_step(ra, t=(0.3, 0, 0), rpy=(0, 0, 0.1)), ra.types.TRANSFORM).reshape(1)
    out = np.full(6, 7.0, F)
    good = ra.motion_noise_params()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rmclhip_motion_noise_sigma_host(C.byref(good), ptr(T), ptr(out)) == ra._capi.OK
    out[:] = 7.0
    for field in mn.FIELDS:
        for k in range(3):
            for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
                p = ra.motion_noise_params()
                getattr(p, field)[k] = bad
                assert L.rmclhip_motion_noise_sigma_host(C.byref(p), ptr(T), ptr(out)) == ra._capi.ERR_INVALID, (field, k, bad)
                assert b"alpha" in L.rmclhip_last_error()
                with pytest.raises(ValueError):
                    d = mn.default_params()
                    d[field][k] = bad
                    mn.sigma_host(d, T)
    for grp, k in [("R", c) for c in "xyzw"] + [("t", c) for c in "xyz"]:
        for bad in (float("nan"), float("inf")):
            Tb = T.copy()
            Tb[grp][k] = bad
            assert L.rmclhip_motion_noise_sigma_host(C.byref(good), ptr(Tb), ptr(out)) == ra._capi.ERR_INVALID, (grp, k, bad)
            assert b"non-finite" in L.rmclhip_last_error()
            with pytest.raises(ValueError):
                mn.sigma_host(mn.default_params(), Tb)
    assert L.rmclhip_motion_noise_sigma_host(None, ptr(T), ptr(out)) == ra._capi.ERR_INVALID
    assert L.rmclhip_motion_noise_sigma_host(C.byref(good), None, ptr(out)) == ra._capi.ERR_INVALID
    assert L.rmclhip_motion_noise_sigma_host(C.byref(good), ptr(T), None) == ra._capi.ERR_INVALID
    assert np.all(out == 7.0), "a refusal wrote sigma_out"
    # a negative zero alpha is zero, not negative
    p = ra.motion_noise_params(alpha_trans_trans=-0.0)
    assert L.rmclhip_motion_noise_sigma_host(C.byref(p), ptr(T), ptr(out)) == ra._capi.OK


def test_device_entry_points_refuse_null_handles(ra):
    L = ra._capi.lib()
    assert L.rmclhip_pf_motion_update_noisy(None, None, None, 0, None, 0.0, 0, None, 0, 0, 0) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_sharded_motion_update_noisy(None, None, 0.0, 0, None, 0, 0) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_sharded_set_motion_noise(None, None) == ra._capi.ERR_INVALID


def test_cpp_example_compiles_and_links_without_gpu(ra, tmp_path):
    """examples/motion_noise_cpp_example.cpp builds with plain g++ against the C ABI; the adapters have the interface the issue names"""
    import os
    import subprocess
    from test_cpp_adapters import _build
    r = subprocess.run([_build(tmp_path, "motion_noise_cpp_example.cpp")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    src = tmp_path / "shape.cpp"
    src.write_text(r'''
#include <type_traits>
#include "rmcl_hip/rmcl_hip.hpp"
namespace rm = rmcl_hip;
static_assert(sizeof(rmclhip_motion_noise_params) == 48 && std::is_base_of<rmclhip_motion_noise_params, rm::MotionNoiseParams>::value, "");
template <typename U> void uses(U& u, const rm::MotionNoiseParams& p) { u.setNoise(p, 7u); u.clearNoise(); u.reset(); }
template void uses<rm::TFMotionUpdaterHip>(rm::TFMotionUpdaterHip&, const rm::MotionNoiseParams&);
template void uses<rm::PCDSensorUpdaterHipSharded>(rm::PCDSensorUpdaterHipSharded&, const rm::MotionNoiseParams&);
int main() {
  rm::MotionNoiseParams p;
  rm::Transform T = rm::identity();
  for (float s : p.sigma(T)) if (s != 0.0f) return 1;       // a robot that stands does not diffuse
  T.t = {0.5f, 0.0f, 0.0f};
  return p.sigma(T)[0] > 0.09f && p.sigma(T)[5] < 0.11f ? 0 : 1;
}
''')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "rmcl_amd")
    exe = str(tmp_path / "shape")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-L" + libdir, "-lrmclhip",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.run([exe]).returncode == 0


def test_streams_are_disjoint():
    """stream 2 is neither the resamplers' (0) nor the initialisers' (1): the same (seed, step, index) gives other words"""
    w2 = mn.noise_words(0, 64, mn.SEED, 3)
    w1 = mn.pref.init_words(0, 64, mn.SEED, 3)
    assert not np.any(w2 == w1)
    assert not np.any(mn.noise_words(0, 64, mn.SEED, 4) == w2) and not np.any(mn.noise_words(0, 64, mn.SEED + 1, 3) == w2)
    assert np.array_equal(mn.noise_words(40, 24, mn.SEED, 3), w2[40:])


def check_statistics(comp, sigma, what):
    """premise (a): comp [n, 6] -- every column's sample standard deviation within 5 / sqrt(2 n) relative of sigma_k and every pairwise
    correlation below 5 / sqrt(n): five standard errors each"""
    n = len(comp)
    comp = comp.astype(np.float64)
    sd = comp.std(axis=0, ddof=1)
    rel = np.abs(sd / sigma.astype(np.float64) - 1.0)
    corr = np.corrcoef(comp.T)
    off = np.abs(corr[~np.eye(6, dtype=bool)])
    print("%s: n %d, sd / sigma - 1 = %s (bound %.4g), max |corr| %.4g (bound %.4g), mean / sigma = %s" %
          (what, n, np.array2string(rel, precision=4), 5.0 / math.sqrt(2 * n), off.max(), 5.0 / math.sqrt(n),
           np.array2string(comp.mean(0) / sigma, precision=4)))
    assert np.all(rel <= 5.0 / math.sqrt(2 * n)), what
    assert off.max() < 5.0 / math.sqrt(n), what


def test_premise_a_the_draws_have_the_spread_they_are_asked_for():
    comp = mn.noise_components(0, N_STAT, STAT_SIGMA, mn.SEED, 1)
    check_statistics(comp, STAT_SIGMA, "restatement")
    # ... and N carries them: its translation is the first three, the Euler angles of its rotation the last three
    N = mn.noise_transforms(0, N_STAT, STAT_SIGMA, mn.SEED, 1)
    got = mn.components_f64(N)
    assert np.array_equal(got[:, :3].astype(F), comp[:, :3])
    assert np.allclose(got[:, 3:], comp[:, 3:], rtol=0, atol=2e-7)


@pytest.fixture(scope="module")
def wall(orc, meshes):
    v, f = meshes("cube")
    mesh = orc.Mesh(v, f)
    poses, attrs = mn.wall_cloud(1000)
    T = mn.wall_step()
    noisy = mn.motion_update(mesh, poses, attrs, T, 0.02, mn.WALL_SIGMA, mn.SEED, mn.WALL_STEP)
    plain = mn.motion_update(mesh, poses, attrs, T, 0.02, np.zeros(6, F), mn.SEED, mn.WALL_STEP)
    return mesh, poses, attrs, noisy, plain


def test_premise_b_the_wall_scene_has_all_four_kinds(wall):
    _, poses, _, (pn, an, kn), (pp, ap, kp) = wall
    kinds = {"noise only": int((kn & ~kp).sum()), "plain only": int((~kn & kp).sum()), "both": int((kn & kp).sum()), "neither": int((~kn & ~kp).sum())}
    print("wall scene:", kinds)
    assert min(kinds.values()) >= len(poses) // 50
    killed = (an["likelihood"]["n_meas"] == 10000) & (an["likelihood"]["mean"] == 0)
    assert np.array_equal(killed, kn)
    # the plain update is the oracle's
    assert pp.tobytes() == mn.xmul(poses, mn.wall_step()).tobytes()


def test_premise_c_few_particles_are_left_out(wall):
    mesh, poses, _, (pn, _, _), (pp, _, _) = wall
    for what, new in (("noisy", pn), ("plain", pp)):
        ex = mn.exclusions(mesh, poses["t"], new["t"])
        print("wall scene, %s: %d of %d left out of the kill comparison" % (what, int(ex.sum()), len(ex)))
        assert ex.sum() <= len(ex) // 100


def test_restatement_of_the_plain_update_is_the_oracles(wall):
    """with all sigmas zero the restatement is the oracle's motion update, bit for bit: poses, forgetting and kills"""
    mesh, poses, attrs, _, (pp, ap, _) = wall
    p, a = poses.copy(), attrs.copy()
    mesh.pf_motion_update(p, a, mn.wall_step(), 0.02, collision=True, bvh=True)
    assert p.tobytes() == pp.tobytes() and a.tobytes() == ap.tobytes()
