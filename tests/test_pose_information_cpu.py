"""Host algebra of the pose information (include/rmclhip.h, POSE COVARIANCE) through ctypes, no GPU: the frame change, the weighted
merge, the Gauss-Newton step, the covariance with its degeneracy report -- against tests/pose_information_ref.py and numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_information_ref as pir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _random_T(T, rng, t_scale=3.0):
    """a transform whose float32 quaternion is as close to unit as float32 allows"""
    q = _unit(rng.normal(size=4))
    return T.transform(q, rng.uniform(-t_scale, t_scale, 3))


def _correspondences(rng, n, extent=2.0, resid=0.05):
    """(D, N, r) in float64: dataset points, unit normals, residuals"""
    return rng.uniform(-extent, extent, (n, 3)), _unit(rng.normal(size=(n, 3))), rng.normal(scale=resid, size=n)


def _u(D, N, r):
    return np.concatenate([N, np.cross(D, N), r[:, None]], axis=1)


def test_transform_is_the_information_of_the_moved_correspondences(ra):
    """A computed from correspondences moved by T == transform(T, A of the unmoved ones): two 6 x 6 products in double, relative 1e-12
    (of the largest entry: the products mix every entry of A)"""
    T = ra.types
    rng = np.random.RandomState(11)
    for trial in range(8):
        D, N, r = _correspondences(rng, 200)
        Tm = _random_T(T, rng)
        R, t = pir.rotation_f64(Tm), np.array([float(Tm["t"][k]) for k in "xyz"])
        ref0 = pir.from_u(_u(D, N, r))
        ref1 = pir.from_u(_u(D @ R.T + t, N @ R.T, r))
        got = T.pose_information_transform(Tm, pir.as_record(T, ref0))
        assert int(got["n_meas"]) == 200 and float(got["rss"]) == ref0["rss"]
        assert np.max(np.abs(got["A"] - ref1["A"])) <= 1e-12 * np.max(np.abs(ref1["A"])), trial
        assert np.max(np.abs(got["g"] - ref1["g"])) <= 1e-12 * np.max(np.abs(ref1["g"])), trial
        assert np.array_equal(got["A"], got["A"].T)
        assert np.allclose(pir.adjoint(Tm) @ ref0["A"] @ pir.adjoint(Tm).T, got["A"], rtol=0, atol=1e-12 * np.max(np.abs(ref1["A"])))
    ident = T.pose_information_transform(T.identity(), pir.as_record(T, ref0))
    assert np.array_equal(ident["A"], ref0["A"]) and np.array_equal(ident["g"], ref0["g"])


def test_merge_adds_with_the_weight_on_b(ra):
    T = ra.types
    rng = np.random.RandomState(12)
    a = pir.as_record(T, pir.from_u(_u(*_correspondences(rng, 50))))
    b = pir.as_record(T, pir.from_u(_u(*_correspondences(rng, 70))))
    for w in (1.0, 0.25, 3.0, 0.0):
        m = T.pose_information_merge(a, b, w)
        assert np.array_equal(m["A"], a["A"] + w * b["A"]) and np.array_equal(m["g"], a["g"] + w * b["g"])
        assert float(m["rss"]) == float(a["rss"]) + w * float(b["rss"]) and int(m["n_meas"]) == 120
    m = T.pose_information_merge(T.pose_information_identity(), b)
    assert m.tobytes() == b.tobytes()
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ra.RmclHipError):
            T.pose_information_merge(a, b, w)


def test_solve_recovers_a_pure_translation(ra):
    """planar correspondences (random unit normals, model points on their planes) whose dataset is the model moved back by a few
    centimetres: the problem is linear, the step is that translation up to the inputs' float32 rounding, 8 eps_f32 max|coordinate|"""
    T = ra.types
    rng = np.random.RandomState(13)
    for t in ((0.03, -0.02, 0.05), (-0.04, 0.0, 0.01)):
        n = 500
        I = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
        N = _unit(rng.normal(size=(n, 3))).astype(np.float32)
        D = (I.astype(np.float64) - np.array(t)).astype(np.float32)
        ref = pir.pose_information(T.identity(), D, None, I, N, None, 1.0)
        assert ref["n_meas"] == n
        xi = T.pose_information_solve(pir.as_record(T, ref), 1e-12)
        tol = 8.0 * EPS32 * float(max(np.abs(I).max(), np.abs(D).max()))
        assert np.max(np.abs(xi[:3] - np.array(t))) <= tol and np.max(np.abs(xi[3:])) <= tol, (xi, tol)
    # a direction the correspondences do not constrain is left alone: normals without an x component, no step along x
    N[:, 0] = 0.0
    N = _unit(N).astype(np.float32)
    ref = pir.pose_information(T.identity(), D, None, I, N, None, 1.0)
    assert T.pose_information_solve(pir.as_record(T, ref), 1e-9)[0] == 0.0


def test_covariance_is_s2_times_the_inverse(ra):
    """on a well-conditioned A: symmetric, s2 inv(A) to 1e-10 of its norm (cyclic Jacobi in double converges to ~1e-15 cond(A);
    cond(A) here is below 1e3), s2 from sigma or from the residuals, eig_trans sums to 1 (unit normals)"""
    T = ra.types
    rng = np.random.RandomState(14)
    D, N, r = _correspondences(rng, 400)
    ref = pir.from_u(_u(D, N, r))
    rec = pir.as_record(T, ref)
    assert np.linalg.cond(ref["A"]) < 1e3
    for sigma, s2 in ((0.02, 0.02 ** 2), (0.0, ref["rss"] / (400 - 6)), (-1.0, ref["rss"] / (400 - 6))):
        cov = T.pose_covariance(rec, sigma=sigma)
        want = s2 * np.linalg.inv(ref["A"])
        assert np.array_equal(cov["covariance"], cov["covariance"].T)
        assert np.linalg.norm(cov["covariance"] - want) <= 1e-10 * np.linalg.norm(want)
        assert abs(float(cov["s2"]) - s2) <= 1e-15 * s2
        np.linalg.cholesky(cov["covariance"])
        assert abs(cov["eig_trans"].sum() - 1.0) < 1e-12 and np.all(np.diff(cov["eig_trans"]) >= 0) and np.all(np.diff(cov["eig_rot"]) >= 0)
        assert int(cov["n_degenerate_trans"]) == 0 and int(cov["n_degenerate_rot"]) == 0
        # the block eigenpairs are eigenpairs: rows of eigvec_* against numpy's on the blocks of A / n_meas
        for blk, ev, evec in ((ref["A"][:3, :3], cov["eig_trans"], cov["eigvec_trans"]), (ref["A"][3:, 3:], cov["eig_rot"], cov["eigvec_rot"])):
            assert np.allclose(ev, np.linalg.eigvalsh(blk / 400.0), rtol=1e-12, atol=0)
            for k in range(3):
                assert np.allclose((blk / 400.0) @ evec[k], ev[k] * evec[k], rtol=0, atol=1e-12 * ev[2])
    # the Gauss-Newton step of the same record == numpy's solve
    assert np.allclose(T.pose_information_solve(rec, 1e-12), np.linalg.solve(ref["A"], ref["g"]), rtol=1e-10, atol=1e-14)


def test_covariance_reports_a_null_direction(ra):
    """normals orthogonal to a direction a: a translation along a changes no residual.  Along a the covariance is degenerate_variance,
    the report counts one degenerate translation with eigenvector +-a; with a = x the row of A is exactly zero and so is the match"""
    T = ra.types
    rng = np.random.RandomState(15)
    for a, exact in ((np.array([1.0, 0.0, 0.0]), True), (np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), False)):
        D, N, r = _correspondences(rng, 300)
        N = _unit(N - np.outer(N @ a, a))
        if exact:
            N[:, 0] = 0.0
        rec = pir.as_record(T, pir.from_u(_u(D, N, r)))
        cov = T.pose_covariance(rec, sigma=0.01, degenerate_variance=123.0, rcond=1e-9)
        d = np.concatenate([a, np.zeros(3)])
        along = float(d @ cov["covariance"] @ d)
        assert along == 123.0 if exact else abs(along - 123.0) < 1e-6 * 123.0
        assert int(cov["n_degenerate_trans"]) == 1 and int(cov["n_degenerate_rot"]) == 0
        assert abs(abs(float(cov["eigvec_trans"][0] @ a)) - 1.0) < 1e-12 and abs(float(cov["eig_trans"][0])) < 1e-12
        if exact:
            assert float(cov["covariance"][0, 0]) == 123.0 and np.all(cov["covariance"][0, 1:] == 0.0)
        # the other five directions keep s2 / lambda: on the complement the covariance inverts A
        P = np.eye(6) - np.outer(d, d)
        assert np.allclose(P @ cov["covariance"] @ rec["A"] @ P, 0.01 ** 2 * P, rtol=0, atol=1e-9 * 0.01 ** 2 * 300)


def test_covariance_refusals_and_defaults(ra):
    T = ra.types
    p = T.pose_covariance_params()
    assert (p.sigma, p.rcond, p.degenerate_variance, p.min_eig_trans, p.min_eig_rot) == (0.0, 1e-9, 1e6, 1e-3, 1e-3)
    rng = np.random.RandomState(16)
    few = pir.as_record(T, pir.from_u(_u(*_correspondences(rng, 6))))
    with pytest.raises(ra.RmclHipError):       # the noise cannot be estimated from six residuals
        T.pose_covariance(few)
    with pytest.raises(ra.RmclHipError):
        T.pose_covariance(few, sigma=-0.5)
    assert T.pose_covariance(few, sigma=0.01)["s2"] == 0.01 ** 2
    seven = pir.as_record(T, pir.from_u(_u(*_correspondences(rng, 7))))
    assert float(T.pose_covariance(seven)["s2"]) == float(seven["rss"]) / 1.0
    with pytest.raises(ra.RmclHipError):
        T.pose_covariance(seven, rcond=-1.0)
    bad = seven.copy()
    bad["A"][2, 2] = np.nan
    with pytest.raises(ra.RmclHipError):
        T.pose_covariance(bad, sigma=0.01)
    # nothing measured, a given sigma: every direction degenerate
    none = T.pose_covariance(T.pose_information_identity(), sigma=0.01, degenerate_variance=7.0)
    assert np.array_equal(none["covariance"], 7.0 * np.eye(6)) and int(none["n_degenerate_trans"]) == 3 and int(none["n_degenerate_rot"]) == 3
    L = ra._capi.lib()
    assert L.rmclhip_pose_covariance_host(None, None, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_pose_information_transform(None, None, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_pose_information_solve_host(None, 0.0, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_pose_information_p2l(None, None, None, None, None, None, None, 0, 1.0, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_pose_information(None, None, 0.0, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_pose_information_batch(None, 1, 0.0, None) == ra._capi.ERR_INVALID


def test_pod_layouts_match_the_header(ra, tmp_path):
    """the new declarations in a plain-C translation unit of their own (C99, pedantic), and the numpy / ctypes layouts against the
    compiler's"""
    T = ra.types
    src = tmp_path / "pi.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "rmclhip.h"
int main(void) {
  rmclhip_pose_information info;
  rmclhip_pose_covariance cov;
  rmclhip_pose_covariance_params p;
  rmclhip_status (*f1)(rmclhip_ctx*, const rmclhip_transform*, const float*, const uint8_t*, const float*, const float*, const uint8_t*,
                       uint32_t, float, rmclhip_pose_information*) = rmclhip_pose_information_p2l;
  rmclhip_status (*f2)(rmclhip_rcc*, const rmclhip_transform*, double, rmclhip_pose_information*) = rmclhip_rcc_pose_information;
  rmclhip_status (*f3)(rmclhip_rcc*, uint32_t, double, rmclhip_pose_information*) = rmclhip_rcc_pose_information_batch;
  rmclhip_status (*f4)(const rmclhip_pose_information*, const rmclhip_pose_covariance_params*, rmclhip_pose_covariance*) = rmclhip_pose_covariance_host;
  (void)info; (void)cov; (void)p; (void)f1; (void)f2; (void)f3; (void)f4;
  printf("%u %u %u %u %u %u %u %u\n", (unsigned)sizeof(rmclhip_pose_information), (unsigned)offsetof(rmclhip_pose_information, g),
         (unsigned)offsetof(rmclhip_pose_information, n_meas), (unsigned)sizeof(rmclhip_pose_covariance),
         (unsigned)offsetof(rmclhip_pose_covariance, eigvec_rot), (unsigned)offsetof(rmclhip_pose_covariance, n_degenerate_trans),
         (unsigned)offsetof(rmclhip_pose_covariance, s2), (unsigned)sizeof(rmclhip_pose_covariance_params));
  return 0;
}
''')
    libdir = os.path.join(ROOT, "rmcl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + libdir, "-lrmclhip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", str(tmp_path / "pi")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "pi")]).split()]
    PI, PC = T.POSE_INFORMATION, T.POSE_COVARIANCE
    assert got == [PI.itemsize, PI.fields["g"][1], PI.fields["n_meas"][1], PC.itemsize, PC.fields["eigvec_rot"][1],
                   PC.fields["n_degenerate_trans"][1], PC.fields["s2"][1], C.sizeof(ra._capi.PoseCovarianceParams)]
