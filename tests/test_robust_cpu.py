"""Host side of ROBUST MICP (include/rmclhip.h) through ctypes, no GPU: the weight on the host against the numpy restatement byte for
byte, the default parameters and every refusal, the structs' layouts against a compiled probe, and the host functions under the
address and undefined-behaviour sanitizers in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import robust_cases as rc
import robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_host_weight_equals_the_restatement_bit_for_bit(ra):
    L = ra._capi.lib()
    checked = 0
    for c in rc.GRID_C:
        r = rc.grid_r(c)
        # the premises of the grid: both zeros, |r| == c, one ulp either side, a denormal
        bits = r.view(np.uint32)
        assert 0x00000000 in bits and 0x80000000 in bits and np.any(r == c) and np.any(r == np.nextafter(c, F(0))) \
            and np.any(r == np.nextafter(c, F(np.inf))) and np.any((np.abs(r) > 0) & (np.abs(r) < F(1.1754944e-38)))
        for kernel in rr.KERNELS:
            want = rr.weight(kernel, c, r)
            got = np.array([L.rmclhip_robust_weight_host(kernel, float(c), float(x)) for x in r], F)
            assert got.tobytes() == want.tobytes(), (rr.NAMES[kernel], c, r[got.view(np.uint32) != want.view(np.uint32)][:4])
            assert np.all((got >= 0) & (got <= 1))
            zero = np.abs(r) == 0
            assert np.all(got[zero] == 1.0)
            checked += len(r)
    assert checked >= 5 * 6 * 50
    assert any(float(c) == float(F(1e-30)) for c in rc.GRID_C)
    # the binding's helper takes names
    assert ra.types.robust_weight("tukey", 0.5, 0.25) == rr.weight(rr.TUKEY, 0.5, [0.25])[0]


def test_weights_at_the_kernels_landmarks():
    """the restatement itself against values known in closed form (exact in float32)"""
    def same(got, want):
        return got.dtype == F and got.tobytes() == np.array(want, F).tobytes()

    assert same(rr.weight(rr.HUBER, 0.5, [0.25, 0.5, 1.0, -2.0]), [1.0, 1.0, 0.5, 0.25])
    assert same(rr.weight(rr.CAUCHY, 0.5, [0.0, 0.5, -1.0]), [1.0, 0.5, 0.2])
    assert same(rr.weight(rr.TUKEY, 1.0, [0.0, 0.5, 1.0, 3.0]), [1.0, 0.5625, 0.0, 0.0])
    assert same(rr.weight(rr.GEMAN_MCCLURE, 2.0, [0.0, 2.0, -2.0]), [1.0, 0.25, 0.25])
    assert same(rr.weight(rr.NONE, 1.0, [5.0]), [1.0])


def test_defaults(ra):
    L = ra._capi.lib()
    for kernel in rr.KERNELS:
        p = ra._capi.RobustParams()
        L.rmclhip_robust_params_default(kernel, C.byref(p))
        assert (p.kernel, p.scale_mode, p.reserved) == (kernel, ra._capi.ROBUST_SCALE_MAD, 0)
        assert F(p.tuning) == rr.TUNING[kernel] and F(p.scale_min) == F(1e-3) and F(p.scale) == F(1.0)
        assert L.rmclhip_robust_params_check(C.byref(p)) == 0
        q = ra.types.robust_params(rr.NAMES[kernel])
        assert bytes(q) == bytes(p)
    p = ra._capi.RobustParams()
    L.rmclhip_robust_params_default(17, C.byref(p))
    assert p.kernel == rr.NONE
    fixed = ra.types.robust_params("huber", scale=0.3)
    assert fixed.scale_mode == ra._capi.ROBUST_SCALE_FIXED and F(fixed.scale) == F(0.3)


BAD = (0.0, -1.0, float("inf"), float("-inf"), float("nan"))


def test_every_rejected_parameter_names_its_field(ra):
    L = ra._capi.lib()

    def refused(p, field):
        assert L.rmclhip_robust_params_check(C.byref(p)) == 1, field
        assert field in L.rmclhip_last_error().decode(), (field, L.rmclhip_last_error())

    def fresh(mode):
        p = ra._capi.RobustParams()
        L.rmclhip_robust_params_default(rr.HUBER, C.byref(p))
        p.scale_mode, p.scale = mode, 0.1
        return p

    for k in (-1, 5, 99):
        p = fresh(rr.MAD)
        p.kernel = k
        refused(p, "kernel")
    for m in (-1, 2):
        p = fresh(m)
        refused(p, "scale_mode")
    for b in BAD:
        for field in ("tuning", "scale_min"):
            p = fresh(rr.MAD)
            setattr(p, field, b)
            refused(p, field)
            p = fresh(rr.FIXED)            # the FIXED mode does not read them
            setattr(p, field, b)
            assert L.rmclhip_robust_params_check(C.byref(p)) == 0
        p = fresh(rr.FIXED)
        p.scale = b
        refused(p, "scale")
        p = fresh(rr.MAD)                  # the MAD mode does not read it
        p.scale = b
        assert L.rmclhip_robust_params_check(C.byref(p)) == 0
    assert L.rmclhip_robust_params_check(None) == 1
    with pytest.raises(ra.RmclHipError):
        ra.types.robust_params("tukey", tuning=-2.0)


def test_struct_layouts_match_the_c_header(ra, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rmclhip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(rmclhip_robust_params), sizeof(rmclhip_robust_statistics),\n'
                   '  offsetof(rmclhip_robust_params, scale_min), offsetof(rmclhip_robust_statistics, weight_sum),\n'
                   '  offsetof(rmclhip_robust_statistics, rss), offsetof(rmclhip_robust_statistics, scale),\n'
                   '  offsetof(rmclhip_robust_statistics, median_abs_residual), RMCLHIP_ROBUST_NONE, RMCLHIP_ROBUST_GEMAN_MCCLURE,\n'
                   '  RMCLHIP_ROBUST_SCALE_FIXED, RMCLHIP_ROBUST_SCALE_MAD); return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    P, S, D = ra._capi.RobustParams, ra._capi.RobustStatistics, ra.types.ROBUST_STATISTICS
    assert got == [C.sizeof(P), C.sizeof(S), P.scale_min.offset, S.weight_sum.offset, S.rss.offset, S.scale.offset,
                   S.median_abs_residual.offset, ra._capi.ROBUST_NONE, ra._capi.ROBUST_GEMAN_MCCLURE, ra._capi.ROBUST_SCALE_FIXED,
                   ra._capi.ROBUST_SCALE_MAD]
    assert C.sizeof(P) == 24 and C.sizeof(S) == 96 == D.itemsize
    assert [D.fields[k][1] for k in ("weight_sum", "wrss", "rss", "scale", "median_abs_residual")] == [64, 72, 80, 88, 92]


def test_host_functions_under_the_sanitizers(tmp_path):
    """tests/robust_host_check.cpp: a program of its own with the weight, the defaults and the parameter check compiled in, built with
    the address and undefined-behaviour sanitizers and run on the CPU"""
    exe = str(tmp_path / "robust_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", os.path.join(ROOT, "tests", "robust_host_check.cpp"),
                           "-I" + os.path.join(ROOT, "rmcl_amd", "csrc"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, (res.stdout.decode(), res.stderr.decode())
    assert res.stdout.decode().strip().endswith("robust host check: OK") and res.stderr == b""
