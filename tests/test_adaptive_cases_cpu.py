"""CPU tests of the adaptive particle count: rmclhip_kld_bound_host (a host function of the library) against the restatement
tests/adaptive_ref.py, the ABI of rmclhip_kld_params, and the properties of systematic resampling on the restatement alone -- on the
clouds the GPU tests (tests/test_gpu_adaptive.py) run on the device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import adaptive_ref as ar

KS = (0, 1, 2, 3, 10, 1000, 10 ** 6, 2 ** 32 - 1)
EPS_Z = ((0.01, 2.3263479), (0.05, 1.6448536), (0.001, 3.0902323), (0.25, 0.0), (0.02, -0.5))


def _lib_bound(ra, k, eps, z, n_min, n_max):
    n = C.c_uint32(0xDEAD)
    st = ra._capi.lib().rmclhip_kld_bound_host(int(k), float(eps), float(z), int(n_min), int(n_max), C.byref(n))
    return st, int(n.value)


@pytest.mark.parametrize("eps,z", EPS_Z)
def test_kld_bound_equals_the_restatement(ra, eps, z):
    for k in KS:
        for n_min, n_max in ((1, 0xFFFFFFFF), (500, 0xFFFFFFFF), (500, 20000), (1, 1), (7, 7), (3000, 3000)):
            st, n = _lib_bound(ra, k, eps, z, n_min, n_max)
            assert st == ra._capi.OK
            assert n == ar.kld_bound(k, eps, z, n_min, n_max), (k, eps, z, n_min, n_max)
            assert n_min <= n <= n_max
            assert ra.kld_bound(k, eps, z, n_min, n_max) == n
    # both ends of the clamp are reached, and 2^32 - 1 bins at epsilon 0.001 saturate
    assert ar.kld_bound(3, 0.01, 2.3263479, 500, 20000) == 500 and ar.kld_bound(10 ** 6, 0.01, 2.3263479, 500, 20000) == 20000
    assert ar.kld_bound(2 ** 32 - 1, 0.001, 3.0902323, 1, 0xFFFFFFFF) == 0xFFFFFFFF
    assert 1 < ar.kld_bound(1000, 0.01, 2.3263479, 1, 0xFFFFFFFF) < 0xFFFFFFFF


def test_kld_bound_known_values(ra):
    """Fox 2003 / AMCL's pf_resample_limit: k = 2, epsilon = 0.01, z = 2.3263479: a = 2/9, x = 7/9 + sqrt(2/9) z, n = ceil(50 x^3)"""
    x = 7.0 / 9.0 + (2.0 / 9.0) ** 0.5 * 2.3263479
    assert abs(ar.kld_bound(2, 0.01, 2.3263479, 1, 0xFFFFFFFF) - 50.0 * x ** 3) < 1.0
    assert _lib_bound(ra, 2, 0.01, 2.3263479, 1, 0xFFFFFFFF)[1] == ar.kld_bound(2, 0.01, 2.3263479, 1, 0xFFFFFFFF)
    # for many bins the bound approaches (k - 1) / (2 epsilon): the chi-square quantile over its degrees of freedom tends to 1
    n = ar.kld_bound(10 ** 6, 0.01, 2.3263479, 1, 0xFFFFFFFF)
    assert 1.0 < n / (999999 / 0.02) < 1.01


def test_kld_bound_is_monotone_in_k(ra):
    for eps, z in EPS_Z[:3]:
        prev = 0
        for k in list(range(0, 300)) + [10 ** e for e in range(3, 10)] + [2 ** 32 - 1]:
            st, n = _lib_bound(ra, k, eps, z, 1, 0xFFFFFFFF)
            assert st == ra._capi.OK and n >= prev, (k, eps, z)
            prev = n


@pytest.mark.parametrize("args", [(10, 0.0, 2.0, 1, 10), (10, -0.01, 2.0, 1, 10), (10, float("nan"), 2.0, 1, 10), (10, float("inf"), 2.0, 1, 10),
                                  (10, 0.01, float("nan"), 1, 10), (10, 0.01, float("inf"), 1, 10), (10, 0.01, 2.0, 0, 10), (10, 0.01, 2.0, 11, 10),
                                  (0, 0.01, 2.0, 0, 10)])
def test_kld_bound_error_cases(ra, args):
    st, _ = _lib_bound(ra, *args)
    assert st == ra._capi.ERR_INVALID
    assert b"kld_bound_host" in ra._capi.lib().rmclhip_last_error()
    with pytest.raises(ValueError):
        ar.kld_bound(*args)
    with pytest.raises(ra.RmclHipError):
        ra.kld_bound(*args)
    assert ra._capi.lib().rmclhip_kld_bound_host(10, 0.01, 2.0, 1, 10, None) == ra._capi.ERR_INVALID


def test_kld_params_abi(ra):
    """sizeof(rmclhip_kld_params) and its defaults, in the C header's layout and through the Python binding"""
    K = ra._capi.KldParams
    assert C.sizeof(K) == 56
    assert [getattr(K, f).offset for f, _ in K._fields_] == [0, 12, 24, 32, 40, 48, 52]
    p = ra.kld_params()
    assert list(p.bin_xyz) == [0.5, 0.5, 0.5] and list(p.bin_rpy) == [np.float32(0.17453292)] * 3
    assert p.min_likelihood_rel == np.float32(0.01) and p.epsilon == 0.01 and p.z == 2.3263479 and (p.n_min, p.n_max) == (500, 0xFFFFFFFF)
    d = ar.Kld()
    assert [np.float32(v) for v in p.bin_xyz] == d.bin_xyz and [np.float32(v) for v in p.bin_rpy] == d.bin_rpy
    assert (np.float32(p.min_likelihood_rel), p.epsilon, p.z, p.n_min, p.n_max) == (d.min_likelihood_rel, d.epsilon, d.z, d.n_min, d.n_max)
    q = ra.kld_params(bin_xyz=(1, 2, 0), bin_rpy=(0, 0, 0.25), min_likelihood_rel=0.5, epsilon=0.1, z=1.0, n_min=3, n_max=9)
    assert list(q.bin_xyz) == [1.0, 2.0, 0.0] and list(q.bin_rpy) == [0.0, 0.0, 0.25] and (q.n_min, q.n_max, q.epsilon, q.z) == (3, 9, 0.1, 1.0)
    ra._capi.lib().rmclhip_kld_params_default(None)   # a null pointer is ignored


def test_c_header_agrees_on_the_struct(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rmclhip.h"\n'
                   "int main(void) { printf(\"%u %u %u %u\\n\", (unsigned)sizeof(rmclhip_kld_params), (unsigned)offsetof(rmclhip_kld_params, epsilon),\n"
                   "  (unsigned)offsetof(rmclhip_kld_params, z), (unsigned)offsetof(rmclhip_kld_params, n_min)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(tmp_path / "t")])
    assert subprocess.check_output([str(tmp_path / "t")]).split() == [b"56", b"32", b"40", b"48"]


# ---- systematic resampling: properties of the rule, on the restatement alone ------------------------------
def test_even_cloud_maps_to_itself():
    for n in ar.SYS_N + (100003,):
        for step in (0, 1, 7):
            src, first, w, T = ar.sys_sources(np.full(n, 0.37, np.float32), n, seed=0xC0FFEE1234567, step=step)
            assert np.array_equal(src, np.arange(n)) and first.all() and T == n << 24
        poses, attrs = ar.cloud(n, 5)
        attrs["likelihood"]["mean"] = 0.37
        pn, an, _ = ar.systematic(poses, attrs, n, ar.gladiator_cfg(), seed=9, step=2)
        assert pn.tobytes() == poses.tobytes() and an.tobytes() == attrs.tobytes()


@pytest.mark.parametrize("n", ar.SYS_N)
def test_every_particle_gets_within_one_copy_of_its_share(n):
    """|c_i - n_new w_i / T| <= 1, in exact arithmetic"""
    for name, L in ar.weight_cases(n).items():
        for n_new in ar.sys_n_new(n) + [max(1, n // 20)]:
            for step in (0, 1):
                src, first, w, T = ar.sys_sources(L, n_new, seed=0xC0FFEE1234567, step=step)
                assert T == sum(w) and len(src) == n_new and src.min() >= 0 and src.max() < n
                assert np.all(np.diff(src) >= 0)
                c = np.bincount(src, minlength=n)
                worst = max(abs(Fraction(int(c[i])) - Fraction(n_new * w[i], T)) for i in range(n))
                assert worst <= 1, (name, n, n_new, step, float(worst))
                assert all(c[i] == 0 for i in range(n) if w[i] == 0)
                if name == "rounds_to_zero" and n > 1:
                    assert w[0] == 0 and L[0] > 0
                if name == "one_holds_all":
                    assert np.all(src == n // 2)


def test_sliced_calls_equal_the_whole_call():
    cfg = ar.gladiator_cfg(min_noise_tz=0.01, min_noise_roll=0.005, min_noise_pitch=0.005)
    for n, n_new in ((1025, 3075), (4097, 585), (65, 65)):
        poses, attrs = ar.cloud(n, 7)
        attrs["likelihood"]["mean"] = ar.weight_cases(n)["span_1e-6_1"]
        whole = ar.systematic(poses, attrs, n_new, cfg, seed=11, step=3)
        assert len(set(whole[2].tolist())) < n_new or n_new <= n   # where the cloud grows, slots beyond a run's first exist
        cuts = [0, n_new // 3, n_new // 3 + 1, n_new]
        parts = [ar.systematic(poses, attrs, n_new, cfg, seed=11, step=3, first=a, count=b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        for k in range(3):
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes()


def test_steps_change_the_gaussians_not_the_rule():
    """two steps draw different Gaussians; for equal u0 words the sources are the rule's -- a function of the weights and u0 alone"""
    n, n_new = 1025, 3075
    poses, attrs = ar.cloud(n, 8)
    attrs["likelihood"]["mean"] = ar.weight_cases(n)["span_1e-6_1"]
    cfg = ar.gladiator_cfg()
    a, b = ar.systematic(poses, attrs, n_new, cfg, 5, 0), ar.systematic(poses, attrs, n_new, cfg, 5, 1)
    assert a[0].tobytes() != b[0].tobytes()
    for step in (0, 1):
        src, _, w, T = ar.sys_sources(attrs["likelihood"]["mean"], n_new, 5, step)
        u0 = ar.sys_u0(5, step)
        C_ = np.cumsum(np.array(w, dtype=object))
        pos = [min(T - 1, int(np.floor((float(j) + u0) * (float(T) / float(n_new))))) for j in range(n_new)]
        assert [int(np.searchsorted(C_.astype(np.uint64), np.uint64(q), side="right")) for q in pos] == list(src)


def test_example_compiles_and_links_without_gpu(ra, tmp_path):
    import subprocess
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "adaptive_resample_cpp_example.cpp")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
