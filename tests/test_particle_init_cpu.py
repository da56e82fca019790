"""CPU tests of the particle cloud's initialisation: the numpy restatement (tests/particle_init_ref.py) against the oracle's Philox
and the Random123 known answers, rmclhip_chol6_host (a host function: no device) against the restatement bit for bit, and the
restatement's own statistics -- uniform draws inside their box with the right mean, Gaussians with identity covariance, x = L z
with the covariance L was factored from."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import particle_init_ref as pref

SEEDS = (42, 0xC0FFEE1234567)
N = 65536
RVIZ_COV, COVS = pref.RVIZ_COV, pref.COVS


def test_philox_matches_oracle_and_known_answers(orc):
    rs = np.random.RandomState(1)
    ctr = rs.randint(0, 1 << 32, size=(300, 4), dtype=np.uint64).astype(np.uint32)
    key = rs.randint(0, 1 << 32, size=(300, 2), dtype=np.uint64).astype(np.uint32)
    ctr[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 1], [0xFFFFFFFF, 0, 1, 1]]
    got = pref.philox4x32_10(ctr, key)
    for k in range(len(ctr)):
        assert np.array_equal(got[k], orc.philox4x32_10(ctr[k], key[k])), k
    # Random123 kat_vectors: philox4x32 10
    assert [int(v) for v in pref.philox4x32_10([0, 0, 0, 0], [0, 0])] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in pref.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_init_words_are_a_function_of_the_global_index():
    w = pref.init_words(0, 1001, SEEDS[1], 3)
    assert np.array_equal(w[334:668], pref.init_words(334, 334, SEEDS[1], 3))
    assert not np.array_equal(w, pref.init_words(0, 1001, SEEDS[1], 4))
    assert not np.array_equal(w, pref.init_words(0, 1001, SEEDS[0], 3))
    # the counter's last word is 1: none of the resamplers' streams (last word 0)
    key = np.array([SEEDS[1] & 0xFFFFFFFF, SEEDS[1] >> 32], dtype=np.uint32)
    assert np.array_equal(w[5, :4], pref.philox4x32_10([5, 3, 0, 1], key))
    assert np.array_equal(w[5, 4:], pref.philox4x32_10([5, 3, 1, 1], key)[:2])
    assert np.array_equal(pref.init_words(0xFFFFFFFF, 1, 7, 0)[0, :4], pref.philox4x32_10([0xFFFFFFFF, 0, 0, 1], [7, 0]))


@pytest.mark.parametrize("name", ["full", "rviz", "rank3"])
def test_chol6_host_gives_the_restatement_bits(ra, name):
    cov = COVS[name]
    L_ref, err_ref = pref.chol6(cov)
    L, err = ra.pf.chol6(cov)
    assert L.dtype == np.float32 and L.tobytes() == L_ref.tobytes()
    assert err == err_ref and np.isfinite(err) and err < 1e-8
    assert np.array_equal(np.triu(L, 1), np.zeros((6, 6), np.float32))
    assert np.abs(L.astype(np.float64) @ L.astype(np.float64).T - cov).max() < 1e-7
    if name == "rviz":
        assert [j for j in range(6) if not L[:, j].any()] == [2, 3, 4]
        assert L[0, 0] == np.float32(0.5) and L[1, 1] == np.float32(0.5) and L[5, 5] == np.float32(np.sqrt(0.0685))
    if name == "rank3":
        assert sum(1 for j in range(6) if not L[:, j].any()) == 3
    # an asymmetric input is symmetrised first
    skew = cov.copy()
    skew[0, 1] += 0.01
    skew[1, 0] -= 0.01
    assert ra.pf.chol6(skew)[0].tobytes() == L_ref.tobytes()


def test_chol6_host_refusals(ra):
    L = ra._capi.lib()
    out, err = np.full(36, 7.0, np.float32), C.c_double(5.0)

    def call(cov):
        cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(36)
        return L.rmclhip_chol6_host(cov.ctypes.data, out.ctypes.data, C.byref(err))

    neg = COVS["full"].copy()
    neg[2, 2] = -0.01
    assert call(neg) == ra._capi.ERR_INVALID and b"positive semidefinite" in L.rmclhip_last_error()
    with pytest.raises(ValueError):
        pref.chol6(neg)
    indefinite = np.eye(6)
    indefinite[0, 1] = indefinite[1, 0] = 2.0
    assert call(indefinite) == ra._capi.ERR_INVALID and b"positive semidefinite" in L.rmclhip_last_error()
    nan = COVS["full"].copy()
    nan[4, 1] = np.nan
    assert call(nan) == ra._capi.ERR_INVALID and b"non-finite" in L.rmclhip_last_error()
    inf = COVS["full"].copy()
    inf[0, 0] = np.inf
    assert call(inf) == ra._capi.ERR_INVALID
    assert np.all(out == 7.0)                                    # a refusal leaves the output alone
    assert L.rmclhip_chol6_host(None, out.ctypes.data, None) == ra._capi.ERR_INVALID
    assert call(np.zeros((6, 6))) == ra._capi.OK and not out.any() and err.value == 0.0   # no variance at all: the zero factor
    with pytest.raises(ra.RmclHipError):
        ra.pf.chol6(neg)


@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_draws_stay_in_the_box_with_the_right_mean(seed):
    w = pref.init_words(0, N, seed, 0)
    for lo, hi in (((-50, -50, 0, 0, 0, -np.pi), (50, 50, 0, 0, 0, np.pi)), ((-9, -7, 0.2, -0.2, -0.1, -1.0), (9, 8, 3.0, 0.2, 0.3, 2.0))):
        lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        v = pref.uniform_values(w, lo, hi)
        assert v.dtype == np.float32 and np.all(v >= lo32[None, :]) and np.all(v <= hi32[None, :])
        for d in range(6):
            if lo32[d] == hi32[d]:
                assert np.all(v[:, d] == lo32[d])                # lo == hi gives exactly lo
                continue
            se = (float(hi32[d]) - float(lo32[d])) / np.sqrt(12.0 * N)
            assert abs(v[:, d].astype(np.float64).mean() - (float(lo32[d]) + float(hi32[d])) / 2.0) < 5.0 * se, d


@pytest.mark.parametrize("seed", SEEDS)
def test_gaussians_and_their_deformation(seed):
    z = pref.gaussians(pref.init_words(0, N, seed, 0)).astype(np.float64)
    assert np.isfinite(z).all()
    assert np.abs(z.mean(0)).max() < 5.0 / np.sqrt(N)
    assert np.abs(z.T @ z / N - np.eye(6)).max() < 8.0 / np.sqrt(N)
    for name in ("rviz", "full"):
        cov = COVS[name]
        L, _ = pref.chol6(cov)
        x = pref.deform(L, z.astype(np.float32)).astype(np.float64)
        assert np.abs(x.T @ x / N - cov).max() < 8.0 * np.diag(cov).max() / np.sqrt(N), name
        if name == "rviz":
            assert not x[:, 2:5].any() and not np.signbit(x[:, 2:5]).any()   # no variance: +0 exactly


def test_cloud_restatement_shapes_and_attributes():
    p, a = pref.init_uniform(5, 300, (-50, -50, 0, 0, 0, -np.pi), (50, 50, 0, 0, 0, np.pi), 42, 1)
    assert len(p) == len(a) == 300 and not p["stamp"].any()
    assert np.all(a["likelihood"]["mean"] == 1.0) and not a["likelihood"]["sigma"].any() and not a["likelihood"]["n_meas"].any()
    assert not a["state_sigma"].any()
    q = np.stack([p["R"][k] for k in "xyzw"], 1).astype(np.float64)
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() < 1e-6
    assert not p["R"]["x"].any() and not p["R"]["y"].any() and not p["t"]["z"].any()   # roll = pitch = 0, z = 0
    from rmcl_amd import types as T
    p2, _ = pref.init_pose(0, 300, T.identity(), RVIZ_COV, 42, 0)
    assert not p2["t"]["z"].any() and not p2["R"]["x"].any() and not p2["R"]["y"].any()
    viz = pref.pack_visualization(p, a)
    assert list(viz) == ["x", "y", "z", "likelihood", "likelihood_sigma", "likelihood_n_meas", "badness"]
    assert np.all(viz["badness"] == 1.0)                         # mean 1, sigma 0, n_meas 0: unc = 1


def test_cpp_example_compiles_and_links_without_gpu(ra, tmp_path):
    """examples/particle_init_cpp_example.cpp against the adapters, the way tests/test_cpp_adapters.py compiles the others"""
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "particle_init_cpp_example.cpp")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
