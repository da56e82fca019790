"""CPU tests of the pose hypotheses' reference (tests/hypotheses_ref.py) on clouds one can count by hand -- the clusters, their ids,
bins, particles and order are written out -- and of the host-side factoring: the argument refusals of the new entry points that
need no device."""
import ctypes as C
import itertools

import numpy as np

import adaptive_ref as ar
import hypotheses_ref as hr

W1 = 1 << 24                                                # the integer weight of a particle with the maximum likelihood
KEY_BASE = 0x5224a0017ffa003                                # (3, -2, 1, 18, 17, 5): 8195 | 8190 << 14 | 8193 << 28 | 18 << 42 | 17 << 49 | 5 << 56


def _clusters(poses, attrs, p, max_h=8):
    r = hr.hypotheses(poses, attrs, p, max_h, estimates=False)
    assert [(h["key_min"], h["weight"], h["n_bins"], h["nparticles"]) for h in r["hypotheses"]] == r["clusters"][:max_h]
    return r


def test_key_packing_and_last_index():
    assert hr.pack_keys([hr.BASE]) == [KEY_BASE] == [8195 | 8190 << 14 | 8193 << 28 | 18 << 42 | 17 << 49 | 5 << 56]
    assert hr.unpack_key(KEY_BASE) == (8195, 8190, 8193, 18, 17, 5)
    assert hr.pack_keys([(0, 0, 0, 0, 0, 0)]) == [8192 | 8192 << 14 | 8192 << 28]          # the ignored dimensions' constant
    assert hr.last_index(0.17453292) == 36 and hr.last_index(1.0) == 6 and hr.last_index(0.05) == 125 and hr.last_index(0.0) == 0
    # the sliver: with the default width +pi alone has index 36, the angles just below it 35
    p, a = hr.exact_pi_particle(5)
    assert ar.bin_tuples(p, a, hr.kld())[1][0, 5] == 36
    below, _ = hr.at_bins([(0, 0, 0, 18, 17, 35)], 0)
    assert ar.bin_tuples(below, a, hr.kld())[1][0, 5] == 35


def test_two_blobs():
    poses, attrs, p, _ = hr.two_blobs(63)
    hr.assert_margin(poses, attrs, p)
    r = _clusters(poses, attrs, p)
    # the upper blob (z index 3) holds 42 of the 63 particles and comes first; each id is the blob's corner (0, -3, z)
    assert r["n_clusters"] == 2
    assert r["clusters"] == [(0x5224a0037ff6000, 42 * W1, 9, 42), (0x5224a0017ff6000, 21 * W1, 9, 21)]
    assert r["total"] == 63 * W1 and [h["weight_share"] for h in r["hypotheses"]] == [42.0 / 63.0, 21.0 / 63.0]
    assert np.array_equal(r["labels"], np.where(np.arange(63) % 3 != 0, 0, 1))


def test_diagonal_touch_and_gap():
    b = np.array(hr.BASE)
    poses, attrs = hr.at_bins(hr.rep(10, [b, b + 1]), 3)
    r = _clusters(poses, attrs, hr.kld())
    assert r["clusters"] == [(KEY_BASE, 10 * W1, 2, 10)] and (r["labels"] == 0).all()
    poses, attrs = hr.at_bins(hr.rep(10, [b, b + (2, 1, 1, 1, 1, 1)]), 3)
    r = _clusters(poses, attrs, hr.kld())
    assert r["clusters"] == [(KEY_BASE, 5 * W1, 1, 5), (0x6244e0027ffe005, 5 * W1, 1, 5)]      # a tie: ascending id
    assert np.array_equal(r["labels"], np.arange(10) % 2)


def test_order_and_cut():
    poses, attrs, p = hr.five_clusters(30)
    r = _clusters(poses, attrs, p, 2)
    # x indices -6, -3, 0, 3, 6 with 10, 8, 6, 4, 2 particles
    assert r["n_clusters"] == 5 and len(r["hypotheses"]) == 2
    assert r["clusters"] == [(0x5224a0017ff9ffa, 10 * W1, 1, 10), (0x5224a0017ff9ffd, 8 * W1, 1, 8), (0x5224a0017ffa000, 6 * W1, 1, 6),
                             (KEY_BASE, 4 * W1, 1, 4), (0x5224a0017ffa006, 2 * W1, 1, 2)]
    share = np.repeat(np.arange(5), [5, 4, 3, 2, 1])[np.arange(30) % 15]
    assert np.array_equal(r["labels"], np.where(share < 2, share, hr.NONE))
    # a likelihood below the floor leaves the particle out of everything
    attrs["likelihood"]["mean"][0] = 0.005
    r = _clusters(poses, attrs, p, 2)
    assert r["clusters"][0] == (0x5224a0017ff9ffa, 9 * W1, 1, 9) and r["labels"][0] == hr.NONE and r["total"] == 29 * W1


def test_yaw_wrap():
    poses, attrs, p, exact = hr.wrap_case(8, 5, 0.17453292, (34, 35, 0, 1), True)
    hr.assert_margin(poses, attrs, p, exact)
    r = _clusters(poses, attrs, p)
    # yaw indices 34, 35, 36 (+pi alone), 0, 1: one cluster, named by its bin with yaw index 0
    assert r["clusters"] == [(0x244a0008002000, 9 * W1, 5, 9)]
    poses, attrs, p, exact = hr.wrap_case(8, 5, 0.17453292, (33, 34, 1, 2), False)
    r = _clusters(poses, attrs, p)
    assert r["clusters"] == [(0x1244a0008002000, 4 * W1, 2, 4), (0x21244a0008002000, 4 * W1, 2, 4)]
    # the rule, field by field: 35 and 0 are neighbours, 34 and 0 are not, 36 and 0 are; pitch does not wrap
    k = hr.kld()
    f = lambda **kw: tuple(kw.get(n, 5) for n in ("x", "y", "z", "roll", "pitch", "yaw"))
    assert hr.adjacent(f(yaw=35), f(yaw=0), k) and hr.adjacent(f(yaw=36), f(yaw=0), k) and not hr.adjacent(f(yaw=34), f(yaw=0), k)
    assert hr.adjacent(f(roll=35), f(roll=0), k) and not hr.adjacent(f(pitch=35), f(pitch=0), k) and not hr.adjacent(f(x=35), f(x=0), k)


def test_components_equal_the_adjacency_rule_on_random_bins():
    """the neighbour enumeration of the reference against the rule itself, pair by pair"""
    for name, (poses, attrs, p) in hr.rnd_cases(257).items():
        counted, tup = ar.bin_tuples(poses, attrs, p)
        keys = sorted(set(hr.pack_keys(tup[counted])))
        root = hr.components(keys, p)
        parent = {k: k for k in keys}

        def find(k):
            while parent[k] != k:
                k = parent[k]
            return k
        for a, b in itertools.combinations(keys, 2):
            if hr.adjacent(hr.unpack_key(a), hr.unpack_key(b), p):
                ra_, rb = find(a), find(b)
                if ra_ != rb:
                    parent[max(ra_, rb)] = min(ra_, rb)
        assert all(root[k] == find(k) for k in keys), name


def test_entry_points_refuse_bad_arguments_without_a_device(ra):
    L = ra._capi.lib()
    est = ra._capi.PoseEstimate()
    est.n_particles = 7
    one = C.c_void_p(16)                                    # never dereferenced: every call below is refused before any device work
    assert L.rmclhip_particles_pose_estimate(None, one, one, 5, 5, C.byref(est)) == ra._capi.ERR_INVALID
    assert b"particles_pose_estimate: null" in L.rmclhip_last_error()
    assert L.rmclhip_particles_pose_estimate(one, one, one, 5, 5, None) == ra._capi.ERR_INVALID
    for n, n_ind in ((0, 5), (5, 0)):
        assert L.rmclhip_particles_pose_estimate(one, one, one, n, n_ind, C.byref(est)) == ra._capi.ERR_INVALID
        assert b"no particles" in L.rmclhip_last_error() and est.n_particles == 0
    est.n_particles = 7
    assert L.rmclhip_particles_pose_estimate(one, None, one, 5, 5, C.byref(est)) == ra._capi.ERR_INVALID
    assert b"null particle buffers" in L.rmclhip_last_error() and est.n_particles == 0
    out = (ra._capi.PoseHypothesis * 64)()
    n_out, n_cl = C.c_uint32(9), C.c_uint32(9)
    kld = ra.kld_params()
    args = lambda k, m: (one, one, one, 5, C.byref(k), m, out, C.byref(n_out), C.byref(n_cl), None)
    for m in (0, 65):
        assert L.rmclhip_particles_pose_hypotheses(*args(kld, m)) == ra._capi.ERR_INVALID
        assert b"max_hypotheses" in L.rmclhip_last_error() and n_out.value == 0 and n_cl.value == 0
    for bad in (dict(bin_xyz=(0.5, -1.0, 0.5)), dict(bin_rpy=(0.01, 0.2, 0.2)), dict(min_likelihood_rel=1.5)):
        assert L.rmclhip_particles_pose_hypotheses(*args(ra.kld_params(**bad), 8)) == ra._capi.ERR_INVALID
        assert b"particles_pose_hypotheses" in L.rmclhip_last_error()
    assert L.rmclhip_particles_pose_hypotheses(None, one, one, 5, C.byref(kld), 8, out, C.byref(n_out), C.byref(n_cl), None) == ra._capi.ERR_INVALID
    assert L.rmclhip_particles_pose_hypotheses(one, one, one, 5, C.byref(kld), 8, None, C.byref(n_out), C.byref(n_cl), None) == ra._capi.ERR_INVALID
    n_out.value = n_cl.value = 9                            # n == 0: OK, zeros, nothing touched
    assert L.rmclhip_particles_pose_hypotheses(one, None, None, 0, C.byref(kld), 8, out, C.byref(n_out), C.byref(n_cl), None) == ra._capi.OK
    assert n_out.value == 0 and n_cl.value == 0
    assert L.rmclhip_pf_sharded_pose_hypotheses(None, C.byref(kld), 8, out, C.byref(n_out), C.byref(n_cl)) == ra._capi.ERR_INVALID
    assert ra.PoseEstimatorHip is ra.pf.PoseEstimatorHip and hasattr(ra.ShardedParticleFilterHip, "pose_hypotheses")


def test_cpp_example_compiles_and_links_without_gpu(ra, tmp_path):
    import subprocess
    from test_cpp_adapters import _build
    exe = _build(tmp_path, "pose_hypotheses_cpp_example.cpp")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
