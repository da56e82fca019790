"""One sharded handle whose cloud changes size, and what the create functions refuse.

The sharded filter's buffers are grow-only and shared between clouds of different sizes: shard buffers hold cap = ceil(n / world)
records, the gathered and padded ones cap * world.  The other sharded tests run one size per handle; here ONE handle is fed sizes at
the partition's edges (ragged and even at the same cap, shrinking, growing after the pad buffers exist, the empty cloud), and every
result is held to the single-device bytes.  Loopback communicators only: ranks share device 0.

The device lists of rmclhip_comm_create, rmclhip_comm_create_loopback and rmclhip_rcc_sharded_create: what each refuses, and the
differences between them (duplicates, what a null list means)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 11
_refs = {}


@pytest.fixture(scope="module")
def single(ra, ctx, meshes):
    """the single-device objects every size is compared against, on the cube"""
    from rmcl_amd import synthetic as syn
    v, f = meshes("cube")
    hm = ra.import_hip_map(ctx, v, f)
    beams = ra.beams_from_points(syn.model_directions(syn.model_pf16())[::16] * np.float32(6.0))
    assert len(beams) == 16
    Tsb = syn.tsb_offset()
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.init()
    upd.setInput(beams, Tsb)
    s = {"upd": upd, "beams": beams, "Tsb": Tsb, "gladiator": ra.GladiatorResamplerHip(ctx, seed=SEED),
         "residual": ra.ResidualResamplerHip(ctx, seed=SEED), "est": ra.PoseEstimatorHip(ctx)}
    yield s
    for k in ("upd", "gladiator", "residual", "est"):
        s[k].close()


def _cloud(n):
    from rmcl_amd import synthetic as syn
    poses, attrs = syn.uniform_particles(n, seed=100 + n, bb_min=(-4, -4, -2, 0, 0, -3.14), bb_max=(4, 4, 2, 0, 0, 3.14))
    attrs["likelihood"]["n_meas"] = np.random.RandomState(n).randint(0, 300, n)
    return poses, attrs


def _reference(ra, ctx, single, n, resampler, step):
    """the single-device update, {sum, max}, estimate and resampled cloud of _cloud(n), computed once per (n, resampler, step)"""
    from rmcl_amd import types as T
    key = (n, resampler, step)
    if key not in _refs:
        poses, attrs = _cloud(n)
        d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        single["upd"].update(d_p, d_a)
        updated = d_a.download()
        stats = single["gladiator"].compute_stats(d_a, n)
        estimate = single["est"].estimate(d_p, d_a, n)
        d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
        rs = single[resampler]
        rs.step = step
        rs.update(d_p, d_a, d_pn, d_an, n)
        _refs[key] = {"poses": poses, "attrs": attrs, "updated": updated, "stats": stats, "estimate": estimate,
                      "resampled": (d_pn.download(), d_an.download())}
        for d in (d_p, d_a, d_pn, d_an):
            d.free()
    return _refs[key]


def _feed(ra, ctx, single, sh, n, position, estimate=False):
    """set_particles, update, resampling of a cloud of n on the live handle `sh`; gladiator at even positions, residual at odd ones"""
    resampler = "residual" if position % 2 else "gladiator"
    if n == 0:
        from rmcl_amd import types as T
        sh.set_particles(np.zeros(0, T.TRANSFORM), np.zeros(0, T.PARTICLE_ATTRIBUTES))
        assert len(sh.update(single["beams"], single["Tsb"])) == 0
        assert sh.stats() == {"sum": 0.0, "max": 0.0}
        sh.resample(seed=SEED, step=position, residual=(resampler == "residual"))
        p, a = sh.download()
        assert len(p) == 0 and len(a) == 0
        return
    ref = _reference(ra, ctx, single, n, resampler, position)
    sh.set_particles(ref["poses"], ref["attrs"])
    sh.update(single["beams"], single["Tsb"])
    p, a = sh.download()
    assert p.tobytes() == ref["poses"].tobytes() and a.tobytes() == ref["updated"].tobytes(), n
    for rank in range(sh.world):
        assert np.array_equal(sh.weights(rank), ref["updated"]["likelihood"]["mean"]), (n, rank)
    st = sh.stats()
    assert st["sum"] == ref["stats"]["sum"] and st["max"] == ref["stats"]["max"], (n, st, ref["stats"])
    if estimate:
        _check_estimate(sh.pose_estimate(), ref["estimate"], sh.world, n)
    sh.resample(seed=SEED, step=position, residual=(resampler == "residual"))
    p, a = sh.download()
    assert p.tobytes() == ref["resampled"][0].tobytes() and a.tobytes() == ref["resampled"][1].tobytes(), (n, resampler)


def _check_estimate(got, ref, world, n):
    """the sharded estimate against the single-device estimator's.  One rank: bit for bit, as include/rmclhip.h states it and
    tests/test_gpu_hypotheses.py compares the two (the same kernels, the same host code, no sum across ranks).  Several ranks: every
    moment sum is all-reduced over the ranks' partial sums, i.e. added in another order than one device adds it, so what comes out of
    sums may move in its last bits (on these clouds the bitwise comparison fails on the code as it was before this file existed:
    world 8, n = 5).  Then: minima, maxima and counts are exact; the likelihood's mean and sigma are doubles from sums of at most nine
    doubles, 1e-9 relative as test_gpu_hypotheses.py bounds them (the reordering itself is worth n * 2^-53); pose and covariance as
    tests/test_gpu_distributed.py bounds a reordered all-reduce: the float32 translation within 1e-6, the covariance within 1e-9
    relative + 1e-12; the float32 quaternion within 1e-6 up to sign."""
    if world == 1:
        from test_gpu_hypotheses import _same_estimate
        assert _same_estimate(got, ref), n
        return
    assert got["nparticles"] == ref["nparticles"] == n
    for k in ("trans_bb_min", "trans_bb_max"):
        assert got[k].tobytes() == ref[k].tobytes(), (n, k)
    for k in ("min", "max"):
        assert got["likelihood"][k] == ref["likelihood"][k], (n, k)
    for k in ("mean", "sigma"):
        print("n", n, "likelihood", k, got["likelihood"][k], ref["likelihood"][k])
        assert abs(got["likelihood"][k] - ref["likelihood"][k]) <= 1e-9 * abs(ref["likelihood"][k]), (n, k)
    qa = np.array([got["pose"]["R"][k] for k in "xyzw"], np.float64)
    qb = np.array([ref["pose"]["R"][k] for k in "xyzw"], np.float64)
    ta = np.array([got["pose"]["t"][k] for k in "xyz"], np.float64)
    tb = np.array([ref["pose"]["t"][k] for k in "xyz"], np.float64)
    print("n", n, "q", qa, qb, "t", ta, tb, "covariance: largest difference", np.abs(got["covariance"] - ref["covariance"]).max())
    assert min(np.linalg.norm(qa - qb), np.linalg.norm(qa + qb)) < 1e-6, n
    assert np.allclose(ta, tb, rtol=0, atol=1e-6), n
    assert np.allclose(got["covariance"], ref["covariance"], rtol=1e-9, atol=1e-12), n


def test_one_handle_many_sizes_on_three_ranks(ra, ctx, meshes, single):
    """world 3, in this order: 1000 (ragged, cap 334), 1002 (even, the SAME cap with a larger n_total: the dense weight vector must have
    been sized by cap * world), 7 (shrink, ragged), 2049 (grow, even, after the pad buffers exist), 2048 (ragged at the same cap: the
    pad buffers must have grown), 0 (the empty cloud), 6 (after it)"""
    v, f = meshes("cube")
    sh = ra.ShardedParticleFilterHip(v, f, devices=(0, 0, 0), loopback=True)
    for position, n in enumerate((1000, 1002, 7, 2049, 2048, 0, 6)):
        _feed(ra, ctx, single, sh, n, position)
    sh.close()


def test_empty_ranks_on_eight_ranks(ra, ctx, meshes, single):
    """world 8: 5 particles (three ranks empty), then 8, then 9; also the pose estimate against the single-device estimator's
    (_check_estimate) -- and the same sizes on one rank, where that comparison is bit for bit"""
    v, f = meshes("cube")
    for world in (8, 1):
        sh = ra.ShardedParticleFilterHip(v, f, devices=(0,) * world, loopback=True)
        for position, n in enumerate((5, 8, 9)):
            _feed(ra, ctx, single, sh, n, position, estimate=True)
        sh.close()


# ---- device lists ----------------------------------------------------------------------------------------------------------------------
def _ints(values):
    return (C.c_int * max(1, len(values)))(*values)


def _rccl_mapped():
    with open("/proc/self/maps") as fh:
        return "librccl" in fh.read()


def test_device_lists(ra, ctx, meshes):
    """(A refused list must leave nothing behind, the HIP runtime's error state included.  When rmclhip_comm_create_loopback still
    checked its list entry by entry, its clean-up made the refused index the current device; hipErrorInvalidDevice then stayed
    behind, and the next call that asks the runtime for its last error -- the rmclhip_rcc_sharded_create with (0, 0) below --
    failed with "invalid device ordinal".)"""
    from rmcl_amd import _capi
    L = _capi.lib()
    count = C.c_int(0)
    assert L.hipGetDeviceCount(C.byref(count)) == 0 and count.value >= 1     # (the HIP runtime librmclhip.so is linked against)
    v, f = meshes("cube")
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1, 3)
    vp, fp = v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    creators = {
        "comm_create": lambda devs, ndev, out: L.rmclhip_comm_create(devs, ndev, C.byref(out)),
        "comm_create_loopback": lambda devs, ndev, out: L.rmclhip_comm_create_loopback(devs, ndev, C.byref(out)),
        "rcc_sharded_create": lambda devs, ndev, out: L.rmclhip_rcc_sharded_create(devs, ndev, vp, len(v), fp, len(f), C.byref(out)),
    }
    refused = {"ndev 0": ([0], 0), "ndev 65": ([0] * 65, 65), "minus one": ([-1], 1), "device count": ([count.value], 1),
               "device count behind a valid entry": ([0, count.value], 2)}
    L.hipGetLastError()                                                      # (whatever earlier tests left behind)
    for name, create in creators.items():
        for what, (devs, ndev) in refused.items():
            out = C.c_void_p()
            assert create(_ints(devs), ndev, out) == _capi.ERR_INVALID, (name, what)
            assert out.value is None, (name, what)
            assert L.hipPeekAtLastError() == 0, (name, what)
            assert L.rmclhip_last_error().decode().startswith(name + ":"), (name, what, L.rmclhip_last_error())

    # a device twice: refused by the RCCL communicator -- before the library is looked for --, accepted by the other two
    rccl_before = _rccl_mapped()
    out = C.c_void_p()
    assert L.rmclhip_comm_create(_ints([0, 0]), 2, C.byref(out)) == _capi.ERR_INVALID and out.value is None
    assert L.rmclhip_last_error().decode() == "comm_create: duplicate device"
    assert rccl_before or not _rccl_mapped()
    out = C.c_void_p()
    _capi.check(L.rmclhip_comm_create_loopback(_ints([0, 0]), 2, C.byref(out)))
    assert L.rmclhip_comm_size(out) == 2
    L.rmclhip_comm_destroy(out)
    out = C.c_void_p()
    _capi.check(L.rmclhip_rcc_sharded_create(_ints([0, 0]), 2, vp, len(v), fp, len(f), C.byref(out)))
    assert L.rmclhip_rcc_sharded_size(out) == 2
    L.rmclhip_rcc_sharded_destroy(out)

    # no list: two loopback ranks, both on device 0 (0 .. ndev - 1 would be refused on a machine with one device); create, use, destroy
    comm = C.c_void_p()
    _capi.check(L.rmclhip_comm_create_loopback(None, 2, C.byref(comm)))
    assert L.rmclhip_comm_size(comm) == 2
    n_ranks, is_rccl = C.c_uint32(0), C.c_int(1)
    _capi.check(L.rmclhip_comm_collective_ranks(comm, C.byref(n_ranks), C.byref(is_rccl)))
    assert (n_ranks.value, is_rccl.value) == (2, 0)
    h = C.c_void_p()
    _capi.check(L.rmclhip_pf_sharded_create(comm, vp, len(v), fp, len(f), C.byref(h)))
    from rmcl_amd import types as T
    lo, hi = np.array([-4, -4, -2, 0, 0, -3], np.float32), np.array([4, 4, 2, 0, 0, 3], np.float32)
    _capi.check(L.rmclhip_pf_sharded_init_uniform(h, 9, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), 5, 0))
    p, a = np.zeros(9, T.TRANSFORM), np.zeros(9, T.PARTICLE_ATTRIBUTES)
    _capi.check(L.rmclhip_pf_sharded_download(h, p.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)))
    L.rmclhip_pf_sharded_destroy(h)
    L.rmclhip_comm_destroy(comm)
    one = ra.ShardedParticleFilterHip(v, f, devices=(0,), loopback=True)     # the same cloud on one rank
    one.init_uniform(9, lo, hi, 5)
    p1, a1 = one.download()
    one.close()
    assert p.tobytes() == p1.tobytes() and a.tobytes() == a1.tobytes()
    for k in "xyz":
        assert np.all(np.abs(p["t"][k]) <= 4.0)
