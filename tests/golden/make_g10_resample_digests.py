"""Writes tests/golden/g10_resample_digests.json: sha256 of what the three resamplers, the likelihood statistics and the pose estimate
write on the device, so that a change which only moves their text cannot move a bit unseen (the single-device tests allow 1e-6 on a
perturbed pose: a reordered float expression passes them).

cases()  name -> function(ra, ctx) -> {field: sha256 hex, or an integer}; tests/test_gpu_resample_digests.py recomputes them one by one.
Clouds come from fixed numpy seeds; the noise is non-zero on all six axes.

    gladiator    n = 3000: metrics 0 and 1, steps 0 and 1; champions [1000, 1500) as a shard; n = 1
    residual     3000 -> 3000, 3000 -> 5000, 5 -> 3; slots [1000, 1500) of the first as a shard; `last_draws` beside the digests
    systematic   3000 -> 2000, 3000 -> 5000 (runs of copies: the perturbed branch), 1500 -> 1500, slots [1000, 1500) of 3000 -> 5000 as a
                 shard, 1024 -> 1024 and 1025 -> 1025 (the edge of one scan block)
    stats        {sum, max} for n = 1, 1023, 300007, from the attributes and from the dense weights
    estimate     the pose estimate (three moment passes) of a 3000-particle cloud

Needs a GPU and the built library; the committed file holds the outputs of the kernels as they were BEFORE the resamplers moved into
resample.hip:

    python tests/golden/make_g10_resample_digests.py
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "g10_resample_digests.json")
SEED = 0x5EED0123456789
NOISE = dict(min_noise_tx=0.03, min_noise_ty=0.02, min_noise_tz=0.01, min_noise_roll=0.004, min_noise_pitch=0.005, min_noise_yaw=0.01)
# the tournament's and the systematic resampler's forget rates: the rotation distance is |q| ~ 1, so with the default 0.2 per radian the
# rotation term wins every time and the translation metric never shows; with 0.001 metric 0 lets translation win, metric 1 rotation
FORGET = dict(likelihood_forget_per_meter=0.3, likelihood_forget_per_radian=0.001)
f32 = np.float32


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def cloud(n, seed, weights):
    """n particles in a room-sized box, stamp = index; weights: `uniform` 0.05 .. 1, `skewed` 1e-3 .. 1 (a few particles take many
    copies), `one_heavy` (all 0.1 but the middle one)"""
    from particle_init_ref import euler_to_quat
    from rmcl_amd.types import PARTICLE_ATTRIBUTES, TRANSFORM
    rs = np.random.RandomState(seed)
    v = rs.uniform((-9, -9, 0.2, -0.4, -0.4, -math.pi), (9, 9, 3.0, 0.4, 0.4, math.pi), size=(n, 6)).astype(f32)
    p = np.zeros(n, dtype=TRANSFORM)
    for k, q in zip("xyzw", euler_to_quat(v[:, 3], v[:, 4], v[:, 5])):
        p["R"][k] = q
    for d, k in enumerate("xyz"):
        p["t"][k] = v[:, d]
    p["stamp"] = np.arange(n, dtype=np.uint32)
    a = np.zeros(n, dtype=PARTICLE_ATTRIBUTES)
    a["likelihood"]["sigma"] = rs.uniform(0, 0.1, n)
    a["likelihood"]["n_meas"] = rs.randint(1, 10001, n)
    a["state_sigma"] = rs.uniform(0, 1, (n, 6))
    if weights == "uniform":
        a["likelihood"]["mean"] = rs.uniform(0.05, 1.0, n)
    elif weights == "skewed":
        a["likelihood"]["mean"] = 10.0 ** rs.uniform(-3, 0, n)
    else:
        a["likelihood"]["mean"] = 0.1
        a["likelihood"]["mean"][n // 2] = 1.0
    return p, a


def _outputs(ra, ctx, count):
    from rmcl_amd import types as T
    return ra.DeviceArray(ctx, T.TRANSFORM, count), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, count)


def _gladiator(n, metric, step, first=0, count=None):
    def run(ra, ctx):
        from rmcl_amd import types as T
        poses, attrs = cloud(n, 101, "uniform")
        cnt = n - first if count is None else count
        rs = ra.GladiatorResamplerHip(ctx, seed=SEED)
        rs.config, rs.step = T.gladiator_config(trans_dist_metric=metric, **NOISE, **FORGET), step
        d_pn, d_an = _outputs(ra, ctx, cnt)
        rs.update(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), d_pn, d_an, n, first=first, count=cnt)
        out = {"poses": sha(d_pn.download().tobytes()), "attrs": sha(d_an.download().tobytes())}
        rs.close()
        return out
    return run


def _residual(n, n_new, weights, first=0, count=None):
    def run(ra, ctx):
        from rmcl_amd import types as T
        poses, attrs = cloud(n, 102, weights)
        cnt = n_new - first if count is None else count
        rs = ra.ResidualResamplerHip(ctx, seed=SEED)
        rs.config, rs.step = T.gladiator_config(**NOISE), 1
        d_pn, d_an = _outputs(ra, ctx, cnt)
        rs.update(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), d_pn, d_an, n, n_new, first=first, count=cnt)
        out = {"poses": sha(d_pn.download().tobytes()), "attrs": sha(d_an.download().tobytes()), "last_draws": int(rs.last_draws)}
        rs.close()
        return out
    return run


def _systematic(n, n_new, first=0, count=None):
    def run(ra, ctx):
        from rmcl_amd import types as T
        poses, attrs = cloud(n, 103, "skewed")
        cnt = n_new - first if count is None else count
        rs = ra.AdaptiveResamplerHip(ctx, seed=SEED)
        rs.config, rs.step = T.gladiator_config(**NOISE, **FORGET), 2
        d_pn, d_an = _outputs(ra, ctx, cnt)
        rs.update_systematic(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), d_pn, d_an, n, n_new, first, cnt)
        out = {"poses": sha(d_pn.download().tobytes()), "attrs": sha(d_an.download().tobytes())}
        rs.close()
        return out
    return run


def _stats(n):
    def run(ra, ctx):
        _, attrs = cloud(n, 104, "uniform")
        w = np.ascontiguousarray(attrs["likelihood"]["mean"])
        rs = ra.GladiatorResamplerHip(ctx)
        s = rs.compute_stats(ra.DeviceArray.from_host(ctx, attrs), n)
        d = rs.compute_stats_weights(ra.DeviceArray.from_host(ctx, w), n)
        rs.close()
        return {"attrs": np.array([s["sum"], s["max"]], dtype=f32).tobytes().hex(), "dense": np.array([d["sum"], d["max"]], dtype=f32).tobytes().hex()}
    return run


def _estimate(n):
    def run(ra, ctx):
        poses, attrs = cloud(n, 105, "uniform")
        est = ra.PoseEstimatorHip(ctx)
        e = est.estimate(ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs), n)
        est.close()
        lik = np.array([e["likelihood"][k] for k in ("mean", "sigma", "min", "max")], dtype=np.float64)
        bb = np.concatenate([np.asarray(e["trans_bb_min"], dtype=np.float64), np.asarray(e["trans_bb_max"], dtype=np.float64)])
        return {"pose": e["pose"].tobytes().hex(), "covariance": sha(e["covariance"].tobytes()), "likelihood": lik.tobytes().hex(),
                "trans_bb": bb.tobytes().hex(), "nparticles": int(e["nparticles"])}
    return run


def cases():
    c = {}
    for metric in (0, 1):
        for step in (0, 1):
            c["gladiator_3000_metric%d_step%d" % (metric, step)] = _gladiator(3000, metric, step)
    c["gladiator_3000_shard_1000_500"] = _gladiator(3000, 0, 1, 1000, 500)
    c["gladiator_1"] = _gladiator(1, 0, 0)
    c["residual_3000_3000"] = _residual(3000, 3000, "uniform")
    c["residual_3000_5000"] = _residual(3000, 5000, "uniform")
    c["residual_5_3"] = _residual(5, 3, "one_heavy")
    c["residual_3000_3000_shard_1000_500"] = _residual(3000, 3000, "uniform", 1000, 500)
    c["systematic_3000_2000"] = _systematic(3000, 2000)
    c["systematic_3000_5000"] = _systematic(3000, 5000)
    c["systematic_1500_1500"] = _systematic(1500, 1500)
    c["systematic_3000_5000_shard_1000_500"] = _systematic(3000, 5000, 1000, 500)
    c["systematic_1024_1024"] = _systematic(1024, 1024)
    c["systematic_1025_1025"] = _systematic(1025, 1025)
    for n in (1, 1023, 300007):
        c["stats_%d" % n] = _stats(n)
    c["estimate_3000"] = _estimate(3000)
    return c


if __name__ == "__main__":
    import rmcl_amd as ra
    ctx = ra.Context(0)
    out = {name: fn(ra, ctx) for name, fn in cases().items()}
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases" % (path, len(out)))
