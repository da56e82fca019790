#!/usr/bin/env python
"""pose hypotheses (rmclhip_particles_pose_hypotheses, max_hypotheses = 8) on three clouds at 50 000 and 1 000 000 particles:

  converged   pose + covariance around one pose: a few bins, one cluster
  bimodal     two such clouds, 2 : 1, six metres apart
  uniform     uniform over a 100 m box (x, y, yaw): nearly a bin and a cluster per particle

Per cloud, ALTERNATED call by call:

  H    PoseEstimatorHip.hypotheses                                  (statistics, bin table, components, ranking, 3 moment passes per hypothesis)
  E    ShardedParticleFilterHip(devices=(0,)).pose_estimate          (the one estimate a caller had: 3 moment passes over the cloud)
  E1   PoseEstimatorHip.estimate                                    (the same passes through the single-device entry point)

and, once per cloud (host clock, one call), what a caller could do without the feature: download of the cloud + the numpy / Python
restatement tests/hypotheses_ref.py -- left out for the uniform cloud of 1 000 000 particles, where its ~364 dictionary look-ups per
bin take minutes.  Host clock around every call (each ends in a synchronise); median of --calls timed calls after --warmup warm-ups.

usage: python tools/pose_hypotheses_time.py [--calls 20] [--warmup 5] [--out profiles/pose_hypotheses_time.txt]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import synthetic as syn, types as T  # noqa: E402
import adaptive_ref as ar  # noqa: E402
import hypotheses_ref as hr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 1000000])
ap.add_argument("--host-limit", type=int, default=100000, help="largest uniform cloud the host restatement is timed on")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_hypotheses_time.txt"))
args = ap.parse_args()
assert args.calls >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"

ctx = ra.Context(0)
v, f = syn.cube_room()
sharded = ra.ShardedParticleFilterHip(v, f, devices=(0,))
est = ra.PoseEstimatorHip(ctx)
COV = np.diag([0.04, 0.04, 0.0, 0.0, 0.0, 0.01])
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def make_cloud(kind, n):
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    if kind == "uniform":
        ra.init_particles_uniform(ctx, d_p, d_a, (-50, -50, 0, 0, 0, -math.pi), (50, 50, 0, 0, 0, math.pi), 42, 0)
        return d_p.download(), d_a.download()
    ra.init_particles_pose(ctx, d_p, d_a, T.transform_from_rpy((1.5, -2.0, 0.0), (0.0, 0.0, 0.4)), COV, 42, 0)
    poses, attrs = d_p.download(), d_a.download()
    if kind == "bimodal":
        ra.init_particles_pose(ctx, d_p, d_a, T.transform_from_rpy((7.5, -2.0, 0.0), (0.0, 0.0, -2.7)), COV, 42, 1)
        other = d_p.download()
        third = np.arange(n) % 3 == 0
        poses[third] = other[third]
    return poses, attrs


say("device: %s   %d timed calls per variant after %d warm-ups, alternated within {H, E, E1}; ms, host clock, median [min .. max]"
    % (ctx.device_name(), args.calls, args.warmup))
for n in args.sizes:
    for kind in ("converged", "bimodal", "uniform"):
        poses, attrs = make_cloud(kind, n)
        attrs["likelihood"]["mean"] = np.random.RandomState(n).uniform(0.2, 1.0, n).astype(np.float32)
        d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        sharded.set_particles(poses, attrs)
        res = {}
        variants = (("H", lambda: res.__setitem__("h", est.hypotheses(d_p, d_a, n, 8))), ("E", lambda: sharded.pose_estimate()),
                    ("E1", lambda: est.estimate(d_p, d_a, n)))
        wall = {k: [] for k, _ in variants}
        for it in range(args.warmup + args.calls):
            for k, fn in variants:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    wall[k].append(dt * 1e3)
        h = res["h"]
        say("n = %d, %s: %d clusters, weight shares of the first hypotheses %s" % (
            n, kind, h["n_clusters"], ", ".join("%.4f" % x["weight_share"] for x in h["hypotheses"][:3])))
        for k, _ in variants:
            w = np.sort(np.array(wall[k]))
            say("  %-3s %9.3f [%9.3f .. %9.3f]" % (k, float(np.median(w)), w[0], w[-1]))
        if kind != "uniform" or n <= args.host_limit:
            t0 = time.perf_counter()
            hp, ha = d_p.download(), d_a.download()
            t1 = time.perf_counter()
            ref = hr.hypotheses(hp, ha, ar.Kld(), 8)
            t2 = time.perf_counter()
            assert ref["n_clusters"] == h["n_clusters"] and [x["key_min"] for x in ref["hypotheses"]] == [x["key_min"] for x in h["hypotheses"]]
            say("  host alternative, one call: download %.1f + restatement %.1f" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        else:
            say("  host alternative: not run at this size")
        d_p.free()
        d_a.free()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
