#!/usr/bin/env python
"""what the adaptive particle count costs and what it saves (include/rmclhip.h, "a particle count that follows the posterior";
DESIGN.md 4.10).  Three measurements, variants ALTERNATED call by call, host clock around the synchronous calls:

  1  rmclhip_particles_count_bins at 50 000 and 1 000 000 particles: `even` -- a cloud uniform in a 100 m box, nearly every particle in
     a bin of its own -- and `one` -- every particle in ONE bin: all inserts meet in one word of the table.
  2  rmclhip_resampler_systematic beside rmclhip_resampler_residual (the yardstick: the parent commit's code, which this change does not
     touch) at the same n -> n_new, 50 000 -> 50 000 and 1 000 000 -> 1 000 000, likelihoods uniform in 0.05 .. 1.
  3  the README's C4 shape (100 000 particles x 256 beams, sphere100k): the sensor update (rmclhip_pf_time_update, device events) on a
     converged cloud ~ N(pose, 0.25 m, 5 deg yaw), one rmclhip_resampler_adaptive, the sensor update on the particles it kept.

median [min .. max] of --calls timed calls after --warmup warm-ups.

usage: python tools/adaptive_resample_time.py [--calls 30] [--warmup 5] [--out profiles/adaptive_resample_time.txt]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import synthetic as syn, types as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 1000000])
ap.add_argument("--c4-particles", type=int, default=100000)
ap.add_argument("--c4-beams", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_resample_time.txt"))
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def alternate(variants):
    """{name: sorted us} of --calls timed calls per variant after --warmup warm-ups, the variants alternated call by call"""
    wall = {k: [] for k, _ in variants}
    for it in range(args.warmup + args.calls):
        for k, fn in variants:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                wall[k].append(dt * 1e6)
    return {k: np.sort(np.array(w)) for k, w in wall.items()}


def row(name, w, note=""):
    say("  %-12s %10.1f [%10.1f .. %10.1f]%s" % (name, float(np.median(w)), w[0], w[-1], note))
    return float(np.median(w))


ctx = ra.Context(0)
say("host clock around each synchronous call, us: median [min .. max]; %d timed calls per variant after %d warm-ups, alternated call by call"
    % (args.calls, args.warmup))

# ---- 1: occupied bins -------------------------------------------------------------------------------------
say("1  rmclhip_particles_count_bins (bins 0.5 m / 10 deg, likelihood floor 0.01; includes the likelihood statistics and the table's clear)")
for n in args.sizes:
    even_p, even_a = syn.uniform_particles(n, seed=5, bb_min=(-50, -50, -50, -math.pi, -1.2, -math.pi), bb_max=(50, 50, 50, math.pi, 1.2, math.pi))
    one_p, one_a = syn.uniform_particles(n, seed=6, bb_min=(1.6, -0.9, 0.6, 0.01, 0.01, 0.36), bb_max=(1.9, -0.6, 0.9, 0.16, 0.16, 0.51))
    rs = ra.AdaptiveResamplerHip(ctx)
    d = {k: (ra.DeviceArray.from_host(ctx, p), ra.DeviceArray.from_host(ctx, a)) for k, (p, a) in (("even", (even_p, even_a)), ("one", (one_p, one_a)))}
    got = {k: rs.count_bins(d[k][0], d[k][1], n) for k in d}
    assert got["one"]["bins"] == 1 and got["even"]["bins"] > n // 2, got
    w = alternate([(k, (lambda k=k: rs.count_bins(d[k][0], d[k][1], n))) for k in ("even", "one")])
    say("n = %d particles" % n)
    me = row("even", w["even"], "   %d bins" % got["even"]["bins"])
    mo = row("one", w["one"], "   1 bin")
    say("  one - even = %+.1f us" % (mo - me))
    rs.close()

# ---- 2: systematic beside residual ------------------------------------------------------------------------
say("2  rmclhip_resampler_systematic beside rmclhip_resampler_residual, n -> n (likelihoods uniform in 0.05 .. 1, the gladiator's default noise)")
for n in args.sizes:
    poses, attrs = syn.uniform_particles(n, seed=7, bb_min=(-9, -9, 0.2, -0.2, -0.2, -math.pi), bb_max=(9, 9, 3.0, 0.2, 0.2, math.pi))
    attrs["likelihood"]["mean"] = np.random.RandomState(8).uniform(0.05, 1.0, n)
    attrs["likelihood"]["n_meas"] = 5000
    d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    sysr, resr = ra.AdaptiveResamplerHip(ctx), ra.ResidualResamplerHip(ctx)
    w = alternate([("systematic", lambda: sysr.update_systematic(d_p, d_a, d_pn, d_an, n, n)), ("residual", lambda: resr.update(d_p, d_a, d_pn, d_an, n, n))])
    say("n = %d -> %d particles" % (n, n))
    ms, mr = row("systematic", w["systematic"]), row("residual", w["residual"])
    say("  systematic / residual = %.2f" % (ms / mr))
    sysr.close()
    resr.close()

# ---- 3: a filter step before and after the cloud has shrunk -------------------------------------------------
n, nb = args.c4_particles, args.c4_beams
say("3  sphere100k, %d particles x %d beams: sensor update (device events, ms per update) before and after ONE adaptive resample of a converged cloud" % (n, nb))
v, f = syn.uv_sphere(100000)
hm = ra.import_hip_map(ctx, v, f)
centre = T.transform_from_rpy((0.4, -0.3, 0.1), (0, 0, 0.4))
poses, attrs = syn.converged_particles(n, centre, 0.25, 5.0, seed=42)
dirs = syn.model_directions(syn.model_pf16())
beams = ra.beams_from_points(dirs[np.linspace(0, len(dirs) - 1, nb).astype(int)] * np.float32(6.0))
upd = ra.PCDSensorUpdaterHip(hm)
upd.init()
upd.setInput(beams, T.identity())
d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
d_pn, d_an = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)


def update_ms(dp, da, count):
    upd.time_update(dp, da, count, iters=1)
    return sorted(upd.time_update(dp, da, count, iters=3) for _ in range(5))[2]


before = update_ms(d_p, d_a, n)
d_a = ra.DeviceArray.from_host(ctx, attrs)     # the timing loop above merged its updates into the likelihoods: start again
upd.update(d_p, d_a, n)
rs = ra.AdaptiveResamplerHip(ctx)
t0 = time.perf_counter()
res = rs.update(d_p, d_a, d_pn, d_an, n, n)
first_call = (time.perf_counter() - t0) * 1e6
w = alternate([("adaptive", lambda: rs.update(d_p, d_a, d_pn, d_an, n, n))])
after = update_ms(d_pn, d_an, res["n_particles"])
say("  sensor update, %7d particles: %.4f ms" % (n, before))
say("  adaptive resample: %d bins -> %d particles" % (res["bins"], res["n_particles"]))
row("adaptive", w["adaptive"], "   us per call (first call, buffers allocated: %.1f us)" % first_call)
say("  sensor update, %7d particles: %.4f ms   (%.1f x less)" % (res["n_particles"], after, before / after))
upd.close()
rs.close()
hm.release()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
