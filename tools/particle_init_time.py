#!/usr/bin/env python
"""creating a particle cloud on the device, and packing its visualisation channels there, against what a caller had before either
existed.  For 50 000 particles (the reference's default for both initialisations), 100 000 (config C4) and 1 000 000 (C5 on one device),
the device variants ALTERNATED call by call among themselves, then the host variants among themselves:

  U    rmclhip_particles_init_uniform                     (the reference's default box)
  P    rmclhip_particles_init_pose                        (RViz's /initialpose covariance)
  V    rmclhip_particles_pack_visualization to the host   (28 B per particle cross the bus)
  hU   what a caller had: synthetic.uniform_particles on the host + two DeviceArray.from_host uploads (68 B per particle)
  hV   what a caller had: download of poses and attributes (68 B per particle) + the channel arithmetic in numpy

Two clocks per device variant: the host clock around the call (every call ends in a synchronise) and the two HIP events the library
puts around what the call enqueues (rmclhip_debug_particles_timing, include/rmclhip_lab.h); the host variants have the host clock only.
Median of --calls timed calls after --warmup warm-ups.  Bytes per particle over the event time give the achieved store / load rate.

usage: python tools/particle_init_time.py [--calls 25] [--warmup 5] [--out profiles/particle_init_time.txt]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/particle_init_time.py --calls 10     (kernel times: k_particles_*)"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import _capi, synthetic as syn, types as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 100000, 1000000])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "particle_init_time.txt"))
args = ap.parse_args()
assert args.calls >= 20 and args.warmup >= 5, "at least 20 timed calls after 5 warm-ups"

ctx = ra.Context(0)
L = _capi.lib()
_capi.check(L.rmclhip_debug_particles_timing(ctx.handle, 1, None))
LO, HI = (-50, -50, 0, 0, 0, -math.pi), (50, 50, 0, 0, 0, math.pi)
RVIZ_COV = np.diag([0.25, 0.25, 0.0, 0.0, 0.0, 0.0685])
GUESS = T.transform_from_rpy((1.5, -2.0, 0.0), (0.0, 0.0, 0.4))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def event_ms():
    ms = C.c_float(0.0)
    _capi.check(L.rmclhip_debug_particles_timing(ctx.handle, 1, C.byref(ms)))
    return ms.value


def host_channels(poses, attrs, max_n_meas=10000):
    lk = attrs["likelihood"]
    unc = (1.0 - lk["n_meas"].astype(np.float64) / np.float64(max_n_meas)).astype(np.float32)
    return (poses["t"]["x"].copy(), poses["t"]["y"].copy(), poses["t"]["z"].copy(), lk["mean"].copy(), lk["sigma"].copy(),
            lk["n_meas"].astype(np.float32), lk["mean"] * (lk["sigma"] * unc + unc))


say("device: %s   %d timed calls per variant after %d warm-ups, alternated within {U, P, V} and {hU, hV}; us, median [min .. max]"
    % (ctx.device_name(), args.calls, args.warmup))
for n in args.sizes:
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    seed = [0]

    def v_u():
        seed[0] += 1
        ra.init_particles_uniform(ctx, d_p, d_a, LO, HI, 42, epoch=seed[0])

    def v_p():
        seed[0] += 1
        ra.init_particles_pose(ctx, d_p, d_a, GUESS, RVIZ_COV, 42, epoch=seed[0])

    def v_v():
        return ra.pack_visualization(ctx, d_p, d_a, n)

    def v_hu():
        seed[0] += 1
        poses, attrs = syn.uniform_particles(n, seed=seed[0], bb_min=LO, bb_max=HI)
        a, b = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        a.free()
        b.free()

    def v_hv():
        return host_channels(d_p.download(), d_a.download())

    variants = (("U", v_u, True, 68), ("P", v_p, True, 68), ("V", v_v, True, 28 + 28), ("hU", v_hu, False, 68), ("hV", v_hv, False, 68))
    wall = {k: [] for k, _, _, _ in variants}
    dev = {k: [] for k, _, _, _ in variants}
    # two groups, each alternated within itself: hU allocates and frees device memory on every call (DeviceArray.from_host); with all
    # five variants in one loop whichever call came after it took 20-28 ms longer (cause not isolated) -- the host path's cost, not U's
    for group in (variants[:3], variants[3:]):
        for it in range(args.warmup + args.calls):
            for k, fn, on_device, _ in group:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    wall[k].append(dt * 1e6)
                    if on_device:
                        dev[k].append(event_ms() * 1e3)
    # the device pack equals the host arithmetic on the same cloud
    got, want = v_v(), v_hv()
    assert all(got[c].tobytes() == w.tobytes() for c, w in zip(ra.pf.VISUALIZATION_CHANNELS, want)), "pack differs from the host arithmetic"
    say("n = %d particles" % n)
    med = {}
    for k, _, on_device, nbytes in variants:
        w = np.sort(np.array(wall[k]))
        med[k] = float(np.median(w))
        s = "  %-3s host clock %10.1f [%10.1f .. %10.1f]" % (k, med[k], w[0], w[-1])
        if on_device:
            e = np.sort(np.array(dev[k]))
            em = float(np.median(e))
            s += "   events %9.1f [%9.1f .. %9.1f]   %d B per particle / events = %7.1f GB/s" % (em, e[0], e[-1], nbytes, n * nbytes / em / 1e3)
        say(s)
    say("  U vs hU: x %.1f   P vs hU: x %.1f   V vs hV: x %.1f   (host clock medians)" % (med["hU"] / med["U"], med["hU"] / med["P"], med["hV"] / med["V"]))
    d_p.free()
    d_a.free()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
