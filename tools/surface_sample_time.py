#!/usr/bin/env python
"""what the surface sampler costs (include/rmclhip.h, SURFACE SAMPLER), beside today's way to the same end:
rmclhip_particles_init_uniform in the map's bounding box followed by rmclhip_pf_constrain_to_surface, both timed in THIS build.  Their
kernels compute what they computed before the sampler existed, but their text is not untouched: the constraint's alignment step moved
into a header of its own (surface_align.hip.h; the recipe runs with align 0 and never enters it) and uniform_in into pf_random.hip.h.
The recipe is not timed through a library built from the commit before.

  create     rmclhip_surface_sampler_create on room100k and on a room of 1 000 000 faces (the build's three launches, the download of the
             areas and prefix sums for the info, the allocations)
  init       rmclhip_particles_init_surface of 50 000 and 1 000 000 particles on each map
  inject     rmclhip_particles_inject_surface at p = 0.05 and p = 1 on the same clouds
  recipe     init_uniform (x, y over the map's box, z in a 3 m band over its floor, yaw free) + constrain_to_surface (axis 0, height 0.2,
             probe 0.3 up / 3.0 down), and the share of its particles that end MISS or STEEP -- they stay where the box put them

Call time: host clock around the synchronous call.  Device time: the two events rmclhip_debug_particles_timing puts around what a
particles call enqueues (the constraint runs on its filter handle's stream and has the call time only).  Median [min .. max] of
--calls timed calls after --warmup warm-ups.

usage: python tools/surface_sample_time.py [--calls 20] [--warmup 3] [--faces 100000 1000000] [--out profiles/surface_sample_time.txt]"""
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
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000])
ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 1000000])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_sample_time.txt"))
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


L = _capi.lib()
ctx = ra.Context(0)
name = C.create_string_buffer(256)
L.rmclhip_ctx_device_name(ctx.handle, name, 256)
say("device: %s" % name.value.decode())
say("us: median [min .. max] of %d timed calls after %d warm-ups; call = host clock around the synchronous call, dev = events around its launches"
    % (args.calls, args.warmup))


def timed(fn, device=True):
    """(call us, device us) arrays of fn over the timed calls"""
    ms = C.c_float(0.0)
    call, dev = [], []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e6
        if device:
            _capi.check(L.rmclhip_debug_particles_timing(ctx.handle, 1, C.byref(ms)))
        if it >= args.warmup:
            call.append(dt)
            dev.append(ms.value * 1e3)
    return np.sort(np.array(call)), np.sort(np.array(dev))


def row(what, call, dev=None):
    s = "  %-34s call %10.1f [%10.1f .. %10.1f]" % (what, float(np.median(call)), call[0], call[-1])
    if dev is not None:
        s += "   dev %10.1f [%10.1f .. %10.1f]" % (float(np.median(dev)), dev[0], dev[-1])
    say(s)
    return float(np.median(call))


_capi.check(L.rmclhip_debug_particles_timing(ctx.handle, 1, None))
SEED = 20240611
for nf in args.faces:
    v, f = syn.noisy_room(nf)
    m = ra.import_hip_map(ctx, v, f)
    mi = m.info()
    say("room of %d faces (%d records)" % (mi["n_faces"], mi["n_tri_records"]))
    samplers = []

    def create():
        samplers.append(ra.SurfaceSamplerHip(m, height=0.2))
        if len(samplers) > 1:
            samplers.pop(0).close()

    call, _ = timed(create, device=False)
    row("create", call)
    s = samplers[-1]
    say("  sampler: %r" % (s.info(),))
    lo, hi = np.array(mi["bbox_min"], np.float32), np.array(mi["bbox_max"], np.float32)
    bb_min = (lo[0], lo[1], lo[2], 0.0, 0.0, -math.pi)
    bb_max = (hi[0], hi[1], lo[2] + 3.0, 0.0, 0.0, math.pi)
    sp = T.surface_params(axis=0, height=0.2, probe_up=0.3, probe_down=3.0, min_up_cos=0.7, align=0, on_miss=0)
    pf = C.c_void_p()
    _capi.check(L.rmclhip_pf_create(ctx.handle, m.handle, C.byref(pf)))
    stats = _capi.SurfaceStats()
    for n in args.sizes:
        d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
        say("  n = %d particles" % n)
        step = [0]
        c_init = row("init_surface", *timed(lambda: s.init(d_p, d_a, SEED, epoch=1)))

        def inject(p):
            step[0] += 1
            return s.inject(d_p, d_a, p, SEED, step[0])

        row("inject p = 0.05", *timed(lambda: inject(0.05)))
        row("inject p = 1", *timed(lambda: inject(1.0)))
        c_uni = row("recipe: init_uniform", *timed(lambda: ra.init_particles_uniform(ctx, d_p, d_a, bb_min, bb_max, SEED, epoch=1)))

        def constrain():
            ra.init_particles_uniform(ctx, d_p, d_a, bb_min, bb_max, SEED, epoch=1)     # (a constrained cloud would snap trivially)
            t0 = time.perf_counter()
            _capi.check(L.rmclhip_pf_constrain_to_surface(pf, C.c_void_p(d_p.ptr), C.c_void_p(d_a.ptr), n, C.byref(sp), C.byref(stats)))
            return (time.perf_counter() - t0) * 1e6

        cs = np.sort(np.array([constrain() for _ in range(args.warmup + args.calls)][args.warmup:]))
        c_con = row("recipe: constrain_to_surface", cs)
        say("  recipe: %d snapped, %d missed, %d steep of %d: %.2f %% stay where the box put them; recipe call %.1f us vs init_surface %.1f us"
            % (stats.n_snapped, stats.n_missed, stats.n_steep, stats.n_particles,
               100.0 * (stats.n_missed + stats.n_steep) / max(stats.n_particles, 1), c_uni + c_con, c_init))
        d_p.free()
        d_a.free()
    L.rmclhip_pf_destroy(pf)
    s.close()
    m.release()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
