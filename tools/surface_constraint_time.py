#!/usr/bin/env python
"""what the surface constraint of the motion update costs (include/rmclhip.h, "surface-constrained motion").  On room100k,
for 50 000 and 1 000 000 particles on the floor's height band (z in -0.3 .. 2.5, roll and pitch within 0.2), every variant ALTERNATED
call by call with the others, each call on a freshly uploaded copy of the same cloud (the upload is not timed):

  a    rmclhip_pf_motion_update with collision, constraint off -- this build
  a0   the same call through the PARENT commit's library (--parent-lib: a librmclhip.so built from the parent commit; both libraries
       live in this process, each with its own context, map and buffers).  The off path is meant to be the same code: a - a0 has to lie
       within the spread.  Left out when no parent library is given.
  b    the same call with the constraint on (axis 1, align 1): its cost over a
  c    rmclhip_pf_constrain_to_surface alone
  d    the host alternative a user has today, as a stated baseline and not a target: download of the poses, one ray per particle
       through the oracle's simulate_ondn on 16 threads, the snap arithmetic in numpy (no alignment), upload of the poses

Host clock around the synchronous call; median [min .. max] of --calls timed calls after --warmup warm-ups (d: --host-calls).

usage: python tools/surface_constraint_time.py [--parent-lib PATH] [--calls 30] [--warmup 5] [--out profiles/surface_constraint_time.txt]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/surface_constraint_time.py --calls 20 --no-host
                                                        (kernel times: k_pf_motion<1, 0>, k_pf_motion<1, 1>, k_surface_constrain)"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import _capi, synthetic as syn, types as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--host-calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 1000000])
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_constraint_time.txt"))
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Raw:
    """context + map + filter handle + one cloud's buffers through the C ABI of ONE library (this build's or the parent's)"""

    def __init__(self, L, v, f, n):
        self.L, self.n = L, n
        for name in ("rmclhip_ctx_create", "rmclhip_map_create", "rmclhip_pf_create", "rmclhip_malloc", "rmclhip_free", "rmclhip_memcpy_h2d",
                     "rmclhip_memcpy_d2h", "rmclhip_pf_motion_update", "rmclhip_pf_destroy", "rmclhip_map_release", "rmclhip_ctx_destroy"):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _capi.SIGNATURES[name]
        L.rmclhip_last_error.restype = C.c_char_p
        self.ctx, self.map, self.pf, self.d_p, self.d_a = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ok(L.rmclhip_ctx_create(0, C.byref(self.ctx)))
        self.ok(L.rmclhip_map_create(self.ctx, T._ptr(v), len(v), T._ptr(f), len(f), C.byref(self.map)))
        self.ok(L.rmclhip_pf_create(self.ctx, self.map, C.byref(self.pf)))
        self.ok(L.rmclhip_malloc(self.ctx, n * 32, C.byref(self.d_p)))
        self.ok(L.rmclhip_malloc(self.ctx, n * 36, C.byref(self.d_a)))

    def ok(self, st):
        if st != 0:
            raise RuntimeError(self.L.rmclhip_last_error().decode())

    def upload(self, poses, attrs):
        self.ok(self.L.rmclhip_memcpy_h2d(self.ctx, self.d_p, T._ptr(poses), self.n * 32))
        self.ok(self.L.rmclhip_memcpy_h2d(self.ctx, self.d_a, T._ptr(attrs), self.n * 36))

    def download(self):
        p, a = np.zeros(self.n, T.TRANSFORM), np.zeros(self.n, T.PARTICLE_ATTRIBUTES)
        self.ok(self.L.rmclhip_memcpy_d2h(self.ctx, T._ptr(p), self.d_p, self.n * 32))
        self.ok(self.L.rmclhip_memcpy_d2h(self.ctx, T._ptr(a), self.d_a, self.n * 36))
        return p, a

    def motion(self, step, rate):
        self.ok(self.L.rmclhip_pf_motion_update(self.pf, self.d_p, self.d_a, self.n, T._ptr(step), rate, 1))

    def close(self):
        self.L.rmclhip_free(self.ctx, self.d_p)
        self.L.rmclhip_free(self.ctx, self.d_a)
        self.L.rmclhip_pf_destroy(self.pf)
        self.L.rmclhip_map_release(self.map)
        self.L.rmclhip_ctx_destroy(self.ctx)


L = _capi.lib()
Lp = C.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
v, f = syn.noisy_room(100000)
sp = T.surface_params(axis=1, height=0.1, probe_up=0.5, probe_down=1.0, min_up_cos=0.7, align=1, on_miss=0)
step = np.ascontiguousarray(T.transform_from_rpy((0.25, 0.0, 0.0), (0.0, 0.0, 0.05)), dtype=T.TRANSFORM).reshape(1)
RATE = 0.01
say("room100k (%d faces), motion step 0.25 m / yaw 0.05, collision on; constraint: axis 1, height 0.1, probe 0.5 up / 1.0 down, align 1" % len(f))
say("host clock around each synchronous call, us: median [min .. max]; %d timed calls per variant after %d warm-ups, alternated call by call"
    % (args.calls, args.warmup))
if Lp is None:
    say("(no --parent-lib: a0 not measured)")

for n in args.sizes:
    poses, attrs = syn.uniform_particles(n, seed=5, bb_min=(-9.9, -9.9, -0.3, -0.2, -0.2, -math.pi), bb_max=(9.9, 9.9, 2.5, 0.2, 0.2, math.pi))
    cur = Raw(L, v, f, n)
    par = Raw(Lp, v, f, n) if Lp is not None else None
    stats = _capi.SurfaceStats()

    def v_a():
        cur.ok(L.rmclhip_pf_set_surface(cur.pf, None))
        cur.upload(poses, attrs)
        t0 = time.perf_counter()
        cur.motion(step, RATE)
        return time.perf_counter() - t0

    def v_a0():
        par.upload(poses, attrs)
        t0 = time.perf_counter()
        par.motion(step, RATE)
        return time.perf_counter() - t0

    def v_b():
        cur.ok(L.rmclhip_pf_set_surface(cur.pf, C.byref(sp)))
        cur.upload(poses, attrs)
        t0 = time.perf_counter()
        cur.motion(step, RATE)
        return time.perf_counter() - t0

    def v_c():
        cur.upload(poses, attrs)
        t0 = time.perf_counter()
        cur.ok(L.rmclhip_pf_constrain_to_surface(cur.pf, cur.d_p, cur.d_a, n, C.byref(sp), C.byref(stats)))
        return time.perf_counter() - t0

    variants = [("a", v_a)] + ([("a0", v_a0)] if par is not None else []) + [("b", v_b), ("c", v_c)]
    wall = {k: [] for k, _ in variants}
    for it in range(args.warmup + args.calls):
        for k, fn in variants:
            dt = fn()
            if it >= args.warmup:
                wall[k].append(dt * 1e6)
    if par is not None:   # the off path returns the parent's bytes
        v_a()
        pa = cur.download()
        v_a0()
        pb = par.download()
        assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes(), "constraint off differs from the parent commit"
    v_c()
    say("n = %d particles   (standalone pass: %d snapped, %d missed, %d steep)" % (n, stats.n_snapped, stats.n_missed, stats.n_steep))
    med = {}
    for k, _ in variants:
        w = np.sort(np.array(wall[k]))
        med[k] = float(np.median(w))
        say("  %-3s %10.1f [%10.1f .. %10.1f]" % (k, med[k], w[0], w[-1]))
    if par is not None:
        wa, w0 = np.array(wall["a"]), np.array(wall["a0"])
        say("  a - a0 = %+.1f us (medians); spread of a: %.1f us, of a0: %.1f us (max - min)" % (med["a"] - med["a0"], wa.max() - wa.min(), w0.max() - w0.min()))
    say("  b - a = %+.1f us: the constraint in the motion update's launch;  c = %.1f us: the pass alone" % (med["b"] - med["a"], med["c"]))

    if not args.no_host:
        import oracle as orc
        m = orc.Mesh(v, f)
        h, pu, pd = np.float32(0.1), np.float32(0.5), np.float32(1.0)
        origs = np.array([[0.0, 0.0, float(pu - h)]], np.float32)
        dirs = np.array([[0.0, 0.0, -1.0]], np.float32)
        host = []
        for it in range(1 + args.host_calls):
            cur.upload(poses, attrs)
            t0 = time.perf_counter()
            p, _ = cur.download()
            out = m.simulate_ondn(1, 1, 0.0, float(pu + pd), origs, dirs, T.identity(), p, bvh=True, nthreads=16, want=("hits", "ranges"))
            hit = out["hits"] > 0
            drop = (out["ranges"] - pu).astype(np.float32)     # how far the contact point lies above the surface, along body z
            q = p["R"]
            ax = 2.0 * (q["x"] * q["z"] + q["w"] * q["y"])
            ay = 2.0 * (q["y"] * q["z"] - q["w"] * q["x"])
            az = 2.0 * (q["w"] * q["w"] + q["z"] * q["z"]) - 1.0
            for k, a in (("x", ax), ("y", ay), ("z", az)):
                p["t"][k] = np.where(hit, p["t"][k] - drop * a, p["t"][k])
            cur.ok(L.rmclhip_memcpy_h2d(cur.ctx, cur.d_p, T._ptr(p), n * 32))
            if it:
                host.append((time.perf_counter() - t0) * 1e6)
        w = np.sort(np.array(host))
        say("  d   %10.1f [%10.1f .. %10.1f]   host: download + simulate_ondn (16 threads) + snap in numpy + upload, %d calls; %d of %d hit"
            % (float(np.median(w)), w[0], w[-1], len(w), int(hit.sum()), n))
    cur.close()
    if par is not None:
        par.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
