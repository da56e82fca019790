#!/usr/bin/env python
"""what the sampled odometry model of the motion update costs (include/rmclhip.h, MOTION NOISE).  On room100k, for 50 000
and 1 000 000 particles, collision off and on, every variant ALTERNATED call by call with the others, each call on a freshly uploaded
copy of the same cloud (the upload is not timed):

  d    rmclhip_pf_motion_update -- this build (the deterministic instantiation, which must be the kernel of before)
  d0   the same call through the PARENT commit's library (--parent-lib: a librmclhip.so built from the parent commit; both libraries
       live in this process, each with its own context, map and buffers).  d - d0 has to lie within the spread, and the bytes are
       compared.  Left out when no parent library is given.
  n    rmclhip_pf_motion_update_noisy with the sigma of the step (AMCL's alphas): two Philox blocks, three Box-Muller pairs and three
       sine / cosine pairs in double per particle beside the 68 B it reads and the 44 B it writes

Host clock around the synchronous call; median [min .. max] of --calls timed calls after --warmup warm-ups.

usage: python tools/motion_noise_time.py [--parent-lib PATH] [--calls 30] [--warmup 5] [--out profiles/motion_noise_time.txt]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/motion_noise_time.py --calls 20
                                                        (kernel times: k_pf_motion<C, 0, 0> against k_pf_motion<C, 0, 1>)"""
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
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 1000000])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_noise_time.txt"))
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

    def close(self):
        self.L.rmclhip_free(self.ctx, self.d_p)
        self.L.rmclhip_free(self.ctx, self.d_a)
        self.L.rmclhip_pf_destroy(self.pf)
        self.L.rmclhip_map_release(self.map)
        self.L.rmclhip_ctx_destroy(self.ctx)


L = _capi.lib()
Lp = C.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
v, f = syn.noisy_room(100000)
step = np.ascontiguousarray(T.transform_from_rpy((0.25, 0.0, 0.0), (0.0, 0.0, 0.05)), dtype=T.TRANSFORM).reshape(1)
sigma = ra.motion_noise_sigma(ra.motion_noise_params(), step)
RATE, SEED = 0.01, 0x5EED
say("room100k (%d faces), motion step 0.25 m / yaw 0.05; noise: AMCL's alphas 0.2, sigma = %s" % (len(f), np.array2string(sigma, precision=5)))
say("host clock around each synchronous call, us: median [min .. max]; %d timed calls per variant after %d warm-ups, alternated call by call"
    % (args.calls, args.warmup))
if Lp is None:
    say("(no --parent-lib: d0 not measured)")

for n in args.sizes:
    poses, attrs = syn.uniform_particles(n, seed=5, bb_min=(-9.9, -9.9, 0.2, -0.2, -0.2, -math.pi), bb_max=(9.9, 9.9, 2.5, 0.2, 0.2, math.pi))
    cur = Raw(L, v, f, n)
    par = Raw(Lp, v, f, n) if Lp is not None else None
    for collision in (0, 1):
        calls = [0]

        def v_d():
            cur.upload(poses, attrs)
            t0 = time.perf_counter()
            cur.ok(L.rmclhip_pf_motion_update(cur.pf, cur.d_p, cur.d_a, n, T._ptr(step), RATE, collision))
            return time.perf_counter() - t0

        def v_d0():
            par.upload(poses, attrs)
            t0 = time.perf_counter()
            par.ok(Lp.rmclhip_pf_motion_update(par.pf, par.d_p, par.d_a, n, T._ptr(step), RATE, collision))
            return time.perf_counter() - t0

        def v_n():
            cur.upload(poses, attrs)
            calls[0] += 1
            t0 = time.perf_counter()
            cur.ok(L.rmclhip_pf_motion_update_noisy(cur.pf, cur.d_p, cur.d_a, n, T._ptr(step), RATE, collision, T._ptr(sigma), SEED, calls[0], 0))
            return time.perf_counter() - t0

        variants = [("d", v_d)] + ([("d0", v_d0)] if par is not None else []) + [("n", v_n)]
        wall = {k: [] for k, _ in variants}
        for it in range(args.warmup + args.calls):
            for k, fn in variants:
                dt = fn()
                if it >= args.warmup:
                    wall[k].append(dt * 1e6)
        v_d()
        pd = cur.download()
        if par is not None:   # the deterministic path returns the parent's bytes
            v_d0()
            pb = par.download()
            assert pd[0].tobytes() == pb[0].tobytes() and pd[1].tobytes() == pb[1].tobytes(), "the deterministic update differs from the parent commit"
        v_n()
        pn = cur.download()
        killed = lambda a: int(((a["likelihood"]["n_meas"] == 10000) & (a["likelihood"]["mean"] == 0)).sum())
        say("n = %d particles, collision %s   (killed: %d deterministic, %d noisy)" % (n, "on" if collision else "off", killed(pd[1]), killed(pn[1])))
        med = {}
        for k, _ in variants:
            w = np.sort(np.array(wall[k]))
            med[k] = float(np.median(w))
            say("  %-3s %10.1f [%10.1f .. %10.1f]" % (k, med[k], w[0], w[-1]))
        if par is not None:
            wd, w0 = np.array(wall["d"]), np.array(wall["d0"])
            say("  d - d0 = %+.1f us (medians); spread of d: %.1f us, of d0: %.1f us (max - min); bytes equal" %
                (med["d"] - med["d0"], wd.max() - wd.min(), w0.max() - w0.min()))
        say("  n - d = %+.1f us (%.2f x): the draw and the product in the motion update's launch, %.2f ns per particle" %
            (med["n"] - med["d"], med["n"] / med["d"], (med["n"] - med["d"]) * 1e3 / n))
    cur.close()
    if par is not None:
        par.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
