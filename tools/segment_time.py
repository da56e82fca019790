#!/usr/bin/env python
"""map segmentation on the device against what a caller did before it existed: config C2's 128 x 1024 model on sphere100k and room100k,
after autotune, the variants ALTERNATED call by call, host clock around calls that end in a synchronise.

  A   simulate(Tbm, {ranges, normals}) into a device bundle + download of both (16 B per ray) into preallocated host arrays -- the
      classification loop on the host that follows is not even counted
  B   segment() from the measured ranges in HOST memory (its 4 B per ray upload included): labels and both clouds stay on the device,
      the two counts come back
  Bd  the same with the measured ranges already in device memory
  S   simulate of the same bundle alone, synchronised: Bd - S is what classification and compaction cost

usage: python tools/segment_time.py [--calls 200] [--warmup 20]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/segment_time.py --calls 50     (kernel times: k_segment_*)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import _capi, synthetic as syn, types as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()

ctx = ra.Context(0)
L = _capi.lib()
for mesh in ("sphere100k", "room100k"):
    v, f = syn.uv_sphere(100000) if mesh.startswith("sphere") else syn.noisy_room(100000)
    hm = ra.import_hip_map(ctx, v, f)
    truth = syn.pose_c2_truth() if mesh.startswith("sphere") else T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    n = int(model.phi.size) * int(model.theta.size)
    est = T.mult(truth, T.transform_from_rpy((0.06, 0.03, 0.02), (0.0, 0.0, np.deg2rad(0.6))))
    rcc.autotune(est)
    # the "measured" scan: the map from the truth pose, an obstacle (a block of beams 40 % shorter), 2 % invalid returns
    real = ra.CorrespondencesHIP.download_bundle(rcc.simulate(truth, attributes=("ranges",)))["ranges"].copy()
    real.reshape(128, 1024)[40:70, 200:330] *= np.float32(0.6)
    real[np.random.RandomState(7).choice(n, n // 50, replace=False)] = np.float32(0.0)
    d_real = ra.DeviceArray.from_host(ctx, real)
    bundle = dict(ranges=ra.DeviceArray(ctx, np.float32, n), normals=ra.DeviceArray(ctx, np.float32, 3 * n))
    h_ranges, h_normals = np.zeros(n, np.float32), np.zeros(3 * n, np.float32)
    into = dict(labels=ra.DeviceArray(ctx, np.uint8, n), outlier_scan=ra.DeviceArray(ctx, np.float32, 3 * n),
                outlier_map=ra.DeviceArray(ctx, np.float32, 3 * n))

    def variant_a():
        rcc.simulate(est, attributes=("ranges", "normals"), into=bundle)
        _capi.check(L.rmclhip_memcpy_d2h(ctx.handle, h_ranges.ctypes.data_as(C.c_void_p), C.c_void_p(bundle["ranges"].ptr), 4 * n))
        _capi.check(L.rmclhip_memcpy_d2h(ctx.handle, h_normals.ctypes.data_as(C.c_void_p), C.c_void_p(bundle["normals"].ptr), 12 * n))

    def variant_b():
        return rcc.segment(est, real, into=into)

    def variant_bd():
        return rcc.segment(est, d_real, into=into)

    def variant_s():
        rcc.simulate(est, attributes=("ranges", "normals"), into=bundle)

    variants = (("A", variant_a), ("B", variant_b), ("Bd", variant_bd), ("S", variant_s))
    times = {k: [] for k, _ in variants}
    for it in range(args.warmup + args.calls):
        for k, fn in variants:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                times[k].append(dt * 1e6)
    counts = variant_bd()
    print("%s  find kind %d  %d rays  outlier_scan %d  outlier_map %d  (%d timed calls per variant, alternated)" %
          (mesh, rcc.find_variant(1), n, counts[0], counts[1], args.calls), flush=True)
    med = {}
    for k, _ in variants:
        t = np.sort(np.array(times[k]))
        med[k] = float(np.median(t))
        print("  %-2s  min %7.1f  median %7.1f  max %7.1f us" % (k, t[0], med[k], t[-1]), flush=True)
    print("  Bd - S = %.1f us (classification + compaction)   B %s A: %.1f vs %.1f us" %
          (med["Bd"] - med["S"], "<=" if med["B"] <= med["A"] else ">", med["B"], med["A"]), flush=True)
    rcc.close()
    hm.release()
