#!/usr/bin/env python
"""the pose information beside the reduction that reads the same bytes: config C2's 128 x 1024 scan on sphere-100k, the find's model
buffers and the dataset in device memory, the three calls ALTERNATED call by call, host clock around synchronous calls.

  P   rmclhip_pose_information_p2l on caller-owned views        (k_pose_information_partials + k_pose_information_finalize, 256 B row copied back)
  R   rmclhip_rcc_pose_information, the operator form           (the same launches on the operator's stream)
  S   rmclhip_statistics_p2l on the same views, the yardstick   (k_reduce_partials + k_reduce_finalize, result in host-mapped memory)

All three stream 38 B per correspondence (12 B dataset point, 1 B + 1 B masks, 12 B model point, 12 B normal).

usage: python tools/pose_information_time.py [--calls 500] [--warmup 50]
       rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/pose_information_time.py --calls 100     (kernel times;
       python tools/prof_summary.py DIR/.../t_results.db)"""
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
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--warmup", type=int, default=50)
args = ap.parse_args()

ctx = ra.Context(0)
L = _capi.lib()
v, f = syn.uv_sphere(100000)
hm = ra.import_hip_map(ctx, v, f)
model = syn.model_c2()
n = int(model.phi.size) * int(model.theta.size)
truth = syn.pose_c2_truth()
est = T.mult(truth, syn.pose_c2_perturbation())
rcc = ra.RCCHipSpherical(hm)
rcc.setTsb(T.identity())
rcc.setModel(model)
rcc.params.max_dist = 1.0
rcc.adaptive_max_dist_min = 0.15
# the "measured" scan: the map from the true pose; its points go to the operator and stay in a buffer of ours for the free functions
real = ra.CorrespondencesHIP.download_bundle(rcc.simulate(truth, attributes=("ranges",)))["ranges"]
ds = (syn.model_directions(model) * real[:, None]).astype(np.float32)
mask = ((real >= np.float32(model.range.min)) & (real <= np.float32(model.range.max))).astype(np.uint8)
d_ds, d_mask = ra.DeviceArray.from_host(ctx, ds), ra.DeviceArray.from_host(ctx, mask)
rcc.set_dataset(ds, mask)
rcc.find(est)
hits, pts, nrm, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
_capi.check(L.rmclhip_rcc_device_views(rcc._h, C.byref(hits), None, C.byref(pts), C.byref(nrm), None, C.byref(cnt)))
assert cnt.value == n
rcc._push_params()

Tid = np.ascontiguousarray(T.identity(), dtype=T.TRANSFORM).reshape(1)
p_tid = Tid.ctypes.data_as(C.c_void_p)
info_p, info_r = np.zeros(1, T.POSE_INFORMATION), np.zeros(1, T.POSE_INFORMATION)
stats = np.zeros(1, T.CROSS_STATISTICS)
p_info_p, p_info_r, p_stats = (a.ctypes.data_as(C.c_void_p) for a in (info_p, info_r, stats))
views = (C.c_void_p(d_ds.ptr), C.c_void_p(d_mask.ptr), pts, nrm, hits, n, 1.0)


def call_p():
    _capi.check(L.rmclhip_pose_information_p2l(ctx.handle, p_tid, *views, p_info_p))


def call_r():
    _capi.check(L.rmclhip_rcc_pose_information(rcc._h, p_tid, 0.0, p_info_r))


def call_s():
    _capi.check(L.rmclhip_statistics_p2l(ctx.handle, p_tid, *views, p_stats))


variants = (("P", call_p), ("R", call_r), ("S", call_s))
times = {k: [] for k, _ in variants}
for it in range(args.warmup + args.calls):
    for k, fn in variants:
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if it >= args.warmup:
            times[k].append(dt * 1e6)
assert info_p.tobytes() == info_r.tobytes() and int(info_p[0]["n_meas"]) == int(stats[0]["n_meas"])
print("sphere100k  find kind %d  %d correspondences, %d kept  (%d timed calls per variant after %d warm-up, alternated)" %
      (rcc.find_variant(1), n, int(info_p[0]["n_meas"]), args.calls, args.warmup), flush=True)
for k, _ in variants:
    t = np.sort(np.array(times[k]))
    print("  %-2s  min %7.1f  median %7.1f  p90 %7.1f  max %7.1f us" % (k, t[0], float(np.median(t)), t[int(0.9 * (len(t) - 1))], t[-1]), flush=True)
rcc.close()
hm.release()
