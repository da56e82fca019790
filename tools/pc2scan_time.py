#!/usr/bin/env python
"""an unorganised PointCloud2 into the spherical operator: the device path against what a caller did before it existed.  A 131 072-point
cloud of 22-byte records (a C2 scan of room-100k from a true pose, hit points shuffled, 2 % of the points NaN) into config C2's
128 x 1024 model; the variants ALTERNATED call by call, host clock around calls that end in a synchronise.

  N    rmclhip_rcc_set_input_pointcloud2_scan from HOST bytes (2.9 MB upload included): image, dataset and counts
  Nd   the same with the cloud already in device memory
  F    rmclhip_pointcloud2_to_scan (the free function), host bytes in, image back to the host
  L    the reference's loop on ONE host thread (tools/ubench/pc2scan_host_loop.cpp: two atan2 and a sqrt per point) -> range image
  R    rmclhip_rcc_set_dataset_from_ranges of that image (what exists without this path: 0.5 MB upload, allocates per call)
  L+R  what a caller does without the device path, timed as one

usage: python tools/pc2scan_time.py [--calls 100] [--warmup 10] [--flags 0]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/pc2scan_time.py --calls 50     (kernel times: k_pc2scan_*)"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import _capi, synthetic as syn, types as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--flags", type=int, default=0)
args = ap.parse_args()

src = os.path.join(ROOT, "tools", "ubench", "pc2scan_host_loop.cpp")
so = os.path.join(tempfile.mkdtemp(prefix="pc2scan_"), "libpc2scan_host_loop.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
host = C.CDLL(so)
host.pc2scan_host_loop.restype = C.c_uint32
host.pc2scan_host_loop.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_float, C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                                                   C.c_float, C.c_float, C.c_void_p]

REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("time", "<f4")])
ctx = ra.Context(0)
L = _capi.lib()
v, f = syn.noisy_room(100000)
hm = ra.import_hip_map(ctx, v, f)
model = syn.model_c2()
H, W = int(model.phi.size), int(model.theta.size)
n = H * W
truth = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
rcc = ra.RCCHipSpherical(hm)
rcc.setTsb(T.identity())
rcc.setModel(model)
# the cloud: every ray of a scan from the truth pose (misses become NaN points, as drivers publish them), shuffled
sim = ra.CorrespondencesHIP.download_bundle(rcc.simulate(truth, attributes=("ranges", "hits")))
pts = (syn.model_directions(model) * sim["ranges"][:, None]).astype(np.float32)
pts[sim["hits"] == 0] = np.nan
rng = np.random.RandomState(7)
pts[rng.choice(n, n // 50, replace=False)] = np.nan
pts = pts[rng.permutation(n)]
cloud = np.zeros(n, REC)
cloud["x"], cloud["y"], cloud["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
data = np.frombuffer(cloud.tobytes(), np.uint8)
lay = dict(width=n, height=1, point_step=REC.itemsize, row_step=n * REC.itemsize, offset_x=0, offset_y=4, offset_z=8)
d_data = ra.DeviceArray.from_host(ctx, data)
h_img = np.zeros(n, np.float32)
rcc2 = ra.RCCHipSpherical(hm)          # the parent-commit caller's operator
rcc2.setTsb(T.identity())
rcc2.setModel(model)


def variant_n():
    return rcc.setInputPointCloud2(data, flags=args.flags, **lay)


def variant_nd():
    return rcc.setInputPointCloud2(d_data, flags=args.flags, device=True, nbytes=data.size, **lay)


def variant_f():
    return ra.wire.pointcloud2_to_scan(ctx, data, model=model, flags=args.flags, **lay)


def variant_l():
    return host.pc2scan_host_loop(data.ctypes.data_as(C.c_void_p), n, REC.itemsize, 0, 4, 8, model.phi.min, model.phi.inc, H, model.theta.min,
                                  model.theta.inc, W, model.range.min, model.range.max, h_img.ctypes.data_as(C.c_void_p))


def variant_r():
    return rcc2.set_dataset_from_ranges(h_img)


def variant_lr():
    variant_l()
    return variant_r()


variant_l()
variants = (("N", variant_n), ("Nd", variant_nd), ("F", variant_f), ("L", variant_l), ("R", variant_r), ("L+R", variant_lr))
times = {k: [] for k, _ in variants}
for it in range(args.warmup + args.calls):
    for k, fn in variants:
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if it >= args.warmup:
            times[k].append(dt * 1e6)
stats = variant_n()
if args.flags == 0:
    assert rcc.rangesView().download().tobytes() == h_img.tobytes(), "the host loop's image differs from the device's"
print("room100k  C2 model %d x %d  cloud of %d points x %d B, unorganised  flags %d  %s  (%d timed calls per variant, alternated, %d warm-up)"
      % (H, W, n, REC.itemsize, args.flags, stats, args.calls, args.warmup), flush=True)
med = {}
for k, _ in variants:
    t = np.sort(np.array(times[k]))
    med[k] = float(np.median(t))
    print("  %-3s  min %8.1f  p10 %8.1f  median %8.1f  p90 %8.1f  max %8.1f us" %
          (k, t[0], t[len(t) // 10], med[k], t[(9 * len(t)) // 10], t[-1]), flush=True)
print("  N %s R alone: %.1f vs %.1f us;  N vs L+R: %.1f vs %.1f us (x %.1f)" %
      ("<=" if med["N"] <= med["R"] else ">", med["N"], med["R"], med["N"], med["L+R"], med["L+R"] / med["N"]), flush=True)
rcc.close()
rcc2.close()
hm.release()
