#!/usr/bin/env python
"""the motion-compensated PointCloud2 input beside what it replaces and what it costs.  A 131 072-point organised cloud of 22-byte
records (a C2 scan of room-100k, time = the column's share of a 0.1 s revolution, 2 % of the points NaN), a motion of 0.4 m and
0.15 rad in 17 knots; the variants ALTERNATED call by call, host clock around calls that end in a synchronise; medians.

  D    rmclhip_rcc_set_input_pointcloud2_deskewed from HOST bytes (2.9 MB upload included): OnDn model + dataset + counts
  Dd   the same with the cloud already in device memory
  P    rmclhip_rcc_set_input_pointcloud2 (one pose for the whole scan: O1Dn model + dataset) from host bytes
  Pd   the same from device memory
  H    the host loop a caller writes without D (tools/ubench/deskew_host_loop.cpp, ONE thread) -> origins, directions, points, mask
  U    set_model_ondn + set_dataset of those arrays (two 1.5 MB uploads + points + mask)
  H+U  what D replaces, timed as one
and one find on the OnDn model D leaves against one find on the O1Dn model P leaves (rmclhip_rcc_time_find: no frontier start for
OnDn, find_kernel.hip.h).

usage: python tools/deskew_time.py [--calls 30] [--warmup 5] [--out profiles/deskew_time.txt]"""
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
from rmcl_amd import synthetic as syn, types as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew_time.txt"))
args = ap.parse_args()

src = os.path.join(ROOT, "tools", "ubench", "deskew_host_loop.cpp")
so = os.path.join(tempfile.mkdtemp(prefix="deskew_"), "libdeskew_host_loop.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
host = C.CDLL(so)
host.deskew_host_loop.restype = C.c_uint32
host.deskew_host_loop.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                                   C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("time", "<f4")])
ctx = ra.Context(0)
v, f = syn.noisy_room(100000)
hm = ra.import_hip_map(ctx, v, f)
model = syn.model_c2()
H, W = int(model.phi.size), int(model.theta.size)
n = H * W
truth = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
sim_op = ra.RCCHipSpherical(hm)
sim_op.setTsb(T.identity())
sim_op.setModel(model)
sim = ra.CorrespondencesHIP.download_bundle(sim_op.simulate(truth, attributes=("ranges", "hits")))
pts = (syn.model_directions(model) * sim["ranges"][:, None]).astype(np.float32)
pts[sim["hits"] == 0] = np.nan
rng = np.random.RandomState(7)
pts[rng.choice(n, n // 50, replace=False)] = np.nan
cloud = np.zeros(n, REC)
cloud["x"], cloud["y"], cloud["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
cloud["time"] = np.tile((np.arange(W, dtype=np.float32) / np.float32(W - 1)) * np.float32(0.1), H)
data = np.frombuffer(cloud.tobytes(), np.uint8)
lay = (W, H, REC.itemsize, W * REC.itemsize, 0, 4, 8)
time_field = (REC.fields["time"][1], 7, 1.0, 0.0)
yaw = lambda a, t: T.transform((0.0, 0.0, np.sin(a / 2), np.cos(a / 2)), t)
last = yaw(0.4, (1.5, -2.0, 1.6))
first = T.mult(last, T.inv(yaw(0.15, (0.4, 0.0, 0.0))))
knots, ktimes = ra.wire.scan_motion(T.identity(), np.array([first, last], T.TRANSFORM), [0.0, 0.1], 0.1, 16)
motion = (knots, ktimes)
kq = np.ascontiguousarray(np.array([[k["R"][c] for c in "xyzw"] for k in knots], np.float32))
kt = np.ascontiguousarray(np.array([[k["t"][c] for c in "xyz"] for k in knots], np.float32))
d_data = ra.DeviceArray.from_host(ctx, data)
RMIN, RMAX = 0.3, 120.0

desk, plain, manual = ra.RCCHipOnDn(hm), ra.RCCHipO1Dn(hm), ra.RCCHipOnDn(hm)
h_origs, h_dirs, h_points = (np.zeros((n, 3), np.float32) for _ in range(3))
h_mask = np.zeros(n, np.uint8)
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def variant_d():
    return desk.setInputPointCloud2Deskewed(data, *lay, time_field, motion, range_min=RMIN, range_max=RMAX)


def variant_dd():
    return desk.setInputPointCloud2Deskewed(d_data, *lay, time_field, motion, range_min=RMIN, range_max=RMAX, device=True, nbytes=data.size)


def variant_p():
    return plain.setInputPointCloud2(data, *lay, 7, RMIN, RMAX)


def variant_pd():
    return plain.setInputPointCloud2(d_data, *lay, 7, RMIN, RMAX, device=True, nbytes=data.size)


def variant_h():
    return host.deskew_host_loop(vp(data), n, REC.itemsize, 0, 4, 8, time_field[0], 1.0, 0.0, vp(ktimes), vp(kq), vp(kt), len(ktimes), RMIN, RMAX,
                                 vp(h_origs), vp(h_dirs), vp(h_points), vp(h_mask))


def variant_u():
    manual.setModel(W, H, RMIN, RMAX, h_origs, h_dirs)
    manual.set_dataset(h_points, h_mask)


def variant_hu():
    variant_h()
    variant_u()


variant_h()
variants = (("D", variant_d), ("Dd", variant_dd), ("P", variant_p), ("Pd", variant_pd), ("H", variant_h), ("U", variant_u), ("H+U", variant_hu))
times = {k: [] for k, _ in variants}
for it in range(args.warmup + args.calls):
    for k, fn in variants:
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if it >= args.warmup:
            times[k].append(dt * 1e6)
w, h, stats = variant_d()
iv = desk.inputView()
same = all(iv[k].tobytes() == a.tobytes() for k, a in (("origs", h_origs), ("dirs", h_dirs), ("points", h_points), ("mask", h_mask)))
lines = ["room100k  C2 cloud %d x %d = %d points x %d B, organised  %d knots  %s  (%d timed calls per variant, alternated, %d warm-up; device: %s)"
         % (H, W, n, REC.itemsize, len(ktimes), stats, args.calls, args.warmup, ctx.device_name()),
         "  host loop's arrays %s the device's" % ("byte-equal to" if same else "DIFFER from")]
med = {}
for k, _ in variants:
    t = np.sort(np.array(times[k]))
    med[k] = float(np.median(t))
    lines.append("  %-3s  min %8.1f  p10 %8.1f  median %8.1f  p90 %8.1f  max %8.1f us" % (k, t[0], t[len(t) // 10], med[k], t[(9 * len(t)) // 10], t[-1]))
lines.append("  D / P (host bytes): %.1f / %.1f us = x %.2f;  Dd / Pd (device bytes): %.1f / %.1f us = x %.2f   (37 B written per point against 25)"
             % (med["D"], med["P"], med["D"] / med["P"], med["Dd"], med["Pd"], med["Dd"] / med["Pd"]))
lines.append("  D vs H+U: %.1f vs %.1f us (x %.1f)" % (med["D"], med["H+U"], med["H+U"] / med["D"]))
est = T.mult(last, T.transform_from_rpy((0.05, 0.05, 0.0), (0.0, 0.0, 0.02)))
variant_d()
variant_p()
finds = {}
for rep in range(3):
    for k, op in (("OnDn", desk), ("O1Dn", plain)):
        finds.setdefault(k, []).append(1e3 * op.time_find(est, 50))
f_on, f_o1 = float(np.median(finds["OnDn"])), float(np.median(finds["O1Dn"]))
lines.append("  find (kind %d / %d, mean of 50 back-to-back launches, median of 3): OnDn model %.1f us, O1Dn model of the same cloud %.1f us = x %.2f"
             % (desk.find_variant(), plain.find_variant(), f_on, f_o1, f_on / f_o1))
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(text)
for op in (desk, plain, manual, sim_op):
    op.close()
hm.release()
