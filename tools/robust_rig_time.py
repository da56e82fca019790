#!/usr/bin/env python
"""ROBUST MICP FOR SENSOR RIGS beside the calls that read the same bytes: rigs of 2 and 4 sensors, each config C2's 128 x 1024 scan on
room-100k from its own mount, every tenth column of sensor 0 shortened; 10 iterations; the calls ALTERNATED call by call, host clock
around synchronous calls at the C ABI.

  RR   rmclhip_micp_correct_once_robust, TUKEY MAD per sensor          (N finds + N selections on N streams, then per iteration ONE
                                                                        k_robust_rig_partials over all sensors + k_robust_rig_step, a
                                                                        closing launch, one synchronisation)
  P0   rmclhip_micp_correct_once with set_micp_fast(0) on every sensor (N finds, per iteration N x k_reduce_partials + k_micp_multi_step:
                                                                        the plain rig call in its per-iteration form, same handles)
  S1   the sum of the sensors' single rmclhip_rcc_correct_once_robust  (N calls one after the other: N synchronisations)
  IW   rmclhip_rcc_pose_information_robust, TUKEY MAD, sensor 0        (selection + weighted pass + fold + copy)
  IP   rmclhip_rcc_pose_information, sensor 0                          (plain pass + fold + copy)

usage: python tools/robust_rig_time.py [--calls 100] [--warmup 20] [--out profiles/robust_rig_time.txt]"""
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
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = ra.Context(0)
L = _capi.lib()
lines = []
MOUNTS = [T.identity(), T.transform_from_rpy((-0.2, 0.1, 0.5), (0.0, 0.1, -1.0)), T.transform_from_rpy((0.0, -0.25, 0.2), (0.05, 0.0, 2.0)),
          T.transform_from_rpy((0.3, 0.0, 0.1), (0.0, -0.05, 0.1))]
WEIGHTS = [1.0, 0.37, 2.0, 0.5]


def say(s):
    print(s, flush=True)
    lines.append(s)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


hm = ra.import_hip_map(ctx, *syn.noisy_room(100000))
truth = T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
est = T.mult(truth, syn.pose_c2_perturbation())
model = syn.model_c2()
H, W = int(model.phi.size), int(model.theta.size)
ops = []
for k in range(4):
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(MOUNTS[k])
    rcc.setModel(model)
    rcc.params.max_dist = rcc.adaptive_max_dist_min = 1.0
    real = ra.CorrespondencesHIP.download_bundle(rcc.simulate(truth, attributes=("ranges",)))["ranges"].copy()
    mask = ((real >= np.float32(model.range.min)) & (real <= np.float32(model.range.max))).astype(np.uint8)
    if k == 0:
        short = np.zeros((H, W), bool)
        short[:, ::10] = True
        real[short.reshape(-1)] *= np.float32(0.9)
    rcc.set_dataset((syn.model_directions(model) * real[:, None]).astype(np.float32), mask)
    rcc._push_params()
    ops.append(rcc)

tid = np.ascontiguousarray(T.identity(), dtype=T.TRANSFORM).reshape(1)
p_est = np.ascontiguousarray(est, dtype=T.TRANSFORM).reshape(1)
tukey = T.robust_params("tukey")
tout, merged, Wout = np.zeros(1, T.TRANSFORM), np.zeros(1, T.CROSS_STATISTICS), C.c_double(0.0)
rs = np.zeros(8, T.ROBUST_STATISTICS)
info, info_r = np.zeros(1, T.POSE_INFORMATION), np.zeros(1, T.POSE_INFORMATION_ROBUST)


def fast(mode, n):
    for op in ops[:n]:
        _capi.check(L.rmclhip_rcc_set_micp_fast(op._h, mode))


def timed(group, note):
    times = {k: [] for k, _ in group}
    for it in range(args.warmup + args.calls):
        for k, fn in group:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                times[k].append(dt * 1e6)
    for k, _ in group:
        t = np.sort(np.array(times[k]))
        say("  %-2s  min %7.1f  median %7.1f  p90 %7.1f  max %7.1f us" % (k, t[0], float(np.median(t)), t[int(0.9 * (len(t) - 1))], t[-1]))
    say("      " + note())


say("room100k  %d x %d rays per sensor, 10 iterations  (%d timed calls per variant after %d warm-up, alternated within a group)" %
    (H, W, args.calls, args.warmup))
for n in (2, 4):
    handles = (C.c_void_p * n)(*[op._h for op in ops[:n]])
    Tbo = np.array([est] * n, dtype=T.TRANSFORM)
    w = np.array(WEIGHTS[:n], dtype=np.float64)
    params = (_capi.RobustParams * n)()
    for k in range(n):
        for name, _ in _capi.RobustParams._fields_:
            setattr(params[k], name, getattr(tukey, name))
    fast(0, n)

    def call_rr():
        _capi.check(L.rmclhip_micp_correct_once_robust(handles, n, ptr(tid), ptr(Tbo), ptr(w), C.cast(params, C.c_void_p), 10, 0.0, ptr(tout),
                                                       ptr(merged), C.byref(Wout), ptr(rs)))

    def call_p0():
        _capi.check(L.rmclhip_micp_correct_once(handles, n, ptr(tid), ptr(Tbo), ptr(w), 10, 0.0, ptr(tout), ptr(merged)))

    def call_s1():
        for op in ops[:n]:
            _capi.check(L.rmclhip_rcc_correct_once_robust(op._h, ptr(tid), ptr(p_est), 10, 0.0, C.byref(tukey), ptr(tout), ptr(rs)))

    say("%d sensors" % n)
    call_rr()
    kept = [int(s["stats"]["n_meas"]) for s in rs[:n]]
    sums = [float(s["weight_sum"]) for s in rs[:n]]
    timed((("RR", call_rr), ("P0", call_p0), ("S1", call_s1)), lambda: "kept %s, sum w %s" % (kept, ["%.1f" % x for x in sums]))
    fast(1, n)

ops[0].find(est)


def call_iw():
    _capi.check(L.rmclhip_rcc_pose_information_robust(ops[0]._h, ptr(tid), 0.0, C.byref(tukey), ptr(info_r)))


def call_ip():
    _capi.check(L.rmclhip_rcc_pose_information(ops[0]._h, ptr(tid), 0.0, ptr(info)))


say("pose information, sensor 0")
timed((("IW", call_iw), ("IP", call_ip)),
      lambda: "kept %d, sum w %.1f" % (int(info[0]["n_meas"]), float(info_r[0]["weight_sum"])))
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
