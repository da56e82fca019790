#!/usr/bin/env python
"""ROBUST MICP beside the plain kernels that read the same bytes: config C2's 128 x 1024 scan on sphere-100k and room-100k, the find's
model buffers and the dataset in device memory, the calls ALTERNATED call by call, host clock around synchronous calls at the C ABI.

  W    rmclhip_rcc_compute_robust_statistics, HUBER at a FIXED scale   (k_robust_partials + k_robust_finalize, result in host-mapped memory,
                                                                        hipStreamSynchronize)
  S    rmclhip_rcc_compute_cross_statistics with set_micp_fast(0)      (k_reduce_partials + k_reduce_finalize, the yardstick: the plain
                                                                        streaming reduction of the parent, result in host-mapped memory)
  Mk   rmclhip_rcc_residual_scale, MAD: the selection alone, the first pass writes the keys, the others read them (the default)
  Mr   ... every pass recomputes the residual (rmclhip_debug_robust_select_recompute)
  CR   rmclhip_rcc_correct_once_robust, TUKEY MAD, 10 iterations       (find + selection + 10 x k_robust_iter + k_robust_close)
  C0   rmclhip_rcc_correct_once with set_micp_fast(0), 10 iterations   (find + 10 x k_micp_iter + k_micp_close: the per-iteration form)
  C1   rmclhip_rcc_correct_once in its default form, 10 iterations     (the moment form: no streaming pass per iteration)

W and S stream 38 B per correspondence (12 B dataset point, 1 B + 1 B masks, 12 B model point, 12 B normal).

usage: python tools/robust_micp_time.py [--calls 200] [--warmup 30] [--out profiles/robust_micp_time.txt]"""
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
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = ra.Context(0)
L = _capi.lib()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(name, v, f, truth):
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    n = int(model.phi.size) * int(model.theta.size)
    est = T.mult(truth, syn.pose_c2_perturbation())
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    rcc.params.max_dist = 1.0
    rcc.adaptive_max_dist_min = 1.0
    real = ra.CorrespondencesHIP.download_bundle(rcc.simulate(truth, attributes=("ranges",)))["ranges"]
    ds = (syn.model_directions(model) * real[:, None]).astype(np.float32)
    mask = ((real >= np.float32(model.range.min)) & (real <= np.float32(model.range.max))).astype(np.uint8)
    rcc.set_dataset(ds, mask)
    rcc.find(est)
    rcc._push_params()
    tid = np.ascontiguousarray(T.identity(), dtype=T.TRANSFORM).reshape(1)
    p_tid = tid.ctypes.data_as(C.c_void_p)
    p_est = np.ascontiguousarray(est, dtype=T.TRANSFORM).reshape(1).ctypes.data_as(C.c_void_p)
    huber, tukey = T.robust_params("huber", scale=0.1), T.robust_params("tukey")
    rs, cs, tout = np.zeros(1, T.ROBUST_STATISTICS), np.zeros(1, T.CROSS_STATISTICS), np.zeros(1, T.TRANSFORM)
    p_rs, p_cs, p_tout = (a.ctypes.data_as(C.c_void_p) for a in (rs, cs, tout))
    c_out, med_out, m_out = C.c_float(0), C.c_float(0), C.c_uint32(0)
    medians = {}

    def fast(mode):
        _capi.check(L.rmclhip_rcc_set_micp_fast(rcc._h, mode))

    def call_w():
        _capi.check(L.rmclhip_rcc_compute_robust_statistics(rcc._h, p_tid, 0.0, C.byref(huber), p_rs))

    def call_s():
        _capi.check(L.rmclhip_rcc_compute_cross_statistics(rcc._h, p_tid, 0.0, p_cs))

    def call_m(recompute, key):
        def run():
            _capi.check(L.rmclhip_debug_robust_select_recompute(recompute))
            _capi.check(L.rmclhip_rcc_residual_scale(rcc._h, p_tid, 0.0, C.byref(tukey), C.byref(c_out), C.byref(med_out), C.byref(m_out)))
            medians[key] = (c_out.value, med_out.value, m_out.value)
        return run

    def call_cr():
        _capi.check(L.rmclhip_rcc_correct_once_robust(rcc._h, p_tid, p_est, 10, 0.0, C.byref(tukey), p_tout, p_rs))

    def call_c(mode):
        def run():
            fast(mode)
            _capi.check(L.rmclhip_rcc_correct_once(rcc._h, p_tid, p_est, 10, 0.0, 0, p_tout, p_cs))
        return run

    groups = ((("W", call_w), ("S", call_s)), (("Mk", call_m(0, "k")), ("Mr", call_m(1, "r"))),
              (("CR", call_cr), ("C0", call_c(0)), ("C1", call_c(1))))
    say("%s  find kind %d  %d correspondences  (%d timed calls per variant after %d warm-up, alternated within a group)" %
        (name, rcc.find_variant(1), n, args.calls, args.warmup))
    for group in groups:
        if group[0][0] == "W":
            fast(0)          # S streams: no moment set answers it
            rcc.find(est)
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
        if group[0][0] == "W":
            assert int(rs[0]["stats"]["n_meas"]) == int(cs[0]["n_meas"])
            say("      kept %d, sum w %.1f" % (int(cs[0]["n_meas"]), float(rs[0]["weight_sum"])))
        fast(1)
    assert medians["k"] == medians["r"], medians
    say("      selection: c %.6f, median %.6f, m %d (both forms)" % medians["k"])
    _capi.check(L.rmclhip_debug_robust_select_recompute(0))
    rcc.close()
    hm.release()


measure("sphere100k", *syn.uv_sphere(100000), syn.pose_c2_truth())
measure("room100k  ", *syn.noisy_room(100000), T.transform_from_rpy((1.5, -2.0, 1.6), (0.02, -0.03, 0.4)))
if args.out:
    with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
