#!/usr/bin/env python
"""profiles/micp_host_split.txt: what moving the MICP corrections' host side into capi_micp.cpp did to the launch sequence and to time.
Run it once per library, each time in a fresh process, and compare the outputs.  Needs a GPU.

  tools/micp_host_split.py calls    one three-sensor rmclhip_micp_correct_once per loop form (per-iteration, host, device) on the cube
                                    map; prints the form each call ended in.  Under `rocprofv3 --kernel-trace -- python ...` the trace's
                                    ordered kernel names and streams are the launch sequence.
  tools/micp_host_split.py time     the figures bench.py reports for this code (its extras c3_schedule_R_*, c3_zero_iterations_ms,
                                    micp_two_sensors_*), by the same calls on the same set-up, median of three each; one JSON line.
  tools/micp_host_split.py table    (no GPU) reads `<label> <json line>` rows from stdin, in the order they were run, and prints the table
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

KEYS = ("headline_ms_per_step", "c3_schedule_R_ms", "c3_schedule_R_device_loop_ms", "c3_schedule_R_separate_moments_pass_ms",
        "c3_schedule_R_per_iteration_form_ms", "c3_zero_iterations_ms", "micp_two_sensors_host_loop_ms", "micp_two_sensors_device_loop_ms",
        "micp_two_sensors_cabi_ms")


def med3(fn):
    return sorted(fn() for _ in range(3))[1]


def calls():
    import micp_multi_cases as mc
    import rmcl_amd as ra
    import test_gpu_micp_multi as tg
    ctx = ra.Context(0)
    six = mc.cases()["cube6"]
    case = mc.Case("cube3", six.mesh_name, six.sensors[:3], six.truth, mc.orc.transform(), n_iter=six.n_iter)
    case.Tom = six.Tom
    v, f, _ = mc.mesh_arrays(case.mesh_name)
    hm = ra.import_hip_map(ctx, v, f)
    for form in ("per-iteration", "host", "device"):
        loc = mc.make_localization(ra, hm, case, tg.FORM_MODE[form])
        T, merged, after = tg.proven_call(loc, case, form)
        print(form, "served; n_meas", int(merged["n_meas"]), "T", T.tobytes().hex()[:56], flush=True)
        mc.close(loc)


def time_():
    import ctypes as C
    import time
    import numpy as np
    import rmcl_amd as ra
    from rmcl_amd import _capi as _c, synthetic as syn, types as T

    def median_call_ms(fn, reps=25, warm=3):   # bench.py _median_call_ms
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t1 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t1)
        return sorted(ts)[len(ts) // 2] * 1e3

    ctx = ra.Context(0)
    v, f = syn.uv_sphere(100000)
    hm = ra.import_hip_map(ctx, v, f)
    model = syn.model_c2()
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(T.identity())
    rcc.setModel(model)
    rcc.find(syn.pose_c2_truth())
    rcc.set_dataset_from_ranges(rcc.modelView()["ranges"])
    rcc.params.max_dist, rcc.adaptive_max_dist_min = 1.0, 0.15
    est = T.mult(syn.pose_c2_truth(), syn.pose_c2_perturbation())
    out = {}

    def once(n_iter=10):
        return med3(lambda: rcc.time_correct_once(est, T.identity(), n_iter, 0.0, False, iters=50))
    for key, mode in (("c3_schedule_R_ms", 1), ("c3_schedule_R_device_loop_ms", 4), ("c3_schedule_R_separate_moments_pass_ms", 3)):
        rcc.set_micp_fast(mode)
        rcc.correct_once(est, T.identity(), 10, 0.0, False)   # the moment form learns its bounds on the first call
        out[key] = once()
    rcc.set_micp_fast(0)
    out["c3_schedule_R_per_iteration_form_ms"] = once()
    out["c3_zero_iterations_ms"] = once(0)
    rcc.close()
    sA, sB = ra.RCCHipSpherical(hm), ra.RCCHipSpherical(hm)
    sens = []
    for rc_, mdl in ((sA, model), (sB, syn.model_vlp16_900())):
        rc_.setTsb(T.identity())
        rc_.setModel(mdl)
        rc_.find(syn.pose_c2_truth())
        rc_.set_dataset_from_ranges(rc_.modelView()["ranges"])
        rc_.params.max_dist, rc_.adaptive_max_dist_min = 1.0, 0.15
        sens.append(ra.MICPSensor("s%d" % len(sens), rc_, Tsb=T.identity(), Tbo=T.identity()))
    loc = ra.MICPLocalization(sens, optimization_iterations=10)
    loc.Tom_ = est
    out["micp_two_sensors_device_loop_ms"] = med3(lambda: median_call_ms(lambda: (setattr(loc, "Tom_", est), loc.correctOnce(device_loop=True)), reps=15))
    out["micp_two_sensors_host_loop_ms"] = med3(lambda: median_call_ms(lambda: (setattr(loc, "Tom_", est), loc.correctOnce()), reps=15))
    hnd = (C.c_void_p * 2)(sA._h, sB._h)
    Tbo2, w2 = np.array([T.identity(), T.identity()], dtype=T.TRANSFORM), np.ones(2, np.float64)
    Tin, Tout, mrg = np.ascontiguousarray(est, dtype=T.TRANSFORM).reshape(1), np.zeros(1, T.TRANSFORM), np.zeros(1, T.CROSS_STATISTICS)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    def cabi():
        return med3(lambda: median_call_ms(
            lambda: _c.check(_c.lib().rmclhip_micp_correct_once(hnd, 2, vp(Tin), vp(Tbo2), vp(w2), 10, 0.0, vp(Tout), vp(mrg))), reps=25))
    out["micp_two_sensors_cabi_ms"] = cabi()
    for mode, key in ((4, "two_sensors_mode4_cabi_ms"), (0, "two_sensors_mode0_cabi_ms")):   # (not bench.py figures: the other two forms)
        sA.set_micp_fast(mode)
        sB.set_micp_fast(mode)
        out[key] = cabi()
    print(json.dumps({k: round(x, 4) for k, x in out.items()}))


def table():
    merged = {}   # label -> figures; a bench.py result line under the same label gives the headline
    for line in sys.stdin:
        label, _, js = line.strip().partition(" ")
        if js.startswith("{"):
            d = json.loads(js)
            merged.setdefault(label, {}).update({"headline_ms_per_step": d["ms_per_step"]} if "ms_per_step" in d else d)
    rows = list(merged.items())
    keys = [k for k in KEYS + ("two_sensors_mode4_cabi_ms", "two_sensors_mode0_cabi_ms") if any(k in r for _, r in rows)]
    print("%-10s" % "process" + "".join("%12s" % ("k%d" % i) for i in range(len(keys))))
    for label, r in rows:
        print("%-10s" % label + "".join("%12s" % ("%.2f" % (r[k] * 1e3) if k in r else "-") for k in keys))
    for tree in sorted({lb.split("_")[0] for lb, _ in rows}):
        vals = {k: sorted(r[k] * 1e3 for lb, r in rows if lb.split("_")[0] == tree and k in r) for k in keys}
        print("%-10s" % (tree + " span") + "".join("%12s" % ("%.1f..%.1f" % (vals[k][0], vals[k][-1])) for k in keys))
        print("%-10s" % (tree + " med") + "".join("%12s" % ("%.2f" % ((vals[k][(len(vals[k]) - 1) // 2] + vals[k][len(vals[k]) // 2]) / 2)) for k in keys))
    print("figures in us; " + "; ".join("k%d = %s" % (i, k) for i, k in enumerate(keys)))


if __name__ == "__main__":
    {"calls": calls, "time": time_, "table": table}[sys.argv[1]]()
