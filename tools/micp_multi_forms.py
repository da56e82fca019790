#!/usr/bin/env python
"""profiles/micp_multi_forms.txt: every case of tests/micp_multi_cases.py in each loop form of rmclhip_micp_correct_once -- the form proven
from fast_info, the undecided count and the deviations from the oracle and from the per-iteration form.  Needs a GPU.
usage: tools/micp_multi_forms.py > profiles/micp_multi_forms.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import micp_multi_cases as mc
import rmcl_amd as ra
import test_gpu_micp_multi as tg

ctx = ra.Context(0)
maps = {}


def hm(name):
    if name not in maps:
        v, f, _ = mc.mesh_arrays(name)
        maps[name] = ra.import_hip_map(ctx, v, f)
    return maps[name]


lines = ["N-sensor MICP correction (rmclhip_micp_correct_once): every case of tests/micp_multi_cases.py in each loop form on an MI355X.",
         "Fresh operators per line; the moment forms' line is the THIRD identical call.  form: proven from rmclhip_rcc_micp_fast_info as",
         "tests/test_gpu_micp_multi.py::prove_form does (overflow: a moment form gave up with code 2 and the per-iteration form served the call).",
         "undecided: last_uncertain of that call (the rig's sum; - where no moment form ran).  Deviations of T_onew_oold: translation [m] and",
         "residual rotation [rad] against the oracle's loop (tests/oracle_micp.py) and against the per-iteration form of the same case.",
         "The bar is 1e-5 of the correction's own translation / angle plus the floors 1e-6 m and 2e-7 rad (_transform_close); `corr` is that size.",
         "",
         "%-16s %-14s %-14s %9s  %-21s  %-21s  %-21s  %s" % ("case", "mode", "form", "undecided", "corr [m, rad]", "vs oracle [m, rad]", "vs per-iteration", "n_meas")]
C = mc.cases()
ident = mc.orc.transform()
for name, case in C.items():
    per = tg.run_form(ra, hm(case.mesh_name), case, "per-iteration", check_views=False)
    rows = [("0", "per-iteration", per)]
    if name in tg.FORM_CASES:
        rows += [("1", "host", tg.run_form(ra, hm(case.mesh_name), case, "host", check_views=False)),
                 ("4", "device", tg.run_form(ra, hm(case.mesh_name), case, "device", check_views=False))]
    elif name == "mid":
        rows += [("1", "device", tg.run_form(ra, hm(case.mesh_name), case, "device", mode=1, check_views=False))]
    elif name == "far":
        for mode in (1, 4):
            loc = mc.make_localization(ra, hm(case.mesh_name), case, mode)
            T, merged, after = tg.proven_call(loc, case, "overflow")
            rows.append((str(mode) + " first call", "overflow", {"T": T, "merged": merged, "last_uncertain": after[0]["last_uncertain"]}))
            mc.close(loc)
    To = mc.oracle(case)[0]
    corr = tg.deviation(To, ident)
    for mode, form, r in rows:
        do, dp = tg.deviation(r["T"], To), tg.deviation(r["T"], per["T"])
        lines.append("%-16s %-14s %-14s %9s  %.3e %.3e  %.3e %.3e  %.3e %.3e  %d" % (
            name, mode, form, "-" if form == "per-iteration" else str(r["last_uncertain"]), corr[0], corr[1], do[0], do[1], dp[0], dp[1],
            int(r["merged"]["n_meas"])))
print("\n".join(lines))
