#!/usr/bin/env python
"""one Stein variational step of a cloud on the map's distance field (rmclhip_pf_stein_step, iterations 1) against its two yardsticks on
the same handle -- the field's sensor update (correspondence_type 1 with rmclhip_pf_set_field) and rmclhip_pf_refine(iterations 1) --
at 100 000 particles x 256 beams on room-100k, at the automatic cell, in one process, alternating.  The drive phase of a Stein step is
one pass and one solve of refine, so what it costs beyond the yardsticks is the cell list plus the pairs.  The two clouds are
tools/refine_time.py's: "uniform" (poses uniform over the room: nearly every bin holds one particle) and "local" (+-0.3 m, +-0.15 rad
around a scan's pose: a few dozen bins of thousands of particles each, thinned to max_per_bin).  Per line: the median of ROUNDS x
PER_ROUND calls, each timed by the host clock around a synchronous call (the start poses are uploaded again before every call, outside
the clock), and the spread of the per-round medians.  The split of a step into its three phases is taken with HIP events on the
handle's stream (rmclhip_debug_stein_timing, include/rmclhip_lab.h): the median over the same calls.  Figures quoted in DESIGN.md 4.16;
written to profiles/stein_time.txt.
usage: python tools/stein_time.py [--particles N] [--out FILE] [--kernels-only]
  --kernels-only: three calls per line and nothing else -- the run to wrap in `rocprofv3 --kernel-trace --stats -- python ...`"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import _capi, synthetic as syn, types as T  # noqa: E402
from refine_time import local_cloud  # noqa: E402

ROUNDS, PER_ROUND, WARMUP = 5, 4, 2
MARGIN = 0.5
PHASES = ("drive", "cell list", "pairs and move")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stein_time.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    n = a.particles
    import oracle as orc
    ctx = ra.Context(0)
    lines = ["# tools/stein_time.py on %s: %d particles x 256 beams on room-100k; per line the median of %d x %d synchronous calls (host clock),"
             % (ctx.device_name(), n, ROUNDS, PER_ROUND), "# spread = min .. max of the %d per-round medians; lines alternate within a round;" % ROUNDS,
             "# phases: HIP events on the handle's stream around the step's three phases, median over the same calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    v, f = syn.noisy_room(100000)
    hm = ra.import_hip_map(ctx, v, f)
    truth = T.transform_from_rpy((1.0, -1.5, 1.2), (0.0, 0.0, 0.5))
    scan = orc.Mesh(v, f).simulate_spherical(syn.model_c1(), T.identity(), truth, bvh=True)["points"]
    clouds = {
        "uniform": (syn.uniform_particles(n, seed=42, bb_min=(-9, -9, 0.3, 0, 0, -math.pi), bb_max=(9, 9, 3, 0, 0, math.pi))[0],
                    ra.beams_from_points(syn.model_directions(syn.model_pf16()) * np.float32(6.0))),
        "local": (local_cloud(truth, n, seed=43), ra.sample_beams(scan, 256, seed=7)),
    }
    attrs = syn.uniform_particles(n, seed=42)[1]
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray.from_host(ctx, attrs)
    d_rows = ra.DeviceArray(ctx, ra.field.STEIN_RESULT, n)
    d_rrows = ra.DeviceArray(ctx, ra.field.REFINE_RESULT, n)
    fd = ra.DistanceFieldHip(hm, cell=0.0, margin=MARGIN)
    i = fd.info()
    if not a.kernels_only:
        say("field auto    cell %.4f m  %4d x %4d x %4d = %9d nodes  %7.1f MB" % (i["cell"], i["n"][0], i["n"][1], i["n"][2], i["n_nodes"], i["bytes"] / 1e6))
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=1)
    upd.init()
    upd.set_field(fd)
    L = _capi.lib()
    _capi.check(L.rmclhip_debug_stein_timing(upd._h, 0 if a.kernels_only else 1, None))
    ms3 = (C.c_float * 3)()
    for cloud, (poses, beams) in clouds.items():
        assert len(beams) == 256
        upd.setInput(beams, T.identity())
        r1, s1 = ra.refine_params(iterations=1), ra.stein_params(iterations=1)
        calls = [("field sensor update", lambda: upd.update(d_p, d_a)),
                 ("refine, iterations 1", lambda: upd.refine(d_p, params=r1, results_dev=d_rrows)),
                 ("stein step, iterations 1", lambda: upd.stein_step(d_p, params=s1, results_dev=d_rows))]
        times = [[[] for _ in range(ROUNDS)] for _ in calls]
        phases = []
        stats = {}
        for r in range(-1, 1 if a.kernels_only else ROUNDS):      # round -1: warm-up
            for k, (name, call) in enumerate(calls):
                for _ in range(WARMUP if r < 0 else (3 if a.kernels_only else PER_ROUND)):
                    d_p.upload(poses)
                    t0 = time.perf_counter()
                    stats[k] = call()
                    if r >= 0:
                        times[k][r].append((time.perf_counter() - t0) * 1e3)
                        if k == 2 and not a.kernels_only:
                            _capi.check(L.rmclhip_debug_stein_timing(upd._h, 1, ms3))
                            phases.append([float(x) for x in ms3])
        if a.kernels_only:
            continue
        med = [float(np.median(np.concatenate(t))) for t in times]
        for k, (name, _) in enumerate(calls):
            per_round = [float(np.median(t)) for t in times[k]]
            say("%-8s %-25s %9.3f ms  (rounds %.3f .. %.3f)  x%.2f of the sensor update, x%.2f of refine" %
                (cloud, name, med[k], min(per_round), max(per_round), med[k] / med[0], med[k] / med[1]))
        ph = np.median(np.array(phases), axis=0)
        say("%-8s phases of the step: %s; sum %.3f ms" % (cloud, ", ".join("%s %.3f ms" % (nm, x) for nm, x in zip(PHASES, ph)), ph.sum()))
        st = stats[2]
        rows = d_rows.download()
        nb = rows["n_neighbours"]
        say("%-8s the step beyond refine: %.3f ms; %d bins, %d thinned; neighbours per particle: mean %.1f, median %d, max %d; mean used beams %.1f" %
            (cloud, med[2] - med[1], st["n_bins"], st["n_thinned_bins"], nb.mean(), int(np.median(nb)), int(nb.max()), rows["n_used"].mean()))
    upd.close()
    fd.close()
    hm.release()
    if not a.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
