#!/usr/bin/env python
"""the refinement of particles on the map's distance field (rmclhip_field_refine) against its yardstick, the field's sensor update
(correspondence_type 1 with rmclhip_pf_set_field), at 100 000 particles x 256 beams on room-100k, at the automatic cell and at 0.05 m,
for iterations 1 and 8, in one process, alternating.  Two clouds: "uniform" is tools/pf_field_time.py's (poses uniform over the room,
256 fixed 6 m beams: most end points are far from any surface, few beams are used), "local" is the refinement's own case (poses
+-0.3 m, +-0.15 rad around the pose a 256-beam scan was taken from).  Per line: the median of ROUNDS x PER_ROUND calls, each timed by
the host clock around a synchronous call (the start poses are uploaded again before every call, outside the clock), and the spread of
the per-round medians.  A pass = (iterations 8 - iterations 1) / 7.  Figures quoted in DESIGN.md 4.15; written to
profiles/refine_time.txt.
usage: python tools/refine_time.py [--particles N] [--out FILE] [--kernels-only]
  --kernels-only: three calls per line and nothing else -- the run to wrap in `rocprofv3 --kernel-trace --stats -- python ...`"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import synthetic as syn, types as T  # noqa: E402

ROUNDS, PER_ROUND, WARMUP = 5, 4, 2
FINE_CELL = 0.05
MARGIN = 0.5


def local_cloud(truth, n, seed):
    """n poses around truth: uniformly +-0.3 m per axis, +-0.15 rad about world z"""
    rng = np.random.RandomState(seed)
    poses = np.zeros(n, T.TRANSFORM)
    yaw = rng.uniform(-0.15, 0.15, n)
    q0 = np.array([truth["R"][k] for k in "xyzw"], np.float64)
    s, c = np.sin(yaw / 2), np.cos(yaw / 2)          # (0, 0, s, c) * q0
    q = np.stack([c * q0[0] - s * q0[1], c * q0[1] + s * q0[0], c * q0[2] + s * q0[3], c * q0[3] - s * q0[2]], -1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for i, k in enumerate("xyzw"):
        poses["R"][k] = q[:, i]
    for k in "xyz":
        poses["t"][k] = float(truth["t"][k]) + rng.uniform(-0.3, 0.3, n)
    return poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_time.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    n = a.particles
    import oracle as orc
    ctx = ra.Context(0)
    lines = ["# tools/refine_time.py on %s: %d particles x 256 beams on room-100k; per line the median of %d x %d synchronous calls (host clock),"
             % (ctx.device_name(), n, ROUNDS, PER_ROUND), "# spread = min .. max of the %d per-round medians; lines alternate within a round" % ROUNDS]

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
    d_rows = ra.DeviceArray(ctx, ra.field.REFINE_RESULT, n)
    for label, cell in (("auto", 0.0), ("%.2f m" % FINE_CELL, FINE_CELL)):
        fd = ra.DistanceFieldHip(hm, cell=cell, margin=MARGIN)
        i = fd.info()
        if not a.kernels_only:
            say("field %-7s cell %.4f m  %4d x %4d x %4d = %9d nodes  %7.1f MB" % (label, i["cell"], i["n"][0], i["n"][1], i["n"][2], i["n_nodes"], i["bytes"] / 1e6))
        upd = ra.PCDSensorUpdaterHip(hm)
        upd.config = T.pf_params(correspondence_type=1)
        upd.init()
        upd.set_field(fd)
        for cloud, (poses, beams) in clouds.items():
            assert len(beams) == 256
            upd.setInput(beams, T.identity())
            p1, p8 = ra.refine_params(iterations=1), ra.refine_params(iterations=8)
            calls = [("field sensor update", lambda: upd.update(d_p, d_a)),
                     ("refine, iterations 1", lambda: fd.refine(d_p, beams, T.identity(), params=p1, results_dev=d_rows)),
                     ("refine, iterations 8", lambda: fd.refine(d_p, beams, T.identity(), params=p8, results_dev=d_rows))]
            times = [[[] for _ in range(ROUNDS)] for _ in calls]
            stats = {}
            for r in range(-1, 1 if a.kernels_only else ROUNDS):      # round -1: warm-up
                for k, (name, call) in enumerate(calls):
                    for _ in range(WARMUP if r < 0 else (3 if a.kernels_only else PER_ROUND)):
                        d_p.upload(poses)
                        t0 = time.perf_counter()
                        stats[k] = call()
                        if r >= 0:
                            times[k][r].append((time.perf_counter() - t0) * 1e3)
            if a.kernels_only:
                continue
            med = [float(np.median(np.concatenate(t))) for t in times]
            for k, (name, _) in enumerate(calls):
                per_round = [float(np.median(t)) for t in times[k]]
                say("%-7s %-8s %-22s %9.3f ms  (rounds %.3f .. %.3f)  x%.2f of the sensor update" % (label, cloud, name, med[k], min(per_round), max(per_round), med[k] / med[0]))
            st = stats[2]
            rows = d_rows.download()
            say("%-7s %-8s a pass: %.3f ms = x%.2f of the sensor update; iterations 8 moved %d of %d (no beams: %d), mean accepted steps %.2f, mean used beams %.1f, cost %.4g -> %.4g"
                % (label, cloud, (med[2] - med[1]) / 7.0, (med[2] - med[1]) / 7.0 / med[0], st["n_moved"], st["n_particles"], st["n_no_beams"],
                   rows["accepted"].mean(), rows["n_used"].mean(), st["cost_before_sum"], st["cost_after_sum"]))
        upd.close()
        fd.close()
    hm.release()
    if not a.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
