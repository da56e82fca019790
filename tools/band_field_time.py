#!/usr/bin/env python
"""the banded distance field (rmclhip_field_create_banded) beside the dense one on the same map, cell and margin, in one process,
alternating: the field's sensor update (correspondence_type 1 with rmclhip_pf_set_field) and one refine iteration
(rmclhip_field_refine, iterations 1, max_dist = band = 0.5) at 100 000 particles x 256 beams, on sphere-100k and room-100k, at the
automatic cell and at 0.05 m.  The clouds are tools/pf_field_time.py's ("uniform": poses uniform over the map, 256 fixed 6 m beams)
and, on the room with tools/refine_time.py's margin of 0.5 m, tools/refine_time.py's "local" cloud (poses around the pose a 256-beam
scan was taken from).  Per line: the median of ROUNDS x PER_ROUND calls, each timed by the host clock around a synchronous call (the
start poses are uploaded again before every call, outside the clock), and the spread of the per-round medians.  Also both layouts'
build times and bytes, and whether the two layouts gave the same bytes (refine: always; update: wherever no beam ends in a FAR
brick).  Figures quoted in DESIGN.md 4.17; written to profiles/band_field_time.txt.
usage: python tools/band_field_time.py [--particles N] [--out FILE]"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import synthetic as syn, types as T  # noqa: E402
from refine_time import local_cloud  # noqa: E402

ROUNDS, PER_ROUND, WARMUP = 5, 4, 2
FINE_CELL = 0.05
BAND = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_field_time.txt"))
    a = ap.parse_args()
    n = a.particles
    import oracle as orc
    ctx = ra.Context(0)
    lines = ["# tools/band_field_time.py on %s: %d particles x 256 beams, band %.2f m; per line the median of %d x %d synchronous calls (host clock),"
             % (ctx.device_name(), n, BAND, ROUNDS, PER_ROUND), "# spread = min .. max of the %d per-round medians; lines alternate within a round" % ROUNDS]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    attrs = syn.uniform_particles(n, seed=42)[1]
    d_p, d_a = ra.DeviceArray(ctx, T.TRANSFORM, n), ra.DeviceArray(ctx, T.PARTICLE_ATTRIBUTES, n)
    d_rows = ra.DeviceArray(ctx, ra.field.REFINE_RESULT, n)
    p1 = ra.refine_params(iterations=1, max_dist=BAND)
    fixed_beams = ra.beams_from_points(syn.model_directions(syn.model_pf16()) * np.float32(6.0))
    for mesh, margin in (("sphere", 0.0), ("room", 0.0), ("room", 0.5)):
        v, f = syn.uv_sphere(100000) if mesh == "sphere" else syn.noisy_room(100000)
        hm = ra.import_hip_map(ctx, v, f)
        bb = ((-5, -5, -1), (5, 5, 1)) if mesh == "sphere" else ((-9, -9, 0.3), (9, 9, 3))
        clouds = {"uniform": (syn.uniform_particles(n, seed=42, bb_min=bb[0] + (0, 0, -math.pi), bb_max=bb[1] + (0, 0, math.pi))[0], fixed_beams)}
        if margin > 0:
            truth = T.transform_from_rpy((1.0, -1.5, 1.2), (0.0, 0.0, 0.5))
            scan = orc.Mesh(v, f).simulate_spherical(syn.model_c1(), T.identity(), truth, bvh=True)["points"]
            clouds["local"] = (local_cloud(truth, n, seed=43), ra.sample_beams(scan, 256, seed=7))
        name = "%s%s" % (mesh, "+%.1f" % margin if margin else "")
        for label, cell in (("auto", 0.0), ("%.2f m" % FINE_CELL, FINE_CELL)):
            fields = {}
            for layout in ("dense", "banded"):
                t0 = time.perf_counter()
                fd = ra.DistanceFieldHip(hm, cell=cell, margin=margin) if layout == "dense" else \
                    ra.DistanceFieldHip.banded(hm, cell=cell, margin=margin, band=BAND)
                build_ms = (time.perf_counter() - t0) * 1e3
                i = fd.info()
                extra = ""
                if layout == "banded":
                    b = fd.band_info()
                    extra = "  %d of %d bricks stored" % (b["n_stored"], b["n_bricks"])
                say("%-8s %-7s %-6s cell %.4f m  %4d x %4d x %4d = %9d nodes  %7.1f MB  built in %8.1f ms%s"
                    % (name, label, layout, i["cell"], i["n"][0], i["n"][1], i["n"][2], i["n_nodes"], i["bytes"] / 1e6, build_ms, extra))
                upd = ra.PCDSensorUpdaterHip(hm)
                upd.config = T.pf_params(correspondence_type=1)
                upd.init()
                upd.set_field(fd)
                fields[layout] = (fd, upd)
            for cloud, (poses, beams) in clouds.items():
                assert len(beams) == 256
                calls, results = [], {}
                for layout, (fd, upd) in fields.items():
                    upd.setInput(beams, T.identity())
                    calls.append(("sensor update, " + layout, lambda upd=upd: upd.update(d_p, d_a)))
                    calls.append(("refine it. 1,  " + layout, lambda fd=fd: fd.refine(d_p, beams, T.identity(), params=p1, results_dev=d_rows)))
                times = [[[] for _ in range(ROUNDS)] for _ in calls]
                for r in range(-1, ROUNDS):      # round -1: warm-up
                    for k, (cname, call) in enumerate(calls):
                        for _ in range(WARMUP if r < 0 else PER_ROUND):
                            d_p.upload(poses)
                            d_a.upload(attrs)
                            t0 = time.perf_counter()
                            call()
                            if r >= 0:
                                times[k][r].append((time.perf_counter() - t0) * 1e3)
                        results[k] = (d_a.download().tobytes() if k % 2 == 0 else d_p.download().tobytes())
                med = [float(np.median(np.concatenate(t))) for t in times]
                for k, (cname, _) in enumerate(calls):
                    per_round = [float(np.median(t)) for t in times[k]]
                    say("%-8s %-7s %-8s %-24s %9.3f ms  (rounds %.3f .. %.3f)  x%.2f of dense"
                        % (name, label, cloud, cname, med[k], min(per_round), max(per_round), med[k] / med[k % 2]))
                say("%-8s %-7s %-8s same bytes from both layouts: attributes after the update %s, poses after the refinement %s"
                    % (name, label, cloud, results[0] == results[2], results[1] == results[3]))
            for fd, upd in fields.values():
                upd.close()
                fd.close()
        hm.release()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
