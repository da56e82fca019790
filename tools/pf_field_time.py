#!/usr/bin/env python
"""the particle filter's sensor update with closest-point errors read from the map's distance field (rmclhip_pf_set_field) against
ray casting (correspondence_type 0) and the exact closest-point mode (correspondence_type 1 without a field), in one process,
alternating.  Per mode: the median of ROUNDS x PER_ROUND updates, each timed by the host clock around a synchronous update, and the
spread of the per-round medians.  Also the field's build time, node count and bytes, and the largest |field error - exact error| on a
sub-cloud against the bound (sqrt(3) / 2) cell.  Figures quoted in DESIGN.md 4.14; written to profiles/pf_field_time.txt.
usage: python tools/pf_field_time.py [--particles N] [--out FILE] [--kernels-only]
  --kernels-only: three updates per mode and nothing else -- the run to wrap in `rocprofv3 --kernel-trace --stats -- python ...`"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import synthetic as syn, types as T  # noqa: E402

ROUNDS, PER_ROUND, WARMUP = 5, 4, 2
FINE_CELL = 0.05
ERR_PARTICLES = 10000


def end_points64(poses, beams):
    """beam end points in float64 (Tsb = identity): only to tell which of them lie inside the lattice"""
    q = np.stack([poses["R"][k] for k in "xyzw"], -1).astype(np.float64)
    t = np.stack([poses["t"][k] for k in "xyz"], -1).astype(np.float64)
    p = np.stack([beams["dir"][k] for k in "xyz"], -1).astype(np.float64) * beams["range"].astype(np.float64)[:, None]
    u, w = q[:, None, :3], q[:, None, 3:]
    c = np.cross(u, p[None]) + w * p[None]
    return t[:, None] + p[None] + 2.0 * np.cross(u, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pf_field_time.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    n = a.particles
    ctx = ra.Context(0)
    lines = ["# tools/pf_field_time.py on %s: %d particles x 256 beams; per mode the median of %d x %d synchronous updates (host clock),"
             % (ctx.device_name(), n, ROUNDS, PER_ROUND), "# spread = min .. max of the %d per-round medians; modes alternate within a round" % ROUNDS]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for mesh in ("sphere", "room"):
        v, f = syn.uv_sphere(100000) if mesh == "sphere" else syn.noisy_room(100000)
        hm = ra.import_hip_map(ctx, v, f)
        bb = ((-5, -5, -1), (5, 5, 1)) if mesh == "sphere" else ((-9, -9, 0.3), (9, 9, 3))
        poses, attrs = syn.uniform_particles(n, seed=42, bb_min=bb[0] + (0, 0, -math.pi), bb_max=bb[1] + (0, 0, math.pi))
        beams = ra.beams_from_points(syn.model_directions(syn.model_pf16()) * np.float32(6.0))
        d_p, d_a = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        fields = {}
        for label, cell in (("auto", 0.0), ("%.2f m" % FINE_CELL, FINE_CELL)):
            t0 = time.perf_counter()
            fd = ra.DistanceFieldHip(hm, cell=cell)
            build_ms = (time.perf_counter() - t0) * 1e3
            i = fd.info()
            fields[label] = fd
            if not a.kernels_only:
                say("%-7s field %-7s cell %.4f m  %4d x %4d x %4d = %9d nodes  %7.1f MB  built in %8.1f ms"
                    % (mesh, label, i["cell"], i["n"][0], i["n"][1], i["n"][2], i["n_nodes"], i["bytes"] / 1e6, build_ms))
        modes = [("ray casting (type 0)", 0, None), ("closest point, exact (type 1)", 1, None)]
        modes += [("closest point, field %s" % k, 1, fd) for k, fd in fields.items()]
        upds = []
        for label, ct, fd in modes:
            upd = ra.PCDSensorUpdaterHip(hm)
            upd.config = T.pf_params(correspondence_type=ct)
            upd.init()
            upd.set_field(fd)
            upd.setInput(beams, T.identity())
            for _ in range(1 if a.kernels_only else WARMUP):
                upd.update(d_p, d_a)
            upds.append(upd)
        if a.kernels_only:
            for upd in upds:
                for _ in range(3):
                    upd.update(d_p, d_a)
        else:
            times = [[[] for _ in range(ROUNDS)] for _ in modes]
            for r in range(ROUNDS):
                for k, upd in enumerate(upds):
                    for _ in range(PER_ROUND):
                        t0 = time.perf_counter()
                        upd.update(d_p, d_a)
                        times[k][r].append((time.perf_counter() - t0) * 1e3)
            med = [float(np.median(np.concatenate(t))) for t in times]
            for k, (label, ct, fd) in enumerate(modes):
                per_round = [float(np.median(t)) for t in times[k]]
                say("%-7s %-32s %9.3f ms  (rounds %.3f .. %.3f)  %7.2f G evals/s  x%.2f of type 0  x%.3f of exact type 1"
                    % (mesh, label, med[k], min(per_round), max(per_round), n * len(beams) / med[k] / 1e6, med[k] / med[0], med[k] / med[1]))
            # the lookup's error on a sub-cloud: against the exact mode's errors, inside the lattice and anywhere
            sub = min(n, ERR_PARTICLES)
            d_ps, d_as = ra.DeviceArray.from_host(ctx, poses[:sub]), ra.DeviceArray.from_host(ctx, attrs[:sub])
            d_err = ra.DeviceArray(ctx, np.float32, sub * len(beams))
            errs = []
            for upd in upds[1:]:
                upd.set_error_output(d_err)
                upd.update(d_ps, d_as)
                upd.set_error_output(None)
                errs.append(d_err.download().reshape(sub, len(beams)).astype(np.float64))
            ends = end_points64(poses[:sub], beams)
            for (label, fd), e in zip(fields.items(), errs[1:]):
                i = fd.info()
                lo = np.array(i["origin"]) + i["cell"]
                hi = np.array(i["origin"]) + (np.array(i["n"]) - 2) * i["cell"]
                inside = ((ends >= lo) & (ends <= hi)).all(axis=2)
                diff = np.abs(e - errs[0])
                say("%-7s field %-7s max |field - exact| = %.4f m inside the lattice (%.0f %% of the end points; bound %.4f m), %.3f m anywhere"
                    % (mesh, label, diff[inside].max(), 100.0 * inside.mean(), math.sqrt(3.0) / 2.0 * i["cell"], diff.max()))
        for upd in upds:
            upd.close()
        for fd in fields.values():
            fd.close()
        hm.release()
    if not a.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
