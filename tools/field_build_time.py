#!/usr/bin/env python
"""the build of both field layouts (rmclhip_field_create, rmclhip_field_create_banded at band 0.5 m) repeated in one process, on
tools/band_field_time.py's maps, margins and cells: per map, cell and layout the median, min and max of REPS builds after two warm-up
builds -- the host clock around the create call, the field closed outside the clock, the layouts alternating.  band_field_time.py
times ONE build per process, which does not resolve a millisecond; to compare two commits run this from a build of each, alternately
(profiles/field_build_unified.txt, section 2).
usage: python tools/field_build_time.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import rmcl_amd as ra  # noqa: E402
from rmcl_amd import synthetic as syn  # noqa: E402

REPS, REPS_SPHERE, WARMUP = 25, 7, 2      # the hollow sphere's builds take 0.04 .. 0.4 s each
BAND = 0.5


def main():
    ctx = ra.Context(0)
    for mesh, margin in (("sphere", 0.0), ("room", 0.0), ("room", 0.5)):
        v, f = syn.uv_sphere(100000) if mesh == "sphere" else syn.noisy_room(100000)
        hm = ra.import_hip_map(ctx, v, f)
        for cell in (0.0, 0.05):
            reps = REPS_SPHERE if mesh == "sphere" else REPS
            t = {"dense": [], "banded": []}
            for r in range(-WARMUP, reps):
                for layout in t:
                    t0 = time.perf_counter()
                    fd = ra.DistanceFieldHip(hm, cell=cell, margin=margin) if layout == "dense" else \
                        ra.DistanceFieldHip.banded(hm, cell=cell, margin=margin, band=BAND)
                    ms = (time.perf_counter() - t0) * 1e3
                    fd.close()
                    if r >= 0:
                        t[layout].append(ms)
            for layout, a in t.items():
                print("%-6s+%.1f cell %-4s %-6s %2d builds: median %8.3f ms  min %8.3f  max %8.3f"
                      % (mesh, margin, cell or "auto", layout, len(a), np.median(a), min(a), max(a)), flush=True)
        hm.release()


if __name__ == "__main__":
    main()
