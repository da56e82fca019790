"""Writes tests/golden/g9_pc2scan.npz: a PointCloud2 -> scan case that keeps tests/pc2scan_ref.py from drifting together with the kernel.

cloud   = 3000 points in 22-byte records (x, y, z, intensity, ring, time: the unaligned layout of tests/test_wire_formats.py), an
          unorganised cloud (height 1): uniform in a 16 x 16 x 8 m box around the sensor, so most cells of the model take several
          points, a few NaN / inf fields, a few points beyond range.max
model   = config C1 (32 x 32 spherical model, +-45 deg, theta from -pi)
ranges  = tests/pc2scan_ref.py on those bytes for flags 0 (the reference's rule), 7 (true elevation + floor + theta wrap), 8 (nearest)

    python tests/golden/make_g9_pc2scan.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pc2scan_ref as pr  # noqa: E402
from rmcl_amd import synthetic as syn  # noqa: E402

REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("time", "<f4")])


def build():
    rng = np.random.RandomState(9)
    n = 3000
    p = np.c_[rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-4, 4, n)].astype(np.float32)
    p[rng.randint(0, n, 12), rng.randint(0, 3, 12)] = np.nan
    p[rng.randint(0, n, 4), 1] = np.inf
    p[rng.randint(0, n, 6)] *= np.float32(40.0)          # beyond range.max = 100 for most of them
    data, lay = pr.make_cloud(REC, p, seed=9)
    out = dict(data=np.frombuffer(data, np.uint8), layout=np.array([lay[k] for k in ("width", "height", "point_step", "row_step",
                                                                                       "offset_x", "offset_y", "offset_z", "datatype")], np.uint32))
    for fl in (0, 7, 8):
        res = pr.convert(data, model=syn.model_c1(), flags=fl, **lay)
        out["ranges_%d" % fl] = res["ranges"]
        out["stats_%d" % fl] = np.array([res["stats"][k] for k in ("n_points", "n_finite", "n_in_image", "n_in_range", "n_cells_filled")], np.uint32)
    return out


if __name__ == "__main__":
    out = build()
    np.savez_compressed(os.path.join(HERE, "g9_pc2scan.npz"), **out)
    for fl in (0, 7, 8):
        print("g9_pc2scan.npz: flags %d -> points / finite / in image / in range / cells filled =" % fl, out["stats_%d" % fl])
