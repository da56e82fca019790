"""Writes tests/golden/g12_deskew.npz: a motion-compensated PointCloud2 case that keeps tests/deskew_ref.py from drifting together
with the kernel.

cloud   = 300 points in 22-byte records (x y z intensity ring time: time FLOAT32 at 18, unaligned), height 1: uniform in a
          16 x 16 x 6 m box, a few NaN / inf coordinates, a NaN time, times before the first and after the last knot, a few points
          beyond range.max
motion  = 0.3 rad about a tilted axis and 0.5 m in 0.1 s, 9 knots (the first the identity), times 100.0 .. 100.1 s
outputs = tests/deskew_ref.py on those bytes: origins, directions, points, mask, the five counters

    python tests/golden/make_g12_deskew.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import deskew_ref as dr  # noqa: E402

STATS = ("n_points", "n_finite", "n_valid", "n_time_clamped", "n_time_nonfinite")
LAYOUT = ("width", "height", "point_step", "row_step", "offset_x", "offset_y", "offset_z", "datatype")


def build():
    rng = np.random.RandomState(12)
    n = 300
    p = np.c_[rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-3, 3, n)].astype(np.float32)
    p[rng.randint(0, n, 5), rng.randint(0, 3, 5)] = np.nan
    p[rng.randint(0, n, 2), 2] = np.inf
    p[rng.randint(0, n, 4)] *= np.float32(20.0)
    t = rng.uniform(0.0, 0.1, n).astype(np.float32)
    t[7] = np.nan
    t[11], t[13], t[17] = -0.01, 0.12, 0.1
    axis = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
    S0 = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    S1 = (np.r_[axis * np.sin(0.15), np.cos(0.15)], np.array([0.45, 0.2, -0.08]))
    kq, kt, ktimes = dr.motion_knots64(S0, S1, (100.0, 100.1), 100.0, 8)
    buf, lay, tf = dr.make_cloud(p, t, dr.FLOAT32, dr.FLOAT32, gap=6)
    tf = tf + (1.0, 100.0)
    res = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.5, 100.0)
    return dict(data=buf, layout=np.array([lay[k] for k in LAYOUT], np.uint32), time_field=np.array(tf, np.float64), knot_q=kq,
                knot_t=kt, knot_times=ktimes, range=np.array([0.5, 100.0], np.float32), origs=res["origs"], dirs=res["dirs"],
                points=res["points"], mask=res["mask"], stats=np.array([res["stats"][k] for k in STATS], np.uint32))


if __name__ == "__main__":
    out = build()
    np.savez_compressed(os.path.join(HERE, "g12_deskew.npz"), **out)
    print("g12_deskew.npz: points / finite / valid / clamped / time non-finite =", out["stats"])
