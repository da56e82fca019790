"""Writes tests/golden/g8_segmentation_cube.npz: the map segmentation's expected output on the committed cube simulation.

simulated = `ranges` and `normals` of pose 0 in g2_cube_32x32.npz (config C1: 32 x 32 spherical model, the 972-triangle cube room);
real      = those ranges doctored as tests/test_cpp_adapters.py::test_simulator_example_matches_oracle doctors its scan (a block x 0.6,
            a block + 1.5 m, two rows of 0.0, four beams of 150.0);
labels and clouds = tests/segmentation_ref.py on them with the default thresholds (0.15, 0.15).

    python tests/golden/make_g8_segmentation.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import segmentation_ref as sr  # noqa: E402
from rmcl_amd import synthetic as syn  # noqa: E402


def build():
    g2 = np.load(os.path.join(HERE, "g2_cube_32x32.npz"))
    n = 32 * 32
    r_sim, n_sim = g2["ranges"][:n], g2["normals"][:n]
    model = syn.model_c1()
    real = sr.doctor_cube_scan(r_sim)
    ref = sr.segment(real, r_sim, n_sim, syn.model_directions(model), np.zeros(3), model.range.min, model.range.max, 0.15, 0.15)
    return dict(ranges_real=real, labels=ref["labels"], outlier_scan=ref["outlier_scan"], outlier_map=ref["outlier_map"])


if __name__ == "__main__":
    out = build()
    np.savez_compressed(os.path.join(HERE, "g8_segmentation_cube.npz"), **out)
    print("g8_segmentation_cube.npz: labels none / inlier / scan / map =", np.bincount(out["labels"], minlength=4))
