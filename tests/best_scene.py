"""The rig and the case table shared by tests/test_oracle_best.py, tests/test_gpu_best.py and tools/best_host_check.py
(DESIGN.md §21): the scenes of tests/dense_scene.py seen by nine cameras, the five of ``dense_scene.RIG`` and four more poses
of the sideways rig, so that a sweep can have the 8 sources the entry point allows."""
import numpy as np

import best_oracle as bo
import dense_scene as ds

# slot -> pose.  0 .. 4: dense_scene.RIG (3 stands beyond the near planes, 4 is the reference's twin); 5 .. 8: the sideways rig
# at other baselines, heights and small rotations
RIG9 = dict(ds.RIG)
RIG9.update({5: ds._pose([0.3, -0.03, 0.02], [0.005, -0.015, 0.0]),
             6: ds._pose([-0.3, 0.04, 0.0], [-0.004, 0.02, 0.003]),
             7: ds._pose([0.7, 0.0, -0.04], [0.0, -0.04, -0.002]),
             8: ds._pose([-0.7, -0.02, 0.03], [0.006, 0.045, 0.0])})
MAX_VIEWS = 9
ALL8 = (1, 2, 3, 4, 5, 6, 7, 8)


def case_views(w, h, scene="step"):
    """slot -> (image, K, pose) of the nine cameras over the step (or the plane) scene at the case's size."""
    make = ds.step_scene if scene == "step" else ds.plane_scene
    return make(RIG9, Kc=ds.K if (w, h) == (ds.W, ds.H) else ds.K_SMALL, w=w, h=h)


def _p(radius, n_best):
    return bo.default_penalties(radius, n_best)


# The exact-equality cases: (name, width, height, planes, radius, trunc, source slots, n_best, census, paths, p1, p2).  Each is
# the smallest shape at which one part can go wrong (the table of DESIGN.md §21.4).
W, H, SW, SH, D = ds.W, ds.H, ds.SMALL_W, ds.SMALL_H, ds.PLANES
CASES = [
    ("v1_b1_r0", W, H, D, 0, 255, (1,), 1, 0, 0, 0, 0),                       # one view: half a pair; radius 0
    ("v2_b1_t20", W, H, D, 1, 20, (1, 2), 1, 0, 0, 0, 0),                     # one full pair
    ("v2_b2_t20", W, H, D, 1, 20, (1, 2), 2, 0, 0, 0, 0),
    ("v3_b1_r4", W, H, D, 4, 255, (1, 2, 3), 1, 0, 0, 0, 0),                  # a half-filled pair; the largest sums; slot 3
    ("v3_b2_r4", W, H, D, 4, 255, (1, 2, 3), 2, 0, 0, 0, 0),
    ("v3_b3_r4", W, H, D, 4, 255, (1, 2, 3), 3, 0, 0, 0, 0),
    ("v8_b1", W, H, D, 1, 255, ALL8, 1, 0, 0, 0, 0),                          # every pair
    ("v8_b4", W, H, D, 1, 255, ALL8, 4, 0, 0, 0, 0),
    ("v8_b7", W, H, D, 2, 40, ALL8, 7, 0, 0, 0, 0),
    ("v8_b8", W, H, D, 1, 255, ALL8, 8, 0, 0, 0, 0),
    ("twin_b2", W, H, D, 1, 255, (2, 3, 4), 2, 0, 0, 0, 0),                   # zero fraction on the last row and column
    ("two_planes", W, H, 2, 1, 255, (1, 2), 1, 0, 0, 0, 0),
    ("small_b1", SW, SH, D, 1, 255, (1, 2), 1, 0, 0, 0, 0),                   # less than a tile
    ("small_two_planes", SW, SH, 2, 2, 40, (1, 2, 5), 2, 0, 0, 0, 0),
    ("census_v2_b1", W, H, D, 2, 62, (1, 2), 1, 1, 0, 0, 0),
    ("census_v3_b2", W, H, D, 1, 40, (1, 2, 3), 2, 1, 0, 0, 0),
    ("census_v8_b4", SW, SH, D, 4, 62, ALL8, 4, 1, 0, 0, 0),
    ("sgm4_v2_b1", W, H, D, 1, 255, (1, 2), 1, 0, 4) + _p(1, 1),
    ("sgm8_v3_b2", W, H, D, 1, 20, (1, 2, 3), 2, 0, 8) + _p(1, 2),
    ("sgm8_planes70", SW, SH, 70, 1, 20, (1, 2), 1, 0, 8) + _p(1, 1),         # more planes than lanes in a wave
    ("sgm4_census_v2_b1", W, H, D, 2, 62, (1, 2), 1, 1, 4) + _p(2, 1),
    ("sgm8_census_v8_b4", W, H, D, 1, 40, ALL8, 4, 1, 8) + _p(1, 4),
    ("sgm8_census_planes70", SW, SH, 70, 1, 20, (1, 2, 5), 2, 1, 8) + _p(1, 2),
]

# n_best = n_src against the existing sweeps: (name, radius, trunc, source slots, census, paths)
IDENTITY_CASES = [
    ("ad", 1, 20, (1, 2), 0, 0),
    ("ad_v3", 4, 255, (1, 2, 3), 0, 0),
    ("census", 2, 62, (1, 2, 3), 1, 0),
    ("sgm", 1, 20, (1, 2), 0, 8),
    ("sgm_census", 1, 40, (1, 2, 3), 1, 4),
]


def case_oracle(case):
    """(views, the oracle's result) of a case of CASES."""
    name, w, h, planes, radius, trunc, src, n_best, census, paths, p1, p2 = case
    views = case_views(w, h)
    want = bo.sweep(views[0][0], views[0][1], views[0][2], [views[s] for s in src], n_best, ds.W_MIN, ds.W_MAX, planes, radius,
                    trunc, bool(census), paths, p1, p2)
    return views, want
