"""Scenes and case tables shared by tests/test_oracle_census.py, tests/test_gpu_census.py and tools/census_host_check.py
(DESIGN.md §20): the scenes of tests/dense_scene.py and tests/sgm_scene.py with the source views re-exposed, as key frames
taken seconds apart by a camera with automatic exposure and gain are."""
import numpy as np

import dense_scene as ds
import sgm_scene as ss

EXPOSURE = {1: (1.25, 15.0), 2: (0.8, -10.0)}             # slot -> (gain, bias)


def expose(img, gain, bias):
    """clip(floor(gain I + bias + 0.5)) to 0 .. 255, uint8."""
    return np.clip(np.floor(gain * np.asarray(img, np.uint8).astype(np.float64) + bias + 0.5), 0, 255).astype(np.uint8)


def exposed(views, exposure=EXPOSURE):
    """slot -> (image, K, pose) with the slots named in `exposure` re-exposed."""
    return {s: ((expose(v[0], *exposure[s]) if s in exposure else v[0]), v[1], v[2]) for s, v in views.items()}


def monotone_table(seed=5):
    """A strictly increasing table on 0 .. 127 with values in 0 .. 255: order-preserving, so descriptors do not change."""
    t = np.sort(np.random.default_rng(seed).choice(256, 128, replace=False)).astype(np.uint8)
    assert (np.diff(t.astype(np.int64)) > 0).all()
    return t


# ---- descriptor cases: (name, width, height, kind) ---------------------------------------------------------------------------
DESCRIPTOR_CASES = [
    ("61x47", 61, 47, "scene"),
    ("37x19", 37, 19, "scene"),
    ("one_tile", 32, 16, "random"),                       # exactly one 32 x 16 tile
    ("past_two_edges", 65, 33, "random"),                 # one pixel past two tile edges
    ("one_row", 33, 1, "random"),
    ("one_column", 1, 19, "random"),
    ("random", 61, 47, "random"),
    ("constant", 61, 47, "constant"),
    ("border255", 37, 19, "border255"),                   # a 255-valued border pixel beside the 255 fill of the halo
]


def descriptor_image(case):
    name, w, h, kind = case
    if kind == "scene":
        return ds.case_views(w, h)[0][0]
    if kind == "constant":
        return np.full((h, w), 93, np.uint8)
    img = np.random.default_rng(w * 131 + h).integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "border255":
        img[0, 0] = img[h - 1, w - 2] = img[h // 2, w - 1] = 255
    return img


# ---- sweep cases: the shapes of dense_scene.CASES with the census cost (trunc bounds a Hamming distance of 62 bits) ----------
SWEEP_CASES = ds.CASES

# ---- semi-global cases: (name, width, height, planes, radius, trunc, source slots, p1, p2, paths, scene), as sgm_scene.CASES --
SGM_CASES = [
    ("paths8", ds.W, ds.H, 12, 1, 20, (1, 2), ss.P1, ss.P2, 8, "step"),
    ("paths4", ds.W, ds.H, 12, 1, 20, (1, 2), ss.P1, ss.P2, 4, "step"),
    ("planes70", ds.SMALL_W, ds.SMALL_H, 70, 1, 20, (1, 2), ss.P1, ss.P2, 8, "step"),
    ("one_row", 33, 1, 12, 1, 255, (1, 2), ss.P1, ss.P2, 8, "step"),
]


def sgm_case_views(case):
    return ss.case_views(case)
