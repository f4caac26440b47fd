"""Scenes and the case table shared by tests/test_oracle_sgm.py, tests/test_gpu_sgm.py and tools/sgm_host_check.py
(DESIGN.md §19): the scenes of tests/dense_scene.py, and the same two surfaces with the texture replaced by a flat grey
128 inside a world rectangle -- a wall without texture, where every plane of the sweep costs the same.
"""
import numpy as np

import dense_oracle as do
import dense_scene as ds

FLAT = 128.0
PLANE_RECT = (-1.0, -0.2, -0.6, 0.6)                      # x0 < X < x1, y0 < Y < y1 in the world
STEP_RECT = (-0.9, -0.3, -0.5, 0.5)                       # on the near level of the step (world x < ds.STEP_EDGE)
PLANE_SURFACE = ("plane", ds.plane_z(ds.TRUE_PLANE))
STEP_SURFACE = ("step", ds.plane_z(ds.NEAR_PLANE), ds.plane_z(ds.FAR_PLANE))
P1, P2 = 36, 288                                          # 2 n and 16 n for radius 1 and two sources
K_ROW = np.array([64.0, 64.0, 16.0, 0.0], np.float64)      # the principal point on the one row / the one column
K_COLUMN = np.array([64.0, 64.0, 0.0, 9.0], np.float64)
UPRIGHT = {0: ds.REF, 1: ds._pose([0, ds.BASELINE, 0], [0, 0, 0]), 2: ds._pose([0, -ds.BASELINE, 0], [0, 0, 0])}   # ds.PURE turned


def render_flat(pose, surface, rect, Kc=ds.K, w=ds.W, h=ds.H):
    """``dense_scene.render`` with the texture replaced by FLAT where the hit point lies inside `rect`."""
    t, q = do.normalise_pose(pose)
    R = do.rotation(q)
    x, y = do.rays(Kc, w, h)
    d = np.stack([x, y, np.ones_like(x)], axis=2) @ R.T
    if surface[0] == "plane":
        P = ds._hit_plane(t, d, surface[1])
    else:
        near, far = ds._hit_plane(t, d, surface[1]), ds._hit_plane(t, d, surface[2])
        P = np.where((near[..., 0] < ds.STEP_EDGE)[..., None], near, far)
    X, Y = P[..., 0], P[..., 1]
    tex = np.where((X > rect[0]) & (X < rect[1]) & (Y > rect[2]) & (Y < rect[3]), FLAT, ds.texture(X, Y))
    return np.clip(np.floor(tex + 0.5), 0, 255).astype(np.uint8)


def flat_views(surface, rect, rig=ds.RIG, Kc=ds.K, w=ds.W, h=ds.H):
    """slot -> (image, K, pose) of the rig over the surface with its flat patch."""
    return {s: (render_flat(rig[s], surface, rect, Kc, w, h), Kc, rig[s]) for s in sorted(rig)}


def flat_plane_scene():
    return flat_views(PLANE_SURFACE, PLANE_RECT)


def flat_step_scene():
    return flat_views(STEP_SURFACE, STEP_RECT)


def flat_share(scene):
    """The share of a flat scene's reference pixels that show the patch."""
    return float((scene[0][0] == int(FLAT)).mean())


# The exact-equality cases: (name, width, height, planes, radius, trunc, source slots, p1, p2, paths, scene).  Each is the
# smallest shape at which one part can go wrong (the table of DESIGN.md §19.4).
CASES = [
    ("paths8", ds.W, ds.H, 12, 1, 20, (1, 2), P1, P2, 8, "step"),
    ("paths4", ds.W, ds.H, 12, 1, 20, (1, 2), P1, P2, 4, "step"),
    ("least_penalties", ds.W, ds.H, 12, 0, 255, (1,), 1, 1, 8, "step"),             # P1 = P2 = 1
    ("largest_values", ds.W, ds.H, 12, 4, 255, (1, 2, 3), 5000, 1 << 20, 8, "step"),  # invalid warps behind the camera
    ("twin", ds.W, ds.H, 12, 1, 255, (2, 3, 4), P1, P2, 4, "step"),
    ("two_planes", ds.W, ds.H, 2, 1, 255, (1, 2), P1, P2, 8, "step"),                # every d is an end of the range
    ("planes70", ds.SMALL_W, ds.SMALL_H, 70, 1, 20, (1, 2), P1, P2, 8, "step"),      # more planes than lanes in a wave
    ("planes130", ds.SMALL_W, ds.SMALL_H, 130, 0, 255, (1, 2), P1, P2, 4, "step"),   # an odd count of planes per lane
    ("one_row", 33, 1, 12, 1, 255, (1, 2), P1, P2, 8, "step"),                       # lines of length 1; two tiles across
    ("one_column", 1, 19, 12, 1, 255, (1, 2), P1, P2, 8, "step"),                    # lines of length 1
    ("flat_plane", ds.W, ds.H, 12, 1, 20, (1, 2), P1, P2, 8, "flat_plane"),          # textureless region
]

# Beyond the table: eight and sixteen planes a lane (D > 256, > 512), the two instantiations the table does not reach.
MANY_PLANES_CASES = [
    ("planes300", 9, 5, 300, 0, 255, (1, 2), P1, P2, 8, "step"),
    ("planes520", 9, 5, 520, 0, 255, (1, 2), P1, P2, 4, "step"),
]


def case_views(case):
    """slot -> (image, K, pose) of a case's scene at its size."""
    w, h, scene = case[1], case[2], case[10]
    if scene == "flat_plane":
        return flat_plane_scene()
    if h == 1:                                            # one row: only a rig that moves along it keeps a warp inside it
        return ds.step_scene(ds.PURE, Kc=K_ROW, w=w, h=h)
    if w == 1:
        return ds.step_scene(UPRIGHT, Kc=K_COLUMN, w=w, h=h)
    return ds.case_views(w, h)


def case_oracle(case, ref=0):
    """The oracle's semi-global sweep of slot `ref` against the case's other slots."""
    import sgm_oracle as so
    name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
    views = case_views(case)
    slots = (0,) + tuple(src)
    return so.sweep_sgm(views[ref][0], views[ref][1], views[ref][2], [views[s] for s in slots if s != ref], ds.W_MIN, ds.W_MAX,
                        D, radius, trunc, p1, p2, paths)
