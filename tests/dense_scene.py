"""Scenes and shapes shared by tests/test_oracle_dense.py and tests/test_gpu_dense.py.

The frame is 61 x 47 (no multiple of the 32 x 16 tile: every tile-edge case occurs), K is dyadic (fx = fy = 64, cx = 30,
cy = 23), the reference camera stands at the origin looking down +z.  A view is rendered by casting the ray of every pixel
onto a surface given in the world (= reference) frame and reading a procedural texture at the hit point: an inverse warp
through a known depth field.  Two surfaces: the plane z = 1/w_k of plane index TRUE_PLANE, and a two-level step (near for
world x < STEP_EDGE, far beyond).  The rig translates sideways and rotates slightly; FORWARD stands beyond the near
planes (they are behind it) and TWIN stands where the reference does (its warp of the last row / column has zero fraction).
"""
import numpy as np

import dense_oracle as do

W, H = 61, 47
SMALL_W, SMALL_H = 37, 19                                 # smaller than one tile
K = np.array([64.0, 64.0, 30.0, 23.0], np.float64)
K_SMALL = np.array([64.0, 64.0, 18.0, 9.0], np.float64)
W_MIN, W_MAX, PLANES = 0.15, 0.40, 12
TRUE_PLANE = 5
NEAR_PLANE, FAR_PLANE = 8, 3
STEP_EDGE = 0.2
BASELINE = 0.5

REF = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _pose(t, rotvec):
    r = np.asarray(rotvec, np.float64)
    ang = float(np.sqrt(r @ r))
    q = np.array([1.0, 0, 0, 0]) if ang == 0 else np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * r / ang])
    return np.concatenate([np.asarray(t, np.float64), q])


# slot -> pose.  1, 2: the sideways rig; 3: FORWARD (beyond the planes nearer than z = 3); 4: TWIN of the reference
RIG = {0: REF,
       1: _pose([BASELINE, 0.02, 0.0], [0.0, -0.03, 0.004]),
       2: _pose([-BASELINE, 0.0, 0.05], [0.01, 0.03, -0.006]),
       3: _pose([0.1, 0.0, 3.0], [0.0, 0.0, 0.0]),
       4: REF.copy()}
PURE = {0: REF, 1: _pose([BASELINE, 0, 0], [0, 0, 0]), 2: _pose([-BASELINE, 0, 0], [0, 0, 0])}


def plane_z(k, w_min=W_MIN, w_max=W_MAX, D=PLANES):
    return float(do.plane_depth(w_min, do.plane_step(w_min, w_max, D), k))


def texture(X, Y):
    """A smooth deterministic pattern with no short period: 0 .. 255 before rounding."""
    v = (np.sin(7.3 * X + 1.1 * Y) + np.sin(2.9 * X - 6.1 * Y + 0.7) + np.sin(11.7 * X + 4.3 * Y + 2.1)
         + np.sin(-4.7 * X + 9.9 * Y + 0.3) + np.sin(17.1 * X - 2.3 * Y) * 0.7 + np.sin(1.3 * X + 15.7 * Y + 1.9) * 0.7)
    return 127.5 + 23.0 * v


def _hit_plane(o, d, z):
    s = (z - o[2]) / d[..., 2]
    return o + s[..., None] * d


def render(pose, surface, Kc=K, w=W, h=H):
    """(image uint8, true depth along the view's own z axis) of `surface` = ("plane", z) or ("step", z_near, z_far)."""
    t, q = do.normalise_pose(pose)
    R = do.rotation(q)
    x, y = do.rays(Kc, w, h)
    d = np.stack([x, y, np.ones_like(x)], axis=2) @ R.T                     # ray directions in the world
    if surface[0] == "plane":
        P = _hit_plane(t, d, surface[1])
    else:
        near, far = _hit_plane(t, d, surface[1]), _hit_plane(t, d, surface[2])
        P = np.where((near[..., 0] < STEP_EDGE)[..., None], near, far)
    img = np.clip(np.floor(texture(P[..., 0], P[..., 1]) + 0.5), 0, 255).astype(np.uint8)
    depth = (P - t) @ R[:, 2]
    return img, depth


def views(surface, rig=RIG, slots=None, Kc=K, w=W, h=H):
    """slot -> (image, K, pose) of the rig."""
    return {s: (render(rig[s], surface, Kc, w, h)[0], Kc, rig[s]) for s in (slots if slots is not None else sorted(rig))}


def plane_scene(rig=RIG, **kw):
    return views(("plane", plane_z(TRUE_PLANE)), rig, **kw)


def step_scene(rig=RIG, **kw):
    return views(("step", plane_z(NEAR_PLANE), plane_z(FAR_PLANE)), rig, **kw)


def true_inverse_depth(surface, w=W, h=H, Kc=K):
    return 1.0 / render(REF, surface, Kc, w, h)[1]


def max_disparity(Kc=K):
    """The largest disparity of the sideways rig over the swept range, in pixels."""
    return float(Kc[0] * BASELINE * W_MAX)


def interior(radius, w=W, h=H):
    m = int(np.ceil(radius + max_disparity()))
    mask = np.zeros((h, w), bool)
    mask[m:h - m, m:w - m] = True
    return mask


# The exact-equality cases of the GPU test: (name, width, height, planes, radius, trunc, source slots)
CASES = [
    ("r0_t255_v1", W, H, PLANES, 0, 255, (1,)),
    ("r1_t20_v2", W, H, PLANES, 1, 20, (1, 2)),
    ("r4_t255_v3", W, H, PLANES, 4, 255, (1, 2, 3)),
    ("r1_t255_twin", W, H, PLANES, 1, 255, (2, 3, 4)),
    ("r4_t20_v2", W, H, PLANES, 4, 20, (1, 2)),
    ("two_planes", W, H, 2, 1, 255, (1, 2)),
    ("small", SMALL_W, SMALL_H, PLANES, 1, 255, (1, 2)),
]


def case_views(w, h):
    """The step scene at the case's size."""
    return step_scene(Kc=K if (w, h) == (W, H) else K_SMALL, w=w, h=h)
