"""Meshes built by hand for the rasteriser's source 4, shared by tests/test_oracle_raster.py, tests/test_gpu_raster.py and
tools/raster_host_check.py; tests/texture_scene.py and tests/component_scene.py are imported read-only.

Every scene has K = (1, 1, 0, 0) and the identity pose, and its vertices lie at z = 1 unless it says otherwise, so that
sx = x and sy = y exactly and a vertex can be put on a pixel centre.  A triangle (a, b, c) with b below a and c to the right of
a has area2 < 0: it faces the camera.
"""
import numpy as np

import component_scene as cs
import texture_scene as ts

K = np.array([1.0, 1.0, 0.0, 0.0], np.float64)
POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], np.float64)
SMALL_LIMITS = (0, 64, 65536)


def _mesh(xy, faces, z=None, colour=False):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z = np.ones(len(xy)) if z is None else np.asarray(z, np.float64)
    X = np.stack([xy[:, 0] * z, xy[:, 1] * z, z], axis=1)                 # sx = x z / z: exact for z a power of two
    n = np.arange(len(X))
    grey = ((n * 37 + 11) % 256).astype(np.uint8)
    bgr = np.stack([(n * 53 + 5) % 256, (n * 29 + 90) % 256, (n * 71 + 200) % 256], axis=1).astype(np.uint8) if colour else None
    return dict(vertices=X, faces=np.asarray(faces, np.int64).reshape(-1, 3), grey=grey, colour=bgr)


# ---- a fan of eight triangles round a vertex on a pixel centre: its spokes run along a row, a column and both diagonals ----------
FAN_SHAPE = (17, 17)
FAN_CENTRE = 4                      # the centre's index lies between the rim's, so that spokes run in both index orders


def fan():
    rim = [(14, 8), (14, 14), (8, 14), (2, 14), (2, 8), (2, 2), (8, 2), (14, 2)]
    xy = rim[:FAN_CENTRE] + [(8, 8)] + rim[FAN_CENTRE:]
    idx = [k if k < FAN_CENTRE else k + 1 for k in range(8)]
    return _mesh(xy, [(FAN_CENTRE, idx[(k + 1) % 8], idx[k]) for k in range(8)], colour=True)


def fan_interior():
    """The pixels strictly inside the rim's square."""
    m = np.zeros(FAN_SHAPE[::-1], bool)
    m[3:14, 3:14] = True
    return m


# ---- a quad split along a diagonal through pixel centres; the second triangle in each of its corner orders ----------------------
QUAD_SHAPE = (11, 11)
QUAD_SECOND = ((0, 2, 1), (2, 1, 0), (1, 0, 2))


def quad(order):
    return _mesh([(1, 1), (9, 1), (9, 9), (1, 9)], [(0, 3, 2), QUAD_SECOND[order]])


def quad_interior():
    m = np.zeros(QUAD_SHAPE[::-1], bool)
    m[2:9, 2:9] = True
    return m


# ---- two coincident triangles: the one with the lower index shows --------------------------------------------------------------
def coincident():
    tri = [(2, 2), (2, 9), (9, 2)]
    return _mesh(tri + tri, [(3, 4, 5), (0, 1, 2)])


# ---- a triangle over the whole of a 64 x 48 image behind 300 small ones: more than one workgroup of triangles, a ragged last one
FULL_SHAPE = (64, 48)


def full():
    xy, z, faces = [(-10, -10), (-10, 200), (300, -10)], [1.0, 1.0, 1.0], [(0, 1, 2)]
    for r in range(15):
        for c in range(20):
            x, y, n = 1.0 + 3.0 * c, 1.0 + 3.0 * r, len(xy)
            xy += [(x, y), (x, y + 2.5), (x + 2.5, y)]
            z += [0.5] * 3
            faces.append((n, n + 1, n + 2))
    return _mesh(xy, faces, z, colour=True)


# ---- triangles partly outside the image, wholly outside it, behind the camera and across z_near ---------------------------------
CLIP_SHAPE, CLIP_NEAR = (16, 12), 0.5


def clip():
    xy = [(-5, -5), (-5, 8), (8, -5),              # partly outside
          (100, 100), (100, 110), (110, 100),       # wholly outside
          (3, 3), (3, 9), (9, 3),                   # behind the camera
          (6, 2), (6, 11), (15, 2),                 # across z_near: one vertex in front of it
          (8, 5), (8, 10), (13, 5),                 # beyond z_near, nearer than the first
          (-3.5, 4.25), (-3.5, 30), (20, 4.25)]     # partly outside, off the pixel centres
    z = [1.0] * 6 + [-1.0] * 3 + [0.25, 1.0, 1.0] + [0.75] * 3 + [2.0] * 3
    return _mesh(xy, [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17)], z)


# ---- a triangle of zero area and one with a repeated index, beside one that shows ------------------------------------------------
DEGENERATE_SHAPE = (8, 8)


def degenerate():
    return _mesh([(1, 1), (3, 3), (5, 5), (1, 2), (1, 6), (5, 2)], [(0, 1, 2), (3, 3, 4), (3, 4, 5), (4, 5, 5)])


def scenes():
    """name -> (mesh, shape, z_near)."""
    out = {"fan": (fan(), FAN_SHAPE, 0.0), "coincident": (coincident(), (12, 12), 0.0), "full": (full(), FULL_SHAPE, 0.0),
           "clip": (clip(), CLIP_SHAPE, CLIP_NEAR), "degenerate": (degenerate(), DEGENERATE_SHAPE, 0.0),
           "one_pixel": (_mesh([(-2, -2), (-2, 3), (3, -2)], [(0, 1, 2)]), (1, 1), 0.0)}
    for order in range(3):
        out["quad%d" % order] = (quad(order), QUAD_SHAPE, 0.0)
    return out


# ---- the sphere's weld and its views ------------------------------------------------------------------------------------------
SPHERE_VIEWS = tuple(ts.AXES) + (ts.POSES[1],)
BIG_SHAPE = (4 * ts.W, 4 * ts.H)                    # 116 x 92
BIG_K = np.array([4.0 * ts.K[0], 4.0 * ts.K[1], 4.0 * ts.K[2] + 1.5, 4.0 * ts.K[3] + 1.5], np.float64)
CENTRE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], np.float64)      # inside the sphere, looking along +z


def sphere():
    return cs.oracle_mesh("sphere", 1)
