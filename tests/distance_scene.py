"""Targets and query points built by hand for the distance's source 4, shared by tests/test_oracle_distance.py,
tests/test_gpu_distance.py and tools/distance_host_check.py; tests/component_scene.py and
tests/simplify_oracle.py are imported read-only.  Coordinates are small integers or dyadic fractions, so that ties are exact.
"""
import functools

import numpy as np

import component_scene as cs
import fusion_scene as fs
import simplify_oracle as so

GRIDS = (1, 2, 5, 7, 128, 0)                 # ekf_distance_set_grid: 0 is automatic
NAN, INF = float("nan"), float("inf")


def _mesh(vertices, faces):
    return dict(vertices=np.asarray(vertices, np.float64).reshape(-1, 3), faces=np.asarray(faces, np.int64).reshape(-1, 3))


# ---- one triangle and points in each of the seven regions of Ericson's routine ---------------------------------------------------
def regions():
    """A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0); n = (0, 0, 16): +z is the positive side."""
    mesh = _mesh([(0, 0, 0), (4, 0, 0), (0, 4, 0)], [(0, 1, 2)])
    points = [(-1, -1, 0), (6, -1, 0), (-1, 6, 0),            # the vertex regions A, B, C, in the plane: side 0
              (2, -2, 0), (-2, 2, 0), (4, 4, 0),              # the edge regions AB, AC, BC
              (1, 1, 3), (1, 1, -3), (1, 1, 0),               # the interior: above (+1), below (-1), in the plane (0, dist 0)
              (4, 0, 0), (0, 0, 0), (2, 0, 0), (2, 2, 0),     # on a vertex and on an edge: dist 0
              (-1, -1, 2), (6, -1, -2), (2, -2, 0.5), (3, 3, -0.25), (0.5, 0.25, 0.125)]
    return mesh, np.asarray(points, np.float64)


REGION_TRUTH = {0: (0, 0, 0), 1: (4, 0, 0), 2: (0, 4, 0), 3: (2, 0, 0), 4: (0, 2, 0), 5: (2, 2, 0), 6: (1, 1, 0), 7: (1, 1, 0), 8: (1, 1, 0)}
REGION_SIDE = {6: 1, 7: -1, 8: 0, 0: 0, 13: 1, 14: -1, 15: 1, 16: -1, 17: 1}


# ---- two triangles that share an edge, in both index orders: a point equidistant from both belongs to the lower index -----------
def shared_edge(order):
    faces = [(0, 1, 2), (1, 3, 2)]
    mesh = _mesh([(0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 0)], faces[::-1] if order else faces)
    points = [(2, 2, 1), (2, 2, 0), (1, 3, -2), (3, 1, 0.5), (4, 0, 3), (0, 4, -1), (1, 1, 1), (3, 3, 1)]
    return mesh, np.asarray(points, np.float64)


def coincident():
    tri = [(0, 0, 1), (4, 0, 1), (0, 4, 1)]
    return _mesh(tri + tri, [(3, 4, 5), (0, 1, 2)]), np.asarray([(1, 1, 2), (1, 1, 1), (-3, -3, 0), (5, 5, 5), (2, 2, 1)], np.float64)


# ---- the tie across shells: the cube [-1, 1]^3 and a small triangle near x = 9 ----------------------------------------------------
def cube_mesh():
    """Face x = +1 is triangles 0 and 1, face x = -1 is 2 and 3; then y = +1, y = -1, z = +1, z = -1; triangle 12 stretches the box
    to x = 9, so that with g = 5 the cells are 2 wide along x, one along y and z: the origin lies in cell 0 with face x = -1, and
    face x = +1 begins cell 1."""
    V = [(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)]            # index = (x > 0) + 2 (y > 0) + 4 (z > 0)
    V += [(9, 0, 0), (9, 0.5, 0), (9, 0, 0.5)]
    F = [(1, 3, 7), (1, 7, 5), (0, 4, 6), (0, 6, 2), (2, 6, 7), (2, 7, 3), (0, 1, 5), (0, 5, 4), (4, 5, 7), (4, 7, 6), (0, 2, 3), (0, 3, 1),
         (8, 9, 10)]
    return _mesh(V, F)


def tie_shells():
    """The origin is at distance exactly 1 from all twelve triangles of the cube, and triangle 0 must win; the other points are far
    outside the box, on its faces and corners, and three that are not finite."""
    points = [(0, 0, 0), (0.5, 0, 0), (-0.5, 0.25, 0), (1000000, 0, 0), (-1000000, 2000000, -3000000), (0, 0, 1048576.5),
              (-1, 0, 0), (9, 1, 1), (9, -1, -1), (-1, -1, -1), (4, 1, 0), (3, 0, 0), (7, 0.125, 0.125), (5, 0, 0),
              (NAN, 0, 0), (0, INF, 0), (0, 0, -INF), (8.75, 0.25, 0.25)]
    return cube_mesh(), np.asarray(points, np.float64)


# ---- a zero-area triangle and two with a repeated index among valid ones: they never win ------------------------------------------
def degenerate():
    V = [(0, 0, 0), (4, 0, 0), (0, 4, 0),           # valid: triangle 3
         (0, 0, 2), (1, 1, 2), (2, 2, 2),           # collinear: zero area, right above the valid one
         (1, 1, 1), (3, 1, 1),                      # the corners of the repeated-index triangles, nearer still
         (8, 8, 8), (8, 9, 8), (9, 8, 8)]           # valid: triangle 4
    F = [(3, 4, 5), (6, 6, 7), (6, 7, 7), (0, 1, 2), (8, 9, 10)]
    points = [(1, 1, 1.5), (1, 1, 2), (3, 1, 1), (8, 8, 9), (2, 2, 2), (5, 5, 5)]
    return _mesh(V, F), np.asarray(points, np.float64)


def only_degenerate():
    mesh, points = degenerate()
    return dict(vertices=mesh["vertices"], faces=mesh["faces"][:3]), points


# ---- a triangle that spans the whole box among 300 small ones, and 301 points: a ragged second workgroup ---------------------------
def spanning():
    rng = np.random.default_rng(31)
    V, F = [(-1, -1, -0.5), (17, -1, 2), (-1, 17, 2)], []
    for k in range(3):
        for j in range(10):
            for i in range(10):
                n, x, y, z = len(V), 1.5 * i, 1.5 * j, 0.5 * k + 0.125 * ((i + j) % 3)
                V += [(x, y, z), (x + 1, y, z + 0.25), (x, y + 1, z)]
                F.append((n, n + 1, n + 2))
    F.insert(150, (0, 1, 2))                         # the spanning triangle in the middle of the list: 301 triangles
    points = rng.integers(-24, 160, size=(301, 3)) / 8.0
    points[7] = (NAN, 1, 1)
    return _mesh(V, F), points


def scenes():
    """name -> (mesh, points)."""
    out = {"regions": regions(), "shared0": shared_edge(0), "shared1": shared_edge(1), "coincident": coincident(), "tie": tie_shells(),
           "degenerate": degenerate(), "spanning": spanning()}
    mesh, points = spanning()
    out["one_point"] = (mesh, points[3:4].copy())
    return out


# ---- the 17 x 15 x 13 sphere: its weld and the weld simplified at a cell of `factor` voxels ----------------------------------------
FACTORS = (1.0, 2.0, 3.5)


def _plain(m):
    return dict(vertices=np.ascontiguousarray(m["vertices"], np.float64), faces=np.ascontiguousarray(m["faces"]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def sphere_weld():
    return _plain(cs.oracle_mesh("sphere", 1))


@functools.lru_cache(maxsize=None)
def sphere_simplified(factor):
    m = cs.oracle_mesh("sphere", 1)
    return _plain(so.as_mesh(so.simplify(m, fs.SPHERE_ORIGIN, fs.SPHERE_DIMS, fs.SPHERE_VOXEL, factor * fs.SPHERE_VOXEL)))
