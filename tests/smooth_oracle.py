"""numpy restatement of the smoothing contract of the welded or pruned mesh, written from the contract.

The input is a mesh (X, F): X (n_vert, 3) float64, F (n_tri, 3) with three distinct indices a triangle.

  1. The adjacency is a function of F alone.  T(v): the ascending list of the triangles that contain v, inc(v) = |T(v)|.
     N(v): the ascending list of the distinct w != v that share a triangle with v, deg(v) = |N(v)|.  m(v, w): the number of
     triangles that hold both.  boundary(v) = 1 iff some w has m(v, w) = 1.
  2. One step with factor f, every operation rounded once: s = X[w0][c], then s = s + X[wi][c] in the order of N(v);
     mean = s / (double) deg(v); X'[v][c] = X[v][c] + f * (mean - X[v][c]).  With pin_boundary, a vertex with boundary(v) = 1
     keeps its bits.
  3. A run is ``iterations`` times a step with lam and then, unless mu == 0, a step with mu.  faces, key, grey and colour
     are the source's rows.
  4. Normals, on request, from the final positions: over t in T(v) ascending, A, B, C = X[F[t][0..2]], e1 = B - A,
     e2 = C - A, the cross products (e1[1] e2[2] - e1[2] e2[1], e1[2] e2[0] - e1[0] e2[2], e1[0] e2[1] - e1[1] e2[0]) summed
     from left to right from the first triangle's; len = sqrt((a0 a0 + a1 a1) + a2 a2); each a_c / len rounded once to
     float32; 0 0 0 where len is 0 or not finite.

Two independent implementations, which tests/test_oracle_smooth.py holds equal to each other bit for bit: a plain loop over
the vertices (``*_loop``), and a vectorised form that adds neighbour i (triangle i) of every vertex in round i.  A mesh is the
dict tests/mesh_oracle.py's ``weld`` returns: vertices, faces, grey, colour, normals, key.
"""
from collections import namedtuple

import numpy as np

# inc, deg (uint32), boundary (uint8); T(v) = tri[tri_first[v]:tri_first[v + 1]], N(v) = nbr[nbr_first[v]:nbr_first[v + 1]];
# mult: m(v, w) beside every entry of nbr
Adjacency = namedtuple("Adjacency", "inc deg boundary tri_first tri nbr_first nbr mult")

LAM, MU, ITERATIONS = 0.5, -0.53, 10


def _pack(lists, dtype=np.int64):
    first = np.zeros(len(lists) + 1, np.int64)
    first[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype) for x in lists]) if len(lists) and first[-1] else np.zeros(0, dtype)
    return first, flat.astype(dtype)


def adjacency_loop(faces, n_vert):
    """The adjacency by a loop over the triangles and then over the vertices, with Python lists and dicts."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    T = [[] for _ in range(n_vert)]
    M = [dict() for _ in range(n_vert)]
    for t, tri in enumerate(faces.tolist()):                         # t ascending: every T(v) comes out ascending
        for v in tri:
            T[v].append(t)
            for w in tri:
                if w != v:
                    M[v][w] = M[v].get(w, 0) + 1
    N = [sorted(m) for m in M]
    mult = [[m[w] for w in n] for m, n in zip(M, N)]
    inc = np.array([len(t) for t in T], np.uint32).reshape(-1)
    deg = np.array([len(n) for n in N], np.uint32).reshape(-1)
    boundary = np.array([1 if 1 in m.values() else 0 for m in M], np.uint8).reshape(-1)
    tri_first, tri = _pack(T)
    nbr_first, nbr = _pack(N)
    return Adjacency(inc, deg, boundary, tri_first, tri, nbr_first, nbr, _pack(mult)[1])


def adjacency(faces, n_vert):
    """The adjacency by sorting: the corners by (vertex, triangle), the ordered pairs of a triangle by (v, w)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    corner = faces.reshape(-1)
    order = np.argsort(corner, kind="stable")                        # stable: the triangles of a vertex stay ascending
    tri = order // 3
    tri_first = np.searchsorted(corner[order], np.arange(n_vert + 1))
    inc = np.diff(tri_first).astype(np.uint32)
    v = np.concatenate([faces[:, a] for a in range(3) for b in range(3) if a != b]) if len(faces) else np.zeros(0, np.int64)
    w = np.concatenate([faces[:, b] for a in range(3) for b in range(3) if a != b]) if len(faces) else np.zeros(0, np.int64)
    pair, mult = np.unique(v * max(n_vert, 1) + w, return_counts=True)
    pv, nbr = pair // max(n_vert, 1), pair % max(n_vert, 1)
    nbr_first = np.searchsorted(pv, np.arange(n_vert + 1))
    deg = np.diff(nbr_first).astype(np.uint32)
    boundary = np.zeros(n_vert, np.uint8)
    boundary[pv[mult == 1]] = 1
    return Adjacency(inc, deg, boundary, tri_first.astype(np.int64), tri.astype(np.int64), nbr_first.astype(np.int64),
                     nbr.astype(np.int64), mult.astype(np.int64))


def step_loop(X, adj, f, pin_boundary=False):
    """One step, vertex by vertex and coordinate by coordinate, on float64 scalars."""
    X = np.asarray(X, np.float64)
    out = X.copy()
    f = np.float64(f)
    for v in range(len(X)):
        if pin_boundary and adj.boundary[v]:
            continue
        ws = adj.nbr[adj.nbr_first[v]:adj.nbr_first[v + 1]]
        for c in range(3):
            s = X[ws[0], c]
            for w in ws[1:]:
                s = s + X[w, c]
            mean = s / np.float64(len(ws))
            out[v, c] = X[v, c] + f * (mean - X[v, c])
    return out


def step(X, adj, f, pin_boundary=False):
    """One step: round i adds neighbour i of every vertex that has one."""
    X = np.asarray(X, np.float64)
    deg = adj.deg.astype(np.int64)
    first = adj.nbr_first[:-1]
    s = np.zeros_like(X)
    for i in range(int(deg.max()) if len(deg) else 0):
        has = np.nonzero(deg > i)[0]
        rows = X[adj.nbr[first[has] + i]]
        s[has] = rows if i == 0 else s[has] + rows
    mean = s / deg.astype(np.float64)[:, None]
    out = X + np.float64(f) * (mean - X)
    if pin_boundary:
        keep = adj.boundary != 0
        out[keep] = X[keep]
    return out


def _cross(X, faces):
    A, B, C = X[faces[:, 0]], X[faces[:, 1]], X[faces[:, 2]]
    e1, e2 = B - A, C - A
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).reshape(-1, 3)


def _normalise(a):
    with np.errstate(all="ignore"):
        length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        ok = (length > 0.0) & (length < np.inf)
        return np.where(ok[:, None], (a / length[:, None]).astype(np.float32), np.float32(0.0)).astype(np.float32).reshape(-1, 3)


def normals_loop(X, faces, adj):
    """(n_vert, 3) float32, vertex by vertex, on float64 scalars."""
    X = np.asarray(X, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros((len(X), 3), np.float32)
    for v in range(len(X)):
        a = None
        for t in adj.tri[adj.tri_first[v]:adj.tri_first[v + 1]]:
            A, B, C = X[faces[t, 0]], X[faces[t, 1]], X[faces[t, 2]]
            e1, e2 = [B[c] - A[c] for c in range(3)], [C[c] - A[c] for c in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            a = n if a is None else [a[c] + n[c] for c in range(3)]
        if a is None:
            continue
        with np.errstate(all="ignore"):
            length = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
            if length > 0.0 and length < np.inf:
                out[v] = [np.float32(a[c] / length) for c in range(3)]
    return out


def normals(X, faces, adj):
    """(n_vert, 3) float32: round i adds triangle i of every vertex that has one."""
    X = np.asarray(X, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n = _cross(X, faces)
    inc = adj.inc.astype(np.int64)
    first = adj.tri_first[:-1]
    a = np.zeros_like(X)
    for i in range(int(inc.max()) if len(inc) else 0):
        has = np.nonzero(inc > i)[0]
        rows = n[adj.tri[first[has] + i]]
        a[has] = rows if i == 0 else a[has] + rows
    return _normalise(a)


def smooth(mesh, iterations=ITERATIONS, lam=LAM, mu=MU, pin_boundary=False, normals=False, loop=False):
    """The smoothed mesh: vertices and normals (None without ``normals``) new, every other row the source's."""
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    X = np.asarray(mesh["vertices"], np.float64).reshape(-1, 3)
    adj = (adjacency_loop if loop else adjacency)(faces, len(X))
    one = step_loop if loop else step
    if len(faces):
        for _ in range(int(iterations)):
            X = one(X, adj, lam, pin_boundary)
            if mu != 0:
                X = one(X, adj, mu, pin_boundary)
    out = dict(mesh)
    out["vertices"] = X.copy()
    out["normals"] = (normals_loop if loop else globals()["normals"])(X, faces, adj) if normals else None
    return out


def roughness(X, adj):
    """The mean distance of a vertex from the centroid of its neighbours (a measure for the tests, not part of the contract)."""
    X = np.asarray(X, np.float64)
    s = np.zeros_like(X)
    np.add.at(s, np.repeat(np.arange(len(X)), adj.deg.astype(np.int64)), X[adj.nbr])
    d = s / adj.deg.astype(np.float64)[:, None] - X
    return float(np.sqrt((d * d).sum(axis=1)).mean())


# two hand-made face lists: a fan of 40 triangles round vertex 0 (inc = deg = 40 there, lists far longer than a weld's), given
# in a scrambled order; and three triangles on the edge (0, 1), so m(0, 1) = 3 and that edge marks no boundary
def fan_mesh(n=40):
    rng = np.random.default_rng(40)
    ang = 2.0 * np.pi * np.arange(n) / n
    X = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.05 * rng.standard_normal(n)], axis=1)])
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int64)[rng.permutation(n)]
    return _mesh(X, faces)


def three_on_an_edge_mesh():
    X = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.1, 0.5], [-0.5, 0.9, 0.4], [-0.6, -0.8, 0.6]], np.float64)
    return _mesh(X, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int64))


def _mesh(X, faces):
    n = len(X)
    return dict(vertices=np.ascontiguousarray(X, np.float64), faces=faces, grey=np.arange(n, dtype=np.uint8), colour=None, normals=None,
                key=np.arange(n, dtype=np.uint64))
