"""numpy restatement of the vertex-clustering contract of the welded, pruned or smoothed mesh, written from
the contract.

The input is a source mesh (X, F, grey, optional colour, optional normals) with n_vert vertices and n_tri triangles, the
volume's origin, dims and voxel, and a cell size ``cell`` (float64, finite, cell >= voxel).  Every float64 operation is rounded
once.

  1. The grid.  G_a = int(floor((float64(dims_a - 1) * voxel) / cell)) + 1 for a = x, y, z, so G_a <= dims_a.  For a vertex,
     q_a = floor((X[v][a] - origin[a]) / cell): a division, not a multiplication by a reciprocal; a result that is not finite
     counts as 0; the result is clamped to [0, G_a - 1].  cell(v) = (q_z G_y + q_y) G_x + q_x, x fastest, as in the volume.
  2. The triangles.  Triangle t has the cells (cell(F[t][0]), cell(F[t][1]), cell(F[t][2])).  It is degenerate iff two of them
     are equal.  A non-degenerate triangle is a duplicate iff a non-degenerate triangle with a smaller index has the same
     unordered triple of cells.  The kept triangles are the rest, in the source's order and with the source's winding.
  3. The vertices.  A cell is used iff a kept triangle has it.  The output has one vertex per used cell, numbered by ascending
     cell id; that cell id is the output's key, so keys ascend strictly.  A cell that holds vertices but no kept triangle gives
     no vertex.  With M(c) the ascending list of the source vertices of cell c and n = |M(c)|:
       position: per coordinate, s = X[m0], then s = s + X[mi] in the order of M(c), then s / float64(n);
       grey, and each of B, G, R of a colour volume: (2 S + n) // (2 n) in unsigned 64-bit integers, S the sum: the mean, with
         halves rounded up;
       normal (iff the source has normals): the members' float32 normals summed as float64 in the order of M(c), starting
         from the first one's; len = sqrt((a0 a0 + a1 a1) + a2 a2); each a_c / len rounded once to float32; 0 0 0 where len is
         0 or not finite.  A source without normals gives a result without normals.
  4. The faces: the kept triangles, each index replaced by the output number of its cell.
  5. The vertex map: for every source vertex, the output number of its cell, or 0xffffffff if the cell is unused.
  6. The counts: n_vert_out, n_tri_out, n_degenerate, n_duplicate, with n_tri_out + n_degenerate + n_duplicate = n_tri.

Two independent implementations, which tests/test_oracle_simplify.py holds equal to each other bit for bit: a plain loop over
the vertices, the triangles and the cells with Python dicts (``simplify_loop``), and a vectorised form that sorts, and adds
member i of every used cell in round i (``simplify``).  A mesh is the dict tests/mesh_oracle.py's ``weld`` returns: vertices,
faces, grey, colour, normals, key; a result has the same rows and beside them ``map``, ``kept`` (the source indices of the kept
triangles), ``cells`` (cell(v) of every source vertex), ``grid``, ``n_degenerate`` and ``n_duplicate``.
"""
import numpy as np

NONE = 0xFFFFFFFF


def grid(dims, voxel, cell):
    """(G_x, G_y, G_z)."""
    return tuple(int(np.floor((np.float64(int(d) - 1) * np.float64(voxel)) / np.float64(cell))) + 1 for d in dims)


def cells(X, origin, cell, G):
    """cell(v) of every vertex, int64."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = np.floor((X - np.asarray(origin, np.float64).reshape(1, 3)) / np.float64(cell))
    q = np.where(np.isfinite(q), q, 0.0)
    q = np.minimum(np.maximum(q, 0.0), np.asarray(G, np.float64).reshape(1, 3) - 1.0).astype(np.int64)
    return (q[:, 2] * G[1] + q[:, 1]) * G[0] + q[:, 0]


def _cell_loop(x, origin, cell, G):
    q = []
    for a in range(3):
        with np.errstate(all="ignore"):
            d = np.floor((np.float64(x[a]) - np.float64(origin[a])) / np.float64(cell))
        if not np.isfinite(d):
            d = np.float64(0.0)
        q.append(int(min(max(d, 0.0), float(G[a] - 1))))
    return (q[2] * G[1] + q[1]) * G[0] + q[0]


def _rows(mesh):
    X = np.asarray(mesh["vertices"], np.float64).reshape(-1, 3)
    F = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    grey = np.asarray(mesh["grey"], np.uint8).reshape(-1)
    colour = None if mesh.get("colour") is None else np.asarray(mesh["colour"], np.uint8).reshape(-1, 3)
    normals = None if mesh.get("normals") is None else np.asarray(mesh["normals"], np.float32).reshape(-1, 3)
    return X, F, grey, colour, normals


def _result(X, grey, colour, normals, faces, key, vmap, kept, vc, G, n_deg, n_dup):
    return dict(vertices=np.ascontiguousarray(X, np.float64).reshape(-1, 3), faces=np.asarray(faces, np.int64).reshape(-1, 3),
                grey=np.asarray(grey, np.uint8).reshape(-1), colour=None if colour is None else np.asarray(colour, np.uint8).reshape(-1, 3),
                normals=None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3),
                key=np.asarray(key, np.uint64).reshape(-1), map=np.asarray(vmap, np.uint32).reshape(-1),
                kept=np.asarray(kept, np.int64).reshape(-1), cells=np.asarray(vc, np.int64).reshape(-1), grid=tuple(G),
                n_degenerate=int(n_deg), n_duplicate=int(n_dup))


def simplify_loop(mesh, origin, dims, voxel, cell):
    """The contract by loops over the vertices, the triangles and the used cells, on Python ints and float64 scalars."""
    X, F, grey, colour, normals = _rows(mesh)
    G = grid(dims, voxel, cell)
    vc = [_cell_loop(X[v], origin, cell, G) for v in range(len(X))]
    members = {}
    for v, c in enumerate(vc):                                       # v ascending: every M(c) comes out ascending
        members.setdefault(c, []).append(v)
    seen, kept, n_deg, n_dup = set(), [], 0, 0
    for t, tri in enumerate(F.tolist()):
        c = [vc[v] for v in tri]
        if c[0] == c[1] or c[0] == c[2] or c[1] == c[2]:
            n_deg += 1
            continue
        triple = tuple(sorted(c))
        if triple in seen:
            n_dup += 1
            continue
        seen.add(triple)
        kept.append(t)
    used = sorted({vc[v] for t in kept for v in F[t].tolist()})
    number = {c: i for i, c in enumerate(used)}
    oX = np.zeros((len(used), 3), np.float64)
    og = np.zeros(len(used), np.uint8)
    oc = None if colour is None else np.zeros((len(used), 3), np.uint8)
    on = None if normals is None else np.zeros((len(used), 3), np.float32)
    for i, c in enumerate(used):
        M = members[c]
        n = len(M)
        for a in range(3):
            s = X[M[0], a]
            for m in M[1:]:
                s = s + X[m, a]
            oX[i, a] = s / np.float64(n)
        og[i] = (2 * sum(int(grey[m]) for m in M) + n) // (2 * n)
        if colour is not None:
            for a in range(3):
                oc[i, a] = (2 * sum(int(colour[m, a]) for m in M) + n) // (2 * n)
        if normals is not None:
            acc = [np.float64(normals[M[0], a]) for a in range(3)]
            for m in M[1:]:
                acc = [acc[a] + np.float64(normals[m, a]) for a in range(3)]
            with np.errstate(all="ignore"):
                length = np.sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2])
                if length > 0.0 and length < np.inf:
                    on[i] = [np.float32(acc[a] / length) for a in range(3)]
    faces = [[number[vc[v]] for v in F[t].tolist()] for t in kept]
    vmap = [number.get(c, NONE) for c in vc]
    return _result(oX, og, oc, on, faces, used, vmap, kept, vc, G, n_deg, n_dup)


def _normalise(a):
    with np.errstate(all="ignore"):
        length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        ok = (length > 0.0) & (length < np.inf)
        return np.where(ok[:, None], (a / length[:, None]).astype(np.float32), np.float32(0.0)).astype(np.float32).reshape(-1, 3)


def simplify(mesh, origin, dims, voxel, cell):
    """The contract by sorting: the triples by (cells, index), the vertices by (cell, index); round i adds member i of every
    used cell that has one."""
    X, F, grey, colour, normals = _rows(mesh)
    G = grid(dims, voxel, cell)
    ncell = G[0] * G[1] * G[2]
    vc = cells(X, origin, cell, G)
    tc = vc[F]                                                       # (n_tri, 3)
    degenerate = (tc[:, 0] == tc[:, 1]) | (tc[:, 0] == tc[:, 2]) | (tc[:, 1] == tc[:, 2])
    nd = np.nonzero(~degenerate)[0]
    st = np.sort(tc[nd], axis=1)
    code = (st[:, 0] * ncell + st[:, 1]) * ncell + st[:, 2] if ncell ** 3 < 2 ** 62 else None
    if code is None:                                                 # (three cell ids do not fit one int64: sort the rows)
        order = np.lexsort((nd, st[:, 2], st[:, 1], st[:, 0]))
        same = np.zeros(len(nd), bool)
        same[1:] = (st[order][1:] == st[order][:-1]).all(axis=1)
        first = order[~same]
    else:
        _, first = np.unique(code, return_index=True)                # the first occurrence: the least index
    kept = np.sort(nd[first])
    used = np.unique(tc[kept].reshape(-1))
    # the members of the used cells, ascending: a stable sort of the vertices by cell
    order = np.argsort(vc, kind="stable")
    start = np.searchsorted(vc[order], used, side="left")
    count = np.searchsorted(vc[order], used, side="right") - start
    s = np.zeros((len(used), 3), np.float64)
    acc = np.zeros((len(used), 3), np.float64)
    gsum = np.zeros(len(used), np.uint64)
    csum = np.zeros((len(used), 3), np.uint64)
    for i in range(int(count.max()) if len(count) else 0):
        has = np.nonzero(count > i)[0]
        m = order[start[has] + i]
        s[has] = X[m] if i == 0 else s[has] + X[m]
        gsum[has] += grey[m].astype(np.uint64)
        if colour is not None:
            csum[has] += colour[m].astype(np.uint64)
        if normals is not None:
            rows = normals[m].astype(np.float64)
            acc[has] = rows if i == 0 else acc[has] + rows
    n64 = count.astype(np.uint64)
    oX = s / count.astype(np.float64)[:, None]
    og = ((np.uint64(2) * gsum + n64) // (np.uint64(2) * n64)).astype(np.uint8)
    oc = None if colour is None else ((np.uint64(2) * csum + n64[:, None]) // (np.uint64(2) * n64[:, None])).astype(np.uint8)
    on = None if normals is None else _normalise(acc)
    faces = np.searchsorted(used, tc[kept])
    at = np.minimum(np.searchsorted(used, vc), max(len(used) - 1, 0))
    vmap = np.where(used[at] == vc, at, NONE) if len(used) else np.full(len(vc), NONE, np.int64)
    return _result(oX, og, oc, on, faces, used, vmap, kept, vc, G, int(degenerate.sum()), len(nd) - len(kept))


FIELDS = ("vertices", "faces", "grey", "colour", "normals", "key", "map", "kept", "cells")


def same(a, b):
    """Two results equal bit for bit, the counts and the grid included."""
    for k in FIELDS:
        x, y = a[k], b[k]
        if x is None or y is None:
            if not (x is None and y is None):
                return False
            continue
        if x.dtype != y.dtype or x.shape != y.shape:
            return False
        if x.dtype.kind == "f":
            x, y = x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]), y.view({4: np.uint32, 8: np.uint64}[y.dtype.itemsize])
        if not np.array_equal(x, y):
            return False
    return a["grid"] == b["grid"] and a["n_degenerate"] == b["n_degenerate"] and a["n_duplicate"] == b["n_duplicate"]


def as_mesh(result):
    """The rows of a result that a mesh has: what a further step would read."""
    return {k: result[k] for k in ("vertices", "faces", "grey", "colour", "normals", "key")}


# hand-made meshes on a 5 x 5 x 5 volume of voxel 1 at the origin
HAND_ORIGIN, HAND_DIMS, HAND_VOXEL = (0.0, 0.0, 0.0), (5, 5, 5), 1.0


def _mesh(X, faces):
    n = len(X)
    return dict(vertices=np.ascontiguousarray(X, np.float64), faces=np.asarray(faces, np.int64).reshape(-1, 3),
                grey=(np.arange(n) * 37 % 256).astype(np.uint8), colour=None, normals=None, key=np.arange(n, dtype=np.uint64))


def opposite_winding_mesh():
    """Two triangles with opposite winding over the same three cells (six vertices): the first is kept."""
    X = [[0.2, 0.2, 0.2], [1.2, 0.2, 0.2], [0.2, 1.2, 0.2], [0.7, 0.7, 0.7], [1.7, 0.7, 0.7], [0.7, 1.7, 0.7]]
    return _mesh(X, [[0, 1, 2], [3, 5, 4]])


def outside_mesh():
    """A triangle with a vertex outside the box on either side, and one at infinity and one that is no number."""
    X = [[-3.5, 0.5, 0.5], [9.0, 0.5, 0.5], [0.5, 2.5, 77.0], [np.inf, 1.5, 1.5], [np.nan, 3.5, -np.inf], [2.5, 2.5, 2.5]]
    return _mesh(X, [[0, 1, 2], [3, 4, 5]])


def fan_mesh(n=40):
    """A fan of n triangles round a vertex in cell 0, every other vertex in a cell of its own, in a scrambled order, and behind
    them every third one again with the opposite winding: n + n / 3 non-degenerate triangles under one least cell (a list far
    longer than a weld's), of which the repeats are duplicates."""
    rng = np.random.default_rng(27)
    ring = 1 + np.arange(n)                                          # the cells 1 .. n of the 5 x 5 x 5 grid
    X = np.concatenate([[[0.5, 0.5, 0.5]], np.stack([ring % 5, ring // 5 % 5, ring // 25], axis=1) + 0.25 + 0.5 * rng.random((n, 3))])
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int64)[rng.permutation(n)]
    return _mesh(X, np.concatenate([faces, faces[::3][:, ::-1]]))
