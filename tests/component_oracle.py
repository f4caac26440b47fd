"""numpy restatement of the component contract of the welded mesh, written from the contract.

  1. Two vertices are linked iff some triangle of ``faces`` has both; a component is a connected component of the links.
     Linking is by index, not by coordinate: two vertices with different keys but equal coordinates are distinct.  Every
     welded vertex lies in at least one triangle.
  2. ``label[v]`` (uint32) is the least vertex index of v's component, ``size[v]`` (uint32) the number of triangles of that
     component, ``count`` the number of distinct labels.  All are functions of ``faces`` alone.
  3. ``prune(mesh, min_triangles >= 1, largest)``: a component is kept iff size >= min_triangles and, with ``largest``, it is
     the component of greatest size, the least label among equals.  The pruned mesh is the weld without the vertices and
     triangles of the other components, order preserved, the kept rows bit for bit, the faces re-indexed by the rank of each
     vertex among the kept ones.

Two independent implementations of 1 and 2, which tests/test_oracle_components.py holds equal to each other: a union-find
over the triangles, and a flood fill over a vertex-to-triangle adjacency.  A mesh is the dict tests/mesh_oracle.py's ``weld``
returns: vertices, faces, grey, colour, normals, key.
"""
import numpy as np


def _sizes(faces, label, n_vert):
    per_root = np.bincount(label[faces[:, 0]], minlength=n_vert) if len(faces) else np.zeros(n_vert, np.int64)
    return per_root[label].astype(np.uint32)


def components_union_find(faces, n_vert):
    """(label, size, count) by a union-find that hooks the larger root to the smaller, so a root is its set's least index."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(n_vert))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for f0, f1, f2 in faces.tolist():
        for other in (f1, f2):
            a, b = find(f0), find(other)
            if a != b:
                parent[max(a, b)] = min(a, b)
    label = np.array([find(v) for v in range(n_vert)], np.int64).reshape(-1)
    return label.astype(np.uint32), _sizes(faces, label, n_vert), int(len(np.unique(label)))


def components_flood(faces, n_vert):
    """(label, size, count) by a flood fill: the vertices in ascending order, each unvisited one the seed (and so the least
    index) of a new component, which spreads over the triangles a frontier vertex lies in."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    corner = faces.reshape(-1)
    order = np.argsort(corner, kind="stable")                        # the corners, grouped by vertex
    tri_of = order // 3
    first = np.searchsorted(corner[order], np.arange(n_vert + 1))    # vertex v's triangles: tri_of[first[v]:first[v + 1]]
    label = np.full(n_vert, -1, np.int64)
    done = np.zeros(len(faces), bool)
    count = 0
    for seed in range(n_vert):
        if label[seed] >= 0:
            continue
        count += 1
        label[seed] = seed
        frontier = np.array([seed], np.int64)
        while len(frontier):
            tris = np.unique(np.concatenate([tri_of[first[v]:first[v + 1]] for v in frontier.tolist()]))
            tris = tris[~done[tris]]
            done[tris] = True
            verts = np.unique(faces[tris].reshape(-1))
            frontier = verts[label[verts] < 0]
            label[frontier] = seed
    return label.astype(np.uint32), _sizes(faces, label, n_vert), count


components = components_union_find


def kept_vertices(label, size, min_triangles=1, largest=False):
    """bool (m,): the vertices of the components that a prune keeps."""
    if min_triangles < 1:
        raise ValueError("min_triangles >= 1")
    keep = size >= min_triangles
    if largest and len(label):
        best = size.max()
        keep &= label == label[size == best].min()                   # the least label among the components of greatest size
    return keep


def prune(mesh, min_triangles=1, largest=False):
    """The mesh without the components that are not kept, by boolean masks; ``components``: the number kept."""
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    n_vert = len(mesh["key"])
    label, size, _ = components(faces, n_vert)
    keep_v = kept_vertices(label, size, min_triangles, largest)
    keep_t = keep_v[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    rank = np.cumsum(keep_v) - 1                                     # the rank of a kept vertex among the kept ones
    out = {k: (None if mesh.get(k) is None else mesh[k][keep_v]) for k in ("vertices", "grey", "colour", "normals", "key")}
    out["faces"] = rank[faces[keep_t]].reshape(-1, 3)
    out["components"] = int(len(np.unique(label[keep_v])))
    return out
