"""numpy restatement of the welded-mesh contract, written from the contract and built beside the fusion and
colour oracles, which stay as they are (tests/fusion_oracle.py §16, tests/colour_oracle.py §18).

A vertex key is 8 la + d: la the lin of the smaller end of a Kuhn edge, d in 1..7 the bits of the steps to its other end
lb = la + (d & 1) + ((d >> 1) & 1) nx + (d >> 2) nx ny.
  1. Edge (la, d) carries a vertex iff lb is in the grid, (sum[la] < 0) != (sum[lb] < 0), and at least one of the cells whose
     corner 0 is la - o, o a subset of ~d & 7, lies in the grid with all eight cnt >= min_count (`edge_masks`).
  2. The vertices are ordered by ascending key; xyz, grey and colour come from the key alone by the arithmetic of the
     extraction (`vertices`).
  3. faces[t, v] is the rank of key (t, v) of the soup among the vertex keys (`faces`).
  4. Normals: fp64 throughout, written order; `gradient` and `normals`.
Nothing here sorts the soup: `tests/test_oracle_mesh.py` holds all of it against `fusion_oracle.weld(fusion_oracle.extract())`.
"""
import numpy as np


def _bits(d):
    return d & 1, (d >> 1) & 1, d >> 2


def valid_cells(cnt, min_count):
    """(nz - 1, ny - 1, nx - 1) bool: all eight corners of the cell have cnt >= min_count."""
    nz, ny, nx = cnt.shape
    valid = cnt >= min_count
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        dx, dy, dz = _bits(c)
        ok &= valid[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
    return ok


def edge_cells(cnt, min_count):
    """(8, nz, ny, nx) int: for d = 1..7, how many valid cells contain edge (la, d) (0 where lb is outside the grid)."""
    nz, ny, nx = cnt.shape
    pad = np.zeros((nz + 1, ny + 1, nx + 1), np.int64)              # pad[k + 1, j + 1, i + 1] = cell (i, j, k); cells -1 and n - 1: 0
    pad[1:nz, 1:ny, 1:nx] = valid_cells(cnt, min_count)
    out = np.zeros((8, nz, ny, nx), np.int64)
    for d in range(1, 8):
        free = ~d & 7
        for o in range(8):
            if o & ~free:
                continue
            ox, oy, oz = _bits(o)
            out[d] += pad[1 - oz:1 - oz + nz, 1 - oy:1 - oy + ny, 1 - ox:1 - ox + nx]
        dx, dy, dz = _bits(d)
        exists = np.zeros((nz, ny, nx), bool)
        exists[:nz - dz, :ny - dy, :nx - dx] = True
        out[d][~exists] = 0
    return out


def edge_masks(vol, min_count=1):
    """(nz, ny, nx) uint8: bit d of a voxel = its edge d carries a vertex."""
    s_, c_ = vol[0], vol[1]
    nz, ny, nx = s_.shape
    inside = s_ < np.float32(0.0)
    cells = edge_cells(c_, min_count)
    mask = np.zeros((nz, ny, nx), np.uint8)
    for d in range(1, 8):
        dx, dy, dz = _bits(d)
        cross = np.zeros((nz, ny, nx), bool)
        cross[:nz - dz, :ny - dy, :nx - dx] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        mask |= ((cross & (cells[d] > 0)).astype(np.uint8) << np.uint8(d))
    return mask


def vertex_keys(vol, min_count=1):
    """The keys of the vertices, ascending: uint64 (m,)."""
    mask = edge_masks(vol, min_count).reshape(-1)
    la = np.nonzero(mask)[0]
    keys = [la[(mask[la] >> d) & 1 == 1].astype(np.uint64) * np.uint64(8) + np.uint64(d) for d in range(1, 8)]
    return np.sort(np.concatenate(keys)) if len(la) else np.zeros(0, np.uint64)


def _ends(key, dims):
    nx, ny, nz = (int(v) for v in dims)
    la = (key >> np.uint64(3)).astype(np.int64)
    d = (key & np.uint64(7)).astype(np.int64)
    ia = (la % nx, (la // nx) % ny, la // (nx * ny))
    ib = (ia[0] + (d & 1), ia[1] + ((d >> 1) & 1), ia[2] + (d >> 2))
    lb = ib[0] + nx * (ib[1] + ny * ib[2])
    return la, lb, ia, ib


def vertices(vol, dims, origin, voxel, key):
    """(xyz (m, 3) fp64, grey (m,) uint8, u (m,) fp64, colour (m, 3) uint8 or None) of the keys, from the keys alone."""
    key = np.asarray(key, np.uint64)
    la, lb, ia, ib = _ends(key, dims)
    s1, c1, g1 = vol[0].reshape(-1), vol[1].reshape(-1), vol[2].reshape(-1)
    o = np.asarray(origin, np.float64)
    vx = np.float64(voxel)
    xyz = np.zeros((len(key), 3), np.float64)
    with np.errstate(all="ignore"):
        na, nb = c1[la].astype(np.float64), c1[lb].astype(np.float64)
        va, vb = s1[la].astype(np.float64) / na, s1[lb].astype(np.float64) / nb
        ga, gb = g1[la].astype(np.float64) / na, g1[lb].astype(np.float64) / nb
        u = va / (va - vb)
        for c in range(3):
            Pa = o[c] + ia[c].astype(np.float64) * vx
            Pb = o[c] + ib[c].astype(np.float64) * vx
            xyz[:, c] = Pa + u * (Pb - Pa)
        gv = ga + u * (gb - ga)
        grey = np.floor(gv + 0.5).astype(np.int64).astype(np.uint8)
        colour = None
        if len(vol) > 3:
            colour = np.zeros((len(key), 3), np.uint8)
            for c in range(3):
                p = vol[3][c].reshape(-1)
                Ca, Cb = p[la].astype(np.float64) / na, p[lb].astype(np.float64) / nb
                cv = Ca + u * (Cb - Ca)
                colour[:, c] = np.floor(cv + 0.5).astype(np.int64).astype(np.uint8)
    return xyz, grey, u, colour


def faces(soup_key, key):
    """(n, 3) int64: the rank of every key of the soup among the ascending vertex keys (each must be there)."""
    soup_key = np.asarray(soup_key, np.uint64).reshape(-1, 3)
    f = np.searchsorted(key, soup_key.reshape(-1)).reshape(-1, 3).astype(np.int64)
    assert f.size == 0 or (f.max() < len(key) and np.array_equal(key[f.reshape(-1)], soup_key.reshape(-1)))
    return f


def gradient(vol, min_count=1):
    """(3, nz, ny, nx) fp64: component c of the gradient of v = (double) sum / (double) cnt at every voxel, in voxel units.
    A neighbour l +- e_c is usable iff it is in the grid and has cnt >= min_count: (v+ - v-) * 0.5 with both, v+ - v with the
    upper one alone, v - v- with the lower one alone, otherwise 0.0."""
    s_, c_ = vol[0], vol[1]
    with np.errstate(all="ignore"):
        v = s_.astype(np.float64) / c_.astype(np.float64)
    ok = c_ >= min_count
    g = np.zeros((3,) + v.shape, np.float64)
    for c in range(3):
        ax = 2 - c                                                   # x is the last axis
        vp, vm = np.zeros_like(v), np.zeros_like(v)
        up, dn = np.zeros(v.shape, bool), np.zeros(v.shape, bool)
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[ax], lo[ax] = slice(1, None), slice(None, -1)
        hi, lo = tuple(hi), tuple(lo)
        vp[lo], up[lo] = v[hi], ok[hi]
        vm[hi], dn[hi] = v[lo], ok[lo]
        with np.errstate(all="ignore"):
            g[c] = np.where(up & dn, (vp - vm) * 0.5, np.where(up, vp - v, np.where(dn, v - vm, 0.0)))
    return g


def normals(vol, dims, key, u, min_count=1):
    """(m, 3) float32: n_c = g_c(la) + u (g_c(lb) - g_c(la)), len = sqrt((n0 n0 + n1 n1) + n2 n2), n_c / len rounded once to
    fp32; 0, 0, 0 where len is 0 or not finite."""
    key = np.asarray(key, np.uint64)
    la, lb, _, _ = _ends(key, dims)
    g = gradient(vol, min_count).reshape(3, -1)
    with np.errstate(all="ignore"):
        n = [g[c][la] + u * (g[c][lb] - g[c][la]) for c in range(3)]
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ok = (length > 0.0) & np.isfinite(length)
        out = np.stack([np.where(ok, n[c] / length, 0.0).astype(np.float32) for c in range(3)], axis=1)
    return out.reshape(-1, 3)


def weld(vol, dims, origin, voxel, soup_key, min_count=1, with_normals=False):
    """dict(vertices, faces, grey, colour, normals, key) of the volume's mesh: the vertices by rule 1 and 2, the faces of the
    given soup by rule 3."""
    key = vertex_keys(vol, min_count)
    xyz, grey, u, colour = vertices(vol, dims, origin, voxel, key)
    return dict(vertices=xyz, faces=faces(soup_key, key), grey=grey, colour=colour, key=key,
                normals=normals(vol, dims, key, u, min_count) if with_normals else None)
