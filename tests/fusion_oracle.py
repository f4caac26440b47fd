"""numpy restatement of the TSDF fusion contract, written from the contract: the integration of one depth
map into the three planes of a volume, and the marching-tetrahedra extraction with its fixed output order.

Every coordinate operation is fp64, rounded once, in the written left-to-right order (sums of three products are spelled
out, numpy never contracts a product and a sum); the running sum of a voxel is one fp32 add per map.  Poses are those of
tests/dense_oracle.py (§15.1), unchanged.
"""
import numpy as np

import dense_oracle as do

MAX_DIM, MAX_VOXELS, MAX_MAPS, MAX_MAP_DIM = 1024, 1 << 28, 65535, 8192

# ---- the tables of the extraction --------------------------------------------------------------------------------------------
# The six Kuhn tetrahedra round the diagonal 0-7 of a cell; corners are numbered c = dx + 2 dy + 4 dz.
TETS = ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7))
# tet-local edges, as pairs of tet-local vertices
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# TET_TRIS[mask], bit i of mask = tet-local vertex i is inside: triangles of tet-local edges, normal to the outside
TET_TRIS = (
    (),
    ((0, 1, 2),),
    ((0, 4, 3),),
    ((1, 2, 4), (1, 4, 3)),
    ((1, 3, 5),),
    ((0, 5, 2), (0, 3, 5)),
    ((0, 4, 5), (0, 5, 1)),
    ((2, 4, 5),),
    ((2, 5, 4),),
    ((0, 1, 5), (0, 5, 4)),
    ((0, 5, 3), (0, 2, 5)),
    ((1, 5, 3),),
    ((1, 3, 4), (1, 4, 2)),
    ((0, 3, 4),),
    ((0, 2, 1),),
    (),
)

BEHIND, OUTSIDE, NO_DEPTH, FAR_BEHIND, FREE, NEAR = range(6)
CLASS_NAMES = ("behind the camera", "outside the image", "depth 0", "s < -trunc", "s >= trunc", "|s| < trunc")


# ---- the volume ----------------------------------------------------------------------------------------------------------
def empty_volume(dims):
    """(sum fp32, cnt uint16, gsum uint32), each of shape (nz, ny, nx): x fastest, lin = i + nx (j + ny k)."""
    nx, ny, nz = (int(v) for v in dims)
    return np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.uint16), np.zeros((nz, ny, nx), np.uint32)


def centres(dims, origin, voxel):
    """P_c = origin_c + (double) idx_c * voxel, each broadcast to (nz, ny, nx)."""
    nx, ny, nz = (int(v) for v in dims)
    o = np.asarray(origin, np.float64)
    vx = np.float64(voxel)
    X = o[0] + np.arange(nx, dtype=np.float64) * vx
    Y = o[1] + np.arange(ny, dtype=np.float64) * vx
    Z = o[2] + np.arange(nz, dtype=np.float64) * vx
    return (np.broadcast_to(X[None, None, :], (nz, ny, nx)), np.broadcast_to(Y[None, :, None], (nz, ny, nx)),
            np.broadcast_to(Z[:, None, None], (nz, ny, nx)))


def integrate(vol, dims, origin, voxel, trunc, depth, image, K, pose7):
    """Integrates one map into vol = (sum, cnt, gsum) in place; returns the class of every voxel (nz, ny, nx)."""
    s_, c_, g_ = vol
    depth = np.ascontiguousarray(depth, np.float32)
    image = np.ascontiguousarray(image, np.uint8)
    H, W = depth.shape
    assert image.shape == (H, W)
    K = np.asarray(K, np.float64)
    t, q = do.normalise_pose(pose7)
    R = do.rotation(q)
    P = centres(dims, origin, voxel)
    tr = np.float64(trunc)
    with np.errstate(all="ignore"):
        d = [P[c] - t[c] for c in range(3)]
        p = [R[0, i] * d[0] + R[1, i] * d[1] + R[2, i] * d[2] for i in range(3)]
        front = p[2] > 0.0
        sx = K[0] * (p[0] / p[2]) + K[2]
        sy = K[1] * (p[1] / p[2]) + K[3]
        jx_, jy_ = np.floor(sx + 0.5), np.floor(sy + 0.5)
        inside = front & (jx_ >= 0.0) & (jx_ <= W - 1.0) & (jy_ >= 0.0) & (jy_ <= H - 1.0)
        jx = np.where(inside, jx_, 0.0).astype(np.int64)
        jy = np.where(inside, jy_, 0.0).astype(np.int64)
        zs = depth[jy, jx].astype(np.float64)
        has = inside & (zs != 0.0)
        s = zs - p[2]
        seen = has & ~(s < -tr)
        tau = np.where(s >= tr, 1.0, s / tr)
    cls = np.full(front.shape, NEAR, np.int8)
    cls[seen & (s >= tr)] = FREE
    cls[has & ~seen] = FAR_BEHIND
    cls[inside & ~has] = NO_DEPTH
    cls[front & ~inside] = OUTSIDE
    cls[~front] = BEHIND
    s_[seen] = s_[seen] + tau[seen].astype(np.float32)              # one fp32 add
    c_[seen] = c_[seen] + np.uint16(1)
    g_[seen] = g_[seen] + image[jy, jx][seen].astype(np.uint32)
    return cls


# ---- extraction ----------------------------------------------------------------------------------------------------------
def _corner(c):
    return c & 1, (c >> 1) & 1, c >> 2


def extract(vol, dims, origin, voxel, min_count=1):
    """(xyz (n, 3, 3) fp64, key (n, 3) uint64, grey (n, 3) uint8, u (n, 3) fp64) in the fixed order: cells by lin of
    their corner 0, tetrahedra 0..5, table order."""
    s_, c_, g_ = vol
    nx, ny, nz = (int(v) for v in dims)
    valid = c_ >= min_count
    with np.errstate(all="ignore"):
        v = s_.astype(np.float64) / c_.astype(np.float64)
        g = g_.astype(np.float64) / c_.astype(np.float64)
    inside = valid & (v < 0.0)
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    sl = lambda c: (slice(_corner(c)[2], _corner(c)[2] + cz), slice(_corner(c)[1], _corner(c)[1] + cy),
                    slice(_corner(c)[0], _corner(c)[0] + cx))
    ok = np.ones((cz, cy, cx), bool)
    for c in range(8):
        ok &= valid[sl(c)]
    K_, J_, I_ = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
    lin0 = (I_ + nx * (J_ + ny * K_)).astype(np.int64)
    rows = []                                                        # (lin0, tet, j, corner a, corner b) x 3 per triangle
    for ti, tet in enumerate(TETS):
        mask = np.zeros((cz, cy, cx), np.int64)
        for j, c in enumerate(tet):
            mask |= inside[sl(c)].astype(np.int64) << j
        mask = np.where(ok, mask, 0)
        for m in range(1, 15):
            cells = lin0[mask == m]
            for j, tri in enumerate(TET_TRIS[m]):
                pairs = []
                for e in tri:
                    ca, cb = tet[TET_EDGES[e][0]], tet[TET_EDGES[e][1]]
                    pairs += [min(ca, cb), max(ca, cb)]
                for cell in cells:
                    rows.append((int(cell), ti, j) + tuple(pairs))
    if not rows:
        return (np.zeros((0, 3, 3), np.float64), np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.uint8),
                np.zeros((0, 3), np.float64))
    rows = np.array(sorted(rows), np.int64)
    n = len(rows)
    i0, j0, k0 = rows[:, 0] % nx, (rows[:, 0] // nx) % ny, rows[:, 0] // (nx * ny)
    o = np.asarray(origin, np.float64)
    vx = np.float64(voxel)
    xyz = np.zeros((n, 3, 3), np.float64)
    key = np.zeros((n, 3), np.uint64)
    grey = np.zeros((n, 3), np.uint8)
    uu = np.zeros((n, 3), np.float64)
    for vtx in range(3):
        ca, cb = rows[:, 3 + 2 * vtx], rows[:, 4 + 2 * vtx]
        ia = (i0 + (ca & 1), j0 + ((ca >> 1) & 1), k0 + (ca >> 2))
        ib = (i0 + (cb & 1), j0 + ((cb >> 1) & 1), k0 + (cb >> 2))
        va, vb = v[ia[2], ia[1], ia[0]], v[ib[2], ib[1], ib[0]]
        ga, gb = g[ia[2], ia[1], ia[0]], g[ib[2], ib[1], ib[0]]
        u = va / (va - vb)
        for c in range(3):
            Pa = o[c] + ia[c].astype(np.float64) * vx
            Pb = o[c] + ib[c].astype(np.float64) * vx
            xyz[:, vtx, c] = Pa + u * (Pb - Pa)
        gv = ga + u * (gb - ga)
        grey[:, vtx] = np.floor(gv + 0.5).astype(np.int64).astype(np.uint8)
        lin_a = ia[0] + nx * (ia[1] + ny * ia[2])
        key[:, vtx] = (lin_a * 8 + (cb - ca)).astype(np.uint64)
        uu[:, vtx] = u
    return xyz, key, grey, uu


def weld(key):
    """(first, faces): the index of the first occurrence of every distinct key in key.ravel() (ascending key), and the
    (n, 3) indices of the triangles into that list."""
    uniq, first, inverse = np.unique(np.asarray(key, np.uint64).reshape(-1), return_index=True, return_inverse=True)
    return first, inverse.reshape(-1, 3)


# ---- the automatic grid of mesh_from_recording ---------------------------------------------------------------------------
def auto_grid(points, voxel=None, bounds=None, trunc=None):
    """(origin (3,), dims (3,), voxel, trunc) as DESIGN §16.3 states it.  points: a list of (..., 3) arrays with NaNs."""
    if bounds is None:
        pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p in points])
        pts = pts[np.isfinite(pts).all(axis=1)]
        lo, hi = pts.min(axis=0), pts.max(axis=0)
    else:
        lo, hi = np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64)
    auto = voxel is None
    vx = np.float64((hi - lo).max()) / 128.0 if auto else np.float64(voxel)
    if not (np.isfinite(vx) and vx > 0.0):
        raise ValueError("the box has no extent")
    while True:
        tr = 4.0 * vx if trunc is None else np.float64(trunc)
        a, b = (lo - tr, hi + tr) if bounds is None else (lo, hi)
        dims = np.maximum(np.ceil((b - a) / vx).astype(np.int64) + 1, 2)
        if dims.max() <= MAX_DIM and int(dims[0]) * int(dims[1]) * int(dims[2]) <= MAX_VOXELS:
            return a, dims, float(vx), float(tr)
        if not auto:
            raise ValueError("the volume exceeds 1024 voxels a side or 2^28 in all")
        vx = vx * 2.0
