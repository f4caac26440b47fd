"""numpy restatement of the rasteriser's contract, written from the contract.

The input is a source mesh (X float64, F, vertex grey and optional B, G, R), an image of W x H, K = (fx, fy, cx, cy), a pose
(through dense_oracle.normalise_pose, as the ray cast takes it), z_near >= 0, ``cull``, ``cover`` and, for shading 1, an atlas of
tests/texture_oracle.py with its patch size P.  Every float64 operation is rounded once, in the written order.

  1. A vertex: p2, sx, sy are texture_oracle.project's (its ``_project_loop`` in the loop form).  It is usable iff p2 > z_near and
     sx and sy are finite.
  2. A triangle t with the vertex indices (i0, i1, i2) is dropped if a vertex is unusable (no clipping).
     area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0); area2 == 0 or NaN drops it; front = area2 < 0; with ``cull`` a triangle that
     is not front is dropped; s = -1 if front else +1.  Its box: x from max(0, ceil(min sx)) to min(W - 1, floor(max sx)), y
     likewise; an empty box drops it.  Pixel (px, py) is sampled at (float64(px), float64(py)).
  3. Edge k runs from corner k to corner k + 1 mod 3 and weighs corner k + 2 mod 3.  If i_a < i_b:
     E = (xb - xa)(py - ya) - (yb - ya)(px - xa), canon = True; otherwise E = -((xa - xb)(py - yb) - (ya - yb)(px - xb)),
     canon = False.  e_k = s E.  The pixel is inside edge k iff e_k > 0, or e_k == 0 and canon != front.  It is covered iff it is
     inside all three edges and ssum = (b0 + b1) + b2 > 0, b_k the e of the edge opposite corner k: b0 = e_1, b1 = e_2, b2 = e_0.
  4. w_k = (b_k / ssum) / p2_k, ws = (w0 + w1) + w2, z = 1.0 / ws, z32 = float32(z); the pixel is skipped unless ws > 0 and z32
     is finite.  l_k = w_k / ws.  key = (uint64(bits(z32)) << 32) | t; the image of keys starts at all ones and takes the minimum.
     With ``cover`` a uint32 image counts the triangles that gave a pixel a key.
  5. Every pixel with a key: depth = z32, tri = t, bary = (float32(l1), float32(l2)), normal = (X1 - X0) x (X2 - X0), each
     component a b - c d, divided by sqrt((n0 n0 + n1 n1) + n2 n2) and converted to float32, 0 where that length is 0 or not
     finite.  Shading 0: per channel floor(((l0 g0 + l1 g1) + l2 g2) + 0.5) clamped to 0..255: grey and, where the mesh has
     colour, B, G, R.  Shading 1: tx = ((l0 c0x + l1 c1x) + l2 c2x) + float64(bx B), ty likewise, clamped to [0, A - 1], then
     texture_oracle's blend on the atlas; 3 channels give the colour image and grey = texture_oracle.grey_of it; 1 channel
     gives grey and no colour image.  A pixel without a key has depth 0, tri -1, bary 0, normal 0 and colour 0.

Two independent implementations, which tests/test_oracle_raster.py holds equal bit for bit: ``rasterise_loop`` walks the
triangles and the pixels of their boxes one at a time and keeps, for every pixel, the winner's own numbers; ``rasterise`` lists
every (triangle, pixel) pair of all boxes at once, reduces the keys and evaluates the winners again, as the device does.  A mesh
is the dict tests/mesh_oracle.py's ``weld`` returns (vertices, faces, grey, colour); a result is a dict of ``depth`` ((H, W)
float32), ``normal`` ((H, W, 3) float32), ``grey`` ((H, W) uint8), ``colour`` ((H, W, 3) uint8 or None), ``tri`` ((H, W) int32),
``bary`` ((H, W, 2) float32) and ``cover`` ((H, W) uint32 or None).
"""
import numpy as np

import dense_oracle as do
import texture_oracle as to

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
FIELDS = ("depth", "normal", "grey", "colour", "tri", "bary", "cover")


def _rows(mesh):
    X = np.asarray(mesh["vertices"], np.float64).reshape(-1, 3)
    F = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    g = np.asarray(mesh["grey"], np.uint8).reshape(-1)
    c = None if mesh.get("colour") is None else np.asarray(mesh["colour"], np.uint8).reshape(-1, 3)
    return X, F, g, c


def _camera(K, pose):
    t, q = do.normalise_pose(pose)
    return np.asarray(K, np.float64).reshape(4), t, do.rotation(q)


def _atlas(atlas, patch, n_tri):
    """(atlas (A, A, C), P, B, Q, A) or None."""
    if atlas is None:
        return None
    a = np.asarray(atlas, np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    B, Q, A = to.layout(n_tri, patch)
    assert a.shape[0] == A and a.shape[1] == A and a.shape[2] in (1, 3)
    return a, int(patch), B, Q, A


def _empty(W, H, colour, cover):
    return dict(depth=np.zeros((H, W), np.float32), normal=np.zeros((H, W, 3), np.float32), grey=np.zeros((H, W), np.uint8),
                colour=np.zeros((H, W, 3), np.uint8) if colour else None, tri=np.full((H, W), -1, np.int32),
                bary=np.zeros((H, W, 2), np.float32), cover=np.zeros((H, W), np.uint32) if cover else None)


# ---- the vectorised form ---------------------------------------------------------------------------------------------------
def _edge(ia, ib, xa, ya, xb, yb, px, py, s, front):
    canon = ia < ib
    E = np.where(canon, (xb - xa) * (py - ya) - (yb - ya) * (px - xa), -((xa - xb) * (py - yb) - (ya - yb) * (px - xb)))
    e = s * E
    return e, (e > 0.0) | ((e == 0.0) & (canon != front))


def _pixels(S, T, px, py):
    """Steps 3 and 4 for the pairs (triangle T, pixel px py): (ok, z32, l0, l1, l2)."""
    F, x, y, z, front = S["F"][T], S["x"][T], S["y"][T], S["z"][T], S["front"][T]
    s = np.where(front, -1.0, 1.0)
    fx, fy = px.astype(np.float64), py.astype(np.float64)
    with np.errstate(all="ignore"):
        e0, in0 = _edge(F[:, 0], F[:, 1], x[:, 0], y[:, 0], x[:, 1], y[:, 1], fx, fy, s, front)
        e1, in1 = _edge(F[:, 1], F[:, 2], x[:, 1], y[:, 1], x[:, 2], y[:, 2], fx, fy, s, front)
        e2, in2 = _edge(F[:, 2], F[:, 0], x[:, 2], y[:, 2], x[:, 0], y[:, 0], fx, fy, s, front)
        ssum = (e1 + e2) + e0
        w0, w1, w2 = (e1 / ssum) / z[:, 0], (e2 / ssum) / z[:, 1], (e0 / ssum) / z[:, 2]
        ws = (w0 + w1) + w2
        z32 = (1.0 / ws).astype(np.float32)
        ok = in0 & in1 & in2 & (ssum > 0.0) & (ws > 0.0) & np.isfinite(z32)
        return ok, z32, w0 / ws, w1 / ws, w2 / ws


def _setup(X, F, K, t, R, W, H, z_near, cull):
    """Steps 1 and 2 for every triangle."""
    p2, sx, sy = to.project(X, K, t, R)
    with np.errstate(all="ignore"):
        usable = (p2 > np.float64(z_near)) & np.isfinite(sx) & np.isfinite(sy)
        x, y, z = sx[F], sy[F], p2[F]
        area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        ok = usable[F].all(axis=1) & (area2 != 0.0) & ~np.isnan(area2)
        front = area2 < 0.0
        if cull:
            ok &= front
        x, y = np.where(ok[:, None], x, 0.0), np.where(ok[:, None], y, 0.0)
        xl, xh = np.maximum(0.0, np.ceil(x.min(axis=1))), np.minimum(W - 1.0, np.floor(x.max(axis=1)))
        yl, yh = np.maximum(0.0, np.ceil(y.min(axis=1))), np.minimum(H - 1.0, np.floor(y.max(axis=1)))
        ok &= (xl <= xh) & (yl <= yh)
    box = np.where(ok[:, None], np.stack([xl, xh, yl, yh], axis=1), 0.0).astype(np.int64)
    return dict(F=F, x=sx[F], y=sy[F], z=z, front=front, ok=ok, box=box)


def _shade(out, hy, hx, T, l0, l1, l2, X, F, g, c, tex):
    f = F[T]
    u, v = X[f[:, 1]] - X[f[:, 0]], X[f[:, 2]] - X[f[:, 0]]
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = (length > 0.0) & np.isfinite(length)
        out["normal"][hy, hx] = np.where(good[:, None], n / length[:, None], 0.0).astype(np.float32)
    if tex is None:
        blend = lambda a: np.minimum(np.maximum(np.floor(((l0 * a[f[:, 0]] + l1 * a[f[:, 1]]) + l2 * a[f[:, 2]]) + 0.5), 0.0), 255.0).astype(np.uint8)
        out["grey"][hy, hx] = blend(g.astype(np.float64))
        if c is not None:
            for ch in range(3):
                out["colour"][hy, hx, ch] = blend(c[:, ch].astype(np.float64))
        return
    atlas, P, B, Q, A = tex
    q, upper = T >> 1, (T & 1).astype(bool)
    c0 = np.where(upper, P + 1, 0).astype(np.float64)
    c1 = np.where(upper, 2, P - 1).astype(np.float64)
    tx = ((l0 * c0 + l1 * c1) + l2 * c0) + ((q % Q) * B).astype(np.float64)
    ty = ((l0 * c0 + l1 * c0) + l2 * c1) + ((q // Q) * B).astype(np.float64)
    val = to.sample(atlas, np.minimum(np.maximum(tx, 0.0), A - 1.0), np.minimum(np.maximum(ty, 0.0), A - 1.0))
    if atlas.shape[2] == 3:
        out["colour"][hy, hx] = val
        out["grey"][hy, hx] = to.grey_of(val)
    else:
        out["grey"][hy, hx] = val[:, 0]


def rasterise(mesh, shape, K, pose, z_near=0.0, cull=True, atlas=None, patch=None, cover=False):
    X, F, g, c = _rows(mesh)
    W, H = int(shape[0]), int(shape[1])
    K, t, R = _camera(K, pose)
    tex = _atlas(atlas, patch, len(F))
    out = _empty(W, H, tex[0].shape[2] == 3 if tex else c is not None, cover)
    S = _setup(X, F, K, t, R, W, H, z_near, cull)
    tids = np.nonzero(S["ok"])[0]
    box = S["box"][tids]
    bw, cnt = box[:, 1] - box[:, 0] + 1, (box[:, 1] - box[:, 0] + 1) * (box[:, 3] - box[:, 2] + 1)
    T = np.repeat(tids, cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    row = local // np.repeat(bw, cnt)
    px, py = np.repeat(box[:, 0], cnt) + (local - row * np.repeat(bw, cnt)), np.repeat(box[:, 2], cnt) + row
    ok, z32, _, _, _ = _pixels(S, T, px, py)
    T, px, py, z32 = T[ok], px[ok], py[ok], z32[ok]
    keys = np.full(H * W, NO_KEY, np.uint64)
    np.minimum.at(keys, py * W + px, (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | T.astype(np.uint64))
    if cover:
        np.add.at(out["cover"].reshape(-1), py * W + px, np.uint32(1))
    hit = np.nonzero(keys != NO_KEY)[0]
    hy, hx, Tw = hit // W, hit % W, (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok, z32, l0, l1, l2 = _pixels(S, Tw, hx, hy)
    assert ok.all() and np.array_equal(z32.view(np.uint32).astype(np.uint64), keys[hit] >> np.uint64(32))
    out["depth"][hy, hx] = z32
    out["tri"][hy, hx] = Tw
    out["bary"][hy, hx] = np.stack([l1, l2], axis=1).astype(np.float32)
    _shade(out, hy, hx, Tw, l0, l1, l2, X, F, g, c, tex)
    return out


# ---- the loop form -----------------------------------------------------------------------------------------------------------
def _edge_loop(ia, ib, xa, ya, xb, yb, px, py, s, front):
    if ia < ib:
        E, canon = (xb - xa) * (py - ya) - (yb - ya) * (px - xa), True
    else:
        E, canon = -((xa - xb) * (py - yb) - (ya - yb) * (px - xb)), False
    e = s * E
    return e, bool(e > 0.0 or (e == 0.0 and canon != front))


def _byte(v):
    return int(min(max(np.floor(v + 0.5), 0.0), 255.0))


def rasterise_loop(mesh, shape, K, pose, z_near=0.0, cull=True, atlas=None, patch=None, cover=False):
    X, F, g, c = _rows(mesh)
    W, H = int(shape[0]), int(shape[1])
    K, t, R = _camera(K, pose)
    tex = _atlas(atlas, patch, len(F))
    out = _empty(W, H, tex[0].shape[2] == 3 if tex else c is not None, cover)
    best = {}                          # pixel -> (bits of z32, t, z32, l0, l1, l2)
    with np.errstate(all="ignore"):
        pr = [to._project_loop(X[v], K, t, R) for v in range(len(X))]
        for tr in range(len(F)):
            i = [int(v) for v in F[tr]]
            (z0, x0, y0), (z1, x1, y1), (z2, x2, y2) = (pr[v] for v in i)
            if not all(pr[v][0] > z_near and np.isfinite(pr[v][1]) and np.isfinite(pr[v][2]) for v in i):
                continue
            area2 = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if area2 == 0.0 or np.isnan(area2):
                continue
            front = bool(area2 < 0.0)
            if cull and not front:
                continue
            s = np.float64(-1.0 if front else 1.0)
            xl, xh = max(0.0, np.ceil(min(x0, x1, x2))), min(W - 1.0, np.floor(max(x0, x1, x2)))
            yl, yh = max(0.0, np.ceil(min(y0, y1, y2))), min(H - 1.0, np.floor(max(y0, y1, y2)))
            if not (xl <= xh and yl <= yh):
                continue
            for iy in range(int(yl), int(yh) + 1):
                for ix in range(int(xl), int(xh) + 1):
                    px, py = np.float64(ix), np.float64(iy)
                    e0, in0 = _edge_loop(i[0], i[1], x0, y0, x1, y1, px, py, s, front)
                    e1, in1 = _edge_loop(i[1], i[2], x1, y1, x2, y2, px, py, s, front)
                    e2, in2 = _edge_loop(i[2], i[0], x2, y2, x0, y0, px, py, s, front)
                    ssum = (e1 + e2) + e0
                    if not (in0 and in1 and in2 and ssum > 0.0):
                        continue
                    w0, w1, w2 = (e1 / ssum) / z0, (e2 / ssum) / z1, (e0 / ssum) / z2
                    ws = (w0 + w1) + w2
                    z32 = np.float32(np.float64(1.0) / ws)
                    if not (ws > 0.0 and np.isfinite(z32)):
                        continue
                    if cover:
                        out["cover"][iy, ix] += 1
                    cand = (int(z32.view(np.uint32)), tr, z32, w0 / ws, w1 / ws, w2 / ws)
                    if (iy, ix) not in best or cand[:2] < best[(iy, ix)][:2]:
                        best[(iy, ix)] = cand
        for (iy, ix), (_, tr, z32, l0, l1, l2) in best.items():
            i = [int(v) for v in F[tr]]
            out["depth"][iy, ix], out["tri"][iy, ix] = z32, tr
            out["bary"][iy, ix] = (np.float32(l1), np.float32(l2))
            u, v = X[i[1]] - X[i[0]], X[i[2]] - X[i[0]]
            n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if length > 0.0 and np.isfinite(length):
                out["normal"][iy, ix] = [np.float32(n[k] / length) for k in range(3)]
            if tex is None:
                out["grey"][iy, ix] = _byte((l0 * np.float64(g[i[0]]) + l1 * np.float64(g[i[1]])) + l2 * np.float64(g[i[2]]))
                if c is not None:
                    for ch in range(3):
                        out["colour"][iy, ix, ch] = _byte((l0 * np.float64(c[i[0], ch]) + l1 * np.float64(c[i[1], ch])) + l2 * np.float64(c[i[2], ch]))
                continue
            a, P, B, Q, A = tex
            q = tr >> 1
            (c0x, c0y), (c1x, c1y), (c2x, c2y) = to.corners(P, tr & 1)
            tx = ((l0 * np.float64(c0x) + l1 * np.float64(c1x)) + l2 * np.float64(c2x)) + np.float64((q % Q) * B)
            ty = ((l0 * np.float64(c0y) + l1 * np.float64(c1y)) + l2 * np.float64(c2y)) + np.float64((q // Q) * B)
            tx, ty = min(max(tx, 0.0), A - 1.0), min(max(ty, 0.0), A - 1.0)
            jx0, jx1, ax = to._tap_loop(a, tx, A)
            jy0, jy1, ay = to._tap_loop(a, ty, A)
            val = [((32 - ax) * (32 - ay) * int(a[jy0, jx0, ch]) + ax * (32 - ay) * int(a[jy0, jx1, ch]) + (32 - ax) * ay * int(a[jy1, jx0, ch]) +
                    ax * ay * int(a[jy1, jx1, ch]) + 512) >> 10 for ch in range(a.shape[2])]
            if len(val) == 3:
                out["colour"][iy, ix] = val
                out["grey"][iy, ix] = (val[0] * 1868 + val[1] * 9617 + val[2] * 4899 + 8192) >> 14
            else:
                out["grey"][iy, ix] = val[0]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b, fields=FIELDS):
    """Two results equal bit for bit."""
    for k in fields:
        x, y = a[k], b[k]
        if (x is None) != (y is None):
            return False
        if x is not None and (x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(bits(x), bits(y))):
            return False
    return True
