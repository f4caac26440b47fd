"""numpy restatement of the texture-atlas contract of the welded, pruned, smoothed or simplified mesh, written
from the contract.

The input is a source mesh (X float64, F, vertex grey and optional B, G, R) with n_tri > 0 triangles, a patch size P in 2..32
and ``channels``, 1 or 3.  Every float64 operation is rounded once, in the written order.

  1. The layout.  Triangles are paired into square blocks of side B = P + 2 texels: block q = t >> 1 holds triangle 2 q (the
     lower one) and 2 q + 1 (the upper one).  n_sq = (n_tri + 1) >> 1, Q is the least integer with Q Q >= n_sq, the atlas is
     A x A texels with A = Q B, row 0 first; block q sits at (bx, by) = (q % Q, q // Q).  A texel with block-local coordinates
     (a, b) belongs to the lower triangle iff a + b <= P, otherwise to the upper one.  Corner texel centres: lower c0 = (0, 0),
     c1 = (P - 1, 0), c2 = (0, P - 1); upper c0 = (P + 1, P + 1), c1 = (2, P + 1), c2 = (P + 1, 2).  Barycentrics of a texel:
     lower l1 = float64(a) / float64(P - 1), l2 = float64(b) / float64(P - 1); upper l1 = float64(P + 1 - a) / float64(P - 1),
     l2 = float64(P + 1 - b) / float64(P - 1); l0 = (1.0 - l1) - l2.  UV of corner i of triangle t:
     (float64(bx B + c_i.x) + 0.5) / float64(A), likewise for y, measured from row 0.
  2. A vertex in a view (an image of W x H, K = fx fy cx cy, a pose, an optional z-buffer): d = X - t, p = R^T d (each entry the
     sum from left to right), sx = fx (p0 / p2) + cx, sy = fy (p1 / p2) + cy.  It is visible iff p2 > 0, 0 <= sx <= W - 1,
     0 <= sy <= H - 1 (a NaN fails) and, with a z-buffer, D = float64(zbuf[floor(sy + 0.5), floor(sx + 0.5)]) has D > 0 and
     p2 <= D + tol.
  3. A triangle in a view is a candidate iff its three vertices are visible.  Its score is SIGMA ((sx1 - sx0) (sy2 - sy0) -
     (sy1 - sy0) (sx2 - sx0)) with SIGMA = -1.  The view wins triangle t iff score > min_area2 and score > best_score[t];
     best_score starts at 0 and best_view at -1.  A view's number is the count of views added since the begin.
  4. The fill, for every texel of a triangle that the current view has just won: Xp = (l0 X0 + l1 X1) + l2 X2 per coordinate,
     projected as in 2; if not p2 > 0 or sx or sy is NaN the texel is left as it is; sx is clamped to [0, W - 1] and sy to
     [0, H - 1]; q = int(floor(s 32 + 0.5)), i = q >> 5, alpha = q & 31, the second tap is min(i + 1, dim - 1), the weights are
     (32 - ax)(32 - ay), ax (32 - ay), (32 - ax) ay and ax ay, the value is (sum w tap + 512) >> 10.  A 3-channel atlas takes B,
     G, R and a grey view replicates its value; a 1-channel atlas takes the view's grey image, of a colour view
     (b 1868 + g 9617 + r 4899 + 8192) >> 14.
  5. The finish: the texels of a triangle with best_view = -1 get, per channel, floor(((l0 g0 + l1 g1) + l2 g2) + 0.5) clamped
     to 0..255, g the vertex grey, or B, G, R where the mesh has colour and the atlas 3 channels.  Padding stays 0.  n_textured
     is the number of triangles with a view.

Two independent implementations, which tests/test_oracle_texture.py holds equal to each other bit for bit: a plain loop over the
vertices, the triangles and the texels of every block (``texture_loop``), and a vectorised form over the whole atlas
(``texture``).  A mesh is the dict tests/mesh_oracle.py's ``weld`` returns (vertices, faces, grey, colour); a view is a dict of
``image`` ((H, W) or (H, W, 3) uint8), ``K``, ``pose`` and optionally ``zbuf`` ((H, W) float32), ``tol`` and ``min_area2``; a
result is a dict of ``atlas`` ((A, A, channels) uint8), ``uv`` ((n_tri, 3, 2) float64), ``view`` (int32), ``score`` (float64),
``n_won`` (one count a view) and ``n_textured``.
"""
import numpy as np

import dense_oracle as do

SIGMA = np.float64(-1.0)
MAX_SIDE = 16384


def layout(n_tri, P):
    """(B, Q, A)."""
    n_sq = (int(n_tri) + 1) >> 1
    Q = 0
    while Q * Q < n_sq:
        Q += 1
    return P + 2, Q, Q * (P + 2)


def corners(P, upper):
    return ((P + 1, P + 1), (2, P + 1), (P + 1, 2)) if upper else ((0, 0), (P - 1, 0), (0, P - 1))


def uv(n_tri, P):
    B, Q, A = layout(n_tri, P)
    out = np.zeros((n_tri, 3, 2), np.float64)
    for t in range(n_tri):
        q = t >> 1
        bx, by = q % Q, q // Q
        for i, (cx, cy) in enumerate(corners(P, t & 1)):
            out[t, i, 0] = (np.float64(bx * B + cx) + 0.5) / np.float64(A)
            out[t, i, 1] = (np.float64(by * B + cy) + 0.5) / np.float64(A)
    return out


def grey_of(bgr):
    a = np.asarray(bgr, np.uint8).astype(np.uint32)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def view_image(image, channels):
    """The (H, W, channels) image a view contributes to an atlas of ``channels``."""
    img = np.asarray(image, np.uint8)
    if channels == 1:
        return (grey_of(img) if img.ndim == 3 else img)[:, :, None]
    return img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)


def _rows(mesh, channels):
    X = np.asarray(mesh["vertices"], np.float64).reshape(-1, 3)
    F = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    if channels == 3 and mesh.get("colour") is not None:
        g = np.asarray(mesh["colour"], np.uint8).reshape(-1, 3)
    else:
        g = np.repeat(np.asarray(mesh["grey"], np.uint8).reshape(-1, 1), channels, axis=1)
    return X, F, g


def _camera(view):
    K = np.asarray(view["K"], np.float64).reshape(4)
    t, q = do.normalise_pose(view["pose"])
    return K, t, do.rotation(q)


# ---- the vectorised form ---------------------------------------------------------------------------------------------------
def project(X, K, t, R):
    """(p2, sx, sy) of the rows of X."""
    with np.errstate(all="ignore"):
        d = [X[..., c] - t[c] for c in range(3)]
        p = [R[0, i] * d[0] + R[1, i] * d[1] + R[2, i] * d[2] for i in range(3)]
        sx = K[0] * (p[0] / p[2]) + K[2]
        sy = K[1] * (p[1] / p[2]) + K[3]
    return p[2], sx, sy


def visible(p2, sx, sy, W, H, zbuf, tol):
    with np.errstate(all="ignore"):
        ok = (p2 > 0.0) & (sx >= 0.0) & (sx <= W - 1.0) & (sy >= 0.0) & (sy <= H - 1.0)
        if zbuf is not None:
            jx = np.where(ok, np.floor(sx + 0.5), 0.0).astype(np.int64)
            jy = np.where(ok, np.floor(sy + 0.5), 0.0).astype(np.int64)
            D = np.asarray(zbuf, np.float32)[jy, jx].astype(np.float64)
            ok = ok & (D > 0.0) & (p2 <= D + np.float64(tol))
    return ok


def texel_map(n_tri, P):
    """(tri (A, A) int64 with -1 for padding, l0, l1, l2 (A, A) float64)."""
    B, Q, A = layout(n_tri, P)
    y, x = np.meshgrid(np.arange(A), np.arange(A), indexing="ij")
    bx, a, by, b = x // B, x % B, y // B, y % B
    upper = a + b > P
    tri = 2 * (by * Q + bx) + upper
    den = np.float64(P - 1)
    l1 = np.where(upper, P + 1 - a, a).astype(np.float64) / den
    l2 = np.where(upper, P + 1 - b, b).astype(np.float64) / den
    l0 = (1.0 - l1) - l2
    return np.where(tri < n_tri, tri, -1), l0, l1, l2


def sample(img, sx, sy):
    """The blend of step 4 at clamped coordinates: (n, channels) uint8."""
    H, W = img.shape[:2]
    qx = np.floor(sx * 32.0 + 0.5).astype(np.int64)
    qy = np.floor(sy * 32.0 + 0.5).astype(np.int64)
    ix, ax, iy, ay = qx >> 5, qx & 31, qy >> 5, qy & 31
    jx, jy = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    im = img.astype(np.int64)
    w = [((32 - ax) * (32 - ay))[:, None], (ax * (32 - ay))[:, None], ((32 - ax) * ay)[:, None], (ax * ay)[:, None]]
    return ((w[0] * im[iy, ix] + w[1] * im[iy, jx] + w[2] * im[jy, ix] + w[3] * im[jy, jx] + 512) >> 10).astype(np.uint8)


def begin(mesh, P, channels):
    assert 2 <= P <= 32 and channels in (1, 3)
    X, F, g = _rows(mesh, channels)
    n_tri = len(F)
    assert n_tri > 0
    B, Q, A = layout(n_tri, P)
    assert A <= MAX_SIDE
    return dict(X=X, F=F, g=g, P=P, channels=channels, A=A, atlas=np.zeros((A, A, channels), np.uint8),
                view=np.full(n_tri, -1, np.int32), score=np.zeros(n_tri, np.float64), n_won=[], map=texel_map(n_tri, P))


def add_view(s, view):
    X, F = s["X"], s["F"]
    img = view_image(view["image"], s["channels"])
    H, W = img.shape[:2]
    K, t, R = _camera(view)
    p2, sx, sy = project(X, K, t, R)
    vis = visible(p2, sx, sy, W, H, view.get("zbuf"), view.get("tol", 0.0))
    cand = vis[F[:, 0]] & vis[F[:, 1]] & vis[F[:, 2]]
    with np.errstate(all="ignore"):
        x0, x1, x2, y0, y1, y2 = sx[F[:, 0]], sx[F[:, 1]], sx[F[:, 2]], sy[F[:, 0]], sy[F[:, 1]], sy[F[:, 2]]
        score = SIGMA * ((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0))
        won = cand & (score > np.float64(view.get("min_area2", 0.0))) & (score > s["score"])
    s["score"][won] = score[won]
    s["view"][won] = len(s["n_won"])
    s["n_won"].append(int(won.sum()))
    tri, l0, l1, l2 = s["map"]
    sel = np.zeros(tri.shape, bool)
    sel[tri >= 0] = won[tri[tri >= 0]]
    ty, tx = np.nonzero(sel)
    if not len(ty):
        return 0
    f = F[tri[ty, tx]]
    a0, a1, a2 = l0[ty, tx][:, None], l1[ty, tx][:, None], l2[ty, tx][:, None]
    Xp = (a0 * X[f[:, 0]] + a1 * X[f[:, 1]]) + a2 * X[f[:, 2]]
    q2, qx, qy = project(Xp, K, t, R)
    with np.errstate(all="ignore"):
        keep = (q2 > 0.0) & ~np.isnan(qx) & ~np.isnan(qy)
    cx = np.minimum(np.maximum(qx[keep], 0.0), W - 1.0)
    cy = np.minimum(np.maximum(qy[keep], 0.0), H - 1.0)
    s["atlas"][ty[keep], tx[keep]] = sample(img, cx, cy)
    return s["n_won"][-1]


def finish(s):
    tri, l0, l1, l2 = s["map"]
    sel = np.zeros(tri.shape, bool)
    sel[tri >= 0] = s["view"][tri[tri >= 0]] < 0
    ty, tx = np.nonzero(sel)
    f = s["F"][tri[ty, tx]]
    g = s["g"].astype(np.float64)
    a0, a1, a2 = l0[ty, tx][:, None], l1[ty, tx][:, None], l2[ty, tx][:, None]
    v = np.floor(((a0 * g[f[:, 0]] + a1 * g[f[:, 1]]) + a2 * g[f[:, 2]]) + 0.5)
    s["atlas"][ty, tx] = np.minimum(np.maximum(v, 0.0), 255.0).astype(np.uint8)
    return result(s)


def result(s):
    return dict(atlas=s["atlas"], uv=uv(len(s["F"]), s["P"]), view=s["view"], score=s["score"], n_won=list(s["n_won"]),
                n_textured=int((s["view"] >= 0).sum()))


def texture(mesh, P, channels, views):
    s = begin(mesh, P, channels)
    for v in views:
        add_view(s, v)
    return finish(s)


# ---- the loop form -----------------------------------------------------------------------------------------------------------
def _project_loop(x, K, t, R):
    with np.errstate(all="ignore"):
        d = [np.float64(x[c]) - t[c] for c in range(3)]
        p0 = R[0, 0] * d[0] + R[1, 0] * d[1] + R[2, 0] * d[2]
        p1 = R[0, 1] * d[0] + R[1, 1] * d[1] + R[2, 1] * d[2]
        p2 = R[0, 2] * d[0] + R[1, 2] * d[1] + R[2, 2] * d[2]
        return p2, K[0] * (p0 / p2) + K[2], K[1] * (p1 / p2) + K[3]


def _tap_loop(img, s, dim):
    q = int(np.floor(s * 32.0 + 0.5))
    i = q >> 5
    return i, min(i + 1, dim - 1), q & 31


def _texels_loop(P, upper):
    """The block-local texels of a triangle with their barycentrics."""
    den = np.float64(P - 1)
    for b in range(P + 2):
        for a in range(P + 2):
            if (a + b > P) != bool(upper):
                continue
            l1 = np.float64(P + 1 - a if upper else a) / den
            l2 = np.float64(P + 1 - b if upper else b) / den
            yield a, b, (np.float64(1.0) - l1) - l2, l1, l2


def texture_loop(mesh, P, channels, views):
    X, F, g = _rows(mesh, channels)
    n_tri = len(F)
    B, Q, A = layout(n_tri, P)
    atlas = np.zeros((A, A, channels), np.uint8)
    best_view, best_score, n_won = [-1] * n_tri, [np.float64(0.0)] * n_tri, []
    for number, view in enumerate(views):
        img = view_image(view["image"], channels)
        H, W = img.shape[:2]
        K, t, R = _camera(view)
        zbuf, tol, min_area2 = view.get("zbuf"), np.float64(view.get("tol", 0.0)), np.float64(view.get("min_area2", 0.0))
        pr = []
        for v in range(len(X)):
            p2, sx, sy = _project_loop(X[v], K, t, R)
            ok = bool(p2 > 0.0 and 0.0 <= sx <= W - 1.0 and 0.0 <= sy <= H - 1.0)
            if ok and zbuf is not None:
                D = np.float64(zbuf[int(np.floor(sy + 0.5)), int(np.floor(sx + 0.5))])
                ok = bool(D > 0.0 and p2 <= D + tol)
            pr.append((ok, sx, sy))
        count = 0
        for tr in range(n_tri):
            (k0, x0, y0), (k1, x1, y1), (k2, x2, y2) = (pr[int(i)] for i in F[tr])
            if not (k0 and k1 and k2):
                continue
            score = SIGMA * ((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0))
            if not (score > min_area2 and score > best_score[tr]):
                continue
            best_score[tr], best_view[tr] = score, number
            count += 1
            q = tr >> 1
            ox, oy = (q % Q) * B, (q // Q) * B
            P0, P1, P2 = (X[int(i)] for i in F[tr])
            for a, b, l0, l1, l2 in _texels_loop(P, tr & 1):
                xp = [(l0 * P0[c] + l1 * P1[c]) + l2 * P2[c] for c in range(3)]
                p2, sx, sy = _project_loop(xp, K, t, R)
                if not p2 > 0.0 or np.isnan(sx) or np.isnan(sy):
                    continue
                sx, sy = min(max(sx, 0.0), W - 1.0), min(max(sy, 0.0), H - 1.0)
                ix, jx, ax = _tap_loop(img, sx, W)
                iy, jy, ay = _tap_loop(img, sy, H)
                for ch in range(channels):
                    acc = ((32 - ax) * (32 - ay) * int(img[iy, ix, ch]) + ax * (32 - ay) * int(img[iy, jx, ch]) +
                           (32 - ax) * ay * int(img[jy, ix, ch]) + ax * ay * int(img[jy, jx, ch]) + 512)
                    atlas[oy + b, ox + a, ch] = acc >> 10
        n_won.append(count)
    for tr in range(n_tri):
        if best_view[tr] >= 0:
            continue
        q = tr >> 1
        ox, oy = (q % Q) * B, (q // Q) * B
        g0, g1, g2 = (g[int(i)].astype(np.float64) for i in F[tr])
        for a, b, l0, l1, l2 in _texels_loop(P, tr & 1):
            for ch in range(channels):
                v = np.floor(((l0 * g0[ch] + l1 * g1[ch]) + l2 * g2[ch]) + 0.5)
                atlas[oy + b, ox + a, ch] = int(min(max(v, 0.0), 255.0))
    return dict(atlas=atlas, uv=uv(n_tri, P), view=np.array(best_view, np.int32), score=np.array(best_score, np.float64), n_won=n_won,
                n_textured=sum(1 for v in best_view if v >= 0))


FIELDS = ("atlas", "uv", "view", "score")


def same(a, b):
    """Two results equal bit for bit."""
    for k in FIELDS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape:
            return False
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        if not np.array_equal(x, y):
            return False
    return a["n_won"] == b["n_won"] and a["n_textured"] == b["n_textured"]
