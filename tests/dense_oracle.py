"""numpy restatement of the dense plane-sweep contract, written from the contract: relative poses, the
plane warp, the 5-bit bilinear sample, truncated absolute differences summed over the views and a square window, the
winner with its sub-plane refinement, the geometric filter and the back-projection.

Every coordinate operation is fp64, rounded once, in the written left-to-right order: sums of three products are spelled
out (never `@`, which may fuse or reorder), and numpy never contracts a product and a sum.  Costs are exact integers.
"""
import numpy as np

MAX_PLANES, MAX_RADIUS, MAX_SOURCES, MAX_VIEWS = 1024, 4, 8, 16


# ---- poses ---------------------------------------------------------------------------------------------------------------
def normalise_pose(pose7):
    """(t, q): the camera centre and q = (w, x, y, z) divided by its norm, sqrt(((w w + x x) + y y) + z z)."""
    p = np.asarray(pose7, np.float64).reshape(7)
    w, x, y, z = p[3], p[4], p[5], p[6]
    n = np.sqrt(w * w + x * x + y * y + z * z)
    return p[:3].copy(), np.array([w / n, x / n, y / n, z / n], np.float64)


def rotation(q):
    """R (camera to world) of a normalised q, x_cam = R^T (X - t): the nine entries in the written order."""
    w, x, y, z = (np.float64(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]], np.float64)


def relative(pose_r, pose_v):
    """A = R_v^T R_r and b = R_v^T (t_r - t_v): each entry the sum over k = 0, 1, 2 from left to right."""
    tr, qr = normalise_pose(pose_r)
    tv, qv = normalise_pose(pose_v)
    Rr, Rv = rotation(qr), rotation(qv)
    d = [tr[k] - tv[k] for k in range(3)]
    A = np.zeros((3, 3), np.float64)
    b = np.zeros(3, np.float64)
    for i in range(3):
        for j in range(3):
            A[i, j] = Rv[0, i] * Rr[0, j] + Rv[1, i] * Rr[1, j] + Rv[2, i] * Rr[2, j]
        b[i] = Rv[0, i] * d[0] + Rv[1, i] * d[1] + Rv[2, i] * d[2]
    return A, b


# ---- planes and the warp -------------------------------------------------------------------------------------------------
def plane_step(w_min, w_max, D):
    return (np.float64(w_max) - np.float64(w_min)) / np.float64(D - 1)


def plane_depth(w_min, step, k):
    return 1.0 / (np.float64(w_min) + np.float64(k) * step)


def rays(K, W, H):
    """x = (X - cx)/fx, y = (Y - cy)/fy on the pixel grid, each (H, W)."""
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return (X - K[2]) / K[0], (Y - K[3]) / K[1]


def project(x, y, z, A, b, Kv):
    """Steps 2-5: (Q_2, sx, sy) of the rays (x, y) at depth z (a scalar or an array) in the view (A, b, Kv)."""
    with np.errstate(all="ignore"):
        a0 = A[0, 0] * x + A[0, 1] * y + A[0, 2]
        a1 = A[1, 0] * x + A[1, 1] * y + A[1, 2]
        a2 = A[2, 0] * x + A[2, 1] * y + A[2, 2]
        Q0 = z * a0 + b[0]
        Q1 = z * a1 + b[1]
        Q2 = z * a2 + b[2]
        sx = Kv[0] * (Q0 / Q2) + Kv[2]
        sy = Kv[1] * (Q1 / Q2) + Kv[3]
    return Q2, sx, sy


INVALID_BEHIND, INVALID_OUTSIDE, VALID, VALID_LAST_EDGE = 0, 1, 2, 3


def warp(x, y, z, A, b, Kv, W, H):
    """(valid, qx, qy, cls) of one plane and view.  cls: INVALID_BEHIND (Q_2 <= 0 or NaN), INVALID_OUTSIDE, VALID, or
    VALID_LAST_EDGE: valid with qx = 32 (W - 1) or qy = 32 (H - 1), where the second tap has weight 0 and a clamped address."""
    Q2, sx, sy = project(x, y, z, A, b, Kv)
    with np.errstate(invalid="ignore"):
        front = Q2 > 0.0
        fx_ = np.floor(sx * 32.0 + 0.5)
        fy_ = np.floor(sy * 32.0 + 0.5)
        inside = (fx_ >= 0.0) & (fx_ <= 32.0 * (W - 1)) & (fy_ >= 0.0) & (fy_ <= 32.0 * (H - 1))
    valid = front & inside
    qx = np.where(valid, fx_, 0.0).astype(np.int64)
    qy = np.where(valid, fy_, 0.0).astype(np.int64)
    cls = np.where(~front, INVALID_BEHIND, np.where(~inside, INVALID_OUTSIDE, VALID))
    cls = np.where(valid & ((qx == 32 * (W - 1)) | (qy == 32 * (H - 1))), VALID_LAST_EDGE, cls)
    return valid, qx, qy, cls


def sample(img, qx, qy):
    """The 5-bit bilinear blend of §14.1 at fixed-point positions inside the image."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    H, W = a.shape
    ix, ax, iy, ay = qx >> 5, qx & 31, qy >> 5, qy & 31
    x1, y1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    acc = ((32 - ax) * (32 - ay) * a[iy, ix] + ax * (32 - ay) * a[iy, x1] + (32 - ax) * ay * a[y1, ix] + ax * ay * a[y1, x1])
    return (acc + 512) >> 10


def box_sum(c, radius):
    """Sum over the (2 radius + 1)^2 window; positions outside the image contribute nothing."""
    H, W = c.shape
    p = np.zeros((H + 2 * radius, W + 2 * radius), np.int64)
    p[radius:radius + H, radius:radius + W] = c
    out = np.zeros((H, W), np.int64)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out += p[dy:dy + H, dx:dx + W]
    return out


def cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc):
    """(C, V): C[k] the aggregated cost of plane k (int64, (D, H, W)), V[k] the number of sources whose warp of the pixel
    itself is valid.  sources: a list of (image, K, pose7)."""
    ref = np.asarray(ref, np.uint8)
    H, W = ref.shape
    x, y = rays(Kr, W, H)
    step = plane_step(w_min, w_max, D)
    rel = [relative(pose_r, p) for (_, _, p) in sources]
    C = np.zeros((D, H, W), np.int64)
    V = np.zeros((D, H, W), np.int64)
    I = ref.astype(np.int64)
    for k in range(D):
        z = plane_depth(w_min, step, k)
        c = np.zeros((H, W), np.int64)
        for (img, Kv, _), (A, b) in zip(sources, rel):
            valid, qx, qy, _ = warp(x, y, z, A, b, Kv, W, H)
            g = sample(img, qx, qy)
            c += np.where(valid, np.minimum(np.abs(I - g), trunc), trunc)
            V[k] += valid
        C[k] = box_sum(c, radius)
    return C, V


def refine_delta(Cm, Cp, C0):
    """delta = (C- - C+) / (2 den) where den = C- - 2 C0 + C+ > 0, otherwise 0."""
    Cm, Cp, C0 = (np.asarray(v, np.int64) for v in (Cm, Cp, C0))
    den = Cm - 2 * C0 + Cp
    with np.errstate(all="ignore"):
        d = (Cm - Cp).astype(np.float64) / (2.0 * den.astype(np.float64))
    return np.where(den > 0, d, 0.0)


def winner(C, V, w_min, w_max):
    """depth float32, plane int32, cost uint32, views uint8, and the refined inverse depth (fp64; NaN where no depth)."""
    D, H, W = C.shape
    step = plane_step(w_min, w_max, D)
    k = np.argmin(C, axis=0)                                      # the first minimum: the smallest k
    take = lambda vol, kk: np.take_along_axis(vol, kk[None], axis=0)[0]
    C0 = take(C, k)
    views = take(V, k)
    inner = (k > 0) & (k < D - 1)
    Cm = take(C, np.maximum(k - 1, 0))
    Cp = take(C, np.minimum(k + 1, D - 1))
    delta = np.where(inner, refine_delta(Cm, Cp, C0), 0.0)
    w = np.float64(w_min) + (k.astype(np.float64) + delta) * step
    depth = (1.0 / w).astype(np.float32)
    none = views == 0
    return dict(depth=np.where(none, np.float32(0), depth).astype(np.float32), plane=np.where(none, -1, k).astype(np.int32),
                cost=C0.astype(np.uint32), views=views.astype(np.uint8), inv_depth=np.where(none, np.nan, w), delta=delta)


def sweep(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc):
    C, V = cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc)
    return winner(C, V, w_min, w_max)


# ---- the geometric filter and the points ----------------------------------------------------------------------------------
def geometric_filter(depth, plane, Kr, pose_r, sources, rel_tol, min_agree):
    """(depth, plane) filtered.  sources: a list of (swept depth of the source, K, pose7)."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    x, y = rays(Kr, W, H)
    z = depth.astype(np.float64)
    agree = np.zeros((H, W), np.int64)
    for (ds, Kv, pv) in sources:
        A, b = relative(pose_r, pv)
        Q2, sx, sy = project(x, y, z, A, b, Kv)
        with np.errstate(invalid="ignore"):
            jx_, jy_ = np.floor(sx + 0.5), np.floor(sy + 0.5)
            ok = (Q2 > 0.0) & (jx_ >= 0.0) & (jx_ <= W - 1.0) & (jy_ >= 0.0) & (jy_ <= H - 1.0)
        jx = np.where(ok, jx_, 0.0).astype(np.int64)
        jy = np.where(ok, jy_, 0.0).astype(np.int64)
        zs = np.asarray(ds, np.float32)[jy, jx].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok &= (zs != 0.0) & (np.abs(Q2 - zs) <= np.float64(rel_tol) * Q2)
        agree += ok
    keep = (depth > 0) & (agree >= min_agree)
    return np.where(keep, depth, np.float32(0)).astype(np.float32), np.where(keep, plane, -1).astype(np.int32)


def points(depth, K, pose):
    """X_w = R (z (x, y, 1)) + t per pixel, (H, W, 3) fp64; NaN where the depth is 0."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    x, y = rays(K, W, H)
    t, q = normalise_pose(pose)
    R = rotation(q)
    z = depth.astype(np.float64)
    p0, p1, p2 = z * x, z * y, z
    out = np.stack([R[i, 0] * p0 + R[i, 1] * p1 + R[i, 2] * p2 + t[i] for i in range(3)], axis=2)
    out[~(depth > 0)] = np.nan
    return out
