"""numpy restatement of the ray-casting contract, written from the contract: the mean plane of a TSDF
volume, the trilinear sample and its gradient, the ray of a pixel and the march that ends at the first outside-to-inside
crossing of two valid samples.

Every coordinate operation is fp64, rounded once, in the written left-to-right order (numpy never contracts a product and a
sum).  Poses are those of tests/dense_oracle.py (§15.1), unchanged; the volume is that of tests/fusion_oracle.py (§16.1).
`raycast(..., skip_box=True)` is the variant a kernel may run: it leaves out the samples it has proved to lie outside the
volume's box, and must give the same bits.
"""
import numpy as np

import dense_oracle as do

MAX_DIM, MAX_SAMPLES, MAX_COUNT = 8192, 65536, 65535


def mean_plane(vol, min_count=1):
    """m = (float) ((double) sum / (double) cnt) where cnt >= min_count, else a quiet NaN; fp32, (nz, ny, nx)."""
    s_, c_, _ = vol
    with np.errstate(all="ignore"):
        m = (s_.astype(np.float64) / c_.astype(np.float64)).astype(np.float32)
    m[c_ < min_count] = np.float32(np.nan)
    return m


def samples(z_near, z_far, step):
    """N = floor((z_far - z_near) / step) + 1."""
    return int(np.floor((np.float64(z_far) - np.float64(z_near)) / np.float64(step))) + 1


def rays(shape, K, pose7):
    """(t, dw): the camera centre and the world direction of every pixel, dw[i] of shape (H W,), for unit camera z."""
    W, H = int(shape[0]), int(shape[1])
    K = np.asarray(K, np.float64)
    t, q = do.normalise_pose(pose7)
    R = do.rotation(q)
    with np.errstate(all="ignore"):
        dc0 = np.broadcast_to(((np.arange(W, dtype=np.float64) - K[2]) / K[0])[None, :], (H, W)).reshape(-1)
        dc1 = np.broadcast_to(((np.arange(H, dtype=np.float64) - K[3]) / K[1])[:, None], (H, W)).reshape(-1)
        dw = [R[i, 0] * dc0 + R[i, 1] * dc1 + R[i, 2] for i in range(3)]
    return t, dw


def _lerp(a, b, f):
    return a + f * (b - a)


def trilinear(v, f):
    a00, a10, a01, a11 = _lerp(v[0], v[1], f[0]), _lerp(v[2], v[3], f[0]), _lerp(v[4], v[5], f[0]), _lerp(v[6], v[7], f[0])
    return _lerp(_lerp(a00, a10, f[1]), _lerp(a01, a11, f[1]), f[2])


def gradient(v, f):
    bil = lambda d, fa, fb: _lerp(_lerp(d[0], d[1], fa), _lerp(d[2], d[3], fa), fb)
    return (bil((v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6]), f[1], f[2]),
            bil((v[2] - v[0], v[3] - v[1], v[6] - v[4], v[7] - v[5]), f[0], f[2]),
            bil((v[4] - v[0], v[5] - v[1], v[6] - v[2], v[7] - v[3]), f[0], f[1]))


def locate(X, dims, origin, inv):
    """(in range (a NaN fails), (i, j, k) of corner 0 (0 where out of range), (fx, fy, fz)) of the world points X[c]."""
    ok = np.ones(X[0].shape, bool)
    idx, fr = [], []
    with np.errstate(all="ignore"):
        for c in range(3):
            g = (X[c] - origin[c]) * inv
            i = np.floor(g)
            ok &= (i >= 0.0) & (i <= np.float64(int(dims[c]) - 2))
            idx.append(i)
            fr.append(g - i)
    return ok, [np.where(ok, i, 0.0).astype(np.int64) for i in idx], fr


def corners(plane, idx):
    """The 8 corner values c = dx + 2 dy + 4 dz of the cells at idx, in the plane's own type."""
    return [plane[idx[2] + (c >> 2), idx[1] + ((c >> 1) & 1), idx[0] + (c & 1)] for c in range(8)]


def cell(mean, dims, origin, inv, X):
    """(valid, v[8] fp64, f[3], idx): valid iff the cell is in range and none of its 8 means is NaN."""
    ok, idx, f = locate(X, dims, origin, inv)
    m = corners(mean, idx)
    for c in range(8):
        ok = ok & ~np.isnan(m[c])
    return ok, [c.astype(np.float64) for c in m], f, idx


def box_range(dims, origin, inv, voxel, t, dw, z_near, step, N):
    """(n_lo, n_hi) per ray: every sample n < n_lo or n > n_hi is out of range on some axis.  An estimate from the slabs of
    the box, two samples wide of it, is accepted only if the sample just beyond it, computed as the march computes it, is out
    of range on an axis on the side that the monotonicity of every rounded operation extends to all samples beyond; a
    direction component of 0 leaves the coordinate at t for every n."""
    m = dw[0].shape
    z_near, step, vx = np.float64(z_near), np.float64(step), np.float64(voxel)
    coord = lambda n, c: ((t[c] + (z_near + n.astype(np.float64) * step) * dw[c]) - origin[c]) * inv
    with np.errstate(all="ignore"):
        z_in, z_out = np.full(m, -np.inf), np.full(m, np.inf)
        empty = np.zeros(m, bool)
        for c in range(3):
            hi = np.float64(int(dims[c]) - 1)
            za, zb = (origin[c] - t[c]) / dw[c], ((origin[c] + hi * vx) - t[c]) / dw[c]
            flat = dw[c] == 0.0
            g0 = (t[c] - origin[c]) * inv
            empty |= flat & ~((g0 >= 0.0) & (g0 < hi))
            z_in = np.where(flat, z_in, np.maximum(z_in, np.minimum(za, zb)))
            z_out = np.where(flat, z_out, np.minimum(z_out, np.maximum(za, zb)))
        lo = np.floor((z_in - z_near) / step) - 2.0
        hi_ = np.ceil((z_out - z_near) / step) + 2.0
        lo = np.where(lo >= 1.0, np.minimum(lo, np.float64(N)), 0.0)            # (a NaN gives 0: the full march)
        hi_ = np.where(hi_ <= np.float64(N - 2), np.maximum(hi_, -1.0), np.float64(N - 1))
        n_lo, n_hi = lo.astype(np.int64), hi_.astype(np.int64)
        before, after = np.maximum(n_lo - 1, 0), np.minimum(n_hi + 1, N - 1)
        out_lo, out_hi = np.zeros(m, bool), np.zeros(m, bool)
        for c in range(3):
            hi = np.float64(int(dims[c]) - 1)
            gb, ga = coord(before, c), coord(after, c)
            out_lo |= ((dw[c] > 0.0) & (gb < 0.0)) | ((dw[c] < 0.0) & (gb >= hi))
            out_hi |= ((dw[c] > 0.0) & (ga >= hi)) | ((dw[c] < 0.0) & (ga < 0.0))
        n_lo = np.where((n_lo > 0) & ~out_lo, 0, n_lo)
        n_hi = np.where((n_hi < N - 1) & ~out_hi, N - 1, n_hi)
        n_lo = np.where(empty, N, n_lo)
    return n_lo, n_hi


def raycast(vol, dims, origin, voxel, shape, K, pose7, z_near, z_far, step, min_count=1, skip_box=False):
    """dict(depth (H, W) fp32, normal (H, W, 3) fp32, grey (H, W) uint8, stats): the view of the volume from pose7.  stats
    counts, over the rays still marching: hits, inside-to-outside pairs, rays whose first valid sample is inside, crossings
    rejected because the cell of X* is invalid, and pairs with exactly one valid sample."""
    W, H = int(shape[0]), int(shape[1])
    origin = np.asarray(origin, np.float64)
    inv = np.float64(1.0) / np.float64(voxel)
    z_near, step = np.float64(z_near), np.float64(step)
    N = samples(z_near, z_far, step)
    mean = mean_plane(vol, min_count)
    t, dw = rays((W, H), K, pose7)
    m = W * H
    depth, normal, grey = np.zeros(m, np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.uint8)
    active = np.ones(m, bool)
    pok, pv = np.zeros(m, bool), np.zeros(m, np.float64)
    seen_valid, first_inside = np.zeros(m, bool), np.zeros(m, bool)
    stats = dict(hits=0, in_to_out=0, first_inside=0, rejected=0, broken=0, samples=N)
    if skip_box:
        n_lo, n_hi = box_range(dims, origin, inv, voxel, t, dw, z_near, step, N)
        stats["skipped"] = int(np.minimum(n_lo, N).sum() + (N - 1 - np.maximum(np.minimum(n_hi, N - 1), n_lo - 1)).sum())
    with np.errstate(all="ignore"):
        for n in range(N):
            z = z_near + np.float64(n) * step
            X = [t[c] + z * dw[c] for c in range(3)]
            ok, v8, f, _ = cell(mean, dims, origin, inv, X)
            if skip_box:
                assert not (ok & ((n < n_lo) | (n > n_hi))).any()
                ok = ok & (n >= n_lo) & (n <= n_hi)
            v = trilinear(v8, f)
            if n > 0:
                stats["broken"] += int((active & (ok != pok)).sum())
                stats["in_to_out"] += int((active & ok & pok & (pv < 0.0) & (v >= 0.0)).sum())
            first_inside |= active & ok & ~seen_valid & (v < 0.0)
            seen_valid |= active & ok
            cross = active & pok & ok & (pv >= 0.0) & (v < 0.0)
            if cross.any():
                u = pv / (pv - v)
                zs = (z_near + np.float64(n - 1) * step) + u * step
                Xs = [t[c] + zs * dw[c] for c in range(3)]
                oks, w8, fs_, idx = cell(mean, dims, origin, inv, Xs)
                hit = cross & oks
                stats["rejected"] += int((cross & ~oks).sum())
                g = gradient(w8, fs_)
                ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
                has = ln > 0.0
                cnt8 = [c.astype(np.float64) for c in corners(vol[1], idx)]
                gs8 = [c.astype(np.float64) for c in corners(vol[2], idx)]
                gv = trilinear([gs8[c] / cnt8[c] for c in range(8)], fs_)
                depth[hit] = zs[hit].astype(np.float32)
                for c in range(3):
                    normal[hit, c] = np.where(has, g[c] / ln, 0.0)[hit].astype(np.float32)
                grey[hit] = np.floor(gv[hit] + 0.5).astype(np.int64).astype(np.uint8)
                active &= ~hit
            pok, pv = ok, v
    stats["hits"] = int((~active).sum())
    stats["first_inside"] = int(first_inside.sum())
    return dict(depth=depth.reshape(H, W), normal=normal.reshape(H, W, 3), grey=grey.reshape(H, W), stats=stats)


def shade(normal, depth, light=(0.0, 0.0, -1.0)):
    """8-bit Lambert image: floor(255 max(0, n . l / |l|) + 0.5) where depth > 0, else 0."""
    l = np.asarray(light, np.float64)
    l = l / np.sqrt(l @ l)
    lam = np.maximum(np.asarray(normal, np.float64) @ l, 0.0)
    return np.where(np.asarray(depth) > 0, np.floor(255.0 * lam + 0.5), 0.0).astype(np.uint8)
