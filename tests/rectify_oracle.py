"""numpy restatement of the rectification contract: the pinhole camera of each resolution, the image remap
and the undistortion of pixel coordinates, operation by operation as csrc/ekf_rectify.hpp performs them.

Every coordinate operation is fp64, rounded once, in the written left-to-right order (numpy never fuses a product and a
sum); the lens parameters are the config's float32 values widened, as the library holds them.  The interpolation is integer.
"""
import numpy as np

LENS_KEYS = ("fx", "fy", "u0", "v0", "k1", "k2", "k3", "p1", "p2")


def lens(cfg):
    """The nine lens parameters of a config (a dict, or an object with attributes) as the library sees them: float32 -> fp64."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, d=0.0: getattr(cfg, k, d))
    return {k: np.float64(np.float32(get(k, 0.0))) for k in LENS_KEYS}


def camera(L, s=1):
    """K = (fx, fy, cx, cy) of the rectified image: s = 1 the matcher frame, s = scale the raw frame."""
    s = np.float64(s)
    return np.array([L["fx"] * s, L["fy"] * s, (L["u0"] + 0.5) * s - 0.5, (L["v0"] + 0.5) * s - 0.5], np.float64)


def to_matcher(X, s):
    """Pixel X of the resolution with factor s -> matcher pixel."""
    return (np.asarray(X, np.float64) + 0.5) / np.float64(s) - 0.5


def from_matcher(u, s):
    return (np.asarray(u, np.float64) + 0.5) * np.float64(s) - 0.5


def distort_matcher(L, u, v):
    """Steps 2-5 of the image contract: where the ray of the rectified matcher pixel (u, v) lands in the distorted matcher
    frame (the forward model of project_distort)."""
    k1, k2, k3, p1, p2 = L["k1"], L["k2"], L["k3"], L["p1"], L["p2"]
    x1 = (u - L["u0"]) / L["fx"]
    y1 = (v - L["v0"]) / L["fy"]
    r2 = x1 * x1 + y1 * y1
    l = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    x2 = x1 * l + 2.0 * p1 * x1 * y1 + p2 * (r2 + 2.0 * x1 * x1)
    y2 = y1 * l + 2.0 * p2 * x1 * y1 + p1 * (r2 + 2.0 * y1 * y1)
    return L["fx"] * x2 + L["u0"], L["fy"] * y2 + L["v0"]


def source_positions(L, W, H, s=1):
    """(sx, sy), each (H, W): the position in the held image that output pixel (X, Y) is read from."""
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all="ignore"):
        ud, vd = distort_matcher(L, to_matcher(X, s), to_matcher(Y, s))
        return from_matcher(ud, s), from_matcher(vd, s)


def tap_classes(L, W, H, s=1):
    """Per output pixel: 0 = source position outside (-1, W) x (-1, H) (the output is 0), 1 = inside with at least one of
    the four taps outside the image, 2 = all four taps inside."""
    sx, sy = source_positions(L, W, H, s)
    with np.errstate(invalid="ignore"):
        inside = (sx > -1.0) & (sx < W) & (sy > -1.0) & (sy < H)
    qx = np.floor(np.where(inside, sx, 0.0) * 32.0 + 0.5).astype(np.int64)
    qy = np.floor(np.where(inside, sy, 0.0) * 32.0 + 0.5).astype(np.int64)
    ix, iy = qx >> 5, qy >> 5
    full = (ix >= 0) & (ix + 1 < W) & (iy >= 0) & (iy + 1 < H)
    return np.where(inside, np.where(full, 2, 1), 0)


def rectify_image(img, L, s=1):
    """The rectified image of `img` ((H, W) or (H, W, C) uint8), byte for byte what k_frame_rectify writes."""
    a = np.asarray(img, np.uint8)
    flat = a.ndim == 2
    if flat:
        a = a[:, :, None]
    H, W, C = a.shape
    sx, sy = source_positions(L, W, H, s)
    with np.errstate(invalid="ignore"):
        inside = (sx > -1.0) & (sx < W) & (sy > -1.0) & (sy < H)
    qx = np.floor(np.where(inside, sx, 0.0) * 32.0 + 0.5).astype(np.int64)
    qy = np.floor(np.where(inside, sy, 0.0) * 32.0 + 0.5).astype(np.int64)
    ix, ax, iy, ay = qx >> 5, qx & 31, qy >> 5, qy & 31
    acc = np.zeros((H, W, C), np.int64)
    for dx, dy, wgt in ((0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)):
        tx, ty = ix + dx, iy + dy
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        p = a[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64)
        acc += np.where(ok, wgt, 0)[:, :, None] * p
    out = np.where(inside[:, :, None], (acc + 512) >> 10, 0).astype(np.uint8)
    return out[:, :, 0] if flat else out


def undistort_pixels(uv, L, s=1):
    """(n, 2) pixels of the resolution with factor s -> the pixels at which the pinhole K of that resolution sees the same
    rays: the 50 fixed-point iterations of undistort_deproject.  A non-finite input row gives NaN, NaN."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    k1, k2, k3, p1, p2 = L["k1"], L["k2"], L["k3"], L["p1"], L["p2"]
    finite = np.isfinite(uv).all(axis=1)
    src = np.where(finite[:, None], uv, 0.0)
    with np.errstate(all="ignore"):
        u, v = to_matcher(src[:, 0], s), to_matcher(src[:, 1], s)
        x2 = (u - L["u0"]) / L["fx"]
        y2 = (v - L["v0"]) / L["fy"]
        x1, y1 = x2.copy(), y2.copy()
        for _ in range(50):
            r2 = x1 * x1 + y1 * y1
            l = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            dx = 2.0 * p1 * x1 * y1 + p2 * (r2 + 2.0 * x1 * x1)
            dy = 2.0 * p2 * x1 * y1 + p1 * (r2 + 2.0 * y1 * y1)
            x1 = (x2 - dx) / l
            y1 = (y2 - dy) / l
        um = L["fx"] * x1 + L["u0"]
        vm = L["fy"] * y1 + L["v0"]
        out = np.stack([from_matcher(um, s), from_matcher(vm, s)], axis=1)
    out[~finite] = np.nan
    return out


def distort_pixels(uv, L, s=1):
    """The inverse direction, for building test data: pinhole pixels of the resolution with factor s -> where the lens puts
    them in the held image of that resolution."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    ud, vd = distort_matcher(L, to_matcher(uv[:, 0], s), to_matcher(uv[:, 1], s))
    return np.stack([from_matcher(ud, s), from_matcher(vd, s)], axis=1)


def round_rows(uv):
    """floor(x + 0.5): the integer rows the recorder writes for the reference's `int u, v` reader."""
    return np.floor(np.asarray(uv, np.float64) + 0.5).astype(np.int64)
