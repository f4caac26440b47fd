"""Numpy restatement of the end of VSlamFilter::update() (vslamRansac.cpp:1294-1317) and of findNewFeatures
(:783-837) with the detector arithmetic pinned in csrc/ekf_features.hpp / DESIGN.md: the mask of the existing
patches, the exact cornerMinEigenVal response and goodFeaturesToTrack's selection.  Also the per-feature track
state (n_tot, center, isInInnovation, the sticky removeFlag) and the end-of-update rule.  Test-side only."""
import numpy as np


# --------------------------------------------------------------------------------------------
# detector
# --------------------------------------------------------------------------------------------
def seed_mask(width, height, window, centers):
    """vR.cpp:788-818: 255 on Rect(w, w, W-2w, H-2w), then 0 on the (2w+1)^2 square of every centre strictly inside
    the margin (float compares, origin (int)(c - w))."""
    w = int(window)
    m = np.zeros((height, width), np.uint8)
    m[w:height - w, w:width - w] = 255
    for cx, cy in np.asarray(centers, np.float32).reshape(-1, 2):
        if cx > np.float32(w) and cy > np.float32(w) and cx < np.float32(width - w) and cy < np.float32(height - w):
            x0, y0 = int(np.float32(cx) - np.float32(w)), int(np.float32(cy) - np.float32(w))
            m[max(y0, 0):y0 + 2 * w + 1, max(x0, 0):x0 + 2 * w + 1] = 0
    return m


def _box3(a):
    p = np.pad(a, 1, mode="reflect")                   # numpy "reflect" = BORDER_REFLECT_101
    H, W = a.shape
    out = np.zeros_like(a)
    for dy in range(3):
        for dx in range(3):
            out += p[dy:dy + H, dx:dx + W]
    return out


def sobel_int(frame):
    """Integer 3x3 Sobel derivatives (Dx, Dy) with BORDER_REFLECT_101."""
    f = np.pad(np.asarray(frame, np.int64), 1, mode="reflect")
    H, W = frame.shape
    s = lambda dy, dx: f[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return dx, dy


def min_eig_from_sums(a, b, c):
    """lambda = 0.5 ((a + c) - sqrt((a - c)^2 + 4 b^2)): integer operands, one correctly rounded fp64 sqrt."""
    a, b, c = (np.asarray(x, np.int64) for x in (a, b, c))
    disc = (a - c) * (a - c) + 4 * b * b
    return 0.5 * ((a + c).astype(np.float64) - np.sqrt(disc.astype(np.float64)))


def corner_response(frame):
    """cornerMinEigenVal(blockSize 3, ksize 3) times (4 * 3 * 255)^2, exactly (ekf_features.hpp)."""
    dx, dy = sobel_int(frame)
    return min_eig_from_sums(_box3(dx * dx), _box3(dx * dy), _box3(dy * dy))


def candidates(lam, mask, quality):
    """goodFeaturesToTrack's local maxima: (values, raster indices), unsorted."""
    H, W = lam.shape
    mx = float(lam[mask != 0].max()) if np.any(mask != 0) else 0.0
    thr = mx * float(quality)
    t = np.where(lam > thr, lam, 0.0)
    p = np.pad(t, 1, mode="constant", constant_values=-np.inf)     # border pixels do not contribute
    dil = np.full_like(t, -np.inf)
    for dy in range(3):
        for dx in range(3):
            dil = np.maximum(dil, p[dy:dy + H, dx:dx + W])
    ok = (t != 0) & (t == dil) & (mask != 0)
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    idx = np.flatnonzero(ok)
    return t.ravel()[idx], idx


def select(vals, idx, width, num, min_distance):
    """lambda descending, ties by raster index descending; greedy min-distance acceptance, at most num corners."""
    order = np.lexsort((-idx, -vals))
    xs, ys = idx % width, idx // width
    md2 = float(min_distance) * float(min_distance)
    acc = []
    ax, ay = [], []
    for k in order:
        if len(acc) >= num:
            break
        x, y = int(xs[k]), int(ys[k])
        if acc:
            d2 = (np.asarray(ax) - x) ** 2 + (np.asarray(ay) - y) ** 2
            if np.any(d2 < md2):
                continue
        acc.append(int(idx[k]))
        ax.append(x)
        ay.append(y)
    return np.asarray(acc, np.int64)


def find_new_features(frame, centers, window, num, quality=0.01, min_distance=12.0, lam=None):
    """(corners (K, 2) float32 in acceptance order, lambda image)."""
    H, W = frame.shape
    if lam is None:
        lam = corner_response(frame)
    mask = seed_mask(W, H, window, centers)
    vals, idx = candidates(lam, mask, quality)
    acc = select(vals, idx, W, num, min_distance)
    uv = np.stack([acc % W, acc // W], axis=1).astype(np.float32) if acc.size else np.zeros((0, 2), np.float32)
    return uv, lam


# --------------------------------------------------------------------------------------------
# track state and the end of update()
# --------------------------------------------------------------------------------------------
def quality_flags(n_tot, n_find, matching_ratio=0.2):
    """Patch::update_quality_index (Patch.cpp:147-149) in fp32: (float)(n_tot - n_find) / (float)n_find > ratio."""
    nt, nf = np.asarray(n_tot, np.int64), np.asarray(n_find, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (nt - nf).astype(np.float32) / nf.astype(np.float32)
    return q > np.float32(matching_ratio)


def end_update_plan(n_tot, n_find, remove_flag, in_innovation, min_features, max_features, matching_ratio=0.2):
    """The integer part of vR.cpp:1294-1315: (removed indices, descending; n_visible; evict feature 0?; seed count)."""
    flag = quality_flags(n_tot, n_find, matching_ratio) | np.asarray(remove_flag, bool)
    removed = np.flatnonzero(flag)[::-1]
    keep = ~flag
    n_vis = int(np.count_nonzero(np.asarray(in_innovation, bool)[keep]))
    n_left = int(np.count_nonzero(keep))
    evict = n_vis < min_features and n_left > max_features
    seed = (min_features - n_vis) if n_vis < min_features else 0
    return removed, n_vis, evict, seed


class Track:
    """n_tot, center, isInInnovation and the sticky removeFlag of every feature, kept beside an oracle filter."""

    def __init__(self):
        self.n_tot, self.center, self.inn, self.rem = [], [], [], []

    def add(self, u, v):                                   # Patch.cpp:85-93
        self.n_tot.append(1)
        self.center.append((np.float32(u), np.float32(v)))
        self.inn.append(False)
        self.rem.append(False)

    def keep(self, keep_idx):                              # removal (any number), conversion keeps everything
        for name in ("n_tot", "center", "inn", "rem"):
            lst = getattr(self, name)
            setattr(self, name, [lst[i] for i in keep_idx])

    def predicted(self, visible, rho_nonpositive):         # vR.cpp:519-520, 532, 561
        self.inn = [bool(v) for v in visible]
        self.rem = [r or bool(p) for r, p in zip(self.rem, rho_nonpositive)]

    def matched(self, z, found):                           # Patch.cpp:218, 253, 279-281
        for i in range(len(self.n_tot)):
            if not self.inn[i]:
                continue
            self.n_tot[i] += 1
            if found[i]:
                self.center[i] = (np.float32(z[i][0]), np.float32(z[i][1]))
            else:
                self.center[i] = (np.float32(-1), np.float32(-1))
                self.inn[i] = False

    def arrays(self):
        return (np.asarray(self.n_tot, np.int32), np.asarray(self.inn, bool),
                np.asarray(self.center, np.float32).reshape(-1, 2), np.asarray(self.rem, bool))
