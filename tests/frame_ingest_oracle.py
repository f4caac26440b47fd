"""Numpy restatement of DESIGN.md §13: the raw camera frame -> the matcher's frame, i.e. captureNewFrame's
cv::resize(INTER_LINEAR) by 1 / scale and cvtColor(BGR2GRAY) (vslamRansac.cpp:235-245) as pinned integer arithmetic.
Written from §13 alone, one pixel formula at a time, without looking at csrc/ekf_image.hpp.  Test-side only."""
import numpy as np

COEF_ONE = 2048                                   # INTER_RESIZE_COEF_SCALE
B2Y, G2Y, R2Y, GRAY_SHIFT = 1868, 9617, 4899, 14


def out_size(W, H, s):
    return W // s, H // s


def mode(W, H, s):
    Wo, Ho = out_size(W, H, s)
    if Wo == W and Ho == H:
        return "copy"
    if W == 2 * Wo and H == 2 * Ho:
        return "area2"
    return "linear"


def _axis_table(n_src, n_dst, zero_frac_at_border):
    """Per destination index: (s0, s1, w0, w1, clamped).  fp64 for the product, fp32 from then on, round half to even."""
    scale = np.float64(n_src) / np.float64(n_dst)
    s0, s1, w0, w1, clamped = [], [], [], [], []
    for d in range(n_dst):
        f = np.float32((np.float64(d) + np.float64(0.5)) * scale - np.float64(0.5))
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        hit = False
        if zero_frac_at_border:
            if s < 0:
                s, f, hit = 0, np.float32(0), True
            if s >= n_src - 1:
                s, f, hit = n_src - 1, np.float32(0), True
        else:
            hit = s < 0 or s + 1 > n_src - 1
        a0 = int(np.rint(np.float32(np.float32(1) - f) * np.float32(COEF_ONE)))
        a1 = int(np.rint(np.float32(f) * np.float32(COEF_ONE)))
        s0.append(min(max(s, 0), n_src - 1))
        s1.append(min(max(s + 1, 0), n_src - 1))
        w0.append(a0)
        w1.append(a1)
        clamped.append(hit)
    return (np.asarray(s0), np.asarray(s1), np.asarray(w0, np.int64), np.asarray(w1, np.int64), np.asarray(clamped))


def tables(W, H, s):
    """{"x": (sx, sx1, a0, a1, clamped), "y": (sy0, sy1, b0, b1, clamped)} of the linear path."""
    Wo, Ho = out_size(W, H, s)
    return {"x": _axis_table(W, Wo, True), "y": _axis_table(H, Ho, False)}


def resize_channel(S, s):
    """One 8-bit channel (H, W) -> (H // s, W // s)."""
    S = np.asarray(S, np.uint8)
    H, W = S.shape
    Wo, Ho = out_size(W, H, s)
    m = mode(W, H, s)
    if m == "copy":
        return S.copy()
    I = S.astype(np.int64)
    if m == "area2":
        return ((I[0::2, 0::2] + I[0::2, 1::2] + I[1::2, 0::2] + I[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    t = tables(W, H, s)
    sx, sx1, a0, a1, _ = t["x"]
    sy0, sy1, b0, b1, _ = t["y"]
    # horizontal pass of every source row that is used (the second tap counts for nothing where a1 == 0)
    tap1 = np.where(a1[None, :] != 0, I[:, sx1], 0)
    rows = I[:, sx] * a0[None, :] + tap1 * a1[None, :]
    r0, r1 = rows[sy0, :], rows[sy1, :]
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def gray(bgr):
    c = np.asarray(bgr, np.uint8).astype(np.int64)
    return ((c[..., 0] * B2Y + c[..., 1] * G2Y + c[..., 2] * R2Y + (1 << (GRAY_SHIFT - 1))) >> GRAY_SHIFT).astype(np.uint8)


def ingest(raw, s):
    """raw: uint8 (H, W) or (H, W, 3) in B, G, R order -> the matcher frame (H // s, W // s)."""
    raw = np.asarray(raw, np.uint8)
    if raw.ndim == 2:
        return resize_channel(raw, s)
    assert raw.ndim == 3 and raw.shape[2] == 3
    return gray(np.stack([resize_channel(raw[:, :, c], s) for c in range(3)], axis=2))


def replicate(gray_frame, s, channels=1):
    """Pixel replication up to raw size: every path of §13 gives the original back (a constant block's mean, its centre
    taps and its point sample are the constant), and B = G = R = v has grey value v (the weights sum to 2^14)."""
    up = np.repeat(np.repeat(np.asarray(gray_frame, np.uint8), s, axis=0), s, axis=1)
    return up if channels == 1 else np.repeat(up[:, :, None], 3, axis=2)
