"""numpy restatement of the census matching cost of the dense sweeps, written from the contract on top of
tests/dense_oracle.py (the warp, the window, the winner) and tests/sgm_oracle.py (the aggregation).  Integers throughout.

Descriptor T(X, Y) of an 8-bit image, uint64: the offsets (dx, dy) run with dy = -3 .. 3 outer and dx = -4 .. 4 inner,
skipping (0, 0); that numbers the bits b = 0 .. 61.  Bit b is 1 iff (X + dx, Y + dy) lies inside the image and
I(X + dx, Y + dy) < I(X, Y).  Bits 62 and 63 are 0.

Cost: the warp, its validity test and (qx, qy) are those of §15.1 (``dense_oracle.warp``); the source's descriptor is read at
the nearest pixel jx = (qx + 16) >> 5, jy = (qy + 16) >> 5, which the validity bound keeps inside the image;
c = min(popcount(T_r(X, Y) xor T_v(jx, jy)), trunc), and an invalid warp costs trunc.  Everything after c is §15.1 and §19.1
unchanged: the sum over the views before the window, the window, V, the winner, its refinement, views = 0, the SGM
recurrence.  Hence C <= 81 * 8 * 62.
"""
import numpy as np

import dense_oracle as do
import sgm_oracle as so

RX, RY = 4, 3
OFFSETS = [(dx, dy) for dy in range(-RY, RY + 1) for dx in range(-RX, RX + 1) if (dx, dy) != (0, 0)]      # bit b: OFFSETS[b]
BITS = len(OFFSETS)                                               # 62
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def census(img):
    """(H, W) uint64 descriptors of an (H, W) uint8 image."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    H, W = a.shape
    p = np.full((H + 2 * RY, W + 2 * RX), 1 << 20, np.int64)      # outside the image: never less than a centre
    p[RY:RY + H, RX:RX + W] = a
    out = np.zeros((H, W), np.uint64)
    for b, (dx, dy) in enumerate(OFFSETS):
        less = p[RY + dy:RY + dy + H, RX + dx:RX + dx + W] < a
        out |= less.astype(np.uint64) << np.uint64(b)
    return out


def census_brute(img):
    """The definition pixel by pixel and bit by bit (small images only)."""
    a = np.asarray(img, np.uint8)
    H, W = a.shape
    out = np.zeros((H, W), np.uint64)
    for Y in range(H):
        for X in range(W):
            t = 0
            for b, (dx, dy) in enumerate(OFFSETS):
                x, y = X + dx, Y + dy
                if 0 <= x < W and 0 <= y < H and int(a[y, x]) < int(a[Y, X]):
                    t |= 1 << b
            out[Y, X] = t
    return out


def popcount(x):
    """The number of set bits of every uint64 of x, int64."""
    x = np.ascontiguousarray(x, np.uint64)
    return _POP8[x.view(np.uint8).reshape(x.shape + (8,))].sum(axis=-1)


def cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc):
    """(C, V) as ``dense_oracle.cost_volume`` gives them, with the census cost.  sources: a list of (image, K, pose7)."""
    ref = np.asarray(ref, np.uint8)
    H, W = ref.shape
    x, y = do.rays(Kr, W, H)
    step = do.plane_step(w_min, w_max, D)
    rel = [do.relative(pose_r, p) for (_, _, p) in sources]
    Tr = census(ref)
    Tv = [census(img) for (img, _, _) in sources]
    C = np.zeros((D, H, W), np.int64)
    V = np.zeros((D, H, W), np.int64)
    for k in range(D):
        z = do.plane_depth(w_min, step, k)
        c = np.zeros((H, W), np.int64)
        for (_, Kv, _), (A, b), T in zip(sources, rel, Tv):
            valid, qx, qy, _ = do.warp(x, y, z, A, b, Kv, W, H)
            jx, jy = (qx + 16) >> 5, (qy + 16) >> 5
            c += np.where(valid, np.minimum(popcount(Tr ^ T[jy, jx]), trunc), trunc)
            V[k] += valid
        C[k] = do.box_sum(c, radius)
    return C, V


def sweep(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc):
    C, V = cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc)
    return do.winner(C, V, w_min, w_max)


def sweep_sgm(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, p1, p2, paths):
    """``dense_oracle.winner`` of the aggregated census volume, with the volumes: C and S as uint32 (D, H, W)."""
    C, V = cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc)
    S = so.aggregate(C, p1, p2, paths)
    assert int(S.max()) < 1 << 24
    out = do.winner(S, V, w_min, w_max)
    out.update(C=C.astype(np.uint32), S=S.astype(np.uint32))
    return out
