"""numpy restatement of the semi-global aggregation contract, written from the contract on top of
tests/dense_oracle.py: the raw volume is ``dense_oracle.cost_volume``, the winner ``dense_oracle.winner`` on the sum of the
path costs.  Integers throughout (int64 here; the device's values fit 32 bits).

A direction is walked one image column (or row, for the vertical ones) at a time, every line of it at once, so a case of
the GPU test takes a fraction of a second; ``aggregate_brute`` is the recurrence spelled out pixel by pixel.
"""
import numpy as np

import dense_oracle as do

DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]      # (dx, dy); paths = 4: the first four
MAX_PENALTY, MAX_ELEMS = 1 << 20, 1 << 28
_BIG = np.int64(1) << 40


def _step(Cc, P, p1, p2):
    """L of one pixel per column of Cc (D, n) from the L of its predecessors P (D, n)."""
    m = P.min(axis=0)
    below = np.full_like(P, _BIG)
    above = np.full_like(P, _BIG)
    below[1:] = P[:-1] + p1
    above[:-1] = P[1:] + p1
    return Cc + np.minimum(np.minimum(P, m[None] + p2), np.minimum(below, above)) - m[None]


def path_cost(C, p1, p2, dx, dy):
    """L_r of the direction r = (dx, dy) over the whole volume C (D, H, W)."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    if dx == 0:                                                   # a vertical direction is the horizontal one of the transpose
        return path_cost(C.transpose(0, 2, 1), p1, p2, dy, 0).transpose(0, 2, 1)
    L = np.zeros_like(C)
    xs = range(W) if dx > 0 else range(W - 1, -1, -1)
    ys = np.arange(H)
    inside = (ys - dy >= 0) & (ys - dy < H)                       # rows whose predecessor row exists
    for i, x in enumerate(xs):
        if i == 0:
            L[:, :, x] = C[:, :, x]
            continue
        P = L[:, np.clip(ys - dy, 0, H - 1), x - dx]
        L[:, :, x] = np.where(inside[None], _step(C[:, :, x], P, p1, p2), C[:, :, x])
    return L


def aggregate(C, p1, p2, paths):
    """S = the sum of L_r over the first `paths` directions (4 or 8)."""
    assert paths in (4, 8) and 1 <= p1 <= p2 <= MAX_PENALTY
    S = np.zeros(np.asarray(C).shape, np.int64)
    for dx, dy in DIRECTIONS[:paths]:
        S += path_cost(C, p1, p2, dx, dy)
    return S


def aggregate_brute(C, p1, p2, paths):
    """The recurrence of §19.1 pixel by pixel and plane by plane (small volumes only)."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        L = np.zeros_like(C)
        for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):
            for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
                px, py = x - dx, y - dy
                if not (0 <= px < W and 0 <= py < H):
                    L[:, y, x] = C[:, y, x]
                    continue
                prev = [int(v) for v in L[:, py, px]]
                m = min(prev)
                for d in range(D):
                    cand = [prev[d], m + p2]
                    if d > 0:
                        cand.append(prev[d - 1] + p1)
                    if d < D - 1:
                        cand.append(prev[d + 1] + p1)
                    L[d, y, x] = int(C[d, y, x]) + min(cand) - m
        S += L
    return S


def default_penalties(radius, n_src):
    """p1 = 2 n, p2 = 16 n with n = (2 radius + 1)^2 n_src: what ``DenseStereo.sweep_sgm`` takes for ``None``."""
    n = (2 * radius + 1) ** 2 * n_src
    return 2 * n, 16 * n


def sweep_sgm(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, p1, p2, paths):
    """``dense_oracle.winner`` of the aggregated volume, with the volumes: C and S as uint32 (D, H, W)."""
    C, V = do.cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc)
    S = aggregate(C, p1, p2, paths)
    assert int(S.max()) < 1 << 24
    out = do.winner(S, V, w_min, w_max)
    out.update(C=C.astype(np.uint32), S=S.astype(np.uint32))
    return out
