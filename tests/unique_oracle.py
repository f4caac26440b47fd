"""numpy restatement of the runner-up cost and the uniqueness test of the dense sweeps, written from the
contract on top of tests/dense_oracle.py (the volume, the winner, the geometric filter), tests/census_oracle.py,
tests/best_oracle.py and tests/sgm_oracle.py (the other three cost curves).  Integers throughout.

For a pixel with cost curve C_0 .. C_{D-1} and winner k* (the smallest k of least cost, strict <):

  C2 = min { C_k : |k - k*| > 1 },   ABSENT = 0xFFFFFFFF where no such plane exists (D <= 3 only),

on the curve the sweep takes its winner from: the summed window cost, the census cost, the best-K cost or the aggregate S.
C2 is defined for every pixel, whatever `views` says.  With u in 0 .. 100 (per cent) and C1 the pixel's cost, a pixel passes
iff C2 is ABSENT or (C2 - C1) 100 >= u C2 in 64-bit integers: u = 0 passes everything, a flat curve (C2 = C1) fails every
u > 0.  The last rule decides the one case the inequality leaves open: C2 = C1 = 0, the curve of an untextured patch seen
alike by every view, reads 0 >= 0 and fails all the same.  The filter keeps a pixel iff ``dense_oracle.geometric_filter``
keeps it and the reference view's own pixel passes.
"""
import numpy as np

import best_oracle as bo
import census_oracle as co
import dense_oracle as do
import sgm_oracle as so

ABSENT = 0xFFFFFFFF


def runner_up(C):
    """(D, H, W) integer volume -> (H, W) uint32: the definition, by masking the winner and its two neighbours out."""
    C = np.asarray(C, np.int64)
    D = C.shape[0]
    ks = np.argmin(C, axis=0)                                     # the first minimum: the smallest k
    far = np.abs(np.arange(D)[:, None, None] - ks[None]) > 1
    big = np.int64(ABSENT)
    assert int(C.max()) < big
    return np.where(far, C, big).min(axis=0).astype(np.uint32)


def runner_up_top4(C):
    """The same map in one pass over the planes, before k* is known, as the pixel-wise kernels find it: the four smallest
    pairs (C_k, k) in lexicographic order; the smallest is the winner, the first of the other three that lies more than
    one plane from it is the runner-up.  Returns (runner-up uint32, the winner's plane, the winner's cost)."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    none = np.int64(1) << 62
    top = np.full((4, H, W), none, np.int64)
    for k in range(D):
        x = C[k] * 1024 + k                                        # k < 1024: the order of the keys is that of the pairs
        for i in range(4):
            lo, x = np.minimum(top[i], x), np.maximum(top[i], x)
            top[i] = lo
    ks = top[0] % 1024
    c2 = np.full((H, W), ABSENT, np.int64)
    for i in (3, 2, 1):                                            # the smallest such key is assigned last
        ok = (top[i] != none) & (np.abs(top[i] % 1024 - ks) > 1)
        c2 = np.where(ok, top[i] // 1024, c2)
    return c2.astype(np.uint32), ks, top[0] // 1024


def unique_pass(cost, runner, u):
    """(H, W) bool: the uniqueness test at u per cent."""
    assert 0 <= int(u) <= 100
    c1, c2 = np.asarray(cost).astype(np.int64), np.asarray(runner).astype(np.int64)
    return (c2 == ABSENT) | (((c2 - c1) * 100 >= int(u) * c2) & ((c2 != c1) | (int(u) == 0)))


def unique_filter(depth, plane, cost, runner, Kr, pose_r, sources, rel_tol, min_agree, u):
    """(depth, plane) filtered: ``dense_oracle.geometric_filter`` AND the uniqueness test on the reference's own pixel."""
    fd, fp = do.geometric_filter(depth, plane, Kr, pose_r, sources, rel_tol, min_agree)
    ok = unique_pass(cost, runner, u)
    return np.where(ok, fd, np.float32(0)).astype(np.float32), np.where(ok, fp, -1).astype(np.int32)


def volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, census=False, n_best=0, paths=0, p1=0, p2=0):
    """(curve, V): the cost curve a sweep takes its winner from, and the valid-view counts.  n_best = 0: all sources."""
    if n_best:
        C, V = bo.cost_volume(ref, Kr, pose_r, sources, n_best, w_min, w_max, D, radius, trunc, census)
    elif census:
        C, V = co.cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc)
    else:
        C, V = do.cost_volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc)
    return (so.aggregate(C, p1, p2, paths) if paths else C), V


def sweep(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, census=False, n_best=0, paths=0, p1=0, p2=0):
    """``dense_oracle.winner`` of that curve with the fifth map, ``runner``."""
    C, V = volume(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, census, n_best, paths, p1, p2)
    out = do.winner(C, V, w_min, w_max)
    out["runner"] = runner_up(C)
    return out


def wrong(out, truth_w, D, w_min, w_max):
    """(H, W) bool: the refined inverse depth is more than one plane step from the truth (no depth: not wrong, not right)."""
    with np.errstate(invalid="ignore"):
        return np.abs(out["inv_depth"] - truth_w) > do.plane_step(w_min, w_max, D)
