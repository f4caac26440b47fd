"""numpy restatement of the best-K source selection of the dense sweeps, written from the contract on top
of tests/dense_oracle.py (the warp, the sample, the window, the winner), tests/census_oracle.py (the descriptors and their
popcount) and tests/sgm_oracle.py (the aggregation).  Integers throughout.

Unchanged from §15.1 / §20: the warp, its validity test, (qx, qy), the per-pixel cost c_v of source v (the truncated absolute
difference of the 5-bit bilinear sample, or the truncated Hamming distance of the descriptors at the nearest pixel; an
invalid warp costs trunc), the planes and the limits.

  C_k^v(p) = the sum of c_v over the (2 radius + 1)^2 window around p; positions outside the image contribute nothing.
             At most 81 * 255 = 20 655.
  C_k(p)   = the sum of the n_best smallest of C_k^0(p) .. C_k^{n_src - 1}(p), 1 <= n_best <= n_src <= 8.  Only the sum is
             defined, so ties need no rule.  For n_best = n_src it is §15.1's (or §20's) value, element for element.
  V_k(p)   = the number of sources whose warp of p itself is valid: of ALL sources, selected or not.

Everything after C is the existing path on the new numbers: ``dense_oracle.winner`` (the first plane of least cost, the
parabola, views = 0 giving plane -1 and depth 0) and, with paths of 4 or 8, ``sgm_oracle.aggregate`` and the winner of S.
"""
import numpy as np

import census_oracle as co
import dense_oracle as do
import sgm_oracle as so

MAX_WINDOW_SUM = 81 * 255


def view_volumes(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, census=False):
    """(Cv, V): Cv[v, k] the windowed cost of source v alone on plane k (int64, (n_src, D, H, W)), V[k] the number of
    sources whose warp of the pixel itself is valid.  sources: a list of (image, K, pose7)."""
    ref = np.asarray(ref, np.uint8)
    H, W = ref.shape
    x, y = do.rays(Kr, W, H)
    step = do.plane_step(w_min, w_max, D)
    rel = [do.relative(pose_r, p) for (_, _, p) in sources]
    I = ref.astype(np.int64)
    if census:
        Tr = co.census(ref)
        Tv = [co.census(img) for (img, _, _) in sources]
    Cv = np.zeros((len(sources), D, H, W), np.int64)
    V = np.zeros((D, H, W), np.int64)
    for k in range(D):
        z = do.plane_depth(w_min, step, k)
        for v, ((img, Kv, _), (A, b)) in enumerate(zip(sources, rel)):
            valid, qx, qy, _ = do.warp(x, y, z, A, b, Kv, W, H)
            if census:
                match = co.popcount(Tr ^ Tv[v][(qy + 16) >> 5, (qx + 16) >> 5])
            else:
                match = np.abs(I - do.sample(img, qx, qy))
            Cv[v, k] = do.box_sum(np.where(valid, np.minimum(match, trunc), trunc), radius)
            V[k] += valid
    return Cv, V


def select(Cv, n_best):
    """The sum of the n_best smallest over the first axis."""
    assert 1 <= n_best <= Cv.shape[0] <= do.MAX_SOURCES
    return np.sort(Cv, axis=0)[:n_best].sum(axis=0)


def cost_volume(ref, Kr, pose_r, sources, n_best, w_min, w_max, D, radius, trunc, census=False):
    """(C, V) as ``dense_oracle.cost_volume`` gives them, of the n_best cheapest sources per pixel and plane."""
    Cv, V = view_volumes(ref, Kr, pose_r, sources, w_min, w_max, D, radius, trunc, census)
    assert int(Cv.max()) <= MAX_WINDOW_SUM
    return select(Cv, n_best), V


def sweep(ref, Kr, pose_r, sources, n_best, w_min, w_max, D, radius, trunc, census=False, paths=0, p1=0, p2=0):
    """``dense_oracle.winner`` of the selected volume (paths = 0) or of its aggregate (paths = 4 or 8; then also the
    volumes C and S as uint32 (D, H, W))."""
    C, V = cost_volume(ref, Kr, pose_r, sources, n_best, w_min, w_max, D, radius, trunc, census)
    if paths == 0:
        assert p1 == 0 and p2 == 0
        return do.winner(C, V, w_min, w_max)
    S = so.aggregate(C, p1, p2, paths)
    assert int(S.max()) < 1 << 24
    out = do.winner(S, V, w_min, w_max)
    out.update(C=C.astype(np.uint32), S=S.astype(np.uint32))
    return out


def default_penalties(radius, n_best):
    """p1 = 2 n, p2 = 16 n with n = (2 radius + 1)^2 n_best: what ``DenseStereo.sweep_sgm(best=n_best)`` takes for ``None``."""
    return so.default_penalties(radius, n_best)


def share_right(out, truth_w, mask=None, D=None, w_min=None, w_max=None):
    """The share of the pixels of `mask` (None: all) whose refined inverse depth is within one plane step of the truth."""
    step = do.plane_step(w_min, w_max, D)
    with np.errstate(invalid="ignore"):
        ok = np.abs(out["inv_depth"] - truth_w) <= step                     # NaN (no depth) is not right
    return float(ok.mean() if mask is None else ok[mask].mean())
