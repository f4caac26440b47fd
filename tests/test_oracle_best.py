"""tests/best_oracle.py against the contract of DESIGN.md §21.1: the identity with the existing oracles for n_best = n_src, a
brute-force selection pixel by pixel, monotony in n_best, the 16-bit bound reached, the invalid warps of the GPU shapes, and
the accuracy conditions on inputs where the sum over all sources fails.  CPU only."""
import numpy as np
import pytest

import best_oracle as bo
import best_scene as bs
import census_oracle as co
import dense_oracle as do
import dense_scene as ds

ARGS = (ds.W_MIN, ds.W_MAX)
SURFACES = {"step": ("step", ds.plane_z(ds.NEAR_PLANE), ds.plane_z(ds.FAR_PLANE)), "plane": ("plane", ds.plane_z(ds.TRUE_PLANE))}


@pytest.fixture(scope="module")
def scenes():
    return {"step": ds.step_scene(), "plane": ds.plane_scene()}


def _parts(views, src):
    return views[0][0], views[0][1], views[0][2], [views[s] for s in src]


@pytest.mark.parametrize("case", [ds.CASES[1], ds.CASES[2]], ids=lambda c: c[0])
def test_all_sources_is_the_absolute_difference_volume(case):
    name, w, h, D, radius, trunc, src = case
    views = ds.case_views(w, h)
    C, V = bo.cost_volume(*_parts(views, src), len(src), *ARGS, D, radius, trunc)
    C0, V0 = do.cost_volume(*_parts(views, src), *ARGS, D, radius, trunc)
    assert np.array_equal(C, C0) and np.array_equal(V, V0) and C.dtype == C0.dtype
    out, ref = bo.sweep(*_parts(views, src), len(src), *ARGS, D, radius, trunc), do.winner(C0, V0, *ARGS)
    assert all(np.array_equal(out[k], ref[k], equal_nan=out[k].dtype.kind == "f") for k in ref)


@pytest.mark.parametrize("case", [ds.CASES[1], ds.CASES[3]], ids=lambda c: c[0])
def test_all_sources_is_the_census_volume(case):
    name, w, h, D, radius, trunc, src = case
    views = ds.case_views(w, h)
    trunc = min(trunc, 62)
    C, V = bo.cost_volume(*_parts(views, src), len(src), *ARGS, D, radius, trunc, census=True)
    C0, V0 = co.cost_volume(*_parts(views, src), *ARGS, D, radius, trunc)
    assert np.array_equal(C, C0) and np.array_equal(V, V0)


@pytest.mark.parametrize("census", [False, True], ids=["ad", "census"])
def test_selection_pixel_by_pixel_on_the_small_shape(census):
    views = bs.case_views(ds.SMALL_W, ds.SMALL_H)
    src, D, radius, trunc = (1, 2, 3, 5, 6), 5, 2, 62
    Cv, V = bo.view_volumes(*_parts(views, src), *ARGS, D, radius, trunc, census)
    # the per-view window sums by the definition: every window position, skipped where it lies outside the image
    x, y = do.rays(views[0][1], ds.SMALL_W, ds.SMALL_H)
    step = do.plane_step(*ARGS, D)
    T0 = co.census(views[0][0])
    for v, s in enumerate(src):
        A, b = do.relative(views[0][2], views[s][2])
        for k in (0, D - 1):
            valid, qx, qy, _ = do.warp(x, y, do.plane_depth(ds.W_MIN, step, k), A, b, views[s][1], ds.SMALL_W, ds.SMALL_H)
            if census:
                c = np.minimum(co.popcount(T0 ^ co.census(views[s][0])[(qy + 16) >> 5, (qx + 16) >> 5]), trunc)
            else:
                c = np.minimum(np.abs(views[0][0].astype(np.int64) - do.sample(views[s][0], qx, qy)), trunc)
            c = np.where(valid, c, trunc)
            for Y in range(ds.SMALL_H):
                for X in range(ds.SMALL_W):
                    want = sum(int(c[yy, xx]) for yy in range(Y - radius, Y + radius + 1) for xx in range(X - radius, X + radius + 1)
                               if 0 <= yy < ds.SMALL_H and 0 <= xx < ds.SMALL_W)
                    assert Cv[v, k, Y, X] == want, (s, k, Y, X)
    for n_best in (1, 3, 5):
        C = bo.select(Cv, n_best)
        for k in range(D):
            for Y in range(ds.SMALL_H):
                for X in range(ds.SMALL_W):
                    assert C[k, Y, X] == sum(sorted(int(c) for c in Cv[:, k, Y, X])[:n_best])
    assert (V <= len(src)).all() and (V == len(src)).any() and (V < len(src)).any()


def test_the_cost_does_not_decrease_with_n_best_and_views_ignore_the_selection():
    views = bs.case_views(ds.W, ds.H)
    Cv, V = bo.view_volumes(*_parts(views, bs.ALL8), *ARGS, ds.PLANES, 1, 255)
    prev = np.zeros_like(Cv[0])
    for n_best in range(1, 9):
        C = bo.select(Cv, n_best)
        assert (C >= prev).all()
        prev = C
    assert np.array_equal(prev, Cv.sum(axis=0))
    assert np.array_equal(bo.cost_volume(*_parts(views, bs.ALL8), 3, *ARGS, ds.PLANES, 1, 255)[1], V)
    assert (bo.select(Cv, 1) < bo.select(Cv, 2)).any()


def test_the_largest_window_sum_is_reached():
    views = ds.case_views(ds.W, ds.H)
    Cv, _ = bo.view_volumes(*_parts(views, (1, 2, 3)), *ARGS, ds.PLANES, 4, 255)
    print("largest per-view window sum:", int(Cv.max()))
    assert int(Cv.max()) == bo.MAX_WINDOW_SUM == 20655 and bo.MAX_WINDOW_SUM < 1 << 16
    assert int(bo.select(Cv, 3).max()) > 1 << 15                    # and the selected sum needs more than one half


def test_every_invalid_warp_class_occurs_in_the_gpu_shapes():
    seen = set()
    for case in bs.CASES:
        name, w, h, D, radius, trunc, src = case[:7]
        Kc = ds.K if (w, h) == (ds.W, ds.H) else ds.K_SMALL
        x, y = do.rays(Kc, w, h)
        step = do.plane_step(*ARGS, D)
        per_case = set()
        for s in src:
            A, b = do.relative(bs.RIG9[0], bs.RIG9[s])
            for k in range(D):
                per_case |= set(np.unique(do.warp(x, y, do.plane_depth(ds.W_MIN, step, k), A, b, Kc, w, h)[3]).tolist())
        assert do.VALID in per_case, name
        seen |= per_case
    assert seen == {do.INVALID_BEHIND, do.INVALID_OUTSIDE, do.VALID, do.VALID_LAST_EDGE}
    assert sorted({len(c[6]) for c in bs.CASES}) == [1, 2, 3, 8] and {c[9] for c in bs.CASES} == {0, 4, 8}
    assert all(1 <= c[7] <= len(c[6]) for c in bs.CASES) and len({c[0] for c in bs.CASES}) == len(bs.CASES)


def _share(scenes, name, src, n_best, radius, trunc, census=False, interior=False):
    out = bo.sweep(*_parts(scenes[name], src), n_best, *ARGS, ds.PLANES, radius, trunc, census)
    mask = ds.interior(radius) if interior else None
    share = bo.share_right(out, ds.true_inverse_depth(SURFACES[name]), mask, ds.PLANES, *ARGS)
    print(name, "census" if census else "ad", "radius", radius, "trunc", trunc, "sources", src, "n_best", n_best,
          "interior" if interior else "whole", "share within one step %.4f" % share)
    return share


@pytest.mark.parametrize("name", ["step", "plane"])
def test_a_source_that_looks_elsewhere_is_left_out(scenes, name):
    """AD, radius 1, trunc 255, sources (1, 2, 3), interior pixels: slot 3 stands beyond the near planes, and the sum of all
    three prefers the planes on which its warp is valid.  The oracle's shares, step / plane: all three 15.3 % / 13.6 %, best 1
    97.8 % / 100 %, best 2 94.3 % / 100 %."""
    assert _share(scenes, name, (1, 2, 3), 3, 1, 255, interior=True) < 0.20
    assert _share(scenes, name, (1, 2, 3), 1, 1, 255, interior=True) >= 0.90
    assert _share(scenes, name, (1, 2, 3), 2, 1, 255, interior=True) >= 0.90


@pytest.mark.parametrize("name", ["step", "plane"])
def test_the_border_of_the_image_with_absolute_differences(scenes, name):
    """AD, radius 1, trunc 255, sources (1, 2), all W H pixels.  The oracle's shares, step / plane: both 74.0 % / 78.9 %,
    best 1 97.3 % / 98.8 %."""
    assert _share(scenes, name, (1, 2), 2, 1, 255) < 0.80
    assert _share(scenes, name, (1, 2), 1, 1, 255) >= 0.90


@pytest.mark.parametrize("name", ["step", "plane"])
def test_the_border_of_the_image_with_census(scenes, name):
    """Census, radius 2, trunc 62, sources (1, 2), all W H pixels.  The oracle's shares, step / plane: both 79.4 % / 84.9 %,
    best 1 94.0 % / 98.2 %."""
    assert _share(scenes, name, (1, 2), 2, 2, 62, census=True) < 0.86
    assert _share(scenes, name, (1, 2), 1, 2, 62, census=True) >= 0.90


def test_the_aggregated_sweep_uses_the_selected_volume(scenes):
    """AD with 8 paths (p1 = 2 n, p2 = 16 n, n = 9 n_best), radius 1, trunc 255, sources (1, 2), all pixels of the step scene:
    the oracle's shares are 74.1 % with both and 97.8 % with the best one."""
    import sgm_oracle as so
    v = scenes["step"]
    truth = ds.true_inverse_depth(SURFACES["step"])
    shares = []
    for n_best in (2, 1):
        p1, p2 = bo.default_penalties(1, n_best)
        out = bo.sweep(*_parts(v, (1, 2)), n_best, *ARGS, ds.PLANES, 1, 255, False, 8, p1, p2)
        C, _ = bo.cost_volume(*_parts(v, (1, 2)), n_best, *ARGS, ds.PLANES, 1, 255)
        assert np.array_equal(out["C"], C) and np.array_equal(out["S"], so.aggregate(C, p1, p2, 8))
        shares.append(bo.share_right(out, truth, None, ds.PLANES, *ARGS))
    print("aggregated shares, both and best 1:", shares)
    assert (p1, p2) == (18, 144) and shares[0] < 0.80 and shares[1] >= 0.90
