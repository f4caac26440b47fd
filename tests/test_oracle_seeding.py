"""CPU checks of the seeding / end-of-update restatement (tests/frame_oracle.py): the detector against an independent
scipy formulation, known answers on synthetic corners, the fp32 quality rule, and the new ABI symbols."""
import numpy as np
import pytest

import frame_oracle as fo
import image_oracle as io_


def _independent_detect(frame, mask, num, quality, min_distance):
    """scipy.ndimage Sobel / correlate with mode='mirror' (= REFLECT_101), maximum_filter, a per-pixel greedy loop."""
    from scipy import ndimage as nd
    f = frame.astype(np.int64)
    dx = nd.sobel(f, axis=1, mode="mirror")
    dy = nd.sobel(f, axis=0, mode="mirror")
    k = np.ones((3, 3), np.int64)
    a = nd.correlate(dx * dx, k, mode="mirror")
    b = nd.correlate(dx * dy, k, mode="mirror")
    c = nd.correlate(dy * dy, k, mode="mirror")
    lam = 0.5 * ((a + c).astype(np.float64) - np.sqrt(((a - c) ** 2 + 4 * b * b).astype(np.float64)))
    thr = lam[mask != 0].max() * quality
    t = np.where(lam > thr, lam, 0.0)
    dil = nd.maximum_filter(t, size=3, mode="constant", cval=-np.inf)
    H, W = frame.shape
    cands = []
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            if mask[y, x] and t[y, x] != 0 and t[y, x] == dil[y, x]:
                cands.append((t[y, x], y * W + x))
    cands.sort(key=lambda p: (p[0], p[1]), reverse=True)
    acc = []
    for v, i in cands:
        if len(acc) == num:
            break
        x, y = i % W, i // W
        if all((x - ax) ** 2 + (y - ay) ** 2 >= min_distance ** 2 for ax, ay in acc):
            acc.append((x, y))
    return lam, np.asarray(acc, np.float32).reshape(-1, 2)


@pytest.mark.parametrize("seed,window,centers", [(1, 15, []), (2, 15, [(100.0, 80.0), (200.5, 150.25)]),
                                                  (3, 30, [(60.0, 60.0)])])
def test_detector_matches_independent_formulation(seed, window, centers):
    frame = io_.random_texture(120, 160, seed=seed, smooth=1)
    mask = fo.seed_mask(160, 120, window, centers)
    uv, lam = fo.find_new_features(frame, centers, window, 40, 0.01, 12.0)
    lam2, uv2 = _independent_detect(frame, mask, 40, 0.01, 12.0)
    assert np.array_equal(lam.view(np.int64), lam2.view(np.int64))        # bit for bit
    assert np.array_equal(uv, uv2)
    assert len(uv) > 0


def test_response_is_nonnegative_and_scaled_like_opencv():
    frame = io_.random_texture(60, 80, seed=7, smooth=1)
    lam = fo.corner_response(frame)
    assert lam.min() >= 0.0
    # the same value from the float formula of cornerMinEigenVal on the normalised derivatives, scaled back
    dx, dy = fo.sobel_int(frame)
    s = 1.0 / (4 * 3 * 255)
    a, b, c = (fo._box3(v) * s * s for v in (dx * dx, dx * dy, dy * dy))
    ref = ((a + c) * 0.5 - np.sqrt(((a - c) * 0.5) ** 2 + b * b)) / (s * s)
    assert np.allclose(lam, ref, rtol=1e-9, atol=1e-3)


def _squares(H=120, W=160):
    img = np.zeros((H, W), np.uint8)
    sq = [(20, 30, 25), (90, 40, 30), (60, 80, 20)]            # (x0, y0, side)
    for x0, y0, s in sq:
        img[y0:y0 + s, x0:x0 + s] = 200
    corners = [(x0 + dx, y0 + dy) for x0, y0, s in sq for dx in (0, s - 1) for dy in (0, s - 1)]
    return img, corners


def test_squares_known_answer():
    img, corners = _squares()
    uv, lam = fo.find_new_features(img, [], 15, 100, 0.01, 12.0)
    assert len(uv) == len(corners)
    for (u, v) in uv:
        assert min(abs(u - cx) + abs(v - cy) for cx, cy in corners) <= 2
        assert min(max(abs(u - cx), abs(v - cy)) for cx, cy in corners) <= 1
    vals = [lam[int(v), int(u)] for u, v in uv]
    assert all(vals[k] >= vals[k + 1] for k in range(len(vals) - 1))        # ordered by lambda
    d2 = ((uv[:, None, :] - uv[None, :, :]) ** 2).sum(-1) + np.eye(len(uv)) * 1e9
    assert d2.min() >= 144


def test_mask_square_removes_exactly_its_corners():
    img, corners = _squares()
    uv0, _ = fo.find_new_features(img, [], 15, 100, 0.01, 12.0)
    c = (np.float32(32.0), np.float32(42.0))                   # near the first square's top-left corner (20, 30)
    uv1, _ = fo.find_new_features(img, [c], 15, 100, 0.01, 12.0)
    x0, y0 = int(c[0] - 15), int(c[1] - 15)
    inside = [(u, v) for u, v in uv0 if x0 <= u <= x0 + 30 and y0 <= v <= y0 + 30]
    assert len(inside) >= 1
    assert sorted(map(tuple, uv1.tolist())) == sorted((u, v) for u, v in uv0.tolist() if (u, v) not in inside)


def test_mask_margin_and_strict_compares():
    m = fo.seed_mask(100, 80, 10, [(10.0, 40.0), (50.0, 40.0), (89.999, 40.0), (90.0, 40.0)])
    assert m[:10].max() == 0 and m[70:].max() == 0 and m[:, :10].max() == 0 and m[:, 90:].max() == 0
    assert m[40, 40:61].max() == 0 and m[40, 39] == 255 and m[40, 61] == 255       # origin 40, side 21
    assert m[40, 79:90].max() == 0                              # 89.999: inside, origin (int)79.999 = 79
    assert m[40, 11] == 255                                     # 10.0 is not > 10: no square


def test_quality_rule_fp32_edge():
    # n_tot - n_find == 0.2 n_find: (float)1 / (float)5 = 0.2f, not > 0.2f -> not flagged
    assert not fo.quality_flags([6], [5], 0.2)[0]
    assert fo.quality_flags([7], [5], 0.2)[0]
    assert not fo.quality_flags([12], [10], 0.2)[0]            # 2 / 10 in fp32 == 0.2f
    assert fo.quality_flags([13], [10], 0.2)[0]
    assert not fo.quality_flags([1], [1], 0.2)[0]


def test_end_update_plan_eviction_and_seed_count():
    n_find = [1] * 6
    # nothing flagged, 4 visible < min 5, 6 features > max 5 -> evict feature 0, seed 1
    r, nv, ev, sd = fo.end_update_plan([1] * 6, n_find, [0] * 6, [1, 1, 1, 1, 0, 0], 5, 5)
    assert list(r) == [] and nv == 4 and ev and sd == 1
    # 6 not > max 6: no eviction
    r, nv, ev, sd = fo.end_update_plan([1] * 6, n_find, [0] * 6, [1, 1, 1, 1, 0, 0], 5, 6)
    assert not ev and sd == 1
    # visible >= min: neither
    r, nv, ev, sd = fo.end_update_plan([1] * 6, n_find, [0] * 6, [1] * 6, 5, 3)
    assert not ev and sd == 0
    # quality (feature 1: 3 searches, 1 found) and the sticky flag (feature 4): removed in descending order
    r, nv, ev, sd = fo.end_update_plan([1, 3, 1, 1, 1, 1], n_find, [0, 0, 0, 0, 1, 0], [1, 1, 1, 0, 1, 1], 3, 10)
    assert list(r) == [4, 1] and nv == 3 and sd == 0


def test_new_abi_symbols_have_prototypes():
    from __graft_entry__ import load_package
    capi = load_package().capi
    syms = capi.declared_symbols()
    for name in ("ekf_get_feature_track", "ekf_set_feature_track", "ekf_find_new_features", "ekf_end_update"):
        assert name in syms
        assert name in capi._PROTOS
