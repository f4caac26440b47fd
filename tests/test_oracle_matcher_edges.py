"""The conditions tests/image_scene.py states for its directed scenes hold for the oracle alone (no GPU): each scene
reaches the edge of the matcher or the blur it is named for, so that the host check and the GPU tests that replay it
exercise that edge on purpose.  Nothing here skips or reseeds."""
import numpy as np
import pytest

import image_scene as isc


@pytest.fixture(scope="module")
def scans():
    """name -> (scene, h, S, visible, templates, [Scan per feature]) in fp32, computed once."""
    out = {}
    for name in isc.SEARCH_SCENES:
        sc = isc.scenes()[name]
        _, h, S, vis, _ = isc.oracle_predictions(sc, np.float32)
        tpl = isc.templates(sc)
        out[name] = (sc, h, S, vis, tpl,
                     [isc.scan(sc.search_frame, tpl[i], h[i], S[i], sc.cfg.sigma_size) for i in range(len(tpl))])
    return out


def test_every_feature_is_visible_and_predicted_where_it_was_added(scans):
    for name, (sc, h, S, vis, tpl, ss) in scans.items():
        assert vis.all(), name
        assert np.abs(h - np.array(sc.pixels)).max() < 1e-2, name
        assert len(sc.pixels) <= 16 and sc.cfg.image_width <= 320 and sc.cfg.image_height <= 240


def test_the_scan_restates_find_match(scans):
    """image_scene.scan (the candidate-by-candidate view the conditions are stated on) and image_oracle.find_match agree."""
    for name, (sc, h, S, vis, tpl, ss) in scans.items():
        found, z, score, after = isc.expected(sc, tpl, h, S, vis)
        for i, s in enumerate(ss):
            c = s.best()
            if c < 0:
                assert not found[i] and score[i] == -1 and tuple(z[i]) == (-1, -1), (name, i)
                continue
            assert score[i] == s.score[c], (name, i)
            assert bool(found[i]) == bool(s.score[c] >= np.float32(0.8)), (name, i)
            if found[i]:
                assert tuple(z[i]) == (s.i0 + c // s.nj, s.j0 + c % s.nj), (name, i)


@pytest.mark.parametrize("name", isc.BORDER_SCENES)
def test_border_scenes_hang_over_the_frame(scans, name):
    sc, h, S, vis, tpl, ss = scans[name]
    fh, fw = sc.shape
    hw, w = sc.cfg.window_size // 2, sc.cfg.window_size
    small = name == "small"
    for i in range(len(tpl) if small else isc.N_BORDER):
        s = ss[i]
        x0, y0, x1, y1 = s.i0 - hw, s.j0 - hw, s.i0 - hw + s.ni + w, s.j0 - hw + s.nj + w
        assert x0 < 0 or y0 < 0 or x1 > fw or y1 > fh, (name, i)
        assert not s.admissible.all() and s.admissible.any(), (name, i)
        if small:                                            # over both opposite borders at once
            assert x0 < 0 and y0 < 0 and x1 > fw and y1 > fh, i


@pytest.mark.parametrize("name", isc.CLAMPED_SCENES)
def test_clamped_scenes_have_the_largest_box(scans, name):
    sc, h, S, vis, tpl, ss = scans[name]
    assert all(s.ni == 41 and s.nj == 41 for s in ss)
    if name == "window_32":                                  # the staged region is at every capacity constant
        assert all(s.ni + 32 == 73 for s in ss)


def test_the_unit_covariance_box_is_small(scans):
    assert all(s.ni in (11, 12) and s.nj in (11, 12) for s in scans["border"][5])


@pytest.mark.parametrize("name", isc.OBLIQUE_SCENES)
def test_oblique_scenes_have_a_live_ellipse(scans, name):
    sc, h, S, vis, tpl, ss = scans[name]
    for i, s in enumerate(ss):
        assert s.inside.sum() >= 1, (name, i)
    # (counted over the scene: image_scene's docstring says why)
    assert sum(s.inside.sum() for s in ss) <= 0.5 * sum(s.admissible.sum() for s in ss)
    swaps = sum(s.swap for s in ss)
    assert (swaps >= 1) if name != "oblique_noswap" else (swaps == 0)


def test_the_true_match_lies_where_the_variant_says(scans):
    """inside the gate (border, oblique_swap); inside the box, outside the ellipse (oblique_outside); beyond the admissible
    band (border_pushed, the six features on the margin)."""
    def true_index(s, sc, i, move):
        u, v = int(sc.pixels[i][0]) + move[0], int(sc.pixels[i][1]) + move[1]
        ci, cj = u - s.i0, v - s.j0
        return ci * s.nj + cj if 0 <= ci < s.ni and 0 <= cj < s.nj else -1
    for name, move in (("border", (2, -1)), ("oblique_swap", (1, 2)), ("clamped", (9, -7))):
        sc, h, S, vis, tpl, ss = scans[name]
        hits = [i for i, s in enumerate(ss) if true_index(s, sc, i, move) >= 0 and s.inside[true_index(s, sc, i, move)]]
        assert len(hits) >= 4, name
        found, z, score, _ = isc.expected(sc, tpl, h, S, vis)
        assert all(found[i] and score[i] > 0.999 for i in hits), name
    sc, h, S, vis, tpl, ss = scans["oblique_outside"]
    out = [i for i, s in enumerate(ss) if true_index(s, sc, i, (5, -6)) >= 0
           and s.admissible[true_index(s, sc, i, (5, -6))] and not s.inside[true_index(s, sc, i, (5, -6))]]
    assert len(out) >= 3
    found, z, score, _ = isc.expected(sc, tpl, h, S, vis)
    assert not found[out].any()
    sc, h, S, vis, tpl, ss = scans["border_pushed"]
    hw = sc.cfg.window_size // 2
    fh, fw = sc.shape
    for i in range(4):                                       # the corners: the true match left the band in u and v
        u, v = int(sc.pixels[i][0]) + (-3 if i % 2 == 0 else 3), int(sc.pixels[i][1]) + (-3 if i < 2 else 3)
        assert not (u > hw and u < fw - hw) and not (v > hw and v < fh - hw), i


def test_tie_scene_has_equal_maxima_in_different_lanes_and_passes(scans):
    sc, h, S, vis, tpl, ss = scans["ties"]
    n_ok = 0
    for s in ss:
        c = s.best()
        assert c >= 0 and s.score[c] == 1.0
        ties = np.flatnonzero(s.score == s.score[c])
        assert ties[0] == c
        d = ties - c
        n_ok += int(len(ties) >= 8 and np.any(d % 256 != 0) and np.any(d // 256 != 0))
    assert n_ok >= 1
    # ties_lanes: some feature's first maximum sits in a higher lane (c mod 256) than a later one: scan order, not lane
    # order, decides
    sc, h, S, vis, tpl, ss = scans["ties_lanes"]
    assert all(s.best() >= 0 and s.score[s.best()] == 1.0 for s in ss)
    assert any(np.any((np.flatnonzero(s.score == 1.0) % 256) < (s.best() % 256)) for s in ss)
    # ties_same_lane: a later maximum lies a multiple of 256 candidates behind the first (for the features whose gate leaves
    # room: the interior ones and more), so one lane visits both and its strict `val > best` has to keep the first
    sc, h, S, vis, tpl, ss = scans["ties_same_lane"]
    same_lane = 0
    for s in ss:
        c = s.best()
        ties = np.flatnonzero(s.score == 1.0)
        assert c >= 0 and s.score[c] == 1.0 and ties[0] == c
        same_lane += bool(np.any((ties[1:] - c) % 256 == 0))
    print("features with a same-lane tie:", same_lane)
    assert same_lane >= 3


@pytest.mark.parametrize("name", isc.NON_PERIODIC)
def test_non_periodic_scenes_have_a_clear_winner(scans, name):
    sc, h, S, vis, tpl, ss = scans[name]
    for i, s in enumerate(ss):
        v = np.unique(s.score[~np.isnan(s.score)].astype(np.float64))
        if len(v) >= 2:
            assert v[-1] - v[-2] > 1e-5, (name, i, v[-1], v[-2])
        # the threshold is no closer than the tolerance either, so `found` cannot flip on rounding
        if len(v):
            assert abs(v[-1] - 0.8) > 1e-5, (name, i)


@pytest.mark.parametrize("name", sorted(isc.DEGENERATE))
def test_degenerate_sums_are_never_chosen(scans, name):
    sc, h, S, vis, tpl, ss = scans[name]
    found, z, score, after = isc.expected(sc, tpl, h, S, vis)
    for i in isc.DEGENERATE[name]:
        assert ss[i].inside.any() and np.isnan(ss[i].score).all(), i
        assert not found[i] and score[i] == -1 and tuple(z[i]) == (-1, -1) and np.array_equal(after[i], tpl[i])
    if name == "flat_occluder":                              # part of the region only: texture is left inside the region
        i = isc.OCCLUDED_FEATURE
        s, hw, w = ss[i], sc.cfg.window_size // 2, sc.cfg.window_size
        reg = sc.search_frame[s.j0 - hw:s.j0 - hw + s.nj + w, s.i0 - hw:s.i0 - hw + s.ni + w]
        assert 0.1 < (reg != isc.FLAT).mean() < 0.9
    if name == "flat_template":
        assert found[[2, 5, 7]].all()                   # the others go on as in `border`


def test_blur_scenes_cover_every_octant_one_row_one_column_and_long_lines():
    octants, one_row, one_col, long_lines, copies = set(), 0, 0, 0, 0
    for name in isc.BLUR_MOTIONS:
        sc = isc.scenes()[name]
        ref, h, S, vis, hb = isc.oracle_predictions(sc, np.float32)
        assert vis.all() and np.abs(h - np.array(sc.pixels)).max() < 0.05, name
        assert len(sc.pixels) <= 16
        for i in range(len(h)):
            dx, dy, rows, cols, length, octant = isc.blur_line(h[i], hb[i])
            if not np.hypot(dx, dy) > sc.cfg.kernel_size:
                copies += name == "blur_copy"
                continue
            assert name != "blur_copy"
            assert length < 1024
            octants.add(octant)
            one_row += rows == 1 and cols > 2
            one_col += cols == 1 and rows > 2
            long_lines += name == "blur_long" and max(rows, cols) > 2 * sc.cfg.window_size
    assert octants == set(range(8))
    assert one_row >= 1 and one_col >= 1 and long_lines >= 3 and copies == 16


def test_blur_fallback_is_reachable_with_a_finite_state():
    (name,) = isc.BLUR_FALLBACK
    sc = isc.scenes()[name]
    ref, h, S, vis, hb = isc.oracle_predictions(sc, np.float32)
    assert np.isfinite(ref.mu).all() and np.isfinite(hb).all()
    lengths = np.array([isc.blur_line(h[i], hb[i])[4] for i in range(len(h))])
    assert (vis & (lengths >= 1024)).sum() >= 1, lengths
