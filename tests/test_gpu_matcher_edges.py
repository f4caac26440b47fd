"""The device patch matcher and the template blur at their edges: the directed scenes of
tests/image_scene.py through VSlamFilter alone, against oracle/image_oracle.py.  As in tests/test_gpu_image.py the oracle
consumes the device's own h and 2 x 2 S, so found, z and the templates are exact and the score is within the project's
1e-6.  tests/test_oracle_matcher_edges.py shows on the CPU that every scene reaches the edge it is named for; the checks of
`_reaches` repeat the decisive ones on the device's own predictions."""
import numpy as np
import pytest

import image_scene as isc
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

SEARCH_CASES = [(n, t) for n in isc.SEARCH_SCENES for t in isc.dtypes(n)]          # names only: collection builds no scene


def _device(sc, dtype):
    """The HIP filter of a scene: features added on the template frame, then the oracle filter's mu and Sigma."""
    pkg = load_package()
    ref = isc.oracle_filter(sc, dtype)
    gcfg = {k: getattr(sc.cfg, k) for k in pkg.kinect_config()}
    gcfg["sigma_size"] = sc.cfg.sigma_size
    g = pkg.VSlamFilter(gcfg, capacity_features=len(sc.pixels), dtype=dtype)
    g.setDt(sc.dT)
    g.setFrame(sc.template_frame)
    for (u, v) in sc.pixels:
        assert g.addFeature((u, v)) == 1
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    tpl = isc.templates(sc)
    for i in sc.flat_templates:
        g.setPatch(i, tpl[i])
    for i in range(len(tpl)):
        assert np.array_equal(g.getPatch(i), tpl[i]) and np.array_equal(g.getPatch(i, matching=True), tpl[i])
    return g, tpl


def _reaches(name, sc, tpl, h, S):
    """The scene's edge is reached with the device's predictions too."""
    ss = [isc.scan(sc.search_frame, tpl[i], h[i], S[i], sc.cfg.sigma_size, scores=False) for i in range(len(tpl))]
    hw, w = sc.cfg.window_size // 2, sc.cfg.window_size
    fh, fw = sc.shape
    if name in isc.CLAMPED_SCENES:
        assert all(s.ni == 41 and s.nj == 41 for s in ss)
    if name in isc.BORDER_SCENES:
        for s in ss[:len(ss) if name == "small" else isc.N_BORDER]:
            assert s.i0 - hw < 0 or s.j0 - hw < 0 or s.i0 - hw + s.ni + w > fw or s.j0 - hw + s.nj + w > fh
            assert not s.admissible.all()
    if name == "small":
        assert all(s.i0 - hw < 0 and s.j0 - hw < 0 and s.i0 - hw + s.ni + w > fw and s.j0 - hw + s.nj + w > fh for s in ss)
    if name in isc.OBLIQUE_SCENES:
        assert all(s.inside.any() for s in ss)
        assert sum(s.inside.sum() for s in ss) <= 0.5 * sum(s.admissible.sum() for s in ss)
        assert any(s.swap for s in ss) == (name != "oblique_noswap")


@pytest.mark.parametrize("name,dtype", SEARCH_CASES, ids=["%s-%s" % (n, np.dtype(t).name) for n, t in SEARCH_CASES])
def test_search_scene_equals_the_oracle(name, dtype):
    """Border overhang and the frame gate, the clamped 41 x 41 box (window 32: the 73 x 73 region), the live ellipse and the
    LU row swap, equal maxima across lanes and passes and within one lane (ties, ties_lanes, ties_same_lane), 0 / 0 scores, windows 15, 32, 9, 5, 4 and the
    48 x 40 frame: found and z exact, score within 1e-6, the matching template the matched window or untouched."""
    sc = isc.scenes()[name]
    g, tpl = _device(sc, dtype)
    g.measure()
    h, vis, rem, S2 = g.predictions()
    assert vis.all() and not rem.any()
    assert np.abs(h - np.array(sc.pixels)).max() < 1e-2          # the camera has not moved
    _reaches(name, sc, tpl, h, S2)
    g.setFrame(sc.search_frame)
    z, found, score = g.findMatches()
    want_found, want_z, want_score, after = isc.expected(sc, tpl, h, S2, vis)
    for i in range(len(tpl)):
        print(name, i, bool(found[i]), z[i], score[i], "oracle", bool(want_found[i]), want_z[i], want_score[i])
    for i in range(len(tpl)):
        assert bool(found[i]) == bool(want_found[i]), i
        assert tuple(int(v) for v in z[i]) == tuple(want_z[i]) and np.all(z[i] == np.floor(z[i])), i
        assert abs(float(score[i]) - float(want_score[i])) < 1e-6, i
        assert np.array_equal(g.getPatch(i, matching=True), after[i]), i      # Patch.cpp:286, or unchanged
        assert np.array_equal(g.getPatch(i), tpl[i]), i
    if name in isc.DEGENERATE:
        for i in isc.DEGENERATE[name]:
            assert not found[i] and score[i] == -1 and tuple(z[i]) == (-1, -1), i
    if name.startswith("ties"):
        assert found.all() and np.all(score == 1.0)


def test_threshold_edge():
    """found iff not score < threshold: a feature's own returned score as the threshold still finds it, the next float
    above does not and reports the score."""
    sc = isc.scenes()["border"]
    g, tpl = _device(sc, np.float32)
    g.measure()
    g.setFrame(sc.search_frame)
    z0, found0, score0 = g.findMatches()
    below_one = [i for i in range(len(tpl)) if found0[i] and score0[i] < 1]
    at_one = [i for i in range(len(tpl)) if found0[i] and score0[i] == 1]
    assert below_one and at_one

    def restore():
        for i in range(len(tpl)):
            g.setPatch(i, tpl[i])

    for i in (below_one[0], at_one[0]):
        s = np.float32(score0[i])
        restore()
        z, found, score = g.findMatches(threshold=float(s))
        assert found[i] and score[i] == s and np.array_equal(z[i], z0[i]), i
        restore()
        z, found, score = g.findMatches(threshold=float(np.nextafter(s, np.float32(2))))
        assert not found[i] and score[i] == s and tuple(z[i]) == (-1, -1), i
        assert np.array_equal(g.getPatch(i, matching=True), tpl[i])


def _blurred():
    """name -> (scene, templates, h, hb, visible, matching templates, templates read back) of every blur scene."""
    out = {}
    for name in list(isc.BLUR_MOTIONS) + list(isc.BLUR_FALLBACK):
        sc = isc.scenes()[name]
        g, tpl = _device(sc, np.float32)
        g.predict()
        h, vis, rem, S2 = g.predictions()
        hb = g.blurPredictions()
        out[name] = (sc, tpl, h, hb, vis, [g.getPatch(i, matching=True) for i in range(len(tpl))],
                     [g.getPatch(i) for i in range(len(tpl))])
    return out


@pytest.fixture(scope="module")
def blurred():
    return _blurred()


@pytest.mark.parametrize("name", sorted(isc.BLUR_MOTIONS))
def test_blur_scene_equals_the_oracle(blurred, name):
    """Blur lines in every direction, one-row and one-column kernels, lines longer than twice the window (reflect101 folds
    more than once) and the plain copy below kernel_size: the matching template bit for bit."""
    sc, tpl, h, hb, vis, got, sharp = blurred[name]
    assert vis.all() and np.abs(h - np.array(sc.pixels)).max() < 0.05
    want = isc.expected_blur(sc.cfg, tpl, h, hb, vis)
    for i in range(len(tpl)):
        assert np.array_equal(got[i], want[i]), (i, isc.blur_line(h[i], hb[i]))
        assert np.array_equal(sharp[i], tpl[i]), i
    if name == "blur_copy":
        assert all(np.array_equal(got[i], tpl[i]) for i in range(len(tpl)))


def test_blur_scenes_reach_their_edges_on_the_device(blurred):
    octants, one_row, one_col, long_lines = set(), 0, 0, 0
    for name in isc.BLUR_MOTIONS:
        sc, tpl, h, hb, vis, got, sharp = blurred[name]
        for i in range(len(tpl)):
            dx, dy, rows, cols, length, octant = isc.blur_line(h[i], hb[i])
            if np.hypot(dx, dy) > sc.cfg.kernel_size:
                octants.add(octant)
                one_row += rows == 1 and cols > 2
                one_col += cols == 1 and rows > 2
                long_lines += name == "blur_long" and max(rows, cols) > 2 * sc.cfg.window_size
    assert octants == set(range(8)) and one_row >= 1 and one_col >= 1 and long_lines >= 3


def test_blur_line_of_1024_pixels_or_more_keeps_the_sharp_template(blurred):
    """The documented deviation (kMaxTaps): the oracle would build the kernel, the device keeps the template.  Reached with
    a finite state: the blur pose looks far away from the feature and projects it beyond 1024 pixels."""
    sc, tpl, h, hb, vis, got, sharp = blurred["blur_fallback"]
    assert np.isfinite(hb).all()
    lengths = np.array([isc.blur_line(h[i], hb[i])[4] for i in range(len(tpl))])
    fallback = vis & (lengths >= isc.MAX_TAPS)
    assert fallback.sum() >= 1
    want = isc.expected_blur(sc.cfg, tpl, h, hb, vis)
    for i in range(len(tpl)):
        assert np.array_equal(got[i], want[i]), (i, lengths[i])
        if fallback[i]:
            assert np.array_equal(got[i], tpl[i]), i
