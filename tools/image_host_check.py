"""Writes the case files tools/image_host_check.cpp reads: the scenes of tests/image_scene.py restated as the raw inputs of
k_ncc_search and k_blur_templates (frame, h, S, flags, templates; the oracle computes h and S on the CPU), the cases the API
cannot reach, and the outputs of oracle/image_oracle.py.  Usage: python tools/image_host_check.py OUT_DIR"""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests"), os.path.join(R, "oracle")]
import image_oracle as io_
import image_scene as isc

SEARCH, BLUR = 0, 1


def _header(fh, kind, T, N, w, fw, fh_, kernel_min_size, sigma_size, threshold):
    fh.write(np.array([kind, int(T == np.float64), N, w, fw, fh_, kernel_min_size, 0], np.int32).tobytes())
    fh.write(np.array([sigma_size, threshold], np.float32).tobytes())


def write_search(path, sc, T, tpl, h, S, visible, threshold=io_.PATCH_MATCHING_THRESHOLD):
    """ints kind is_double N w fw fh 0 0; floats sigma_size threshold; frame; h, S (s00 s01 s10 s11 a feature), flags,
    matching templates; the oracle: found, z, score, matching templates after."""
    found, z, score, after = isc.expected(sc, tpl, h, S, visible, threshold)
    N, w = len(tpl), sc.cfg.window_size
    with open(path, "wb") as fh:
        _header(fh, SEARCH, T, N, w, sc.search_frame.shape[1], sc.search_frame.shape[0], 0, sc.cfg.sigma_size, threshold)
        fh.write(np.ascontiguousarray(sc.search_frame, np.uint8).tobytes())
        fh.write(np.asarray(h, T).tobytes() + np.asarray(S, T).reshape(N, 4).tobytes())
        fh.write(np.asarray(visible, np.uint8).tobytes() + np.stack(tpl).astype(np.uint8).tobytes())
        fh.write(found.astype(np.uint8).tobytes() + z.astype(T).tobytes() + score.astype(np.float32).tobytes())
        fh.write(np.stack(after).astype(np.uint8).tobytes())
    print("%s: %d features, %d found" % (os.path.basename(path), N, int(found.sum())))
    return found


def write_blur(path, cfg, T, tpl, h, hb, visible):
    """ints kind is_double N w 0 0 kernel_size 0; floats 0 0; h, hb, flags, templates, matching templates before (the
    templates inverted: an invisible feature keeps them); the oracle: matching templates after."""
    N, w = len(tpl), cfg.window_size
    before = [255 - t for t in tpl]
    after = isc.expected_blur(cfg, tpl, h, hb, visible, before)
    with open(path, "wb") as fh:
        _header(fh, BLUR, T, N, w, 0, 0, cfg.kernel_size, 0, 0)
        fh.write(np.asarray(h, T).tobytes() + np.asarray(hb, T).tobytes() + np.asarray(visible, np.uint8).tobytes())
        fh.write(np.stack(tpl).astype(np.uint8).tobytes() + np.stack(before).astype(np.uint8).tobytes())
        fh.write(np.stack(after).astype(np.uint8).tobytes())
    print("%s: %d features, %d blurred" % (os.path.basename(path), N, sum(not np.array_equal(a, t) for a, t in zip(after, tpl))))


def raw_search(name):
    """(scene, T, templates, h, S, visible[, threshold]) of a case the API cannot reach (or, the threshold pair, reaches
    only with a score the device returned)."""
    sc = isc.scenes()["border"]
    frame = sc.search_frame
    w = sc.cfg.window_size
    eye = 8.0 * np.eye(2)
    if name.startswith("frac_below"):
        # a fraction just below an integer: fp32 truncates to the pixel below (rounding to nearest would give the pixel
        # above); the fp64 values round UP when cast to float (the reference's cv::Point2f), so the centre is the pixel above
        # what truncating the double would give.  S = 0.05 I: the box is two candidates wide and the ellipse passes the
        # centre alone, and each template is the window AT the right centre -- so found, z and the score all hang on the
        # centre, which the asserts below show with the oracle: the other centre gives another result for every feature.
        T = np.float32 if name.endswith("f32") else np.float64
        at = np.array([(100, 57), (9, 120), (311, 10), (200, 231)])
        below = (lambda v: np.nextafter(np.float32(v), np.float32(0))) if T == np.float32 else (lambda v: np.float64(v) - 1e-12)
        h = np.array([[below(u), below(v)] for u, v in at], T)
        centre = at - 1 if T == np.float32 else at
        other = (at if T == np.float32 else at - 1).astype(T)          # rintf(h) / (int) of the double
        assert all(int(np.float32(x)) == c for x, c in zip(h.ravel(), centre.ravel()))
        assert np.array_equal(np.rint(h) if T == np.float32 else np.floor(h), other)
        tpl = [io_.capture_patch(frame, u, v, w) for u, v in centre]
        S = np.stack([0.05 * np.eye(2)] * len(at)).astype(T)
        vis = np.ones(len(at), bool)
        found, z, score, _ = isc.expected(sc, tpl, h, S, vis)
        assert found.all() and np.array_equal(z, centre) and np.all(score == 1)
        found_o, z_o, score_o, _ = isc.expected(sc, tpl, other, S, vis)
        assert np.all((z_o != z).any(axis=1)) and np.all(score_o != score), (z_o, score_o)
        return sc, T, tpl, h, S, vis
    if name == "outside_frame":
        # visible-flagged features whose whole region lies outside the frame, on every side and far away
        h = np.array([[-100.5, 50.0], [500.25, 300.75], [160.0, -60.0], [-40.0, -40.0], [352.0, 120.0], [160.0, 275.5]], np.float32)
        tpl = [io_.capture_patch(frame, 100 + 10 * i, 100, w) for i in range(len(h))]
        return sc, np.float32, tpl, h, np.stack([25.0 * eye] * len(h)).astype(np.float32), np.ones(len(h), bool)
    if name == "invisible":
        _, h, S, vis, _ = isc.oracle_predictions(sc, np.float32)
        vis = vis.copy()
        vis[[0, 3, 6]] = False
        return sc, np.float32, isc.templates(sc), h, S, vis
    if name.startswith("threshold"):
        # the threshold is a feature's own score (found: the test is `not score < threshold`) and the next float above it
        _, h, S, vis, _ = isc.oracle_predictions(sc, np.float32)
        s = isc.expected(sc, isc.templates(sc), h, S, vis)[2][isc.THRESHOLD_FEATURE]
        assert 0.8 < s < 1
        thr = float(s if name == "threshold_equal" else np.nextafter(s, np.float32(2)))
        return sc, np.float32, isc.templates(sc), h, S, vis, thr
    sc = isc.host_only_scenes()[name]
    _, h, S, vis, _ = isc.oracle_predictions(sc, np.float32)
    return sc, np.float32, isc.templates(sc), h, S, vis


def raw_blur(name):
    """(config, T, templates, h, hb, visible)"""
    if name == "blur_fallback":                       # the scene that reaches the fallback through the API
        sc = isc.scenes()[name]
        _, h, S, vis, hb = isc.oracle_predictions(sc, np.float32)
        return sc.cfg, np.float32, isc.templates(sc), h, hb, vis
    cfg = isc.config(9, kernel_size=2, T_camera=0.5)
    rng = np.random.default_rng(7)
    ang = np.array([0.0, 0.5, 1.2, np.pi / 2, 2.0, 3.0, np.pi, 3.7, 4.4, 5.3, 6.0])
    # lines of kMaxTaps pixels and a little more (the sharp template is kept) or a little less (the longest kernel the
    # builder accepts: reflect101 folds a 9-pixel patch over a hundred times)
    length = 1024.0 + (rng.uniform(0.0, 40.0, ang.size) if name == "blur_raw_fallback" else -rng.uniform(0.05, 1.5, ang.size))
    h = np.stack([rng.uniform(20, 300, ang.size), rng.uniform(20, 220, ang.size)], 1)
    hb = h - length[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    tpl = [rng.integers(0, 256, (9, 9)).astype(np.uint8) for _ in ang]
    vis = np.ones(ang.size, bool)
    vis[4] = False
    h, hb = h.astype(np.float64), hb.astype(np.float64)
    n_fb = sum(isc.blur_line(a, b)[4] >= isc.MAX_TAPS for a, b in zip(h, hb))
    assert n_fb == (ang.size if name == "blur_raw_fallback" else 0), n_fb
    return cfg, np.float64, tpl, h, hb, vis


def main(out):
    os.makedirs(out, exist_ok=True)
    scenes = isc.scenes()
    for name, types in isc.HOST_CHECK_TYPES.items():
        sc = scenes[name]
        for T in types:
            path = os.path.join(out, "%s_%s.bin" % (name, "f64" if T == np.float64 else "f32"))
            _, h, S, vis, hb = isc.oracle_predictions(sc, T)
            if sc.blur:
                write_blur(path, sc.cfg, T, isc.templates(sc), h, hb, vis)
            else:
                write_search(path, sc, T, isc.templates(sc), h, S, vis)
    for name in isc.RAW_SEARCH:
        found = write_search(os.path.join(out, name + ".bin"), *raw_search(name))
        if name.startswith("threshold"):
            assert bool(found[isc.THRESHOLD_FEATURE]) == (name == "threshold_equal")
    for name in isc.RAW_BLUR:
        write_blur(os.path.join(out, name + ".bin"), *raw_blur(name))


if __name__ == "__main__":
    main(sys.argv[1])
