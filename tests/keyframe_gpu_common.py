"""Drivers shared by tests/test_gpu_keyframes.py and the measurement behind tests/golden/keyframe_bounds.json: a scripted
scene (tests/keyframe_scene.py) through a real filter's setters and the device selector, next to the numpy oracle."""
import json
import os

import numpy as np

import keyframe_oracle as ko
import keyframe_scene as ks

BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_bounds.json")
EMITS = (ko.EMIT_CURRENT, ko.EMIT_CANDIDATE, ko.EMIT_FIRST)


def load_bounds():
    return json.load(open(BOUNDS))


def scripted_filter(pkg, dtype, first_frame):
    """A filter with N_FEATURES features, converted to XYZ where the linearity test allows after their rows of Sigma were
    shrunk (as test_filter_stream_keyframes_to_sba_add forces conversions), so that Point4sba rows exist."""
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=32, dtype=dtype)
    for (u, v) in first_frame["centers"]:
        assert g.addFeature((float(u), float(v))) == 1
    S = g.getFullSigma()
    n0 = g.camera_dim
    S[n0:, :] *= 1e-4
    S[:, n0:] *= 1e-4
    g.setSigmaBlock(S)
    g.convert2XYZ_ifLinearAll()
    return g


def image_of(frame_id, shape):
    """A frame image that names its id in every byte pattern."""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 3 + y * 5 + 37 * int(frame_id)) % 251).astype(np.uint8)


def run_scripted(pkg, frames, dtype, move_thresh=ks.MOVE_THRESH, keep=False, images=False, selector=None, filt=None):
    """One scene on the device and through the oracle.  Returns (device results, oracle results, deviations, selector,
    filter); a device result is (KeyframeResult, image or None)."""
    g = filt if filt is not None else scripted_filter(pkg, dtype, frames[0])
    sel = selector if selector is not None else pkg.KeyframeSelector(g, move_thresh, keep_current_projections=keep)
    ora = ko.Selector(move_thresh, keep)
    dev, ref = [], []
    worst = {"D": 0.0, "c": 0.0, "pose": 0.0, "sigma": 0.0, "vrot": 0.0}
    for fr in frames:
        mu = g.getFullState()
        mu[:7] = fr["pose"]
        g.setFullState(mu)
        g.setSigmaBlock(fr["sigma"].astype(dtype), 0, 0)
        for i in range(len(fr["centers"])):
            g.setFeatureTrack(i, in_innovation=int(fr["in_innovation"][i]), center=fr["centers"][i])
        img = None
        if images:
            img = image_of(fr["id"], sel.image_shape)
            g.setFrame(img)
        prj = g.keyframeProjections()                     # the host's own builder (formats.point4sba_rows)
        o = ora.observe(fr["id"], fr["pose"], fr["sigma"], prj, img)
        r = sel.observe(fr["id"])
        got_img = sel.emitted_image() if (images and r.emitted) else None
        dev.append((r, got_img))
        ref.append(o)
        if np.isfinite(o["dist"]) and np.isfinite(r.dist):
            worst["D"] = max(worst["D"], abs(float(r.dist) - float(o["dist"])))
        worst["c"] = max(worst["c"], abs(float(r.cov) - float(o["cov"])))
        if r.emitted and o["action"] in EMITS:
            worst["pose"] = max(worst["pose"], float(np.nanmax(np.abs(r.record.pose - o["pose"]))))
            worst["sigma"] = max(worst["sigma"], float(np.nanmax(np.abs(r.record.sigma - o["sigma"]))))
            # last_vrot = quat2vec of the current state, the one stored value that went through the device's acos / sin
            worst["vrot"] = max(worst["vrot"], float(np.abs(sel.state()["last_vrot"] - ora.last_vrot).max()))
    return dev, ref, worst, sel, g


def assert_scene(dev, ref, bound, images=False):
    """Actions, ids, projection rows (and images) exactly; D, c, pose and the 7 x 7 block within `bound`."""
    for k, ((r, img), o) in enumerate(zip(dev, ref)):
        assert r.action == o["action"], (k, r.action_name, ko.ACTION_NAMES[o["action"]], r.dist, float(o["dist"]))
        assert np.isnan(r.dist) == bool(np.isnan(o["dist"])), k
        if not np.isnan(r.dist):
            assert abs(float(r.dist) - float(o["dist"])) <= bound["D"], (k, r.dist, float(o["dist"]))
        assert abs(float(r.cov) - float(o["cov"])) <= bound["c"], (k, r.cov, float(o["cov"]))
        assert r.emitted == (o["action"] in EMITS), k
        if r.emitted:
            assert r.record.id == o["id"], (k, r.record.id, o["id"])
            assert np.array_equal(r.record.projections, o["projections"]), (k, r.record.projections, o["projections"])
            assert float(np.abs(r.record.pose - o["pose"]).max()) <= bound["pose"], k
            assert float(np.abs(r.record.sigma - o["sigma"]).max()) <= bound["sigma"], k
            if images:
                assert img is not None and o["image"] is not None and np.array_equal(img, o["image"]), k
