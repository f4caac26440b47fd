"""Rectification on the device against tests/rectify_oracle.py: k_frame_rectify byte for byte, on the held
frame of a filter and on the emit slot of a key-frame selector, at both resolutions; k_undistort_pixels within 1e-9 px
(the oracle is the same fp64 op sequence, so the deviation is expected to be 0; 1e-9 is 1000 x the rounding of these
magnitudes); the error paths; that none of it touches the filter; and end to end, that the pinhole bundle adjuster fits
the rectified rows of a distorted camera and not the distorted ones.  Shapes and lenses: tests/rectify_scene.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_ingest_oracle as fi
import keyframe_oracle as ko
import keyframe_scene as ks
import rectify_oracle as ro
import rectify_scene as rs

pytestmark = pytest.mark.gpu

N_FEAT = ks.N_FEATURES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _filter(pkg, lens_name, scale=rs.SCALE, features=False):
    g = pkg.VSlamFilter(rs.config(pkg.kinect_config(), rs.LENSES[lens_name], scale), capacity_features=16, dtype=np.float32)
    if features:                                               # XYZ features, so that Point4sba rows exist (as test_gpu_keyframes_raw.py)
        for i in range(N_FEAT):
            assert g.addFeature((8.0 + 8.0 * i, 8.0 + 6.0 * i)) == 1
        S = g.getFullSigma()
        n0 = g.camera_dim
        S[n0:, :] *= 1e-4
        S[:, n0:] *= 1e-4
        g.setSigmaBlock(S)
        g.convert2XYZ_ifLinearAll()
    return g


def _lens(g):
    return ro.lens({k: getattr(g._cfg, k) for k in ro.LENS_KEYS})


def _centers(k):
    """Track centres with fractions, inside the 61 x 47 frame, different in every frame."""
    return np.array([[6.25 + 8.5 * i + 0.125 * k, 5.75 + 6.25 * i + 0.375 * (k % 3)] for i in range(N_FEAT)], np.float32)


def _script(g, fr, k):
    mu = g.getFullState()
    mu[:7] = fr["pose"]
    g.setFullState(mu)
    g.setSigmaBlock(fr["sigma"].astype(g.dtype), 0, 0)
    c = _centers(k)
    for i in range(N_FEAT):
        g.setFeatureTrack(i, in_innovation=int(fr["in_innovation"][i]), center=c[i])
    return c


def _snapshot(g):
    return g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts()


@pytest.mark.parametrize("lens_name", sorted(rs.LENSES))
def test_held_frame_rectified_at_both_resolutions(pkg, lens_name):
    g = _filter(pkg, lens_name, features=True)
    L = _lens(g)
    raw = rs.raw_image(11)
    g.setFrameRaw(raw)
    before = _snapshot(g)
    gray = g.getFrame()
    assert np.array_equal(gray, fi.ingest(raw, rs.SCALE))
    got0, got1 = g.getFrameRectified(), g.getFrameRectified(raw=True)
    want0, want1 = ro.rectify_image(gray, L, 1), ro.rectify_image(raw, L, rs.SCALE)
    print(lens_name, "differing bytes: matcher", int((got0 != want0).sum()), "raw", int((got1 != want1).sum()),
          "zero pixels (oracle): matcher", int((ro.tap_classes(L, rs.MW, rs.MH, 1) == 0).sum()))
    assert got0.shape == (rs.MH, rs.MW) and np.array_equal(got0, want0)
    assert got1.shape == (rs.RH, rs.RW, 3) and np.array_equal(got1, want1)
    assert not np.array_equal(got0, gray)                                    # the lens is not a pinhole
    # a stride larger than the width: the bytes between the rows stay as they were
    lib = pkg.load_library()
    buf = np.full((rs.MH, rs.MW + 7), 0xA5, np.uint8)
    assert lib.ekf_get_frame_rectified(g._h, 0, buf.ctypes.data_as(C.c_void_p), buf.strides[0]) == 0
    assert np.array_equal(buf[:, :rs.MW], want0) and (buf[:, rs.MW:] == 0xA5).all()
    bufr = np.full((rs.RH, rs.RW * 3 + 5), 0x5A, np.uint8)
    assert lib.ekf_get_frame_rectified(g._h, 1, bufr.ctypes.data_as(C.c_void_p), bufr.strides[0]) == 0
    assert np.array_equal(bufr[:, :rs.RW * 3].reshape(rs.RH, rs.RW, 3), want1) and (bufr[:, rs.RW * 3:] == 0x5A).all()
    # the cameras of the two resolutions
    assert np.array_equal(g.rectifiedCamera(), ro.camera(L, 1)) and np.array_equal(g.rectifiedCamera(True), ro.camera(L, rs.SCALE))
    # the filter is untouched: state, Sigma and the launch counters, bitwise
    assert _snapshot(g) == before
    g.close()


def test_one_channel_raw_frame_and_a_plain_frame(pkg):
    g = _filter(pkg, "pincushion")
    L = _lens(g)
    raw = rs.raw_image(12, channels=1)
    g.setFrameRaw(raw)
    got = g.getFrameRectified(raw=True)
    assert got.shape == (rs.RH, rs.RW) and np.array_equal(got, ro.rectify_image(raw, L, rs.SCALE))
    assert np.array_equal(g.getFrameRectified(), ro.rectify_image(fi.ingest(raw, rs.SCALE), L, 1))
    # a frame set without its raw one: the matcher frame is rectified, the raw one is gone
    gray = rs.gray_image(13)
    g.setFrame(gray)
    assert np.array_equal(g.getFrameRectified(), ro.rectify_image(gray, L, 1))
    with pytest.raises(pkg.EkfError) as ei:
        g.getFrameRectified(raw=True)
    assert ei.value.status == 4
    out = np.zeros((rs.RH, rs.RW), np.uint8)
    assert pkg.load_library().ekf_get_frame_rectified(g._h, 1, out.ctypes.data_as(C.c_void_p), out.strides[0]) == 4
    g.close()


@pytest.mark.parametrize("lens_name", sorted(rs.LENSES))
def test_undistort_pixels_matches_the_oracle(pkg, lens_name):
    g = _filter(pkg, lens_name, features=True)
    L = _lens(g)
    g.setFrameRaw(rs.raw_image(14))
    before = _snapshot(g)
    for raw, s, w, h in ((False, 1, rs.MW, rs.MH), (True, rs.SCALE, rs.RW, rs.RH)):
        pts = rs.probe_points(w, h)
        assert pts.shape == (64, 2) and np.isnan(pts[5, 0])
        got, want = g.undistortPixels(pts, raw=raw), ro.undistort_pixels(pts, L, s)
        ok = np.isfinite(want).all(axis=1)
        assert ok.sum() == 63 and np.isnan(got[5]).all() and np.isfinite(got[ok]).all()
        err = float(np.abs(got[ok] - want[ok]).max())
        print(lens_name, "raw" if raw else "matcher", "max |device - oracle| =", err, "px; largest shift",
              float(np.abs(want[ok] - pts[ok]).max()), "px")
        assert err <= 1e-9
    assert g.undistortPixels(np.zeros((0, 2))).shape == (0, 2)
    assert _snapshot(g) == before
    g.close()


def _walk(pkg, lens_name, keep, raw_shape, upto=7):
    """Frames 1 .. upto of the hand-built walk on a 61 x 47 matcher frame fed from random 122 x 94 raw frames.  Returns the
    filter, the selector, and per emit: (frame at which it was emitted, action, record, rows rectified at both resolutions,
    rectified images at both resolutions)."""
    g = _filter(pkg, lens_name, features=True)
    sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, keep_current_projections=keep, raw_shape=raw_shape)
    raws, centers, emits = {}, {}, []
    for k, fr in enumerate(ks.scene_walk()[:upto]):
        raws[fr["id"]] = rs.raw_image(100 + fr["id"], channels=1 if len(raw_shape) == 2 else 3)
        g.setFrameRaw(raws[fr["id"]])
        centers[fr["id"]] = _script(g, fr, k)
        r = sel.observe(fr["id"])
        if r.emitted:
            emits.append(dict(at=fr["id"], action=r.action, record=r.record,
                              rows=(sel.emitted_rows_rectified(False), sel.emitted_rows_rectified(True)),
                              images=(sel.emitted_image_rectified(False), sel.emitted_image_rectified(True))))
    return g, sel, raws, centers, emits


@pytest.mark.parametrize("lens_name,channels", [("barrel", 3), ("pincushion", 3), ("pincushion", 1)])
def test_emitted_key_frame_rectified(pkg, lens_name, channels):
    raw_shape = (rs.RH, rs.RW, 3) if channels == 3 else (rs.RH, rs.RW)
    g, sel, raws, centers, emits = _walk(pkg, lens_name, True, raw_shape)
    L = _lens(g)
    assert [(e["at"], e["action"], e["record"].id) for e in emits] == [(2, ko.EMIT_FIRST, 2), (7, ko.EMIT_CANDIDATE, 6)]
    ids = list(g.featureIds()[0])
    for e in emits:
        kid = e["record"].id
        # images: from the emit slot (for the candidate: the frame of id 6, not the current one)
        assert np.array_equal(e["images"][1], ro.rectify_image(raws[kid], L, rs.SCALE)), kid
        assert np.array_equal(e["images"][0], ro.rectify_image(fi.ingest(raws[kid], rs.SCALE), L, 1)), kid
        # rows: those of ekf_keyframe_get_emitted, same order; the coordinates are the undistorted FLOAT centres
        prj = e["record"].projections
        assert len(prj) >= 2 and prj[0, 0] != 0, prj
        feat = [ids.index(int(ri)) for ri in prj[:, 0]]
        c = centers[kid][feat].astype(np.float64)
        assert np.array_equal(prj[:, 1:], c.astype(np.int64))                # the truncated ints of the plain getter
        want0 = ro.undistort_pixels(c, L, 1)
        want1 = ro.undistort_pixels(ro.from_matcher(c, rs.SCALE), L, rs.SCALE)
        for got, want in ((e["rows"][0], want0), (e["rows"][1], want1)):
            assert got.shape == want.shape
            err = float(np.abs(got - want).max())
            print(lens_name, "key frame", kid, "rows", len(prj), "max |device - oracle| =", err)
            assert err <= 1e-9
        assert float(np.abs(e["rows"][0] - c).max()) > 0.05                  # not the distorted centres
    # the rectified getters are reads: the plain ones still deliver what they delivered
    assert np.array_equal(sel.emitted_raw_image(), raws[6]) and np.array_equal(sel.emitted_image(), fi.ingest(raws[6], rs.SCALE))
    assert np.array_equal(sel.rectified_camera(True), g.rectifiedCamera(True)) and np.array_equal(sel.rectified_camera(), ro.camera(L, 1))
    sel.close()
    g.close()


def test_placeholder_row_and_error_paths(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    g = _filter(pkg, "barrel", features=True)
    img, rimg = np.zeros((rs.MH, rs.MW), np.uint8), np.zeros((rs.RH, rs.RW, 3), np.uint8)
    K, uv, n = pkg.capi.EkfSbaCamera(), np.zeros((4, 2)), C.c_int(-1)
    # ---- the filter, before any frame
    assert lib.ekf_get_frame_rectified(g._h, 0, P(img), img.strides[0]) == 4             # no frame
    assert lib.ekf_rectified_camera(g._h, 0, C.byref(K)) == 0
    assert lib.ekf_rectified_camera(g._h, 1, C.byref(K)) == 4                            # no raw geometry yet
    assert lib.ekf_undistort_pixels(g._h, 1, P(uv), 4, P(uv)) == 4
    assert lib.ekf_rectified_camera(g._h, 0, None) == 1 and lib.ekf_rectified_camera(g._h, 2, C.byref(K)) == 1
    assert lib.ekf_rectified_camera(None, 0, C.byref(K)) == 1
    assert lib.ekf_get_frame_rectified(g._h, 0, None, 64) == 1 and lib.ekf_get_frame_rectified(g._h, -1, P(img), 64) == 1
    assert lib.ekf_undistort_pixels(g._h, 0, None, 4, P(uv)) == 1 and lib.ekf_undistort_pixels(g._h, 0, P(uv), 4, None) == 1
    assert lib.ekf_undistort_pixels(g._h, 0, P(uv), -1, P(uv)) == 1 and lib.ekf_undistort_pixels(g._h, 3, P(uv), 4, P(uv)) == 1
    assert lib.ekf_undistort_pixels(g._h, 0, None, 0, None) == 0
    # ---- a plain selector of that filter, before an emit
    sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH)
    assert lib.ekf_keyframe_get_image_rectified(sel._h, 0, P(img), img.strides[0]) == 4
    assert lib.ekf_keyframe_get_emitted_rectified(sel._h, 0, 0, None, C.byref(n)) == 4
    assert lib.ekf_keyframe_get_image_rectified(None, 0, P(img), img.strides[0]) == 1
    assert lib.ekf_keyframe_get_image_rectified(sel._h, 0, None, img.strides[0]) == 1
    assert lib.ekf_keyframe_get_image_rectified(sel._h, 0, P(img), rs.MW - 1) == 1      # small stride
    assert lib.ekf_keyframe_get_image_rectified(sel._h, 2, P(img), img.strides[0]) == 1
    assert lib.ekf_keyframe_get_emitted_rectified(sel._h, 0, 2, None, C.byref(n)) == 1
    assert lib.ekf_keyframe_get_emitted_rectified(sel._h, 0, -1, P(uv), C.byref(n)) == 1
    assert lib.ekf_keyframe_get_emitted_rectified(sel._h, 5, 0, None, C.byref(n)) == 1
    # ---- frames 1 and 2 of the walk: EMIT_FIRST of the current frame, which carries the "0 0 0" placeholder
    frames = ks.scene_walk()
    for k, fr in enumerate(frames[:2]):
        g.setFrameRaw(rs.raw_image(100 + fr["id"]))
        _script(g, fr, k)
        r = sel.observe(fr["id"])
    assert r.action == ko.EMIT_FIRST and np.array_equal(r.record.projections, [[0, 0, 0]])
    assert lib.ekf_keyframe_get_emitted_rectified(sel._h, 0, 0, None, C.byref(n)) == 0 and n.value == 0
    assert sel.emitted_rows_rectified().shape == (0, 2)
    L = _lens(g)
    assert np.array_equal(sel.emitted_image_rectified(), ro.rectify_image(fi.ingest(rs.raw_image(102), rs.SCALE), L, 1))
    # a plain selector has no raw image and no raw geometry
    assert lib.ekf_keyframe_get_image_rectified(sel._h, 1, P(rimg), rimg.strides[0]) == 4
    assert lib.ekf_keyframe_get_emitted_rectified(sel._h, 1, 0, None, C.byref(n)) == 4
    # ---- the filter with a raw frame: small strides at either resolution
    assert lib.ekf_get_frame_rectified(g._h, 0, P(img), rs.MW - 1) == 1
    assert lib.ekf_get_frame_rectified(g._h, 1, P(rimg), rs.RW * 3 - 1) == 1
    assert lib.ekf_get_frame_rectified(g._h, 1, P(rimg), rimg.strides[0]) == 0
    assert lib.ekf_rectified_camera(g._h, 1, C.byref(K)) == 0 and K.fx == float(ro.camera(L, rs.SCALE)[0])
    sel.close()
    g.close()


def test_recorder_rectify_writes_pinhole_records_and_default_is_unchanged(pkg, tmp_path):
    """Three recorders over the same walk: built without the argument, with rectify=False and with rectify=True."""
    runs = {}
    for name, kw in (("plain", {}), ("off", {"rectify": False}), ("on", {"rectify": True})):
        g = _filter(pkg, "barrel", features=True)
        sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, keep_current_projections=True, raw_shape=(rs.RH, rs.RW, 3))
        rec = pkg.KeyframeRecorder(sel, str(tmp_path / name), images=True, **kw)
        rows, raws = {}, {}
        for k, fr in enumerate(ks.scene_walk()[:9]):
            raws[fr["id"]] = rs.raw_image(100 + fr["id"])
            g.setFrameRaw(raws[fr["id"]])
            _script(g, fr, k)
            r = rec.observe(fr["id"])
            if r.emitted:
                rows[r.record.id] = (r.record.projections, sel.emitted_rows_rectified(True))
        files = rec.finish()
        runs[name] = dict(rec=rec, files=files, rows=rows, raws=raws, K=g.rectifiedCamera(True), L=_lens(g))
        sel.close()
        g.close()
    plain, off, on = runs["plain"], runs["off"], runs["on"]
    assert plain["rec"].ids == off["rec"].ids == on["rec"].ids and len(on["rec"].ids) >= 3
    for d in (plain, off):
        assert sorted(os.listdir(d["rec"].directory)) == sorted(os.listdir(plain["rec"].directory))
        assert "camera.txt" not in os.listdir(d["rec"].directory)
    for fn in os.listdir(plain["rec"].directory):
        a = open(os.path.join(plain["rec"].directory, fn), "rb").read()
        assert a == open(os.path.join(off["rec"].directory, fn), "rb").read(), fn
    # rectify=True: same file names plus camera.txt; images and rows are the rectified ones at raw resolution
    assert sorted(os.listdir(on["rec"].directory)) == sorted(os.listdir(plain["rec"].directory) + ["camera.txt"])
    K = [float(t) for t in open(os.path.join(on["rec"].directory, "camera.txt")).read().split()]
    assert K == [float(v) for v in on["K"]]
    formats = pkg.formats
    records = formats.read_pose_records(on["files"][1])
    assert [r[0] for r in records] == on["rec"].ids
    moved = 0
    for kid, _, prj in records:
        base, uv = on["rows"][kid]
        want = base.copy()
        want[:, 1:] = ro.round_rows(uv)
        assert np.array_equal(prj, want), kid
        moved += int((prj != formats.read_pose_records(plain["files"][1])[on["rec"].ids.index(kid)][2]).any())
        data = open(os.path.join(on["rec"].directory, "%d.ppm" % kid), "rb").read()
        m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
        assert m and (int(m.group(1)), int(m.group(2))) == (rs.RW, rs.RH)
        rgb = np.frombuffer(data[m.end():], np.uint8).reshape(rs.RH, rs.RW, 3)
        assert np.array_equal(rgb[:, :, ::-1], ro.rectify_image(on["raws"][kid], on["L"], rs.SCALE)), kid
    assert moved >= 1
    for k in (0, 2):                                                         # points.txt and cams_cov.txt do not change
        assert open(on["files"][k], "rb").read() == open(plain["files"][k], "rb").read()
    # ... and sba_add reads the camera from the file
    out, nodes, ids = pkg.sba_add(*on["files"], camera=on["rec"].camera_path, every=3)
    assert ids == on["rec"].ids and len(nodes) == len(ids) and np.isfinite(nodes).all()


def test_bundle_adjuster_fits_the_rectified_rows(pkg):
    """tests/rectify_scene.sba_case: true poses and points, K(raw = 0) of the distorted camera.  Rows undistorted on the
    device and rounded to integers start at most 0.5 sqrt(2) px RMS from the truth, and LM accepts only decreases: the
    final RMS is <= 0.7072.  The distorted rows (the CPU test shows them to start above 4 px) must end above that."""
    case = rs.sba_case()
    cfg = dict(pkg.kinect_config(), image_width=640, image_height=480, scale=1,
               **{k: float(v) for k, v in rs.SBA_LENS.items()})
    g = pkg.VSlamFilter(cfg, capacity_features=4, dtype=np.float32)
    K = g.rectifiedCamera()
    assert np.array_equal(K, case["camera"])
    rect = g.undistortPixels(case["distorted"])
    g.close()
    assert float(np.abs(rect - case["pinhole"]).max()) <= 1e-9
    final = {}
    for name, rows in (("rectified", ro.round_rows(rect).astype(np.float64)), ("distorted", case["distorted"])):
        ba = pkg.BundleAdjuster(tuple(K), capacity_nodes=4, capacity_points=32, capacity_projections=64)
        ba.add_nodes(case["nodes"])
        ba.add_points(case["points"])
        assert ba.add_projections(case["node"], case["point"], rows) == len(rows)
        start = ba.rms_cost()
        ba.run(10, 1e-4)
        final[name] = ba.rms_cost()
        print(name, "rows: RMS at the true poses and points", start, "-> after doSBA(10)", final[name])
        ba.close()
    assert final["rectified"] <= 0.7072
    assert final["distorted"] > final["rectified"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_mirror_rectifies_key_frames(pkg, tmp_path):
    """examples/rectify_demo.cpp: VSlamFilterHip / KeyframeSelectorHip with the rectified getters; the demo checks the
    emitted rectified images against the filter's own and exits non-zero on a mismatch."""
    exe, src = str(tmp_path / "rectify_demo"), os.path.join(ROOT, "examples", "rectify_demo.cpp")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    rows = [tuple(int(t) for t in ln.split()) for ln in run.stdout.strip().splitlines()[:24]]
    assert len(rows) == 24 and sum(1 for r_ in rows if r_[2] >= 0) >= 3
