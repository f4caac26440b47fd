"""A raw key-frame selector (ekf_keyframe_create_raw) on the hand-built walk of tests/keyframe_scene.py: it
keeps the camera's own frame of the candidate and of the emitted key frame beside the matcher's grey one, decides exactly
as a plain selector does, and the recorder writes the raw frames as P6.  Every frame is a distinct random 40 x 30 x 3 image
at scale 2 (a 20 x 15 matcher frame)."""
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

pytestmark = pytest.mark.gpu

RAW_W, RAW_H, SCALE = 40, 30, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")
EMITS = (ko.EMIT_CURRENT, ko.EMIT_CANDIDATE, ko.EMIT_FIRST)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _raw_of(frame_id):
    return np.random.default_rng(5000 + int(frame_id)).integers(0, 256, size=(RAW_H, RAW_W, 3)).astype(np.uint8)


def _filter(pkg):
    """kc.scripted_filter for a 20 x 15 matcher frame: N_FEATURES features inside it (window 5), converted to XYZ where the
    linearity test allows after their rows of Sigma were shrunk, so that Point4sba rows exist."""
    cfg = dict(pkg.kinect_config(), image_width=RAW_W // SCALE, image_height=RAW_H // SCALE, scale=SCALE, window_size=5,
               fx=17.0, fy=17.0, u0=10.0, v0=7.5)
    g = pkg.VSlamFilter(cfg, capacity_features=32, dtype=np.float32)
    for i in range(ks.N_FEATURES):
        assert g.addFeature((4.0 + 2.0 * i, 4.0 + 1.0 * i)) == 1
    S = g.getFullSigma()
    n0 = g.camera_dim
    S[n0:, :] *= 1e-4
    S[:, n0:] *= 1e-4
    g.setSigmaBlock(S)
    g.convert2XYZ_ifLinearAll()
    return g


def _script(g, fr):
    mu = g.getFullState()
    mu[:7] = fr["pose"]
    g.setFullState(mu)
    g.setSigmaBlock(fr["sigma"].astype(g.dtype), 0, 0)
    for i in range(len(fr["centers"])):
        g.setFeatureTrack(i, in_innovation=int(fr["in_innovation"][i]), center=fr["centers"][i])


def _same_record(a, b):
    return (a.id == b.id and a.pose.tobytes() == b.pose.tobytes() and a.sigma.tobytes() == b.sigma.tobytes()
            and np.array_equal(a.projections, b.projections))


def test_walk_raw_selector_against_plain_twin(pkg, tmp_path):
    frames = ks.scene_walk()
    A, B = _filter(pkg), _filter(pkg)
    sel = pkg.KeyframeSelector(A, ks.MOVE_THRESH, raw_shape=(RAW_H, RAW_W, 3))
    twin = pkg.KeyframeSelector(B, ks.MOVE_THRESH)
    rec = pkg.KeyframeRecorder(sel, str(tmp_path / "raw"), images=True)
    rec_twin = pkg.KeyframeRecorder(twin, str(tmp_path / "plain"), images=True)
    raws, kinds, with_rows = {}, set(), 0
    for fr in frames:
        raw = raws[fr["id"]] = _raw_of(fr["id"])
        A.captureNewFrame(raw)
        B.setFrame(fi.ingest(raw, SCALE))
        _script(A, fr)
        _script(B, fr)
        r, t = rec.observe(fr["id"]), rec_twin.observe(fr["id"])
        kinds.add(r.action)
        assert r.action == t.action, (fr["id"], r.action_name, t.action_name)
        assert np.float32(r.dist).tobytes() == np.float32(t.dist).tobytes() and r.cov == t.cov
        assert r.emitted == (r.action in EMITS)
        if not r.emitted:
            continue
        assert _same_record(r.record, t.record), fr["id"]
        with_rows += int(r.record.projections[0, 0] != 0)
        kid = r.record.id
        if r.action == ko.EMIT_CANDIDATE:
            assert kid < fr["id"]                              # the candidate's frame, not the current one
        else:
            assert kid == fr["id"]
        assert np.array_equal(sel.emitted_raw_image(), raws[kid]), (fr["id"], kid)
        assert np.array_equal(sel.emitted_image(), fi.ingest(raws[kid], SCALE)), (fr["id"], kid)
        assert np.array_equal(twin.emitted_image(), sel.emitted_image())
    assert kinds == {ko.NONE, ko.CANDIDATE, ko.EMIT_CURRENT, ko.EMIT_CANDIDATE, ko.EMIT_FIRST}
    assert with_rows > 0, "no emitted record carries projections"
    assert sel.state()["candidate_id"] == twin.state()["candidate_id"]

    # the recorder: <id>.ppm decodes to the emitted raw frame (R and B swapped back); the text files are the plain recorder's
    assert rec.ids == rec_twin.ids and len(rec.ids) >= 4
    for kid in rec.ids:
        data = open(os.path.join(rec.directory, "%d.ppm" % kid), "rb").read()
        m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
        assert m and (int(m.group(1)), int(m.group(2))) == (RAW_W, RAW_H)
        rgb = np.frombuffer(data[m.end():], np.uint8).reshape(RAW_H, RAW_W, 3)
        assert np.array_equal(rgb[:, :, ::-1], raws[kid]), kid
        assert not os.path.exists(os.path.join(rec.directory, "%d.pgm" % kid))
        pgm = open(os.path.join(rec_twin.directory, "%d.pgm" % kid), "rb").read()
        assert pgm == b"P5\n%d %d\n255\n" % (RAW_W // SCALE, RAW_H // SCALE) + fi.ingest(raws[kid], SCALE).tobytes()
    for a, b in zip(rec.finish(), rec_twin.finish()):
        assert open(a, "rb").read() == open(b, "rb").read(), os.path.basename(a)
    for h in (sel, twin, A, B):
        h.close()


def test_one_channel_raw_selector_writes_pgm_at_raw_size(pkg, tmp_path):
    g = _filter(pkg)
    sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, raw_shape=(RAW_H, RAW_W))
    rec = pkg.KeyframeRecorder(sel, str(tmp_path / "raw1"), images=True)
    fr = ks.scene_walk()[1]                                    # EMIT_FIRST
    raw = _raw_of(fr["id"])[:, :, 1].copy()
    g.captureNewFrame(raw)
    _script(g, fr)
    r = rec.observe(fr["id"])
    assert r.action == ko.EMIT_FIRST
    assert np.array_equal(sel.emitted_raw_image(), raw) and np.array_equal(sel.emitted_image(), fi.ingest(raw, SCALE))
    data = open(os.path.join(rec.directory, "%d.pgm" % fr["id"]), "rb").read()
    assert data == b"P5\n%d %d\n255\n" % (RAW_W, RAW_H) + raw.tobytes()
    # a 3-channel frame of the same size is another geometry: the grey image is kept, the raw one is not
    fr2 = dict(ks.scene_walk()[1], id=3)
    fr2["pose"] = fr2["pose"].copy()
    fr2["pose"][0] *= 2
    g.captureNewFrame(_raw_of(3))
    _script(g, fr2)
    r = sel.observe(3)
    assert r.action == ko.EMIT_FIRST and np.array_equal(sel.emitted_image(), fi.ingest(_raw_of(3), SCALE))
    with pytest.raises(pkg.EkfError) as ei:
        sel.emitted_raw_image()
    assert ei.value.status == 4
    sel.close()
    g.close()


def _hip():
    """The HIP runtime the library itself has loaded (the process's own copy, found in its memory map)."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    return C.CDLL(path)


def _device_copy(a):
    hip, p = _hip(), C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0       # hipMemcpyHostToDevice
    return p.value


def test_failed_observe_stops_vouching_for_the_raw_images_too(pkg):
    """The failed-observe case of tests/test_gpu_keyframes.py (an update with a device-resident list that is not ascending)
    on a raw selector: the raw images are refused exactly as the grey ones are, the candidate's record is still emitted
    without either, and from the next candidate on both are there again."""
    I = ks._quat([0, 0, 1], 0.0)
    frames = ks.scene_walk()
    g = _filter(pkg)
    g.setDt(1.0 / 30.0)
    sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, raw_shape=(RAW_H, RAW_W, 3))

    def show(fr):
        g.captureNewFrame(_raw_of(fr["id"]))
        _script(g, fr)

    for fr in frames[:4]:
        show(fr)
        r = sel.observe(fr["id"])
    assert r.action == ko.CANDIDATE                          # frame 4; frame 2 was emitted (EMIT_FIRST)
    before = sel.state()
    assert sel.emitted().id == 2 and np.array_equal(sel.emitted_raw_image(), _raw_of(2))

    g.captureNewFrame(_raw_of(99))
    g.predict()
    d_z, d_bad = _device_copy(np.zeros(6, np.float32)), _device_copy(np.array([2, 1, 0], np.int32))
    g.update_device(d_z, d_bad, 3, False)
    with pytest.raises(pkg.EkfError) as ei:
        sel.observe(5)
    g.synchronize()
    _hip().hipFree(C.c_void_p(d_z))
    _hip().hipFree(C.c_void_p(d_bad))
    assert ei.value.status == 1 and "device-resident index" in str(ei.value)
    after = sel.state()
    assert before["min_cov"] == after["min_cov"] and before["candidate_id"] == after["candidate_id"] == 4
    assert sel.emitted().id == 2
    for read in (sel.emitted_raw_image, sel.emitted_image):
        with pytest.raises(pkg.EkfError) as ei:
            read()
        assert ei.value.status == 4

    show(ks._frame(7, [ks._x(39), 0, 0], I, 0.6, 6))
    r = sel.observe(7)
    assert r.action == ko.EMIT_CANDIDATE and r.record.id == 4
    for read in (sel.emitted_raw_image, sel.emitted_image):
        with pytest.raises(pkg.EkfError) as ei:
            read()
        assert ei.value.status == 4
    show(ks._frame(8, [ks._x(39), ks._x(11), 0], I, 0.4, 7))
    assert sel.observe(8).action == ko.CANDIDATE
    show(ks._frame(9, [ks._x(39), ks._x(20), 0], I, 0.7, 8))
    r = sel.observe(9)
    assert r.action == ko.EMIT_CANDIDATE and r.record.id == 8
    assert np.array_equal(sel.emitted_raw_image(), _raw_of(8))
    assert np.array_equal(sel.emitted_image(), fi.ingest(_raw_of(8), SCALE))
    sel.close()
    g.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_mirror_runs_the_chain_from_a_raw_frame(pkg, tmp_path):
    """examples/raw_frame_demo.cpp: VSlamFilterHip::captureNewFrame with pixels, a raw KeyframeSelectorHip; the demo checks
    every emitted raw and grey image itself and exits non-zero on a mismatch."""
    exe, src = str(tmp_path / "raw_frame_demo"), os.path.join(ROOT, "examples", "raw_frame_demo.cpp")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    rows = [tuple(int(t) for t in ln.split()) for ln in run.stdout.strip().splitlines()[:-1]]
    assert len(rows) == 24 and sum(1 for r_ in rows if r_[2] >= 0) >= 3
    assert any(r_[1] == ko.EMIT_CANDIDATE and r_[2] < r_[0] for r_ in rows)
