"""The device key-frame selector (ekf_keyframe_*) against the numpy oracle tests/keyframe_oracle.py.

The bounds are 10 x the deviation measured on the MI355X over the scenes of tests/keyframe_scene.py, fp32 and fp64 filters
(tests/golden/keyframe_bounds.json: the figures, the bounds used here, the 100 x margins of tests/test_oracle_keyframes.py).
Measured: D differs from the oracle by at most 2.8e-5 (the device's acos / sin; 1.9e-6 on the hand-built walk, 0 on the
first-frames scene); last_vrot by at most 2.4e-7 rad; c, the pose and the 7 x 7 block are bit-equal, so their bounds are 0.
tools/keyframe_bounds.py measures and rewrites the file."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import keyframe_gpu_common as kc
import keyframe_oracle as ko
import keyframe_scene as ks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("scene", sorted(ks.SCENES))
def test_scripted_scene_matches_oracle(pkg, scene, dtype):
    """Every frame: action, emitted id, projection rows and the emitted image exactly; D, c, pose and the 7 x 7 block within
    10 x the deviation measured on the MI355X."""
    frames = ks.SCENES[scene]()
    dev, ref, worst, sel, g = kc.run_scripted(pkg, frames, dtype, images=True)
    print(scene, np.dtype(dtype).name, "largest deviations:", worst)
    kc.assert_scene(dev, ref, kc.load_bounds()["bound"], images=True)
    want = ks.run_oracle(frames)[0].state()
    got = sel.state()
    assert got["candidate_id"] == want["candidate_id"] and got["min_cov"] == want["min_cov"]
    b = kc.load_bounds()["bound"]
    assert float(np.abs(got["last_pose"] - want["last_pose"]).max()) <= b["pose"]
    assert float(np.abs(got["last_vrot"] - want["last_vrot"]).max()) <= b["vrot"]
    sel.close()
    g.close()


def test_walk_scene_reaches_every_action_on_the_device(pkg):
    dev, ref, _, sel, g = kc.run_scripted(pkg, ks.scene_walk(), np.float32)
    assert {r.action for r, _ in dev} == {ko.NONE, ko.CANDIDATE, ko.EMIT_CURRENT, ko.EMIT_CANDIDATE, ko.EMIT_FIRST}
    assert any(r.emitted and r.record.projections[0, 0] != 0 for r, _ in dev), "no emitted record carries projections"
    sel.close()
    g.close()


def test_two_runs_are_identical_and_reset_restores_the_initial_state(pkg):
    frames = ks.scene_random(seed=11, frames=60)
    a, _, _, sel, g = kc.run_scripted(pkg, frames, np.float32, images=True)

    def flat(run):
        out = []
        for r, img in run:
            out.append((r.action, np.float32(r.dist).tobytes(), np.float32(r.cov).tobytes()))
            if r.emitted:
                out.append((r.record.id, r.record.pose.tobytes(), r.record.sigma.tobytes(), r.record.projections.tobytes(),
                            img.tobytes()))
        return out

    b, _, _, sel2, g2 = kc.run_scripted(pkg, frames, np.float32, images=True)
    assert flat(a) == flat(b)
    # reset: the initial state, and the same stream again gives the same records on the SAME selector
    sel.reset()
    st = sel.state()
    assert st["min_cov"] == 1e7 and st["candidate_id"] == 0 and not st["last_pose"].any() and not st["last_vrot"].any()
    with pytest.raises(pkg.EkfError) as ei:
        sel.emitted()
    assert ei.value.status == 4
    c, _, _, _, _ = kc.run_scripted(pkg, frames, np.float32, images=True, selector=sel, filt=g)
    assert flat(a) == flat(c)
    for h in (sel, sel2, g, g2):
        h.close()


def test_keep_current_projections_changes_only_current_emits(pkg):
    frames = ks.scene_walk()
    a, ra, _, s1, g1 = kc.run_scripted(pkg, frames, np.float32)
    b, rb, _, s2, g2 = kc.run_scripted(pkg, frames, np.float32, keep=True)
    kc.assert_scene(b, rb, kc.load_bounds()["bound"])
    changed = 0
    for (x, _), (y, _) in zip(a, b):
        assert x.action == y.action and x.cov == y.cov
        assert np.float32(x.dist).tobytes() == np.float32(y.dist).tobytes()          # (the NaN frame included)
        if not x.emitted:
            continue
        assert x.record.id == y.record.id and np.array_equal(x.record.pose, y.record.pose)
        assert np.array_equal(x.record.sigma, y.record.sigma)
        if x.action == ko.EMIT_CANDIDATE:
            assert np.array_equal(x.record.projections, y.record.projections)
        else:
            assert np.array_equal(x.record.projections, [[0, 0, 0]])
            changed += int(not np.array_equal(x.record.projections, y.record.projections))
    assert changed > 0
    for h in (s1, s2, g1, g2):
        h.close()


def test_argument_errors_and_sharded_handle(pkg):
    lib = pkg.load_library()
    g = kc.scripted_filter(pkg, np.float32, ks.scene_walk()[0])
    other = kc.scripted_filter(pkg, np.float32, ks.scene_walk()[0])
    h = C.c_void_p()
    assert lib.ekf_keyframe_create(g._h, 0.0, C.byref(h)) == 1 and not h.value
    assert lib.ekf_keyframe_create(g._h, float("nan"), C.byref(h)) == 1
    sel = pkg.KeyframeSelector(g)
    a = C.c_int(0)
    assert lib.ekf_keyframe_observe(sel._h, g._h, -1, C.byref(a), None, None) == 1
    assert lib.ekf_keyframe_observe(sel._h, g._h, 1, None, None, None) == 1
    assert lib.ekf_keyframe_observe(sel._h, other._h, 1, C.byref(a), None, None) == 1
    assert lib.ekf_keyframe_set_option(sel._h, 5, 1) == 1 and lib.ekf_keyframe_set_option(sel._h, 0, 2) == 1
    assert lib.ekf_keyframe_get_emitted(sel._h, None, None, None, -1, None, None) == 1
    assert lib.ekf_keyframe_get_emitted(sel._h, None, None, None, 0, None, None) == 4          # nothing emitted yet
    buf = np.zeros(sel.image_shape, np.uint8)
    assert lib.ekf_keyframe_get_image(sel._h, buf.ctypes.data_as(C.c_void_p), sel.image_shape[1] - 1) == 1
    assert lib.ekf_keyframe_get_image(sel._h, buf.ctypes.data_as(C.c_void_p), sel.image_shape[1]) == 4
    # an emit without a frame ever set: the record is there, the image is EKF_ERR_STATE
    mu = g.getFullState()
    mu[:7] = [6.0, 0, 0, 1, 0, 0, 0]
    g.setFullState(mu)
    r = sel.observe(2)
    assert r.action == ko.EMIT_FIRST and r.record.id == 2
    with pytest.raises(pkg.EkfError) as ei:
        sel.emitted_image()
    assert ei.value.status == 4
    # a sharded handle is refused, at create and at observe, with a message
    assert lib.ekf_shard_configure(other._h, 0, 1, None, None) == 0
    assert lib.ekf_keyframe_create(other._h, 18.0, C.byref(h)) == 4 and not h.value
    assert b"sharded" in lib.ekf_keyframe_last_error(None)
    assert lib.ekf_shard_configure(g._h, 0, 1, None, None) == 0
    with pytest.raises(pkg.EkfError) as ei:
        sel.observe(3)
    assert ei.value.status == 4 and "sharded" in str(ei.value)
    for h_ in (sel, g, other):
        h_.close()


def _show(g, sel, fr, image_id=None):
    """One scripted frame into the filter as run_scripted does it, with an image that names `image_id`."""
    mu = g.getFullState()
    mu[:7] = fr["pose"]
    g.setFullState(mu)
    g.setSigmaBlock(fr["sigma"].astype(g.dtype), 0, 0)
    img = kc.image_of(fr["id"] if image_id is None else image_id, sel.image_shape)
    g.setFrame(img)
    return img


def test_observe_folds_the_track_flags_a_predict_left_unread(pkg):
    """After a predict the visibility flags are still on the device; observe reads them in its own round trip and builds
    the emitted rows from them.  A first predict tells which features are visible; the host's flags are then set to the
    opposite, so rows built without folding the second predict's flags differ from the rows the filter's own builder
    gives afterwards, whatever the predict finds visible."""
    g = kc.scripted_filter(pkg, np.float32, ks.scene_walk()[0])
    g.setDt(1.0 / 30.0)
    sel = pkg.KeyframeSelector(g, 0.001, keep_current_projections=True)
    mu = g.getFullState()
    mu[:7] = [0.001, 0, 0, 1, 0, 0, 0]                      # D = 0.00333 >= move_thresh
    g.setFullState(mu)
    g.predict()
    vis = g.featureTrack()[1]
    for i in range(ks.N_FEATURES):
        g.setFeatureTrack(i, in_innovation=int(not vis[i]))
    stale = g.keyframeProjections()
    g.predict()
    r = sel.observe(2)                                      # (nothing read the filter between the predict and this)
    assert r.action == ko.EMIT_FIRST and r.record.id == 2
    want = g.keyframeProjections()
    assert np.array_equal(g.featureTrack()[1], vis)
    assert not np.array_equal(stale, want), "no converted feature: the scene shows nothing"
    assert np.array_equal(r.record.projections, want)
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


def test_failed_observe_keeps_the_rule_and_stops_vouching_for_the_images(pkg):
    """An update with a device-resident list that is not ascending raises the status word on the device; the observe
    behind it is the first call to read it and fails with EKF_ERR_ARG.  The rule's state and the last record are what
    they were, but the image launch ran on a record nobody read: the stored images are refused (EKF_ERR_STATE) rather
    than paired with an id they may not belong to, the candidate's record is still emitted, and the selector goes on."""
    I = ks._quat([0, 0, 1], 0.0)
    frames = ks.scene_walk()
    g = kc.scripted_filter(pkg, np.float32, frames[0])
    g.setDt(1.0 / 30.0)
    sel = pkg.KeyframeSelector(g)
    imgs = {}
    for fr in frames[:4]:
        imgs[fr["id"]] = _show(g, sel, fr)
        r = sel.observe(fr["id"])
    assert r.action == ko.CANDIDATE                          # frame 4; frame 2 was emitted (EMIT_FIRST)
    before, rec = sel.state(), sel.emitted()
    assert rec.id == 2 and np.array_equal(sel.emitted_image(), imgs[2])

    g.setFrame(kc.image_of(99, sel.image_shape))
    g.predict()
    d_z, d_bad = _device_copy(np.zeros(6, np.float32)), _device_copy(np.array([2, 1, 0], np.int32))
    g.update_device(d_z, d_bad, 3, False)
    with pytest.raises(pkg.EkfError) as ei:
        sel.observe(5)
    g.synchronize()
    _hip().hipFree(C.c_void_p(d_z))
    _hip().hipFree(C.c_void_p(d_bad))
    assert ei.value.status == 1 and "device-resident index" in str(ei.value)
    after, rec2 = sel.state(), sel.emitted()
    for k in ("last_pose", "last_vrot"):
        assert before[k].tobytes() == after[k].tobytes()
    assert before["min_cov"] == after["min_cov"] and before["candidate_id"] == after["candidate_id"] == 4
    assert rec2.id == 2 and np.array_equal(rec2.pose, rec.pose) and np.array_equal(rec2.sigma, rec.sigma)
    with pytest.raises(pkg.EkfError) as ei:
        sel.emitted_image()
    assert ei.value.status == 4

    # the candidate stored before the failure is still emitted, without an image
    _show(g, sel, ks._frame(7, [ks._x(39), 0, 0], I, 0.6, 6))
    r = sel.observe(7)
    assert r.action == ko.EMIT_CANDIDATE and r.record.id == 4
    assert np.array_equal(r.record.pose, frames[3]["pose"]) and np.array_equal(r.record.sigma, frames[3]["sigma"])
    with pytest.raises(pkg.EkfError) as ei:
        sel.emitted_image()
    assert ei.value.status == 4
    # ... and from the next candidate on the images are there again
    imgs[8] = _show(g, sel, ks._frame(8, [ks._x(39), ks._x(11), 0], I, 0.4, 7))
    assert sel.observe(8).action == ko.CANDIDATE
    _show(g, sel, ks._frame(9, [ks._x(39), ks._x(20), 0], I, 0.7, 8))
    r = sel.observe(9)
    assert r.action == ko.EMIT_CANDIDATE and r.record.id == 8 and np.array_equal(sel.emitted_image(), imgs[8])
    sel.close()
    g.close()


# ---- a real filter stream: the image stream of test_gpu_end_update.py ------------------------------------------------
STREAM_FRAMES = 40


def _stream_filter(pkg):
    import ekf_oracle as o
    import test_gpu_end_update as ge
    cfg = ge._stream_config()
    ref = o.StructuredFilter(o.Config.kinect(), np.float64)
    g = pkg.VSlamFilter(cfg, capacity_features=128, dtype=np.float64)
    g.setDt(1.0 / 30.0)
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    world = ge._stream_world()
    g.setFrame(ge._stream_frame(world, 0))
    g.findNewFeatures(-1)
    return g, world, cfg


def _stream_step(g, world, f):
    """One frame as test_filter_stream_keyframes_to_sba_add runs it (conversions to XYZ forced); returns the frame."""
    import test_gpu_end_update as ge
    frame = ge._stream_frame(world, f)
    ge._device_frame(g, frame, False)
    pos, cod = g.featureLayout()
    S = g.getFullSigma()
    for i in [i for i in range(len(cod)) if cod[i] == 0][:4]:
        p = int(pos[i])
        S[p:p + 6, :] *= 1e-4
        S[:, p:p + 6] *= 1e-4
    g.setSigmaBlock(S)
    g.convert2XYZ_ifLinearAll()
    return frame


def _choose_move_thresh(poses, sigmas, margin):
    """On the CPU, from the stream's own poses and blocks: the first threshold of a fixed ladder for which the oracle
    selects at least 4 key frames, both kinds of emit occur (the current frame and the stored candidate) and every
    decision keeps the committed margins."""
    for t in np.geomspace(0.02, 20.0, 61):
        sel = ko.Selector(float(t))
        res = [sel.observe(f + 1, poses[f], sigmas[f]) for f in range(len(poses))]
        acts = [r["action"] for r in res]
        emits = [a for a in acts if a in kc.EMITS]
        if len(emits) >= 4 and ko.EMIT_CANDIDATE in emits and (ko.EMIT_CURRENT in emits or ko.EMIT_FIRST in emits) and \
                not ko.margin_violations(sel.margins, margin["D"], margin["c"]):
            return float(t)
    return None


def test_real_stream_recorder_to_sba_add(pkg, tmp_path):
    """Pass 1 runs the stream without a selector and keeps each frame's pose and block; the oracle chooses move_thresh from
    them on the CPU.  Pass 2 runs the same stream with a KeyframeRecorder: the selector makes the oracle's decisions, the
    emitted images are the frames that were set when their ids were observed (the candidate's is older than the current
    one), sba_add runs on the recorder's files and returns the selected ids.  The filter's state, Sigma and launch
    counters of pass 2 are bitwise those of pass 1: observe changes nothing in the filter."""
    g, world, cfg = _stream_filter(pkg)
    poses, sigmas = [], []
    for f in range(1, STREAM_FRAMES + 1):
        _stream_step(g, world, f)
        poses.append(g.getFullState()[:7])
        sigmas.append(g.getSigmaBlock(0, 0, 7, 7))
    mu1, S1, lc1 = g.getFullState(), g.getFullSigma(), g.launch_counts()
    g.close()
    thresh = _choose_move_thresh(poses, sigmas, kc.load_bounds()["margin"])
    print("move_thresh chosen by the oracle:", thresh)
    assert thresh is not None, "no threshold of the ladder gives 4 key frames with both kinds of emit"
    ora = ko.Selector(thresh)
    bound = kc.load_bounds()["bound"]

    g, world, cfg = _stream_filter(pkg)
    sel = pkg.KeyframeSelector(g, thresh)
    rec = pkg.KeyframeRecorder(sel, str(tmp_path / "kf"), images=True)
    shown, kinds = {}, set()
    for f in range(1, STREAM_FRAMES + 1):
        shown[f] = _stream_step(g, world, f)
        prj = g.keyframeProjections()
        o = ora.observe(f, poses[f - 1], sigmas[f - 1], prj)
        r = rec.observe(f)
        assert r.action == o["action"], (f, r.action_name, ko.ACTION_NAMES[o["action"]], r.dist, float(o["dist"]))
        if r.emitted:
            kinds.add(r.action)
            assert r.record.id == o["id"] and np.array_equal(r.record.projections, o["projections"]), f
            # the pose and the block of the frame with that id, as pass 1 read them (a real Sigma: not exactly symmetric)
            want_pose = poses[r.record.id - 1].astype(np.float32)
            want_sig = sigmas[r.record.id - 1].astype(np.float32)
            assert float(np.abs(r.record.pose - want_pose).max()) <= bound["pose"], (f, r.record.id)
            assert float(np.abs(r.record.sigma - want_sig).max()) <= bound["sigma"], (f, r.record.id)
            assert np.array_equal(sel.emitted_image(), shown[r.record.id]), (f, r.record.id)
            if r.action == ko.EMIT_CANDIDATE:
                assert r.record.id < f
            pgm = open(os.path.join(rec.directory, "%d.pgm" % r.record.id), "rb").read()
            assert pgm.endswith(shown[r.record.id].tobytes())
    mu2, S2, lc2 = g.getFullState(), g.getFullSigma(), g.launch_counts()
    assert mu1.tobytes() == mu2.tobytes() and S1.tobytes() == S2.tobytes() and lc1 == lc2
    assert len(rec.ids) >= 4 and ko.EMIT_CANDIDATE in kinds and (kinds - {ko.EMIT_CANDIDATE}), (rec.ids, kinds)
    files = rec.finish()
    sel.close()
    g.close()
    cam = (cfg["fx"], cfg["fy"], cfg["u0"], cfg["v0"])
    out, nodes, ids = pkg.sba_add(*files, camera=cam, every=3)
    print("key frames:", rec.ids, "kinds:", sorted(kinds), "nodes", nodes.shape, "points", out.shape)
    assert ids == rec.ids and len(nodes) == len(ids)


# ---- the C++ mirror ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_demo_prints_the_python_selectors_ids(pkg, tmp_path):
    exe, src = str(tmp_path / "keyframe_demo"), os.path.join(ROOT, "examples", "keyframe_demo.cpp")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    frames = ks.scene_walk() + [dict(fr, id=fr["id"] + 100) for fr in ks.scene_random(seed=5, frames=40)]
    with open(tmp_path / "stream.txt", "w") as fh:
        for fr in frames:
            fh.write("%d %s %s\n" % (fr["id"], " ".join("%.9g" % v for v in fr["pose"]),
                                     " ".join("%.9g" % v for v in fr["sigma"].reshape(-1))))
    run = subprocess.run([exe, str(tmp_path / "stream.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    got = [tuple(int(t) for t in ln.split()) for ln in run.stdout.strip().splitlines()[:-1]]
    # the Python selector on the same stream (a filter without features: every emit carries the 0 0 0 row, as in the demo)
    g = pkg.VSlamFilter(None, capacity_features=16, dtype=np.float32)
    sel = pkg.KeyframeSelector(g)
    want = []
    for fr in frames:
        g.setStateSegment(0, fr["pose"])
        g.setSigmaBlock(fr["sigma"], 0, 0)
        r = sel.observe(fr["id"])
        want.append((fr["id"], r.action, r.record.id if r.emitted else -1))
    assert got == want
    # ... and both are the oracle's selection
    ora = ko.Selector(ks.MOVE_THRESH)
    ref = [ora.observe(fr["id"], fr["pose"], fr["sigma"]) for fr in frames]
    assert [(w[1], w[2]) for w in want] == [(o["action"], o.get("id", -1) if o["action"] in kc.EMITS else -1) for o in ref]
    assert sum(1 for w in want if w[2] >= 0) >= 3
    sel.close()
    g.close()
