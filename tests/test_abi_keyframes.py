"""The key-frame part of the C ABI without a device: symbols, prototypes, argument checks, and the recorder's files
through `formats`.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry

NAMES = ["ekf_keyframe_create", "ekf_keyframe_destroy", "ekf_keyframe_set_option", "ekf_keyframe_observe",
         "ekf_keyframe_get_emitted", "ekf_keyframe_get_image", "ekf_keyframe_get_state", "ekf_keyframe_reset"]


@pytest.fixture(scope="module")
def pkg():
    entry.build()
    return entry.load_package()


def test_keyframe_symbols_are_declared_exported_and_prototyped(pkg):
    from ekf_monoslam_amd import capi
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in NAMES:
        assert name in declared and name in capi._PROTOS and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 6
    assert hasattr(pkg, "KeyframeSelector") and hasattr(pkg, "KeyframeRecorder")


def test_null_handles_are_rejected_without_a_device(pkg):
    lib = pkg.load_library()
    h = C.c_void_p(1234)
    a, d, c = C.c_int(7), C.c_float(0), C.c_float(0)
    assert lib.ekf_keyframe_create(None, 18.0, C.byref(h)) == 1 and not h.value
    assert lib.ekf_keyframe_create(None, 18.0, None) == 1
    assert b"ekf_keyframe_create" in lib.ekf_keyframe_last_error(None)
    assert lib.ekf_keyframe_set_option(None, 0, 1) == 1
    assert lib.ekf_keyframe_observe(None, None, 1, C.byref(a), C.byref(d), C.byref(c)) == 1 and a.value == 7
    assert lib.ekf_keyframe_get_emitted(None, None, None, None, 0, None, None) == 1
    buf = np.zeros(16, np.uint8)
    assert lib.ekf_keyframe_get_image(None, buf.ctypes.data_as(C.c_void_p), 4) == 1
    assert lib.ekf_keyframe_get_state(None, None, None, None, None) == 1
    assert lib.ekf_keyframe_reset(None) == 1
    lib.ekf_keyframe_destroy(None)


def test_recorder_files_round_trip_through_formats(pkg, tmp_path):
    """KeyframeRecorder.append writes what formats.read_pose_records / read_camera_covs read back."""
    from ekf_monoslam_amd import formats, keyframes
    rec = keyframes.KeyframeRecorder.__new__(keyframes.KeyframeRecorder)
    rec.directory = str(tmp_path)
    rec.nodes_path, rec.covs_path = str(tmp_path / "nodes_and_prjcts.txt"), str(tmp_path / "cams_cov.txt")
    rec.ids, rec.images = [], False
    rng = np.random.default_rng(3)
    want = []
    for kid, prj in ((2, np.zeros((1, 3), np.int64)), (9, np.array([[4, 11, 21], [5, 300, 22]], np.int64)),
                     (14, np.array([[7, 1, 2]], np.int64))):
        pose = rng.normal(size=7).astype(np.float32)
        A = rng.normal(size=(7, 7))
        sigma = (A @ A.T * 1e-3).astype(np.float32)
        rec.append(keyframes.KeyframeRecord(kid, pose, sigma, prj))
        want.append((kid, pose, sigma, prj))
    assert rec.ids == [2, 9, 14]
    recs = formats.read_pose_records(rec.nodes_path)
    covs = formats.read_camera_covs(rec.covs_path)
    assert len(recs) == 3 and covs.shape == (3, 7, 7)
    for (kid, pose, sigma, prj), (rid, rpose, rprj), rcov in zip(want, recs, covs):
        assert rid == kid and np.array_equal(rprj, prj)
        np.testing.assert_allclose(rpose, pose, rtol=1e-5, atol=0)                       # 6 significant digits
        np.testing.assert_allclose(rcov, sigma, rtol=1e-5, atol=0)
    img = (np.arange(12 * 7) % 251).astype(np.uint8).reshape(7, 12)
    keyframes.write_pgm(str(tmp_path / "9.pgm"), img)
    raw = open(tmp_path / "9.pgm", "rb").read()
    assert raw.startswith(b"P5\n12 7\n255\n") and raw[len(b"P5\n12 7\n255\n"):] == img.tobytes()
