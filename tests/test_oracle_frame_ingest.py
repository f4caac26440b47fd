"""DESIGN.md §13 without a device: known answers of the pinned resize / grey arithmetic worked by hand, the properties of
the coefficient tables, the new entry points of the C ABI (symbols, prototypes, argument checks that touch no device) and
the recorder's P6 / P5 writer.  CPU only."""
import ctypes as C
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import frame_ingest_oracle as fi

NEW_SYMBOLS = ["ekf_set_frame_raw", "ekf_set_frame_raw_device", "ekf_get_frame", "ekf_keyframe_create_raw",
               "ekf_keyframe_get_raw_image"]
# (raw W, raw H, s): the parity shapes of tests/test_gpu_frame_ingest.py
SHAPES = [(64, 48, 1), (64, 48, 2), (66, 50, 2), (65, 48, 2), (64, 49, 2), (99, 66, 3), (101, 67, 3), (320, 240, 10),
          (327, 243, 10), (1280, 960, 10)]


@pytest.fixture(scope="module")
def pkg():
    entry.build()
    return entry.load_package()


# ---- known answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,s", [sh for sh in SHAPES if sh[0] < 1000])
def test_constant_image_stays_constant(W, H, s):
    for v in (0, 1, 127, 200, 255):
        assert np.all(fi.ingest(np.full((H, W), v, np.uint8), s) == v)
        assert np.all(fi.ingest(np.full((H, W, 3), v, np.uint8), s) == v)
    assert fi.ingest(np.zeros((H, W), np.uint8), s).shape == (H // s, W // s)


def test_grey_weights():
    px = lambda b, g, r: int(fi.gray(np.array([[[b, g, r]]], np.uint8))[0, 0])
    assert (px(255, 0, 0), px(0, 255, 0), px(0, 0, 255)) == (29, 150, 76)
    assert px(255, 255, 255) == 255 and px(0, 0, 0) == 0
    assert fi.B2Y + fi.G2Y + fi.R2Y == 1 << fi.GRAY_SHIFT
    # the colour order is B, G, R: swapping the outer channels changes the answer
    assert px(10, 20, 200) == (10 * 1868 + 20 * 9617 + 200 * 4899 + 8192) >> 14 != px(200, 20, 10)


def test_odd_factor_is_a_point_sample():
    """s = 3: fx = 3 dx + 1 exactly, a1 = 0: the output is the source at (3 dx + 1, 3 dy + 1)."""
    H, W = 12, 18
    ramp = (np.arange(W)[None, :] * 7 + np.arange(H)[:, None] * 13).astype(np.uint8)
    assert fi.mode(W, H, 3) == "linear"
    assert np.array_equal(fi.resize_channel(ramp, 3), ramp[1::3, 1::3])
    sx, _, a0, a1, _ = fi.tables(W, H, 3)["x"]
    assert np.array_equal(sx, 3 * np.arange(W // 3) + 1) and np.all(a0 == 2048) and np.all(a1 == 0)


def test_factor_ten_is_the_central_two_by_two():
    """s = 10 on a hand-filled 20 x 20 patch: taps at (10 d + 4, 10 d + 5) with a0 = a1 = b0 = b1 = 1024."""
    S = np.zeros((20, 20), np.uint8)
    S[:] = 99                                              # everything but the taps: must not matter
    blocks = {(0, 0): [[10, 20], [30, 41]], (0, 1): [[255, 255], [255, 254]], (1, 0): [[0, 1], [0, 0]],
              (1, 1): [[7, 200], [7, 200]]}
    for (dy, dx), b in blocks.items():
        S[10 * dy + 4:10 * dy + 6, 10 * dx + 4:10 * dx + 6] = b
    got = fi.resize_channel(S, 10)
    assert got.shape == (2, 2)
    for (dy, dx), b in blocks.items():
        r0, r1 = (b[0][0] + b[0][1]) * 1024, (b[1][0] + b[1][1]) * 1024
        want = (((1024 * (r0 >> 4)) >> 16) + ((1024 * (r1 >> 4)) >> 16) + 2) >> 2
        assert got[dy, dx] == want, (dy, dx)
    # the block with two equal rows, in the form with one r: (((1024 (r >> 4)) >> 16) 2 + 2) >> 2
    r = (7 + 200) * 1024
    assert got[1, 1] == (((1024 * (r >> 4)) >> 16) * 2 + 2) >> 2 == 104          # (207 + 207 + 2) >> 2
    assert (got[0, 0], got[0, 1], got[1, 0]) == (25, 255, 0)                      # 103 >> 2, 1021 >> 2, 3 >> 2


def test_exact_half_is_the_rounded_block_mean():
    """W = 2 W' and H = 2 H': (p00 + p01 + p10 + p11 + 2) >> 2, halves rounded up.  The block (1, 1, 0, 0) has mean 0.5:
    the area path gives 1 where a float bilinear sample rounded half to even gives 0.  In §13's own fixed point the linear
    formula at a0 = a1 = b0 = b1 = 1024 is exact and agrees with the area path for every block (checked here for every pair
    of row sums), so which of the two paths an exact factor of 2 takes cannot show in the output."""
    S = np.array([[1, 1, 9, 9, 255, 254, 3, 0],
                  [0, 0, 9, 9, 255, 255, 0, 0]], np.uint8)
    assert fi.mode(8, 2, 2) == "area2"
    assert fi.resize_channel(S, 2).tolist() == [[1, 9, 255, 1]]
    assert int(np.rint(np.float32(0.5))) == 0                                   # the float route would say 0
    s0, s1 = np.meshgrid(np.arange(511), np.arange(511))
    lin = (((1024 * ((s0 * 1024) >> 4)) >> 16) + ((1024 * ((s1 * 1024) >> 4)) >> 16) + 2) >> 2
    assert np.array_equal(lin, (s0 + s1 + 2) >> 2)


def test_inexact_half_takes_the_linear_path():
    assert fi.mode(65, 48, 2) == "linear" and fi.mode(64, 49, 2) == "linear" and fi.mode(66, 50, 2) == "area2"
    assert fi.mode(64, 48, 1) == "copy"
    rng = np.random.default_rng(1)
    S = rng.integers(0, 256, size=(48, 65)).astype(np.uint8)
    t = fi.tables(65, 48, 2)
    sx, sx1, a0, a1, _ = t["x"]
    # column 5 by hand: scale_x = 65 / 32, fx = 5.5 * 2.03125 - 0.5 = 10.671875 -> sx = 10, a1 = rint(0.671875 * 2048) = 1376
    assert (sx[5], sx1[5], a0[5], a1[5]) == (10, 11, 672, 1376)
    got = fi.resize_channel(S, 2)
    sy0, sy1, b0, b1, _ = t["y"]
    assert (sy0[7], sy1[7], b0[7], b1[7]) == (14, 15, 1024, 1024)              # scale_y = 2 exactly
    r0 = int(S[14, 10]) * 672 + int(S[14, 11]) * 1376
    r1 = int(S[15, 10]) * 672 + int(S[15, 11]) * 1376
    assert got[7, 5] == (((1024 * (r0 >> 4)) >> 16) + ((1024 * (r1 >> 4)) >> 16) + 2) >> 2


def test_replication_is_inverted_by_every_path():
    g = np.random.default_rng(2).integers(0, 256, size=(6, 9)).astype(np.uint8)
    for s in (1, 2, 3, 4, 10):
        assert np.array_equal(fi.ingest(fi.replicate(g, s), s), g)
        assert np.array_equal(fi.ingest(fi.replicate(g, s, 3), s), g)


# ---- tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,s", SHAPES)
def test_table_weights_sum_to_one_and_no_clamp_from_factor_two(W, H, s):
    t = fi.tables(W, H, s)
    for key, n_src in (("x", W), ("y", H)):
        i0, i1, w0, w1, clamped = t[key]
        assert np.all(w0 + w1 == fi.COEF_ONE), key
        assert np.all(w0 >= 0) and np.all(w1 >= 0)
        assert np.all(i0 >= 0) and np.all(i1 <= n_src - 1)
        if s >= 2:
            assert not clamped.any(), key
            assert np.all(i1 == i0 + 1) and i0.max() <= n_src - 2, key


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def _declared_arity(name):
    text = re.sub(r"/\*.*?\*/", "", open(entry.load_package().capi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), text)
    assert m, name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def test_new_symbols_are_declared_exported_and_prototyped(pkg):
    """Fails on the parent commit: none of the five exists there."""
    from ekf_monoslam_amd import capi
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in capi._PROTOS and hasattr(lib, name), name
        res, args = capi._PROTOS[name]
        assert res is C.c_int and len(args) == _declared_arity(name), name
    assert lib.ekf_abi_version() == 6
    assert capi._PROTOS["ekf_set_frame_raw"][1][2:] == [C.c_int] * 4
    assert capi._PROTOS["ekf_set_frame_raw_device"][1] == capi._PROTOS["ekf_set_frame_raw"][1]
    assert capi._PROTOS["ekf_keyframe_create_raw"][1][1:5] == [C.c_float, C.c_int, C.c_int, C.c_int]
    assert hasattr(pkg.VSlamFilter, "getFrame") and hasattr(pkg.VSlamFilter, "setFrameRaw")
    assert hasattr(pkg.KeyframeSelector, "emitted_raw_image")
    names = [lib.ekf_profile_kernel_name(k).decode() for k in range(lib.ekf_profile_kernels())]
    assert "frame_upload" in names and "frame_ingest" in names


def test_null_handles_are_rejected_without_a_device(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.ekf_set_frame_raw(None, p, 4, 4, 1, 4) == 1
    assert lib.ekf_set_frame_raw_device(None, p, 4, 4, 1, 4) == 1
    assert lib.ekf_get_frame(None, p, 4) == 1
    assert lib.ekf_keyframe_get_raw_image(None, p, 4) == 1
    h = C.c_void_p(1234)
    assert lib.ekf_keyframe_create_raw(None, 18.0, 4, 4, 3, C.byref(h)) == 1 and not h.value
    assert lib.ekf_keyframe_create_raw(None, 18.0, 4, 4, 3, None) == 1
    h = C.c_void_p(1234)
    assert lib.ekf_keyframe_create_raw(None, 18.0, 4, 4, 2, C.byref(h)) == 1 and not h.value
    assert b"ekf_keyframe_create_raw" in lib.ekf_keyframe_last_error(None)


# ---- the recorder's writers ------------------------------------------------------------------------------------------
def _read_pnm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"(P[56])\n(\d+) (\d+)\n255\n", raw)
    assert m, raw[:20]
    w, h = int(m.group(2)), int(m.group(3))
    ch = 3 if m.group(1) == b"P6" else 1
    body = np.frombuffer(raw[m.end():], np.uint8)
    assert body.size == w * h * ch
    return m.group(1), body.reshape(h, w, ch) if ch == 3 else body.reshape(h, w)


def test_recorder_writers_round_trip(pkg, tmp_path):
    from ekf_monoslam_amd import keyframes
    bgr = np.random.default_rng(4).integers(0, 256, size=(7, 12, 3)).astype(np.uint8)
    bgr[0, 0] = (1, 2, 3)                                  # B, G, R
    keyframes.write_ppm(str(tmp_path / "5.ppm"), bgr)
    magic, rgb = _read_pnm(tmp_path / "5.ppm")
    assert magic == b"P6" and rgb.shape == (7, 12, 3)
    assert tuple(rgb[0, 0]) == (3, 2, 1)                   # R, G, B in the file
    assert np.array_equal(rgb[:, :, ::-1], bgr)
    assert open(tmp_path / "5.ppm", "rb").read().startswith(b"P6\n12 7\n255\n")
    keyframes.write_pgm(str(tmp_path / "5.pgm"), bgr[:, :, 1])
    magic, g = _read_pnm(tmp_path / "5.pgm")
    assert magic == b"P5" and np.array_equal(g, bgr[:, :, 1])
    with pytest.raises(ValueError):
        keyframes.write_ppm(str(tmp_path / "bad.ppm"), bgr[:, :, 0])
