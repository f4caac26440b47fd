"""k_frame_ingest through ekf_set_frame_raw / ekf_set_frame_raw_device / ekf_get_frame against the numpy
restatement tests/frame_ingest_oracle.py.  Every comparison is bit-exact: the arithmetic is integer.

The launch is capped at 1024 workgroups of 256 lanes, so the 1280 x 960 x 3, s = 10 frame (12288 output pixels) is still one
pass of the grid-stride loop; LOOP_SHAPES adds one frame per path that is large enough to go round the loop."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_ingest_oracle as fi

pytestmark = pytest.mark.gpu

# raw W, raw H, s: copy / area (vector-wide and not) / x-inexact / y-inexact / odd factor / non-dividing / the reference's factor
SHAPES = [(64, 48, 1), (64, 48, 2), (66, 50, 2), (65, 48, 2), (64, 49, 2), (99, 66, 3), (101, 67, 3), (320, 240, 10),
          (327, 243, 10)]
# raw W, raw H, s, C: more lanes than 1024 x 256 on the copy, the area and the linear path
LOOP_SHAPES = [(1280, 960, 1, 3), (2560, 1920, 2, 1), (1283, 962, 2, 3)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _config(pkg, W, H, s):
    return dict(pkg.kinect_config(), image_width=W // s, image_height=H // s, scale=s)


def _filter(pkg, W, H, s, capacity=8):
    return pkg.VSlamFilter(_config(pkg, W, H, s), capacity_features=capacity, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _case(W, H, s, channels):
    """(raw frame, the oracle's matcher frame), computed once per shape and left unchanged."""
    rng = np.random.default_rng(1000 * W + 10 * H + s + channels)
    raw = rng.integers(0, 256, size=(H, W) if channels == 1 else (H, W, 3)).astype(np.uint8)
    want = fi.ingest(raw, s)
    raw.setflags(write=False)
    want.setflags(write=False)
    return raw, want


def _set_raw(g, raw, pad):
    """Through the C entry itself, with rows `pad` bytes longer than the pixels (the padding is filled with 0xAB)."""
    H, W = raw.shape[:2]
    ch = 1 if raw.ndim == 2 else 3
    buf = np.full((H, W * ch + pad), 0xAB, np.uint8)
    buf[:, :W * ch] = raw.reshape(H, W * ch)
    return g._lib.ekf_set_frame_raw(g._h, buf.ctypes.data_as(C.c_void_p), W, H, ch, W * ch + pad)


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("W,H,s", SHAPES)
def test_parity_with_the_oracle(pkg, W, H, s, channels, pad):
    raw, want = _case(W, H, s, channels)
    g = _filter(pkg, W, H, s)
    assert _set_raw(g, raw, pad) == 0, g._lib.ekf_last_error(g._h)
    got = g.getFrame()
    g.close()
    assert got.shape == want.shape
    assert np.array_equal(got, want), (fi.mode(W, H, s), np.argwhere(got != want)[:5])


def test_parity_larger_frame_at_the_reference_factor(pkg):
    raw, want = _case(1280, 960, 10, 3)
    g = _filter(pkg, 1280, 960, 10)
    g.setFrameRaw(raw)
    assert np.array_equal(g.getFrame(), want)
    g.close()


@pytest.mark.parametrize("W,H,s,channels", LOOP_SHAPES)
def test_parity_beyond_one_pass_of_the_grid(pkg, W, H, s, channels):
    raw, want = _case(W, H, s, channels)
    g = _filter(pkg, W, H, s)
    g.setFrameRaw(raw)
    got = g.getFrame()
    g.close()
    assert np.array_equal(got, want), (fi.mode(W, H, s), np.argwhere(got != want)[:5])


def test_a_second_geometry_and_a_second_frame_on_one_filter(pkg):
    """The buffers grow and the tables follow the geometry: 3 channels after 1, a non-dividing raw size after a dividing
    one (both derive 32 x 24 at s = 10), then the first again."""
    g = _filter(pkg, 320, 240, 10)
    for (W, H, ch) in ((320, 240, 1), (327, 243, 3), (320, 240, 3), (327, 243, 1)):
        raw, want = _case(W, H, 10, ch)
        g.setFrameRaw(raw)
        assert np.array_equal(g.getFrame(), want), (W, H, ch)
    g.close()


def test_device_pointer_path(pkg):
    import torch
    W, H, s = 101, 67, 3
    raw, want = _case(W, H, s, 3)
    g = _filter(pkg, W, H, s)
    t = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    g.setFrameRaw(t)
    g.synchronize()
    assert np.array_equal(g.getFrame(), want)
    # rows may be strided ...
    wide = torch.zeros((H, W + 3, 3), dtype=torch.uint8, device="cuda")
    wide[:, :W] = t
    torch.cuda.synchronize()
    g.setFrame(np.zeros_like(want))
    g.captureNewFrame(wide[:, :W], 1.0)
    g.synchronize()
    assert np.array_equal(g.getFrame(), want)
    # ... pixels may not
    for bad in (wide[:, ::2], t.permute(1, 0, 2), t[:, :, :1].expand(-1, -1, 3)):
        assert not bad.is_contiguous()
        with pytest.raises(ValueError):
            g.setFrameRaw(bad)
    with pytest.raises(ValueError):
        g.setFrameRaw(t.to(torch.int8))
    # one channel from a device tensor; the time-stamp half of captureNewFrame still only sets dT
    raw1, want1 = _case(W, H, s, 1)
    t1 = torch.from_numpy(raw1.copy()).cuda()
    torch.cuda.synchronize()
    g.captureNewFrame(t1, 1.5)
    g.synchronize()
    assert np.array_equal(g.getFrame(), want1) and abs(g.getDt() - 0.5) < 1e-12
    g.captureNewFrame(2.0)                                  # the call as it was: a time stamp alone
    assert abs(g.getDt() - 0.5) < 1e-12 and np.array_equal(g.getFrame(), want1)
    g.captureNewFrame(time_stamp=2.25)
    assert abs(g.getDt() - 0.25) < 1e-12
    g.close()


def test_equivalence_with_the_grey_entry(pkg):
    """Filter A is given the raw colour frame, filter B the oracle's grey frame through ekf_set_frame: corners, templates,
    z, found and score are bitwise equal.  The raw frames are the image stream of tests/test_gpu_end_update.py replicated
    to raw size (so that corners exist) with a little noise on every channel (so that the ingest has something to average)."""
    import ekf_oracle as o
    import test_gpu_end_update as ge
    cfg = ge._stream_config()
    s = cfg["scale"]
    world = ge._stream_world()
    ref = o.StructuredFilter(o.Config.kinect(), np.float64)
    rng = np.random.default_rng(77)

    def raw_of(f):
        up = fi.replicate(ge._stream_frame(world, f), s, 3).astype(np.int64)
        return np.clip(up + rng.integers(-6, 7, size=up.shape), 0, 255).astype(np.uint8)

    filters = []
    for _ in range(2):
        g = pkg.VSlamFilter(cfg, capacity_features=128, dtype=np.float64)
        g.setDt(1.0 / 30.0)
        g.setFullState(ref.mu)
        g.setSigmaBlock(ref.Sigma)
        filters.append(g)
    A, B = filters
    raw0 = raw_of(0)
    A.setFrameRaw(raw0)
    B.setFrame(fi.ingest(raw0, s))
    assert np.array_equal(A.getFrame(), B.getFrame())
    ca, cb = A.findNewFeatures(-1), B.findNewFeatures(-1)
    assert len(ca) >= 20 and np.asarray(ca).tobytes() == np.asarray(cb).tobytes()
    N = A.numOfFeatures()
    assert N == B.numOfFeatures() and N >= 20
    for i in range(N):
        assert np.array_equal(A.getPatch(i), B.getPatch(i)), i
    for f in (1, 2):
        raw = raw_of(f)
        A.setFrameRaw(raw)
        B.setFrame(fi.ingest(raw, s))
        A.predict()
        B.predict()
        za, fa, sa = A.findMatches()
        zb, fb, sb = B.findMatches()
        assert fa.any()
        assert za.tobytes() == zb.tobytes() and fa.tobytes() == fb.tobytes() and sa.tobytes() == sb.tobytes()
        for i in range(N):
            assert np.array_equal(A.getPatch(i, matching=True), B.getPatch(i, matching=True)), (f, i)
    assert A.getFullState().tobytes() == B.getFullState().tobytes()
    A.close()
    B.close()


def test_errors_leave_the_previous_frame_readable(pkg):
    W, H, s = 64, 48, 2
    lib = pkg.load_library()
    g = _filter(pkg, W, H, s)
    out = np.zeros((H // s, W // s), np.uint8)
    assert lib.ekf_get_frame(g._h, out.ctypes.data_as(C.c_void_p), W // s) == 4          # no frame yet
    raw, want = _case(W, H, s, 3)
    g.setFrameRaw(raw)
    buf = np.zeros((H + 2, (W + 2) * 3), np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.ekf_set_frame_raw(g._h, p, W + 2, H, 3, (W + 2) * 3) == 1                  # derived width 33 != 32
    assert lib.ekf_set_frame_raw(g._h, p, W, H + 2, 3, W * 3) == 1                        # derived height 25 != 24
    assert lib.ekf_set_frame_raw(g._h, p, W, H, 2, W * 3) == 1                            # channels
    assert lib.ekf_set_frame_raw(g._h, p, W, H, 3, W * 3 - 1) == 1                        # short stride
    assert lib.ekf_set_frame_raw(g._h, None, W, H, 3, W * 3) == 1                         # null
    assert lib.ekf_set_frame_raw_device(g._h, None, W, H, 3, W * 3) == 1
    assert lib.ekf_set_frame_raw_device(g._h, p, W, H, 4, W * 4) == 1                     # (refused before the pointer is used)
    assert lib.ekf_get_frame(g._h, None, W // s) == 1
    assert lib.ekf_get_frame(g._h, out.ctypes.data_as(C.c_void_p), W // s - 1) == 1
    assert np.array_equal(g.getFrame(), want)
    wide = np.zeros((H // s, W // s + 7), np.uint8)
    assert lib.ekf_get_frame(g._h, wide.ctypes.data_as(C.c_void_p), W // s + 7) == 0
    assert np.array_equal(wide[:, :W // s], want) and not wide[:, W // s:].any()
    g.close()
    bad = pkg.VSlamFilter(dict(_config(pkg, W, H, s), scale=0), capacity_features=8)
    assert lib.ekf_set_frame_raw(bad._h, p, W, H, 3, W * 3) == 1                          # scale < 1
    bad.close()


def test_set_frame_after_a_raw_frame_drops_the_raw_frame(pkg):
    """A key frame must not pair a new grey frame with an old colour one."""
    W, H, s = 64, 48, 2
    g = _filter(pkg, W, H, s)
    sel = pkg.KeyframeSelector(g, raw_shape=(H, W, 3))
    raw, want = _case(W, H, s, 3)

    def move(x):
        mu = g.getFullState()
        mu[:7] = [x, 0, 0, 1, 0, 0, 0]
        g.setFullState(mu)

    g.setFrameRaw(raw)
    move(6.0)
    r = sel.observe(2)
    assert r.action == 4 and r.record.id == 2                                              # EMIT_FIRST
    assert np.array_equal(sel.emitted_raw_image(), raw) and np.array_equal(sel.emitted_image(), want)
    newer = (255 - want).astype(np.uint8)
    g.setFrame(newer)
    move(12.0)
    r = sel.observe(3)
    assert r.action == 4 and r.record.id == 3
    with pytest.raises(pkg.EkfError) as ei:
        sel.emitted_raw_image()
    assert ei.value.status == 4
    assert np.array_equal(sel.emitted_image(), newer)
    # a plain selector never has one
    plain = pkg.KeyframeSelector(g)
    g.setFrameRaw(raw)
    move(18.0)
    assert plain.observe(4).action == 4
    assert np.array_equal(plain.emitted_image(), want)
    buf = np.zeros((H, W, 3), np.uint8)
    assert g._lib.ekf_keyframe_get_raw_image(plain._h, buf.ctypes.data_as(C.c_void_p), W * 3) == 4
    with pytest.raises(pkg.EkfError):
        plain.emitted_raw_image()
    for h in (sel, plain, g):
        h.close()
