"""Growth of the library's device and pinned buffers (csrc/ekf_buffers.hpp): one filter is driven small, then large, then
small again, and every answer is compared BIT FOR BIT with a fresh filter that only ever saw that one request.  The step is
reproducible to the bit (tools/step_fingerprint.py), so a buffer that lost its contents, kept a stale capacity or was read
past its end shows as a difference; there is no tolerance anywhere in this file.

Where the fresh filter has to stand where the long-lived one stands, it is given that filter's state and covariance
(getFullState / getFullSigma -> setFullState / setSigmaBlock: exact copies) and the same capacity, hence the same launch
schedule.

A filter's matcher frame has ONE size (ekf_set_frame refuses any other: the size belongs to ekf_config), so d_frame never
grows on a filter; what grows with the request are the raw frame (its size within the scale's remainder, its channels),
the resident ingest tables and the rectification scratch (matcher frame <-> raw frame)."""
import numpy as np
import pytest

import sba_scene

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. frames ---------------------------------------------------------------------------------------------------------
SMALL_CFG = dict(image_width=32, image_height=24, scale=2)


def _frame_filter(pkg):
    return pkg.VSlamFilter(dict(pkg.kinect_config(), **SMALL_CFG), capacity_features=4, dtype=F32)


def _images():
    rng = np.random.default_rng(77)
    return dict(gray=rng.integers(0, 256, (24, 32)).astype(np.uint8),           # the matcher frame itself
                gray_big=rng.integers(0, 256, (48, 64)).astype(np.uint8),       # ... at a size the filter must refuse
                raw1=rng.integers(0, 256, (48, 64)).astype(np.uint8),           # 64 x 48 x 1: 2 x 2 area path, 3072 bytes
                raw3=rng.integers(0, 256, (49, 65, 3)).astype(np.uint8))        # 65 x 49 x 3: table path, 9555 bytes


def test_plain_frame_small_large_small(pkg):
    im = _images()
    g, fresh = _frame_filter(pkg), _frame_filter(pkg)
    g.setFrame(im["gray"])
    with pytest.raises(pkg.EkfError):
        g.setFrame(im["gray_big"])                             # 64 x 48 on a 32 x 24 filter: refused, nothing is reallocated
    g.setFrameRaw(im["raw3"])                                  # (the frame buffer is rewritten by a larger request's ingest)
    g.setFrame(im["gray"])
    fresh.setFrame(im["gray"])
    assert same(g.getFrame(), fresh.getFrame()) and same(g.getFrame(), im["gray"])
    assert same(g.getFrameRectified(), fresh.getFrameRectified())
    with pytest.raises(pkg.EkfError):
        g.getFrameRectified(raw=True)                          # the plain frame dropped the raw one
    g.close(); fresh.close()


def test_raw_frame_small_large_small(pkg):
    im = _images()
    g = _frame_filter(pkg)
    seen = {}
    for name in ("raw1", "raw3", "raw1"):                      # d_raw: 3072 -> 9555 bytes -> a 3072-byte request in the larger block
        g.setFrameRaw(im[name])
        seen[name] = (g.getFrame(), g.getFrameRectified(), g.getFrameRectified(raw=True))
    for name in ("raw1", "raw3"):
        fresh = _frame_filter(pkg)
        fresh.setFrameRaw(im[name])
        want = (fresh.getFrame(), fresh.getFrameRectified(), fresh.getFrameRectified(raw=True))
        assert want[2].shape == im[name].shape
        for got, w in zip(seen[name], want):
            assert same(got, w), name
        fresh.close()
    g.close()


def test_rectified_frame_scratch_small_large_small(pkg):
    im = _images()
    g, fresh = _frame_filter(pkg), _frame_filter(pkg)
    g.setFrameRaw(im["raw3"])
    fresh.setFrameRaw(im["raw3"])
    small0 = g.getFrameRectified()                             # 768 bytes of scratch
    large = g.getFrameRectified(raw=True)                      # 9555
    small1 = g.getFrameRectified()                             # 768 again, in the larger block
    uv = np.array([[3.0, 4.0], [30.5, 20.25], [0.0, 0.0]])
    pts = [g.undistortPixels(uv[:1]), g.undistortPixels(uv), g.undistortPixels(uv[:1])]
    assert same(small0, small1) and same(small1, fresh.getFrameRectified())
    assert same(pts[0], pts[2]) and same(pts[2], fresh.undistortPixels(uv[:1]))
    fresh2 = _frame_filter(pkg)
    fresh2.setFrameRaw(im["raw3"])
    assert same(large, fresh2.getFrameRectified(raw=True)) and same(pts[1], fresh2.undistortPixels(uv))
    g.close(); fresh.close(); fresh2.close()


# ---- 2. the archive keeps its rows across growth -----------------------------------------------------------------------------
def test_archive_keeps_rows_across_growth(pkg):
    """The recipe of test_points_table_with_archived_patches: XYZ features with n_find > 5 are archived at removal.  Three
    batches of 100; the archive starts at 256 rows, so the third batch makes it allocate, copy and swap."""
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    px = synthetic.initial_pixels(cfg, 100, 1234)
    g = pkg.VSlamFilter(cfg, capacity_features=104, dtype=F64)
    g.setDt(1 / 30.0)

    def batch(keep_last):
        for (u, v) in px:
            assert g.addFeature((u, v)) == 1
        S = g.getFullSigma()
        pos, cod = g.featureLayout()
        for p in pos[cod == 0]:                                 # make every inverse-depth feature pass the linearity test
            S[p + 5, :] *= 1e-4
            S[:, p + 5] *= 1e-4
        g.setSigmaBlock(S)
        g.convert2XYZ_ifLinearAll()
        assert (g.featureLayout()[1] != 0).all()
        n_now = g.numOfFeatures()
        for i in range(n_now):
            g.setFeatureMeta(i, n_find=7)
        g.removeFeatures(list(range(n_now - 1 if keep_last else n_now)))

    batch(False)
    batch(False)
    assert g.numArchived() == 200 and g.numOfFeatures() == 0
    assert g.addFeature((100.0, 90.0)) == 1                    # (a table needs a live feature: its rows end at the last real_index)
    before = g.getPointsTable()
    assert before.shape == (202, 12) and before[1:201].any(axis=1).all() and not before[0].any()
    batch(True)                                                # 300 rows > 256: the archive grows, its 200 rows are copied
    assert g.numArchived() == 300 and g.numOfFeatures() == 1   # (that feature and 99 of the batch; the batch's last one lives on)
    after = g.getPointsTable()
    assert after.shape == (302, 12) and after[201:302].any(axis=1).all()
    assert same(after[:201], before[:201])
    g.close()


# ---- 3. RANSAC mask, gain buffer, work lists ------------------------------------------------------------------------------------
def _ekf_filter(pkg, dtype, px, capacity, mu=None, Sigma=None):
    f = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=capacity, dtype=dtype)
    f.setDt(1 / 30.0)
    for (u, v) in px:
        assert f.addFeature((u, v)) == 1
    if mu is not None:
        f.setFullState(mu)
        f.setSigmaBlock(Sigma)
    return f


def _stream(pkg, n, frames, dtype):
    from ekf_monoslam_amd import synthetic
    px, z = synthetic.measurement_stream(pkg.kinect_config(), n, frames, sigma_px=0.5)
    return px, z.astype(dtype)


def test_ransac_mask_small_large_small(pkg):
    px, z = _stream(pkg, 24, 1, F32)
    idx = np.arange(24, dtype=np.int32)

    def ask(f, M):
        counts, best, inl = f.ransac1Point(z[0][:M].reshape(-1), idx[:M])
        return counts, np.int64(best), inl

    g = _ekf_filter(pkg, F32, px, 32)
    g.predict()
    got = [ask(g, 8), ask(g, 24), ask(g, 8)]
    for M, which in ((8, (0, 2)), (24, (1,))):
        fresh = _ekf_filter(pkg, F32, px, 32)
        fresh.predict()
        want = ask(fresh, M)
        assert want[0].shape == (M,)
        for k in which:
            assert all(same(a, b) for a, b in zip(got[k], want)), (M, k)
        fresh.close()
    g.close()


def test_gain_buffer_small_large_small(pkg):
    """The gain buffer holds 2 npad_live m_pad scalars, m_pad = 2 M rounded up to 128 on fp32: 8 and 24 measurements need
    the same room, 70 (m_pad = 256) twice as much, and the last 8 run in the larger block."""
    px, z = _stream(pkg, 72, 4, F32)
    idx = np.arange(72, dtype=np.int32)

    def ask(f, k, M):
        f.predict()
        f.update(z[k][:M].reshape(-1), idx[:M], plane_constraint=False)
        return f.getGain(), f.getFullState(), f.getFullSigma()

    g = _ekf_filter(pkg, F32, px, 80)
    for k, M in enumerate((8, 24, 70, 8)):
        mu, Sigma = g.getFullState(), g.getFullSigma()
        got = ask(g, k, M)
        fresh = _ekf_filter(pkg, F32, px, 80, mu, Sigma)
        want = ask(fresh, k, M)
        assert got[0].shape == (g.stateDim(), 2 * M)
        assert np.isfinite(got[0]).all() and got[0].any()
        assert all(same(a, b) for a, b in zip(got, want)), (k, M)
        fresh.close()
    g.close()


def test_work_lists_rebuilt_both_ways(pkg):
    """fp32, N = 200 (one chunk, fused block steps) -> N = 40 (one diagonal block) -> N = 200: tile maps and step lists are
    rebuilt for the smaller state and again for the larger one."""
    px, z = _stream(pkg, 200, 3, F32)
    cap = 208

    def step(f, zk):
        f.predict()
        _, vis, _, _ = f.predictions()
        sel = np.nonzero(vis.astype(bool))[0].astype(np.int32)
        assert sel.size > zk.shape[0] // 2
        f.update(zk[sel].reshape(-1), sel, plane_constraint=False)
        f.synchronize()
        return f.getFullState(), f.getFullSigma(), sel

    g = _ekf_filter(pkg, F32, px, cap)
    step(g, z[0])
    g.removeFeatures(list(range(40, 200)))
    for k, n_now in ((1, 40), (2, 200)):
        if n_now == 200:
            for (u, v) in px[40:]:
                assert g.addFeature((u, v)) == 1
        assert g.numOfFeatures() == n_now
        mu, Sigma = g.getFullState(), g.getFullSigma()
        got = step(g, z[k][:n_now])
        fresh = _ekf_filter(pkg, F32, px[:n_now], cap, mu, Sigma)
        want = step(fresh, z[k][:n_now])
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert all(same(a, b) for a, b in zip(got, want)), n_now
        fresh.close()
    g.close()


def test_trail_diag_lists_survive_a_small_update(pkg):
    """The lists of the fused trailing-update + next-diagonal launch (k_trail_diag) belong to one chunk plan.  A large
    update builds them, an update of 8 measurements (one diagonal block: no chain lists) makes them another plan's, and the
    next large update has the same plan as the first: it must take the fused launch as often as a fresh filter does.  The
    two schedules give the same bits, so only the launch counters can tell."""
    n = 640                                                    # 10 block steps: the first ones have >= 24 blocks to update
    px, z = _stream(pkg, n, 3, F32)
    idx = np.arange(n, dtype=np.int32)

    def full(f, k):
        f.predict()
        f.profile_reset()                                      # launch counters from zero
        f.update(z[k].reshape(-1), idx, plane_constraint=False)
        f.synchronize()
        return f.launch_counts(), f.getFullState(), f.getFullSigma()

    g = _ekf_filter(pkg, F32, px, n + 8)
    first = full(g, 0)[0]
    assert first.get("chain_trail_diag", 0) > 0
    g.predict()
    g.update(z[1][:8].reshape(-1), idx[:8], plane_constraint=False)
    mu, Sigma = g.getFullState(), g.getFullSigma()
    got = full(g, 2)
    fresh = _ekf_filter(pkg, F32, px, n + 8, mu, Sigma)
    want = full(fresh, 2)
    assert got[0] == want[0] and got[0]["chain_trail_diag"] == first["chain_trail_diag"]
    assert same(got[1], want[1]) and same(got[2], want[2])
    g.close(); fresh.close()


def test_readback_delivers_pending_pieces_at_the_edge(pkg):
    """The pinned read-back buffer (ReadBack, csrc/ekf_buffers.hpp) starts at 64 KiB.  fp32, 81 features (n = 500): the block
    Sigma[0:33, 0:496] is 33 * 496 * 4 = 65472 bytes and fills the buffer to its 64 bytes of slack, so the status words queued
    behind it find no room and the block is delivered mid-batch; the full matrix (1 MB) then makes the buffer grow, and the
    same block is read again out of the larger one.  Both block reads equal the slice of the full matrix, and a fresh filter
    with the same inputs agrees on every read, bit for bit."""
    px, z = _stream(pkg, 81, 1, F32)
    idx = np.arange(81, dtype=np.int32)

    def reads():
        f = _ekf_filter(pkg, F32, px, 81)
        f.predict()
        f.update(z[0].reshape(-1), idx, plane_constraint=False)
        assert f.stateDim() == 500
        out = (f.getFullState(), f.getSigmaBlock(0, 0, 33, 496), f.getFullSigma(), f.getSigmaBlock(0, 0, 33, 496))
        f.close()
        return out

    mu, edge, full, again = reads()
    assert edge.shape == (33, 496) and edge.nbytes == 65472 and np.isfinite(full).all() and full.any()
    assert same(edge, full[:33, :496]) and same(again, full[:33, :496])
    for got, want in zip((mu, edge, full), reads()[:3]):
        assert same(got, want)


# ---- 4. bundle adjustment ---------------------------------------------------------------------------------------------------------
def test_bundle_adjuster_grows_between_runs(pkg):
    """3 nodes / 20 points, a run, then 40 more points and their projections, a second run -- against an adjuster that is
    given the final problem at once.  The first run builds the structure and every buffer at the small size and evaluates
    the cost, with no LM iteration: estimates that a first run had moved could not be handed to a fresh adjuster exactly
    (ekf_sba_add_nodes re-derives qw from the vector part, the device normalises by |q|: an ulp apart)."""
    sc = sba_scene.make_scene(2, 60, seed=5, lonely_node=False)
    first = sc["point"] < 20

    a = pkg.BundleAdjuster(camera=sc["camera"])
    a.add_nodes(sc["nodes"])
    a.add_points(sc["points"][:20])
    a.add_projections(sc["node"][first], sc["point"][first], sc["uv"][first])
    assert a.run(0, 1e-4) == 0 and a.cost()[0] > 0
    a.add_points(sc["points"][20:])
    a.add_projections(sc["node"][~first], sc["point"][~first], sc["uv"][~first])

    b = pkg.BundleAdjuster(camera=sc["camera"])
    b.add_nodes(sc["nodes"])
    b.add_points(sc["points"])
    b.add_projections(sc["node"], sc["point"], sc["uv"])
    assert a.counts() == b.counts() and a.counts()[:2] == (3, 60)
    assert same(a.nodes(), b.nodes()) and same(a.points(), b.points())
    assert all(same(x, y) for x, y in zip(a.projections(), b.projections()))

    it = a.run(6, 1e-4)
    assert it == b.run(6, 1e-4) and it > 0
    cost0 = a.log()[0][0]                                      # cost before the first iteration
    assert same(np.array(a.cost()), np.array(b.cost())) and same(np.asarray(a.log()), np.asarray(b.log()))
    assert same(a.nodes(), b.nodes()) and same(a.points(), b.points())
    assert np.isfinite(a.nodes()).all() and a.cost()[0] < cost0
    a.close(); b.close()
