"""End-of-update housekeeping and corner seeding through the C ABI, against tests/frame_oracle.py:
ekf_find_new_features (bit-exact lambda and corners), the track state (n_tot, center, in_innovation, sticky remove
flag) across ekf_find_matches / removal / conversion, and ekf_end_update over a short frame stream."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import ekf_oracle as o
import frame_oracle as fo
import image_oracle as io_
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


def _filter(config, capacity=256, dtype=np.float32):
    pkg = load_package()
    return pkg.VSlamFilter(config, capacity_features=capacity, dtype=dtype)


def _lambda(g, H, W):
    out = np.zeros((H, W), np.float64)
    rc = g._lib.ekf_peek_workspace(g._h, 4, out.ctypes.data_as(C.c_void_p), 0, 0, H, W)
    assert rc == 0
    return out


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W)).astype(np.uint8)


def _plateaus(H, W, seed):
    base = np.random.default_rng(seed).integers(0, 4, size=(H // 8 + 1, W // 8 + 1)).astype(np.uint8) * 60
    return np.kron(base, np.ones((8, 8), np.uint8))[:H, :W].copy()


def _squares(H, W):
    img = np.zeros((H, W), np.uint8)
    for x0, y0, s in [(30, 40, 40), (150, 60, 50), (90, 150, 35), (220, 120, 30)]:
        if x0 + s < W and y0 + s < H:
            img[y0:y0 + s, x0:x0 + s] = 220
    return img


def _check_detector(g, frame, window, num, centers=(), quality=0.01, min_distance=12.0):
    H, W = frame.shape
    g.setFrame(frame)
    uv = g.findNewFeatures(num, quality, min_distance, add=False)
    lam = _lambda(g, H, W)
    ref_uv, ref_lam = fo.find_new_features(frame, list(centers), window, num if num > 0 else g._cfg.nInitFeatures,
                                           quality, min_distance)
    assert np.array_equal(lam.view(np.int64), ref_lam.view(np.int64)), "lambda differs"
    assert np.array_equal(uv, ref_uv), (uv[:8], ref_uv[:8])
    return uv


@pytest.mark.parametrize("image", ["texture", "squares", "plateaus", "noise"])
def test_detector_bit_exact_kinect(image):
    cfg = load_package().kinect_config()
    H, W = cfg["image_height"], cfg["image_width"]
    frame = {"texture": lambda: io_.random_texture(H, W, seed=41),
             "squares": lambda: _squares(H, W),
             "plateaus": lambda: _plateaus(H, W, 42),
             "noise": lambda: _noise(H, W, 43)}[image]()
    g = _filter(cfg)
    uv = _check_detector(g, frame, cfg["window_size"], 60)
    assert len(uv) > 0
    g.close()


def test_detector_bit_exact_noise_640x480():
    """i.i.d. per-pixel noise: a local maximum every few pixels, K beyond the LDS-resident selection (4096)."""
    cfg = dict(load_package().kinect_config(), image_width=640, image_height=480, window_size=21)
    frame = _noise(480, 640, 43)
    lam = fo.corner_response(frame)
    vals, idx = fo.candidates(lam, fo.seed_mask(640, 480, 21, []), 0.01)
    assert idx.size > 4096
    g = _filter(cfg)
    _check_detector(g, frame, 21, 60)
    uv_all = _check_detector(g, frame, 21, 5000)
    assert 100 < len(uv_all) < 5000                                          # num larger than the corners available
    g.close()


def test_detector_window30_with_live_features_masking():
    pkg = load_package()
    cfg = pkg.sim_config()
    H, W = cfg["image_height"], cfg["image_width"]
    frame = io_.random_texture(H, W, seed=44)
    g = _filter(cfg, dtype=np.float64)
    g.setFrame(frame)
    first = g.findNewFeatures(4, add=True)                        # the map now masks these four
    assert len(first) == 4
    _, _, cen, _ = g.featureTrack()
    assert np.array_equal(cen, first)
    _check_detector(g, frame, cfg["window_size"], 50, centers=[tuple(c) for c in cen])
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_seeding_empty_map_and_capacity(dtype):
    pkg = load_package()
    cfg = pkg.kinect_config()
    cfg["nInitFeatures"] = 10
    H, W = cfg["image_height"], cfg["image_width"]
    frame = io_.random_texture(H, W, seed=45)
    g = _filter(cfg, dtype=dtype)
    g.setFrame(frame)
    uv = g.findNewFeatures(-1)                                     # findNewFeatures(10) of frame 0: num <= 0 -> nInitFeatures
    ref_uv, _ = fo.find_new_features(frame, [], cfg["window_size"], 10)
    assert np.array_equal(uv, ref_uv) and len(uv) == 10
    ri, nf = g.featureIds()
    assert list(ri) == list(range(1, 11)) and list(nf) == [1] * 10
    nt, inn, cen, rem = g.featureTrack()
    assert list(nt) == [1] * 10 and not inn.any() and not rem.any() and np.array_equal(cen, uv)
    for i, (u, v) in enumerate(uv):
        assert np.array_equal(g.getPatch(i), io_.capture_patch(frame, float(u), float(v), cfg["window_size"]))
    # the same corners through ekf_add_feature: mu / Sigma identical (the add path itself is held to the oracle elsewhere)
    h = _filter(cfg, dtype=dtype)
    h.setFrame(frame)
    for (u, v) in uv:
        assert h.addFeature((float(u), float(v))) == 1
    assert np.array_equal(g.getFullState(), h.getFullState())
    assert np.array_equal(g.getFullSigma(), h.getFullSigma())
    h.close()
    # at capacity: what fits is added, the rest reported
    c = _filter(cfg, capacity=6, dtype=dtype)
    c.setFrame(frame)
    uv2 = c.findNewFeatures(10)
    assert np.array_equal(uv2, ref_uv) and c.numOfFeatures() == 6
    assert len(c.findNewFeatures(10)) > 0 and c.numOfFeatures() == 6
    c.close()
    g.close()


def test_errors_and_empty_map():
    pkg = load_package()
    g = _filter(pkg.kinect_config())
    with pytest.raises(pkg.EkfError) as e:
        g.findNewFeatures(5)
    assert e.value.status == 4                                     # EKF_ERR_STATE: no frame
    g.setFrame(io_.random_texture(240, 320, seed=46))
    with pytest.raises(pkg.EkfError) as e:
        g.findNewFeatures(5, min_distance=-1.0)
    assert e.value.status == 1
    assert len(g.findNewFeatures(2000, add=False)) > 0             # num above capacity is not an error
    r = g.endUpdate(seed=True)                                     # empty map: a no-op reporting 0
    assert len(r["removed"]) == 0 and r["n_visible"] == 0 and r["n_seeded"] == 0
    assert g.numOfFeatures() == 0
    g.close()


def _pair(n_feat, dtype, frame):
    pkg = load_package()
    cfg = dataclasses.replace(o.Config.kinect(), kernel_size=1000, T_camera=0.0)
    ref = o.build_scenario(o.StructuredFilter, cfg, n_feat, dtype, w=(0.0, 0.05, 0.0))
    gcfg = dict(pkg.kinect_config())
    g = pkg.VSlamFilter(gcfg, capacity_features=n_feat + 64, dtype=dtype)
    g.setDt(ref.dT)
    full = g.getFullState()
    full[7:13] = ref.mu[7:13]
    g.setFullState(full)
    g.setFrame(frame)
    px = o.synthetic_pixels(cfg, n_feat)
    tr = fo.Track()
    for (u, v) in px:
        assert g.addFeature((u, v)) == 1
        tr.add(u, v)
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    tpl = [io_.capture_patch(frame, u, v, cfg.window_size) for (u, v) in px]
    return ref, g, tpl, cfg, tr, px


def _assert_track(g, tr):
    nt, inn, cen, rem = g.featureTrack()
    ent, einn, ecen, erem = tr.arrays()
    assert np.array_equal(nt, ent)
    assert np.array_equal(inn, einn)
    assert np.array_equal(cen, ecen)
    assert np.array_equal(rem, erem)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_track_state_follows_matches_removal_and_conversion(dtype):
    frame = io_.random_texture(240, 320, seed=24)
    ref, g, tpl, cfg, tr, px = _pair(40, dtype, frame)
    _assert_track(g, tr)
    ref.predict()
    g.predict()
    tr.predicted([ft.is_in_innovation for ft in ref.features], [False] * 40)
    _assert_track(g, tr)
    moved = np.roll(np.roll(frame, 2, axis=1), -1, axis=0)
    for k in (0, 1, 2):
        u, v = int(px[k][0]) + 2, int(px[k][1]) - 1
        moved[max(v - 30, 0):v + 30, max(u - 30, 0):u + 30] = 128
    g.setFrame(moved)
    h, vis, rem, S2 = g.predictions()
    z, found, score = g.findMatches()
    # the oracle's findMatch on the device predictions decides found / z (as test_ncc_search_matches_oracle)
    oz, of = [], []
    for i in range(40):
        if tr.inn[i]:
            ok, zz, sc, win = io_.find_match(moved, tpl[i], h[i], S2[i], cfg.sigma_size)
        else:
            ok, zz = False, (-1, -1)
        oz.append(zz)
        of.append(ok)
    tr.matched(oz, of)
    _assert_track(g, tr)
    nt, inn, cen, _ = g.featureTrack()
    assert nt.max() == 2 and not inn[0] and tuple(cen[0]) == (-1.0, -1.0)
    g.removeFeatures([5, 17])                                       # a removal in the middle of the list
    keep = [i for i in range(40) if i not in (5, 17)]
    tr.keep(keep)
    _assert_track(g, tr)
    # a conversion in the middle of the list: feature 10 made linear (small inverse-depth variance)
    pos, cod = g.featureLayout()
    S = g.getFullSigma()
    p10 = int(pos[10])
    blk = S[p10:p10 + 6, p10:p10 + 6].copy() * 1e-8
    g.setSigmaBlock(blk, p10, p10)
    g.convert2XYZ_ifLinear(10)
    _assert_track(g, tr)                                           # conversion keeps the order and the state
    # a feature set by hand (a caller's own matcher)
    g.setFeatureTrack(3, n_tot=9, in_innovation=0, center=(7.5, 8.5), remove_flag=1)
    nt, inn, cen, rem = g.featureTrack()
    assert nt[3] == 9 and not inn[3] and tuple(cen[3]) == (7.5, 8.5) and rem[3]
    g.setFeatureTrack(3, remove_flag=-1)
    assert g.featureTrack()[3][3]
    g.close()


def test_sticky_remove_flag_from_rho():
    frame = io_.random_texture(240, 320, seed=26)
    ref, g, tpl, cfg, tr, px = _pair(12, np.float32, frame)
    pos, cod = g.featureLayout()
    mu = g.getFullState()
    mu[pos[4] + 5] = -0.1                                          # rho <= 0: flagged (vR.cpp:517-521)
    g.setFullState(mu)
    g.predict()
    _, _, rem_now, _ = g.predictions()
    assert rem_now[4]
    mu = g.getFullState()
    mu[pos[4] + 5] = 0.2
    g.setFullState(mu)
    g.predict()
    _, _, rem_now, _ = g.predictions()
    assert not rem_now[4]                                          # the per-call flag keeps its meaning ...
    assert g.featureTrack()[3][4]                                  # ... the track's flag is sticky
    r = g.endUpdate(seed=False)
    assert 4 in list(r["removed"])
    g.close()


def test_feature_records_follow_a_python_model():
    """The host records of the features (FeatureTable, csrc/ekf_feature_table.hpp) through the C ABI against the plain Python
    model the host check replays (tools/filter_host_check.py): additions, distinct meta and track values, a removal at both
    ends and in the middle, additions behind it, two forced conversions and the removal of a converted feature.  Ids, track
    state and layout are compared after every operation."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from filter_host_check import FeatureModel
    g = _filter(load_package().kinect_config(), capacity=16)
    m = FeatureModel(g.camera_dim)
    px = o.synthetic_pixels(o.Config.kinect(), 14)

    def compare():
        N = g.numOfFeatures()
        assert N == len(m) and g.stateDim() == m.n
        ri, nf = g.featureIds()
        nt, inn, cen, rem = g.featureTrack()
        pos, cod = g.featureLayout()
        assert list(ri) == m.real_index and list(nf) == m.n_find and list(nt) == m.n_tot
        assert list(inn) == [bool(x) for x in m.inn] and list(rem) == [bool(x) for x in m.rem]
        assert np.array_equal(cen, np.asarray(m.center, np.float32).reshape(N, 2))
        assert list(pos) == m.pos and list(cod) == m.coding

    def add(k):
        assert g.addFeature(px[k]) == 1
        m.add(float(px[k][0]), float(px[k][1]))
        compare()

    compare()
    for k in range(12):
        add(k)
    for i in range(12):
        meta = dict(real_index=200 + 7 * i, n_find=3 + i)
        track = dict(n_tot=20 + 2 * i, in_innovation=(i + 1) % 2, center=(10.5 + i, 99.25 - 3 * i), remove_flag=int(i % 4 == 1))
        g.setFeatureMeta(i, **meta)
        m.set_meta(i, **meta)
        compare()
        g.setFeatureTrack(i, **track)
        m.set_track(i, **track)
        compare()
    g.removeFeatures([0, 5, 11])
    m.compact(remove=[0, 5, 11])
    compare()
    add(12)
    add(13)
    assert m.real_index[-2:] == [13, 14]                               # the counter went on behind the removed features
    pos, _ = g.featureLayout()
    n = g.stateDim()
    for fi in (1, 4):                                                  # a known depth: the feature passes the linearity test
        r = int(pos[fi]) + 5
        g.setSigmaBlock(np.zeros((1, n), np.float32), r, 0)
        g.setSigmaBlock(np.zeros((n, 1), np.float32), 0, r)
        g.setSigmaBlock(np.array([[1e-9]], np.float32), r, r)
    assert g.convert2XYZ_ifLinearAll() == 2
    m.compact(convert=[1, 4])
    compare()
    assert m.coding.count(1) == 2 and m.n == g.camera_dim + 6 * 9 + 3 * 2
    g.removeFeatures([1])                                              # a converted feature goes
    m.compact(remove=[1])
    compare()
    g.close()


# ---------------------------------------------------------------------------------------------
# the frame stream: set frame -> predict -> find matches -> two-stage update -> end of update
# ---------------------------------------------------------------------------------------------
STREAM_FRAMES = 30
MIN_FEATURES, MAX_FEATURES, N_INIT = 25, 24, 40     # max < min: every short frame with N > 24 evicts feature 0 (vR.cpp:1313)


def _stream_config():
    pkg = load_package()
    cfg = dict(pkg.kinect_config())
    cfg.update(min_features=MIN_FEATURES, max_features=MAX_FEATURES, nInitFeatures=N_INIT)
    return cfg


def _stream_world():
    return io_.random_texture(240 + 160, 320 + 160, seed=50)


def _stream_frame(world, f):
    """The view drifts right and up; an occluder covers part of it for frames 6-11 (the quality rule fires)."""
    dx, dy = 80 + 2 * f, 80 - f
    frame = world[dy:dy + 240, dx:dx + 320].copy()
    if 6 <= f < 12:
        frame[40:200, 60:220] = 128
    return frame


def _device_frame(g, frame, want_predictions):
    """One frame through the ABI: the records every stream test compares."""
    g.setFrame(frame)
    g.predict()
    pred = g.predictions() + (g.blurPredictions(),) if want_predictions else None
    z, found, score = g.findMatches()
    idx = np.flatnonzero(found).astype(np.int32)
    if idx.size:
        g.updateTwoStage(z[idx], idx, seed=0)
    track_before = g.featureTrack()
    ids_before = g.featureIds()
    r = g.endUpdate(0.2, seed=True)
    return pred, z, found, track_before, ids_before, r


def test_end_update_stream_against_oracle():
    """30 frames in fp64 against ekf_oracle.StructuredFilter + frame_oracle.Track, both driven independently: every
    frame the removed set, n_visible, n_seeded, real_index, n_find, n_tot, centres, in_innovation, the layout and the
    archive count are equal, mu / Sigma within 1e-8 (relative) of the fp64 oracle, the invariants hold; the quality rule,
    the eviction of feature 0 and the re-seeding each fire."""
    pkg = load_package()
    cfg = _stream_config()
    ocfg = dataclasses.replace(o.Config.kinect(), min_features=MIN_FEATURES, max_features=MAX_FEATURES)
    w = cfg["window_size"]
    world = _stream_world()
    ref = o.StructuredFilter(ocfg, np.float64)
    ref.dT = 1.0 / 30.0
    g = pkg.VSlamFilter(cfg, capacity_features=128, dtype=np.float64)
    g.setDt(ref.dT)
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    tr, tpl, mtpl = fo.Track(), [], []
    frame = _stream_frame(world, 0)
    g.setFrame(frame)
    uv = g.findNewFeatures(-1)                                        # frame 0's map (monoslam_ransac.cpp:406)
    ouv, _ = fo.find_new_features(frame, [], w, N_INIT)
    assert np.array_equal(uv, ouv) and len(uv) == N_INIT
    for (u, v) in ouv:
        assert ref.add_feature(float(u), float(v)) == 1
        tr.add(u, v)
        tpl.append(io_.capture_patch(frame, float(u), float(v), w))
        mtpl.append(tpl[-1].copy())
    hits = {"quality": 0, "evict": 0, "seed": 0, "convert": 0}
    for f in range(1, STREAM_FRAMES + 1):
        frame = _stream_frame(world, f)
        ref.predict()
        tr.predicted([ft.is_in_innovation for ft in ref.features], [ft.remove_flag for ft in ref.features])
        (h, vis, rem, S2, hb), z, found, (nt_b, inn_b, cen_b, rem_b), (ri_b, nf_b), r = _device_frame(g, frame, True)
        assert np.array_equal(vis, [ft.is_in_innovation for ft in ref.features]), f
        for i in range(len(tr.n_tot)):                                # Patch::blur at predict (vR.cpp:546-548)
            if tr.inn[i]:
                mtpl[i] = io_.matching_patch(tpl[i], h[i], hb[i], ocfg.kernel_size)
        # the oracle's matcher on the device predictions (as test_ncc_search_matches_oracle), its own templates
        oz, of = [], []
        for i in range(len(tr.n_tot)):
            ok, zz = False, (-1, -1)
            if tr.inn[i]:
                ok, zz, sc, win = io_.find_match(frame, mtpl[i], h[i], S2[i], ocfg.sigma_size)
                if ok:
                    mtpl[i] = win
            oz.append(zz)
            of.append(ok)
        assert np.array_equal(found, of), f
        tr.matched(oz, of)
        idx = [i for i in range(len(of)) if of[i]]
        if idx:
            o.update_two_stage(ref, np.asarray([oz[i] for i in idx], np.float64).reshape(-1), idx, seed=0)
        ent, einn, ecen, erem = tr.arrays()
        enf = np.asarray([ft.n_find for ft in ref.features])
        assert np.array_equal(nt_b, ent) and np.array_equal(inn_b, einn) and np.array_equal(cen_b, ecen), f
        assert np.array_equal(rem_b, erem) and np.array_equal(nf_b, enf), f
        # the end of update() on the oracle side
        removed, n_vis, evict, n_seed = fo.end_update_plan(ent, enf, erem, einn, MIN_FEATURES, MAX_FEATURES)
        hits["quality"] += int(np.count_nonzero(fo.quality_flags(ent, enf)))
        for i in removed:
            ref.remove_feature(int(i))
        keep = [i for i in range(len(ent)) if i not in set(removed.tolist())]
        tr.keep(keep)
        tpl, mtpl = [tpl[i] for i in keep], [mtpl[i] for i in keep]
        if evict:
            hits["evict"] += 1
            ref.remove_feature(0)
            tr.keep(list(range(1, len(tr.n_tot))))
            tpl, mtpl = tpl[1:], mtpl[1:]
        suv = np.zeros((0, 2), np.float32)
        if n_seed:
            suv, _ = fo.find_new_features(frame, [tuple(c) for c in tr.center], w, n_seed)
            for (u, v) in suv:
                assert ref.add_feature(float(u), float(v)) == 1
                tr.add(u, v)
                tpl.append(io_.capture_patch(frame, float(u), float(v), w))
                mtpl.append(tpl[-1].copy())
            hits["seed"] += int(len(suv) > 0)
        hits["convert"] += ref.convert2xyz_if_linear_all()
        # device against oracle
        assert list(r["removed"]) == list(removed), f
        assert r["n_visible"] == n_vis and r["n_seeded"] == len(suv), f
        ri, nf = g.featureIds()
        assert list(ri) == [ft.real_index for ft in ref.features], f
        assert list(nf) == [ft.n_find for ft in ref.features], f
        _assert_track(g, tr)
        pos, cod = g.featureLayout()
        assert list(pos) == [ft.position_in_state for ft in ref.features], f
        assert list(cod) == [ft.coding for ft in ref.features], f
        assert g.numArchived() == len(ref.deleted_patches), f
        for i in range(0, g.numOfFeatures(), 7):
            assert np.array_equal(g.getPatch(i, matching=True), mtpl[i]), (f, i)
        mu, S = g.getFullState(), g.getFullSigma()
        e_mu = np.linalg.norm(mu - ref.mu) / np.linalg.norm(ref.mu)
        e_S = np.linalg.norm(S - ref.Sigma) / np.linalg.norm(ref.Sigma)
        # fp64 filter against the fp64 oracle: the same arithmetic in another order (the suite's fp64 bar is 1e-10 per
        # update; 30 frames of resizing updates are held to 1e-8)
        assert e_mu < 1e-8 and e_S < 1e-8, (f, e_mu, e_S)
        pad, asym, big = g.checkInvariants()
        assert pad == 0 and asym == 0 and np.isfinite(big), f
    print("stream branches:", hits)
    assert hits["quality"] > 0 and hits["evict"] > 0 and hits["seed"] > 0, hits
    g.close()


def test_detector_partial_tiles_odd_frame():
    """A frame whose sides are not multiples of the 16-pixel response tile (partial tiles, halo reflection past W + 1)."""
    cfg = dict(load_package().kinect_config(), image_width=250, image_height=190)
    frame = io_.random_texture(190, 250, seed=47)
    g = _filter(cfg)
    _check_detector(g, frame, cfg["window_size"], 60)
    _check_detector(g, _noise(190, 250, 48), cfg["window_size"], 300)
    g.close()


def test_errors_leave_the_map_unchanged_and_reject_non_finite():
    pkg = load_package()
    cfg = _stream_config()
    g = _filter(cfg)
    g.setFrame(io_.random_texture(240, 320, seed=49))
    g.findNewFeatures(10)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(pkg.EkfError) as e:
            g.findNewFeatures(5, min_distance=bad)
        assert e.value.status == 1
    # a huge finite distance: exactly one corner (the strongest) is accepted
    assert len(g.findNewFeatures(50, min_distance=1e300, add=False)) == 1
    # seed without a frame: refused before any change
    h = _filter(cfg)
    for (u, v) in g.findNewFeatures(10, add=False):
        h.addFeature((float(u), float(v)))
    h.setFeatureTrack(2, remove_flag=1)
    n0 = h.numOfFeatures()
    with pytest.raises(pkg.EkfError) as e:
        h.endUpdate(seed=True)
    assert e.value.status == 4 and h.numOfFeatures() == n0
    r = h.endUpdate(seed=False)                                       # the rest of the rule works without a frame
    assert list(r["removed"]) == [2] and r["n_seeded"] == MIN_FEATURES - r["n_visible"]
    g.close()
    h.close()


# ---------------------------------------------------------------------------------------------
# the stream on 2 ranks sharing the GPU, against the plain filter
# ---------------------------------------------------------------------------------------------
SHARD_FRAMES = 16


def _shard_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = load_package()
    from ekf_monoslam_amd import sharded
    cfg = _stream_config()
    world_img = _stream_world()
    res = {}
    for tag in ("plain", "sharded"):
        g = pkg.VSlamFilter(cfg, capacity_features=128, dtype=np.float32)
        g.setDt(1.0 / 30.0)
        g.setFrame(_stream_frame(world_img, 0))
        g.findNewFeatures(-1)
        if tag == "sharded":
            sharded.configure(g, rank, world)
        recs = []
        for f in range(1, SHARD_FRAMES + 1):
            _, z, found, tb, ib, r = _device_frame(g, _stream_frame(world_img, f), False)
            ri, nf = g.featureIds()
            nt, inn, cen, rem = g.featureTrack()
            pos, cod = g.featureLayout()
            mu = g.getFullState()
            S = g.getFullSigma()
            if tag == "sharded":
                info = sharded.shard_info(g)
                rb, re_ = info.row_begin, info.row_end                  # the rows this rank keeps valid
            else:
                rb, re_ = 0, len(mu)
            recs.append(dict(found=found, z=z, removed=np.asarray(r["removed"]), n_visible=r["n_visible"],
                             n_seeded=r["n_seeded"], ri=ri, nf=nf, nt=nt, inn=inn, cen=cen, rem=rem, pos=pos, cod=cod,
                             arch=g.numArchived(), mu=mu, S=S, own=(rb, re_)))
        g.synchronize()
        res[tag] = recs
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_end_update_stream_sharded_two_ranks_matches_plain():
    """The fp32 stream on 2 ranks sharing the GPU: every integer output (matches, removed set, n_visible, n_seeded,
    real_index, n_find, the track state, the layout, the archive count) is identical to the plain filter's, each rank's
    rows of mu / Sigma equal to fp32 rounding."""
    import torch.multiprocessing as mp
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    fired = {"removed": 0, "seeded": 0}
    worst = 0.0
    for rank in range(world):
        P, Sh = out[rank]["plain"], out[rank]["sharded"]
        for f, (p, s) in enumerate(zip(P, Sh)):
            for k in ("found", "z", "removed", "ri", "nf", "nt", "inn", "cen", "rem", "pos", "cod"):
                assert np.array_equal(p[k], s[k]), (rank, f, k)
            for k in ("n_visible", "n_seeded", "arch"):
                assert p[k] == s[k], (rank, f, k)
            rb, re_ = s["own"]
            rows = sorted(set(range(14)) | set(range(rb, re_)))            # camera rows + the rank's own rows
            # mu / Sigma: the sharded update sums its products in another order than the plain one at this size (the
            # image-side sharded test sees the same: scores equal to rounding after a sharded update); the rows are
            # held to fp32 rounding, everything the end of update decides on is exact (above)
            e_mu = float(np.abs(p["mu"] - s["mu"]).max() / np.abs(p["mu"]).max())
            e_S = float(np.abs(p["S"][rows] - s["S"][rows]).max() / np.abs(p["S"][rows]).max())
            worst = max(worst, e_mu, e_S)
            assert e_mu < 1e-4 and e_S < 1e-4, (rank, f, e_mu, e_S)
            fired["removed"] += len(p["removed"])
            fired["seeded"] += p["n_seeded"]
    print("sharded stream: largest relative mu / Sigma-row difference", worst, fired)
    assert fired["removed"] > 0 and fired["seeded"] > 0, fired
