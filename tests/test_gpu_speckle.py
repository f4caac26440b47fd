"""The speckle filter on the device against tests/speckle_oracle.py, everything bit for bit: label, size, depth
bits and plane of every case of tests/speckle_scene.py through ``speckle_maps`` (the shapes and patterns at which a tiled
labelling kernel can go wrong), the two 640 x 480 maps against analytic expectations, a slot's filtered map with its points,
segments and fusion, the state and argument errors, the launch counts, and a recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py)

import dense_oracle as do
import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs
import speckle_oracle as so
import speckle_scene as sc
import unique_oracle as uo
import unique_scene as us

pytestmark = pytest.mark.gpu

KINDS = ("k_speckle_label", "k_speckle_merge", "k_speckle_count", "k_speckle_apply")
_ORACLE = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got) if got.dtype.kind == "f" else got,
                                                                                  _bits(want) if want.dtype.kind == "f" else want)


def _launches(d):
    return [v[1] for v in d.get_speckle_profile().values()]


def _other_profiles(d):
    """Every launch count of the five existing profile getters, in one list."""
    return [v[1] for g in (d.get_profile, d.get_sgm_profile, d.get_census_profile, d.get_best_profile, d.get_unique_profile)
            for v in g().values()]


def _flat():
    """(scene, the oracle's sweeps of slots 0, 1, 2) of the first row of the flat-patch table, computed once and shared."""
    if "flat" not in _ORACLE:
        _ORACLE["flat"] = us.flat_row(us.FLAT_ROWS[0])[:2]
    return _ORACLE["flat"]


def _flat_filtered(pkg):
    """A handle with the flat-plane scene in slots 0, 1, 2, each swept against the other two with its runner-up, and slot 0
    filtered at u = 5; with the scene, the oracle's sweeps and the oracle's filtered (depth, plane)."""
    scene, swept = _flat()
    d = pkg.DenseStereo(ds.W, ds.H, max_views=3)
    for s in (0, 1, 2):
        d.set_view(s, *scene[s])
    d.keep_runner_up(True)
    row = us.FLAT_ROWS[0]
    for s in (0, 1, 2):
        d.sweep(s, [o for o in (0, 1, 2) if o != s], ds.W_MIN, ds.W_MAX, us.FLAT_PLANES, row[3], row[4])
    d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=us.FLAT_U)
    if "flat_filter" not in _ORACLE:
        _ORACLE["flat_filter"] = us.flat_filter(scene, swept, us.FLAT_U)
    return d, scene, swept, _ORACLE["flat_filter"]


@pytest.mark.parametrize("case", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_speckle_maps_equal_the_oracle(pkg, case):
    name, w, h, _, max_diff, min_size = case
    plane = sc.plane_map(case)
    depth = sc.depth_map(plane)
    want = so.speckle_filter(depth, plane, min_size, max_diff)
    keep_p, keep_d = plane.copy(), depth.copy()
    d = pkg.DenseStereo(w, h, max_views=1)
    d.profile(True)
    got = d.speckle_maps(depth, plane, min_size, max_diff)
    for key in ("label", "size", "plane", "depth"):
        print(name, key, "differing elements:", int((_bits(got[key]) != _bits(want[key])).sum()) if key == "depth"
              else int((got[key] != want[key]).sum()), "of", want[key].size)
    print(name, "segments", int((want["label"].reshape(-1) == np.arange(w * h)).sum()), "kept", int((want["plane"] >= 0).sum()))
    for key in ("label", "size", "plane", "depth"):
        assert _same(got[key], want[key]), (name, key)
    assert np.array_equal(plane, keep_p) and np.array_equal(_bits(depth), _bits(keep_d))      # the inputs are not modified
    assert _launches(d) == [1, 1, 1, 1] and sum(_other_profiles(d)) == 0
    # min_size = 1 removes nothing; a second pass over the output removes nothing more
    one = d.speckle_maps(depth, plane, 1, max_diff)
    valid = plane >= 0
    assert np.array_equal(one["plane"][valid], plane[valid]) and np.array_equal(_bits(one["depth"])[valid], _bits(depth)[valid])
    assert _same(one["label"], want["label"]) and _same(one["size"], want["size"])
    again = d.speckle_maps(got["depth"], got["plane"], min_size, max_diff)
    assert _same(again["depth"], got["depth"]) and _same(again["plane"], got["plane"])
    d.profile(False)
    d.close()


def test_a_difference_that_would_overflow_links_nothing(pkg):
    top = 2 ** 31 - 1
    plane = np.full((sc.TH + 1, sc.TW + 1), -1, np.int32)
    plane[0, :3] = (0, top, 0)                                       # inside a tile
    plane[1, :3] = (top, top - 1, top)
    plane[5, sc.TW - 1:] = (0, top)                                  # across a vertical border
    plane[sc.TH - 1:, 7] = (top, 0)                                  # across a horizontal one
    plane[sc.TH - 1:, 9] = (top, top - 1023)                         # ... and a link at the largest max_diff
    depth = sc.depth_map(plane)
    want = so.speckle_filter(depth, plane, 2, 1023)
    d = pkg.DenseStereo(plane.shape[1], plane.shape[0], max_views=1)
    got = d.speckle_maps(depth, plane, 2, 1023)
    assert all(_same(got[k], want[k]) for k in ("label", "size", "plane", "depth"))
    assert sorted(np.unique(want["size"]).tolist()) == [0, 1, 2, 4]
    d.close()


def test_vga_one_plane_and_serpentine_analytically(pkg):
    """640 x 480.  One plane: label 0 and size 307 200 everywhere, 307 200 counts to one word (more than 16 bits).  The
    serpentine: one segment of 153 840 pixels across 600 tiles.  No oracle: the expectations are closed forms."""
    w, h = 640, 480
    d = pkg.DenseStereo(w, h, max_views=1)
    plane = sc.one_plane(w, h)
    depth = sc.depth_map(plane)
    got = d.speckle_maps(depth, plane, w * h, 0)
    assert (got["label"] == 0).all() and (got["size"] == w * h).all()
    assert np.array_equal(got["plane"], plane) and np.array_equal(_bits(got["depth"]), _bits(depth))
    got = d.speckle_maps(depth, plane, w * h + 1, 0)                 # one pixel more than there is: everything goes
    assert (got["size"] == w * h).all() and (got["plane"] == -1).all() and (got["depth"] == 0).all()
    plane = sc.serpentine(w, h)
    depth = sc.depth_map(plane)
    n = sc.serpentine_size(w, h)
    valid = plane >= 0
    assert n == 153840 == int(valid.sum())
    got = d.speckle_maps(depth, plane, n, 0)
    assert (got["label"][valid] == 0).all() and (got["label"][~valid] == so.NONE).all()
    assert (got["size"][valid] == n).all() and (got["size"][~valid] == 0).all()
    assert np.array_equal(got["plane"], plane) and np.array_equal(_bits(got["depth"])[valid], _bits(depth)[valid])
    assert (got["depth"][~valid] == 0).all()
    d.close()


def test_launch_counts_do_not_depend_on_the_content(pkg):
    d = pkg.DenseStereo(sc.W3, sc.H3, max_views=1)
    counts = []
    for pat in ("all_invalid", "serpentine"):
        plane = sc.PATTERNS[pat](sc.W3, sc.H3)
        d.profile(True)
        d.speckle_maps(sc.depth_map(plane), plane, sc.MIN_SIZE, 0)
        counts.append(_launches(d))
        assert all(v[0] > 0 for v in d.get_speckle_profile().values())
    assert counts[0] == counts[1] == [1, 1, 1, 1]
    assert tuple(d.get_speckle_profile()) == KINDS
    d.profile(False)
    d.close()


def test_a_slot_through_the_filter_its_points_segments_and_the_fusion(pkg):
    d, scene, swept, (fd, fp) = _flat_filtered(pkg)
    want = so.speckle_filter(fd, fp, 4, 1)
    assert int((want["plane"] >= 0).sum()) < int((fp >= 0).sum())   # the scene has speckles at u = 5
    before = {s: d.depth(s) for s in (0, 1, 2)}
    runner = {s: d.runner_up(s) for s in (0, 1, 2)}
    d.profile(True)
    for call in (1, 2):                                             # a second identical call changes nothing
        d.filter_speckle(0, 4, 1)
        f = d.depth(0, filtered=True)
        print("call", call, "kept", int((f["plane"] >= 0).sum()), "of", int((fp >= 0).sum()))
        assert _same(f["depth"], want["depth"]) and _same(f["plane"], want["plane"])
        assert _same(d.points(0, filtered=True), do.points(want["depth"], scene[0][1], scene[0][2]))
        label, size = d.segments(0)
        if call == 1:
            assert _same(label, want["label"]) and _same(size, want["size"])
        else:                                                       # the segments of what the first call left
            kept = want["plane"] >= 0
            assert np.array_equal(label[kept], want["label"][kept]) and np.array_equal(size[kept], want["size"][kept])
            assert (label[~kept] == so.NONE).all() and (size[~kept] == 0).all()
        assert _launches(d) == [call] * 4
    # the swept map and the other slots are byte for byte what they were
    for s in (0, 1, 2):
        now = d.depth(s)
        assert all(now[k].tobytes() == before[s][k].tobytes() for k in now) and d.runner_up(s).tobytes() == runner[s].tobytes()
        assert all(_same(now[k], swept[s][k]) for k in ("plane", "cost", "views", "depth"))
    d.profile(False)
    # the filtered map integrates as any other map does
    origin, voxel, tr = np.array([-2.7, -1.8, 2.0]), 0.3, 0.6
    v = pkg.TsdfVolume(fs.DIMS, origin, voxel, tr)
    v.integrate(d, 0, True)
    vol = fo.empty_volume(fs.DIMS)
    fo.integrate(vol, fs.DIMS, origin, voxel, tr, want["depth"], *scene[0])
    got = v.volume()
    print("voxels updated:", int(got["cnt"].sum()))
    assert _same(got["sum"], vol[0]) and _same(got["cnt"], vol[1]) and _same(got["gsum"], vol[2]) and int(got["cnt"].sum()) > 0
    v.close()
    # filter afterwards gives today's filtered map again, and the segments are gone with the map they belonged to
    d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=us.FLAT_U)
    f = d.depth(0, filtered=True)
    assert _same(f["depth"], fd) and _same(f["plane"], fp)
    with pytest.raises(pkg.EkfError) as ei:
        d.segments(0)
    assert ei.value.status == 4
    d.close()


def test_state_and_argument_errors_launch_nothing(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    d, scene, swept, (fd, fp) = _flat_filtered(pkg)
    row = us.FLAT_ROWS[0]
    d.profile(True)
    n = ds.W * ds.H
    lab, siz = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    dep, pla = np.ones(n, np.float32), np.zeros(n, np.int32)
    seg = lambda slot=0: lib.ekf_dense_get_segments(d._h, slot, P(lab), P(siz))

    def intact():
        f = d.depth(0, filtered=True)
        return _same(f["depth"], fd) and _same(f["plane"], fp) and _launches(d) == [0, 0, 0, 0]

    # arguments: EKF_ERR_ARG (1), before the device is touched
    flt = lib.ekf_dense_filter_speckle
    assert flt(d._h, 0, 0, 1) == 1 and b"min_size" in lib.ekf_dense_last_error(d._h) and flt(d._h, 0, (1 << 26) + 1, 1) == 1
    assert flt(d._h, 0, 4, -1) == 1 and flt(d._h, 0, 4, 1024) == 1 and flt(d._h, -1, 4, 1) == 1 and flt(d._h, 3, 4, 1) == 1
    assert flt(None, 0, 4, 1) == 1
    host = lib.ekf_dense_speckle_host
    assert host(d._h, P(dep), P(pla), 0, 1, None, None) == 1 and host(d._h, P(dep), P(pla), 4, -1, None, None) == 1
    assert host(d._h, P(dep), P(pla), 4, 1024, None, None) == 1 and host(d._h, None, P(pla), 4, 1, None, None) == 1
    assert host(d._h, P(dep), None, 4, 1, None, None) == 1 and host(None, P(dep), P(pla), 4, 1, None, None) == 1
    assert seg(-1) == 1 and seg(3) == 1 and lib.ekf_dense_get_segments(None, 0, P(lab), P(siz)) == 1
    buf = np.zeros(4, np.float64)
    assert lib.ekf_dense_get_speckle_profile(d._h, None, None) == 1 and lib.ekf_dense_get_speckle_profile(None, P(buf), P(buf)) == 1
    with pytest.raises(pkg.EkfError) as ei:
        d.filter_speckle(0, 0)
    assert ei.value.status == 1
    with pytest.raises(ValueError):
        d.speckle_maps(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.int32), 4)
    # state: EKF_ERR_STATE (4).  Slots 1 and 2 are swept, not filtered; no call has made segments yet
    assert flt(d._h, 1, 4, 1) == 4 and b"no such map" in lib.ekf_dense_last_error(d._h) and seg(0) == 4 and seg(1) == 4
    assert intact()
    # ... and after a call: its slot alone, until a setter, a sweep, a filter or the host call
    want = so.speckle_filter(fd, fp, 4, 1)
    refilter = lambda: d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=us.FLAT_U)

    def fresh():
        refilter()
        d.filter_speckle(0, 4, 1)
        assert seg(0) == 0 and np.array_equal(lab.reshape(ds.H, ds.W), want["label"]) and np.array_equal(siz.reshape(ds.H, ds.W), want["size"])
        assert lib.ekf_dense_get_segments(d._h, 0, None, None) == 0 and seg(1) == 4 and seg(2) == 4

    fresh()
    refilter()                                                      # a filter of the slot
    assert seg(0) == 4
    fresh()
    assert host(d._h, P(dep), P(pla), 4, 1, None, P(siz)) == 0 and (siz == n).all() and seg(0) == 4      # the host call takes the planes
    assert _same(d.depth(0, filtered=True)["plane"], want["plane"])                                    # ... and touches no slot
    fresh()
    d.sweep(0, [1, 2], ds.W_MIN, ds.W_MAX, us.FLAT_PLANES, row[3], row[4])                              # a sweep
    assert seg(0) == 4 and flt(d._h, 0, 4, 1) == 4
    fresh()
    d.set_pose(0, scene[0][2])                                      # a setter
    assert seg(0) == 4 and flt(d._h, 0, 4, 1) == 4
    d.sweep(0, [1, 2], ds.W_MIN, ds.W_MAX, us.FLAT_PLANES, row[3], row[4])
    fresh()
    d.filter(1, [0, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE)          # another slot's filter reads the swept maps: slot 0 keeps its segments
    assert seg(0) == 0 and seg(1) == 4
    d.filter_speckle(1, 4, 1)                                       # ... until the planes change hands
    assert seg(1) == 0 and seg(0) == 4
    d.profile(False)
    d.close()


def test_a_living_filter_is_untouched(pkg):
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=16, dtype=np.float32)
    for i in range(4):
        assert g.addFeature((40.0 + 30.0 * i, 50.0 + 20.0 * i)) == 1
    g.synchronize()
    snap = lambda: (g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts())
    before = snap()
    d, scene, swept, (fd, fp) = _flat_filtered(pkg)
    d.filter_speckle(0, 4, 1)
    assert _same(d.depth(0, filtered=True)["plane"], so.speckle_filter(fd, fp, 4, 1)["plane"])
    d.close()
    assert snap() == before
    g.close()


def test_recording_with_the_speckle_filter(pkg, tmp_path):
    """The five synthetic key frames of test_gpu_unique.py's recording through
    depth_maps_from_recording(speckle=(4, 1), uniqueness=5) against the oracles driven from the same files; speckle=None is the
    parent's output and launches nothing of the speckle filter."""
    from ekf_monoslam_amd import dense, keyframes
    n, w, h = 5, 24, 16
    K = np.array([32.0, 32.0, 11.5, 7.5])
    rec = tmp_path / "rec"
    rec.mkdir()
    pkg.formats.write_camera(str(rec / "camera.txt"), K)
    ids = [3 + 2 * i for i in range(n)]
    with open(rec / "nodes_and_prjcts.txt", "w") as fh:
        for i, kid in enumerate(ids):
            pose = np.array([0.11 * i, 0.01 * (i % 3), 0.0, 1.0, 0.002 * i, -0.001 * i, 0.0], np.float32)
            fh.write(pkg.formats.pose_record(kid, pose, None))
            img = np.clip(ds.texture(0.13 * np.arange(w)[None, :] + 0.11 * i, 0.17 * np.arange(h)[:, None]), 0, 255).astype(np.uint8)
            img[4:12, 8:17] = 128
            keyframes.write_pgm(str(rec / ("%d.pgm" % kid)), img)
    kw = dict(w_min=0.1, w_max=0.6, planes=5, radius=1, trunc=50)
    Kf, fids, poses, images = dense.read_recording(str(rec))
    near = [dense.neighbours_of(i, n, 1) for i in range(n)]
    swept = [uo.sweep(images[i], K, poses[i], [(images[j], K, poses[j]) for j in near[i]], kw["w_min"], kw["w_max"], kw["planes"],
                      kw["radius"], kw["trunc"]) for i in range(n)]
    run = lambda **extra: pkg.depth_maps_from_recording(str(rec), None, neighbours=1, rel_tol=0.3, min_agree=1, uniqueness=5, **kw, **extra)
    seen = []
    real = pkg.DenseStereo.get_speckle_profile

    class Spy(pkg.DenseStereo):                                     # the handle depth_maps_from_recording makes: its counts at close
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.profile(True)

        def close(self):
            if getattr(self, "_h", None):
                seen.append([v[1] for v in real(self).values()])
            super().close()

    dropped = 0
    old = dense.DenseStereo
    dense.DenseStereo = Spy
    try:
        results = [(spk, run(**({} if spk is None else dict(speckle=spk)))) for spk in ((4, 1), 4, (3, 0), None)]
    finally:
        dense.DenseStereo = old
    print("launches of the four kernels per run:", seen)
    assert seen == [[n] * 4, [n] * 4, [n] * 4, [0] * 4]
    for spk, maps in results:
        for i, m in enumerate(maps):
            fd, fp = uo.unique_filter(swept[i]["depth"], swept[i]["plane"], swept[i]["cost"], swept[i]["runner"], K, poses[i],
                                      [(swept[j]["depth"], K, poses[j]) for j in near[i]], 0.3, 1, 5)
            assert _same(m.swept_depth, swept[i]["depth"]) and _same(m.cost, swept[i]["cost"]) and _same(m.runner_up, swept[i]["runner"])
            if spk is None:
                assert m.segment_size is None and _same(m.depth, fd) and _same(m.plane, fp)
                assert _same(m.points, do.points(fd, K, poses[i]))
                continue
            min_size, max_diff = (spk, 1) if isinstance(spk, int) else spk
            want = so.speckle_filter(fd, fp, min_size, max_diff)
            assert _same(m.depth, want["depth"]) and _same(m.plane, want["plane"]) and _same(m.segment_size, want["size"]), (spk, i)
            assert _same(m.points, do.points(want["depth"], K, poses[i]))
            dropped += int(((fp >= 0) & (want["plane"] < 0)).sum())
    print("pixels the speckle filter dropped over the runs:", dropped)
    assert dropped > 0
