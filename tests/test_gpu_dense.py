"""Dense plane sweep on the device against tests/dense_oracle.py: depth (as bits), plane, cost and views of
k_plane_sweep, the filtered maps and the points of k_depth_filter_points, all exactly equal on the shapes of
tests/dense_scene.py (61 x 47 and 37 x 19: no multiple of the 32 x 16 tile; radius 0, 1, 4; trunc 255, 20; 1-3 sources;
2 and 12 planes); a view taken from a key-frame selector; set_pose; the error paths; that a filter alive in the process is
untouched; and end to end from a rectified recording through sba_add to depth maps and a PLY file."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded: the device-tensor test needs both to share one HIP runtime)

import dense_oracle as do
import dense_scene as ds
import keyframe_gpu_common as kg
import keyframe_oracle as ko
import keyframe_scene as ks
import rectify_oracle as ro
import rectify_scene as rs

pytestmark = pytest.mark.gpu

REL_TOL = 0.05
_ORACLE = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want):
    """Equal bit for bit (NaNs at equal positions with equal payload included)."""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got) if got.dtype.kind == "f" else got,
                                                                                  _bits(want) if want.dtype.kind == "f" else want)


def _oracle(case):
    """Computed once per case and shared: the sweep of every slot the filter needs, the filter of slot 0, the points."""
    name, w, h, D, radius, trunc, src = case
    if name in _ORACLE:
        return _ORACLE[name]
    views = ds.case_views(w, h)
    slots = (0,) + tuple(src)
    swept = {}
    for r in slots:
        others = [s for s in slots if s != r]
        swept[r] = do.sweep(views[r][0], views[r][1], views[r][2], [views[s] for s in others], ds.W_MIN, ds.W_MAX, D, radius, trunc)
    agree = min(2, len(src))
    fd, fp = do.geometric_filter(swept[0]["depth"], swept[0]["plane"], views[0][1], views[0][2],
                                 [(swept[s]["depth"], views[s][1], views[s][2]) for s in src], REL_TOL, agree)
    _ORACLE[name] = dict(views=views, slots=slots, swept=swept, fdepth=fd, fplane=fp, agree=agree,
                         points=do.points(swept[0]["depth"], views[0][1], views[0][2]),
                         fpoints=do.points(fd, views[0][1], views[0][2]))
    return _ORACLE[name]


def _loaded(pkg, case):
    name, w, h, D, radius, trunc, src = case
    o = _oracle(case)
    d = pkg.DenseStereo(w, h, max_views=5)
    for s in o["slots"]:
        d.set_view(s, *o["views"][s])
    return d, o


def _sweep_all(d, case, o):
    _, w, h, D, radius, trunc, src = case
    for r in o["slots"]:
        d.sweep(r, [s for s in o["slots"] if s != r], ds.W_MIN, ds.W_MAX, D, radius, trunc)


@pytest.mark.parametrize("case", ds.CASES, ids=[c[0] for c in ds.CASES])
def test_sweep_filter_and_points_equal_the_oracle(pkg, case):
    d, o = _loaded(pkg, case)
    _sweep_all(d, case, o)
    first = {r: d.depth(r) for r in o["slots"]}
    for r in o["slots"]:
        want = o["swept"][r]
        for key in ("plane", "cost", "views", "depth"):
            diff = int((_bits(first[r][key]) != _bits(want[key])).sum()) if key == "depth" else int((first[r][key] != want[key]).sum())
            print(case[0], "slot", r, key, "differing pixels:", diff, "of", want[key].size)
        for key in ("plane", "cost", "views", "depth"):
            assert _same(first[r][key], want[key]), (case[0], r, key)
    assert (first[0]["views"] > 0).any()
    # a second sweep gives identical bytes
    _sweep_all(d, case, o)
    for r in o["slots"]:
        again = d.depth(r)
        assert all(again[key].tobytes() == first[r][key].tobytes() for key in again), r
    # the filter reads swept maps only; its outputs and both point maps
    d.filter(0, case[6], REL_TOL, o["agree"])
    f = d.depth(0, filtered=True)
    print(case[0], "kept by the filter:", int((o["fdepth"] > 0).sum()), "of", int((o["swept"][0]["depth"] > 0).sum()))
    assert _same(f["depth"], o["fdepth"]) and _same(f["plane"], o["fplane"])
    assert _same(f["cost"], o["swept"][0]["cost"]) and _same(d.depth(0)["depth"], o["swept"][0]["depth"])   # swept map untouched
    assert _same(d.points(0), o["points"]) and _same(d.points(0, filtered=True), o["fpoints"])
    d.close()


def test_ply_round_trip(pkg, tmp_path):
    from ekf_monoslam_amd import dense
    case = ds.CASES[1]
    d, o = _loaded(pkg, case)
    _sweep_all(d, case, o)
    d.filter(0, case[6], REL_TOL, o["agree"])
    path = str(tmp_path / "cloud.ply")
    n = d.write_ply(path, 0, filtered=True)
    xyz, grey = dense.read_ply(path)
    ok = np.isfinite(o["fpoints"]).all(axis=2)
    assert n == int(ok.sum()) > 0 and _same(xyz, o["fpoints"][ok]) and np.array_equal(grey, o["views"][0][0][ok])
    d.close()


def test_set_pose_then_sweep_equals_a_fresh_handle(pkg):
    case = ds.CASES[1]
    name, w, h, D, radius, trunc, src = case
    d, o = _loaded(pkg, case)
    _sweep_all(d, case, o)
    moved = o["views"][1][2].copy()
    moved[:3] += [0.05, -0.02, 0.01]
    moved[3:] = [2.0, 0.02, -0.06, 0.01]                             # not normalised: normalised on entry
    d.set_pose(1, moved)
    with pytest.raises(pkg.EkfError) as ei:                         # slot 1 is stale: its map is gone, the filter refuses
        d.depth(1)
    assert ei.value.status == 4
    with pytest.raises(pkg.EkfError) as ei:
        d.filter(0, src, REL_TOL, 1)
    assert ei.value.status == 4
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)
    fresh = pkg.DenseStereo(w, h, max_views=3)
    for s in o["slots"]:
        fresh.set_view(s, o["views"][s][0], o["views"][s][1], moved if s == 1 else o["views"][s][2])
    fresh.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)
    a, b = d.depth(0), fresh.depth(0)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    views = dict(o["views"])
    views[1] = (views[1][0], views[1][1], moved)
    want = do.sweep(views[0][0], views[0][1], views[0][2], [views[s] for s in src], ds.W_MIN, ds.W_MAX, D, radius, trunc)
    assert all(_same(a[k], want[k]) for k in a)
    assert not _same(a["depth"], o["swept"][0]["depth"])             # the pose mattered
    got = d.view(1)
    assert np.array_equal(got[0], views[1][0]) and np.array_equal(got[2], np.concatenate(do.normalise_pose(moved)))
    fresh.close()
    d.close()


def test_error_paths_leave_the_results_readable(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    for bad in ((0, 47, 4), (61, 0, 4), (61, 47, 0), (61, 47, 17), (8193, 47, 4)):
        assert lib.ekf_dense_create(bad[0], bad[1], bad[2], 0, C.byref(h)) == 1 and not h
    assert lib.ekf_dense_create(61, 47, 4, 0, None) == 1
    assert lib.ekf_dense_create(61, 47, 4, 99, C.byref(h)) == 3
    case = ds.CASES[1]
    name, w, hh, D, radius, trunc, src = case
    d, o = _loaded(pkg, case)                                       # max_views = 5, slots 0, 1, 2 set
    _sweep_all(d, case, o)
    d.filter(0, src, REL_TOL, 2)
    img, K, pose = o["views"][1]
    img = np.ascontiguousarray(img)
    s12, s1 = np.array([1, 2], np.int32), np.array([1], np.int32)
    sweep = lambda ref, s, n, w0=ds.W_MIN, w1=ds.W_MAX, pl=D, r=radius, t=trunc: lib.ekf_dense_sweep(
        d._h, ref, None if s is None else P(s), n, w0, w1, pl, r, t)
    # set_view*
    assert lib.ekf_dense_set_view(None, 0, P(img), w, P(K), P(pose)) == 1
    assert lib.ekf_dense_set_view(d._h, -1, P(img), w, P(K), P(pose)) == 1 and lib.ekf_dense_set_view(d._h, 5, P(img), w, P(K), P(pose)) == 1
    assert lib.ekf_dense_set_view(d._h, 3, None, w, P(K), P(pose)) == 1 and lib.ekf_dense_set_view(d._h, 3, P(img), w - 1, P(K), P(pose)) == 1
    assert lib.ekf_dense_set_view(d._h, 3, P(img), w, None, P(pose)) == 1 and lib.ekf_dense_set_view(d._h, 3, P(img), w, P(K), None) == 1
    assert lib.ekf_dense_set_view(d._h, 3, P(img), w, P(np.array([0.0, 64, 30, 23])), P(pose)) == 1
    assert lib.ekf_dense_set_view(d._h, 3, P(img), w, P(np.array([64.0, np.nan, 30, 23])), P(pose)) == 1
    assert lib.ekf_dense_set_view(d._h, 3, P(img), w, P(K), P(np.array([0.0, 0, 0, 0, 0, 0, 0]))) == 1          # q = 0
    assert lib.ekf_dense_set_view(d._h, 3, P(img), w, P(K), P(np.array([np.inf, 0, 0, 1, 0, 0, 0]))) == 1
    assert lib.ekf_dense_set_view_device(d._h, 3, None, w, P(K), P(pose)) == 1
    assert lib.ekf_dense_set_pose(d._h, 3, P(pose)) == 1                                                           # not set
    assert lib.ekf_dense_set_pose(d._h, 1, None) == 1 and lib.ekf_dense_set_pose(d._h, 9, P(pose)) == 1
    assert lib.ekf_dense_get_view(d._h, 3, None, 0, None, None) == 4 and lib.ekf_dense_get_view(d._h, 7, None, 0, None, None) == 1
    # sweep: every limit of 15.1
    assert sweep(0, s12, 2, pl=1) == 1 and sweep(0, s12, 2, pl=1025) == 1
    assert sweep(0, s12, 2, r=-1) == 1 and sweep(0, s12, 2, r=5) == 1
    assert sweep(0, s12, 2, t=0) == 1 and sweep(0, s12, 2, t=256) == 1
    assert sweep(0, s12, 0) == 1 and sweep(0, np.arange(1, 10, dtype=np.int32), 9) == 1 and sweep(0, None, 2) == 1
    assert sweep(0, s12, 2, w0=0.0) == 1 and sweep(0, s12, 2, w0=0.4, w1=0.4) == 1 and sweep(0, s12, 2, w0=0.5, w1=0.4) == 1
    assert sweep(0, s12, 2, w1=np.inf) == 1 and sweep(0, s12, 2, w0=np.nan) == 1
    assert sweep(0, np.array([1, 0], np.int32), 2) == 1                                                           # ref among the sources
    assert sweep(0, np.array([1, 3], np.int32), 2) == 1 and sweep(3, s12, 2) == 1                                   # a slot that is not set
    assert sweep(0, np.array([1, 5], np.int32), 2) == 1 and sweep(-1, s12, 2) == 1
    # filter
    flt = lambda ref, s, n, tol=REL_TOL, m=1: lib.ekf_dense_filter(d._h, ref, P(s), n, tol, m)
    assert flt(0, s12, 2, tol=-0.1) == 1 and flt(0, s12, 2, tol=np.nan) == 1 and flt(0, s12, 2, m=0) == 1 and flt(0, s12, 2, m=3) == 1
    assert flt(0, np.array([0, 1], np.int32), 2) == 1 and flt(0, np.array([1, 3], np.int32), 2) == 1 and flt(0, s12, 0) == 1
    # getters
    buf = np.zeros((hh, w), np.float32)
    assert lib.ekf_dense_get_depth(d._h, 9, 0, P(buf), None, None, None) == 1 and lib.ekf_dense_get_depth(d._h, 0, 2, P(buf), None, None, None) == 1
    assert lib.ekf_dense_get_depth(d._h, 3, 0, P(buf), None, None, None) == 4                                       # never set
    assert lib.ekf_dense_get_depth(d._h, 1, 1, P(buf), None, None, None) == 4                                       # swept, never filtered
    assert lib.ekf_dense_get_points(d._h, 0, 0, None) == 1 and lib.ekf_dense_get_points(d._h, 1, 1, P(np.zeros((hh, w, 3)))) == 4
    assert lib.ekf_dense_get_depth(d._h, 0, 0, None, None, None, None) == 0                                         # every output may be NULL
    assert lib.ekf_dense_get_profile(d._h, None, None) == 1 and lib.ekf_dense_profile(None, 1) == 1
    assert lib.ekf_dense_last_error(d._h)                                                                           # a message was left
    # ... and every earlier result is still there
    got, f = d.depth(0), d.depth(0, filtered=True)
    assert all(_same(got[k], o["swept"][0][k]) for k in got) and _same(f["depth"], o["fdepth"]) and _same(d.depth(1)["depth"], o["swept"][1]["depth"])
    # the profile: one timed launch of each kernel
    d.profile(True)
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)
    d.filter(0, src, REL_TOL, 2)
    prof = d.get_profile()
    print("profile", prof)
    assert prof["k_plane_sweep"][1] == 1 and prof["k_depth_filter_points"][1] == 1 and prof["k_plane_sweep"][0] > 0
    d.profile(True)                                                 # a second profile(True) starts from zero
    assert set(d.get_profile().values()) == {(0.0, 0)}
    d.profile(False)
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)           # switched off, launches leave the counts where they were
    d.filter(0, src, REL_TOL, 2)
    assert set(d.get_profile().values()) == {(0.0, 0)}
    d.close()


def _kf_filter(pkg):
    """The 61 x 47 / 122 x 94 filter of tests/rectify_scene.py with XYZ features (so that Point4sba rows exist)."""
    g = pkg.VSlamFilter(rs.config(pkg.kinect_config(), rs.BARREL), capacity_features=16, dtype=np.float32)
    for i in range(ks.N_FEATURES):
        assert g.addFeature((8.0 + 8.0 * i, 8.0 + 6.0 * i)) == 1
    S = g.getFullSigma()
    n0 = g.camera_dim
    S[n0:, :] *= 1e-4
    S[:, n0:] *= 1e-4
    g.setSigmaBlock(S)
    g.convert2XYZ_ifLinearAll()
    return g


def _script(g, fr, k):
    mu = g.getFullState()
    mu[:7] = fr["pose"]
    g.setFullState(mu)
    g.setSigmaBlock(fr["sigma"].astype(g.dtype), 0, 0)
    for i in range(ks.N_FEATURES):
        g.setFeatureTrack(i, in_innovation=int(fr["in_innovation"][i]),
                          center=np.array([6.25 + 8.5 * i + 0.125 * k, 5.75 + 6.25 * i + 0.375 * (k % 3)], np.float32))


def _snapshot(g):
    return g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts()


def test_view_from_a_keyframe_selector_and_the_filter_is_untouched(pkg):
    lib = pkg.load_library()
    g = _kf_filter(pkg)
    L = ro.lens({k: getattr(g._cfg, k) for k in ro.LENS_KEYS})
    pose = np.array([0.3, 0.1, -0.2, 0.9, 0.1, 0.0, 0.2])
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    for raw in (False, True):
        sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, raw_shape=(rs.RH, rs.RW))        # a 1-channel raw selector
        w, h = (rs.RW, rs.RH) if raw else (rs.MW, rs.MH)
        d, twin = pkg.DenseStereo(w, h, 2), pkg.DenseStereo(w, h, 2)
        assert lib.ekf_dense_set_view_from_keyframe(d._h, 0, sel._h, int(raw), P(pose)) == 4        # nothing emitted yet
        for k, fr in enumerate(ks.scene_walk()[:2]):
            g.setFrameRaw(rs.raw_image(100 + fr["id"], channels=1))
            _script(g, fr, k)
            r = sel.observe(fr["id"])
        assert r.action == ko.EMIT_FIRST
        before = _snapshot(g)
        d.set_view_from_keyframe(0, sel, pose, raw=raw)
        rect = sel.emitted_image_rectified(raw)
        twin.set_view(0, rect, sel.rectified_camera(raw), pose)
        a, b = d.view(0), twin.view(0)
        assert np.array_equal(a[0], rect) and np.array_equal(a[0], b[0]) and not np.array_equal(rect, sel.emitted_raw_image() if raw else sel.emitted_image())
        assert np.array_equal(a[1], ro.camera(L, rs.SCALE if raw else 1)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        # a sweep beside the living filter: its state, Sigma and launch counters stay bitwise the same
        d.set_view(1, np.roll(rect, 1, axis=1), a[1], [0.2, 0, 0, 1, 0, 0, 0])
        twin.set_view(1, np.roll(rect, 1, axis=1), a[1], [0.2, 0, 0, 1, 0, 0, 0])
        for x in (d, twin):
            x.sweep(0, [1], 0.1, 0.5, 6, 1, 40)
        ra, rb = d.depth(0), twin.depth(0)
        assert all(ra[key].tobytes() == rb[key].tobytes() for key in ra)
        assert _snapshot(g) == before
        # the argument rules: a size mismatch, raw out of range, a NULL selector
        small = pkg.DenseStereo(rs.MW - 1, rs.MH, 1)
        assert lib.ekf_dense_set_view_from_keyframe(small._h, 0, sel._h, int(raw), P(pose)) == 1
        assert lib.ekf_dense_set_view_from_keyframe(d._h, 0, sel._h, 2, P(pose)) == 1
        assert lib.ekf_dense_set_view_from_keyframe(d._h, 0, None, 0, P(pose)) == 1
        assert lib.ekf_dense_set_view_from_keyframe(d._h, 2, sel._h, int(raw), P(pose)) == 1
        assert lib.ekf_dense_set_view_from_keyframe(d._h, 0, sel._h, int(raw), None) == 1
        assert np.array_equal(d.view(0)[0], rect)                                       # the slot kept its view
        for x in (small, twin, d, sel):
            x.close()
    # a 3-channel raw selector has no 1-channel raw image: EKF_ERR_ARG; a plain selector has no raw geometry at all
    d = pkg.DenseStereo(rs.RW, rs.RH, 1)
    for shape in ((rs.RH, rs.RW, 3), None):
        sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, raw_shape=shape)
        assert lib.ekf_dense_set_view_from_keyframe(d._h, 0, sel._h, 1, P(pose)) == 1
        sel.close()
    d.close()
    g.close()


def test_recording_to_depth_maps_end_to_end(pkg, tmp_path):
    """KeyframeRecorder(rectify=True, images=True) over the walk -> sba_add -> depth_maps_from_recording, against the oracle
    driven from the same files."""
    from ekf_monoslam_amd import dense
    g = _kf_filter(pkg)
    sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, keep_current_projections=True)
    rec = pkg.KeyframeRecorder(sel, str(tmp_path / "rec"), images=True, rectify=True)
    for k, fr in enumerate(ks.scene_walk()[:9]):
        g.setFrame(kg.image_of(fr["id"], (rs.MH, rs.MW)))
        _script(g, fr, k)
        rec.observe(fr["id"])
    files = rec.finish()
    sel.close()
    g.close()
    assert len(rec.ids) >= 3
    nodes_out = str(tmp_path / "Nodes_Out.txt")
    pkg.sba_add(*files, camera=rec.camera_path, every=3, nodes_out=nodes_out)
    kw = dict(w_min=0.02, w_max=0.3, planes=8, radius=1, trunc=60)
    maps = pkg.depth_maps_from_recording(rec.directory, nodes_out, neighbours=1, rel_tol=0.2, min_agree=1, **kw)
    K, ids, poses, images = dense.read_recording(rec.directory, nodes_out)
    assert [m.id for m in maps] == ids == rec.ids and images[0].shape == (rs.MH, rs.MW)
    assert np.array_equal(poses, pkg.formats.read_nodes_out(nodes_out)[1])              # the adjusted poses were used
    n = len(ids)
    nb = [dense.neighbours_of(i, n, 1) for i in range(n)]
    swept = [do.sweep(images[i], K, poses[i], [(images[j], K, poses[j]) for j in nb[i]], kw["w_min"], kw["w_max"], kw["planes"],
                      kw["radius"], kw["trunc"]) for i in range(n)]
    some = 0
    for i, m in enumerate(maps):
        fd, fp = do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i],
                                     [(swept[j]["depth"], K, poses[j]) for j in nb[i]], 0.2, 1)
        assert m.sources == tuple(ids[j] for j in nb[i])
        assert _same(m.swept_depth, swept[i]["depth"]) and _same(m.cost, swept[i]["cost"]) and _same(m.views, swept[i]["views"]), i
        assert _same(m.depth, fd) and _same(m.plane, fp) and _same(m.points, do.points(fd, K, poses[i])), i
        some += int((swept[i]["depth"] > 0).sum())
    assert some > 0


def test_view_from_device_memory_equals_the_host_upload(pkg):
    """A torch tensor on the device, as a column slice of a wider buffer (pitch > width): no host round trip, same slot."""
    case = ds.CASES[1]
    name, w, h, D, radius, trunc, src = case
    d, o = _loaded(pkg, case)                                       # every view uploaded from the host
    dev = pkg.DenseStereo(w, h, max_views=5)
    keep = []
    for s in o["slots"]:
        img, K, pose = o["views"][s]
        wide = torch.full((h, w + 11), 0xA5, dtype=torch.uint8, device="cuda")
        wide[:, 3:3 + w] = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        part = wide[:, 3:3 + w]
        assert part.stride(0) == w + 11 and not part.is_contiguous()
        dev.set_view(s, part, K, pose)
        keep.append(wide)
        got = dev.view(s)
        assert np.array_equal(got[0], img) and np.array_equal(got[1], K) and np.array_equal(got[2], d.view(s)[2])
    torch.cuda.synchronize()
    for x in (d, dev):
        x.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)
    a, b = d.depth(0), dev.depth(0)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and all(_same(b[k], o["swept"][0][k]) for k in b)
    # what the binding refuses before the library is called: another element type, a transposed view, a short pitch
    img, K, pose = o["views"][0]
    for bad in (torch.zeros((h, w), dtype=torch.int8, device="cuda"), torch.zeros((h, w), dtype=torch.bool, device="cuda"),
                torch.zeros((w, h), dtype=torch.uint8, device="cuda").t(), torch.zeros((h, w + 1), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            dev.set_view(0, bad, K, pose)
    assert np.array_equal(dev.view(0)[0], img)
    # a source slot named twice is an argument error, for the sweep and for the filter
    lib = pkg.load_library()
    twice = np.array([1, 1], np.int32)
    assert lib.ekf_dense_sweep(dev._h, 0, twice.ctypes.data_as(C.c_void_p), 2, ds.W_MIN, ds.W_MAX, D, radius, trunc) == 1
    assert lib.ekf_dense_filter(dev._h, 0, twice.ctypes.data_as(C.c_void_p), 2, REL_TOL, 1) == 1
    dev.close()
    d.close()


def test_recording_longer_than_the_slot_ring(pkg, tmp_path):
    """19 small synthetic key frames with 2 neighbours on each side: the 16 device slots are reused (key frame j sits in
    slot j % 16), and every map still equals the oracle driven from the same files."""
    from ekf_monoslam_amd import dense, keyframes
    n, w, h, nb = 19, 24, 16, 2
    K = np.array([32.0, 32.0, 11.5, 7.5])
    rec = tmp_path / "long"
    rec.mkdir()
    pkg.formats.write_camera(str(rec / "camera.txt"), K)
    rng = np.random.default_rng(17)
    ids = [3 + 2 * i for i in range(n)]
    with open(rec / "nodes_and_prjcts.txt", "w") as fh:
        for i, kid in enumerate(ids):
            pose = np.array([0.11 * i, 0.01 * (i % 3), 0.0, 1.0, 0.002 * i, -0.001 * i, 0.0], np.float32)
            fh.write(pkg.formats.pose_record(kid, pose, None))
            base = ds.texture(0.13 * np.arange(w)[None, :] + 0.11 * i, 0.17 * np.arange(h)[:, None])
            keyframes.write_pgm(str(rec / ("%d.pgm" % kid)), np.clip(base + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8))
    kw = dict(w_min=0.1, w_max=0.6, planes=5, radius=1, trunc=50)
    maps = pkg.depth_maps_from_recording(str(rec), None, neighbours=nb, rel_tol=0.3, min_agree=2, **kw)
    Kf, fids, poses, images = dense.read_recording(str(rec))
    assert fids == ids == [m.id for m in maps] and np.array_equal(Kf, K) and n > dense.MAX_VIEWS
    near = [dense.neighbours_of(i, n, nb) for i in range(n)]
    assert near[0] == [1, 2] and near[9] == [7, 8, 10, 11] and near[n - 1] == [n - 3, n - 2]
    swept = [do.sweep(images[i], K, poses[i], [(images[j], K, poses[j]) for j in near[i]], kw["w_min"], kw["w_max"], kw["planes"],
                      kw["radius"], kw["trunc"]) for i in range(n)]
    kept = 0
    for i, m in enumerate(maps):
        fd, fp = do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i],
                                     [(swept[j]["depth"], K, poses[j]) for j in near[i]], 0.3, min(2, len(near[i])))
        assert m.sources == tuple(ids[j] for j in near[i]), i
        assert _same(m.swept_depth, swept[i]["depth"]) and _same(m.cost, swept[i]["cost"]) and _same(m.views, swept[i]["views"]), i
        assert _same(m.depth, fd) and _same(m.plane, fp) and _same(m.points, do.points(fd, K, poses[i])), i
        kept += int((fd > 0).sum())
    assert kept > 0
