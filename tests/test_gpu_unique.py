"""The runner-up cost and the uniqueness test on the device against tests/unique_oracle.py: the runner-up of
every cost curve exactly equal on the cases of tests/unique_scene.py; the four existing maps byte for byte through the twins;
the switch off; the filter at u = 0 against ekf_dense_filter and at u = 5, 30, 100 against the oracle, with its points and
the fusion; the argument and state errors; a living filter; and a recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py)

import dense_oracle as do
import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs
import unique_oracle as uo
import unique_scene as us

pytestmark = pytest.mark.gpu

MAPS = ("plane", "cost", "views", "depth")
KINDS = ("k_plane_sweep_unique", "k_plane_sweep_census_unique", "k_plane_sweep_best_unique", "k_plane_sweep_best_census_unique",
         "k_sgm_winner_unique", "k_depth_filter_unique")
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


def _case(case):
    """(views, the oracle's five maps) of a case, computed once and shared."""
    if case[0] not in _ORACLE:
        _ORACLE[case[0]] = us.case_oracle(case)
    return _ORACLE[case[0]]


def _flat():
    """(scene, the oracle's sweeps of slots 0, 1, 2) of the first row of the flat-patch table, computed once and shared."""
    if "flat" not in _ORACLE:
        _ORACLE["flat"] = us.flat_row(us.FLAT_ROWS[0])[:2]
    return _ORACLE["flat"]


def _loaded(pkg, views, slots, w, h, keep=True):
    d = pkg.DenseStereo(w, h, max_views=max(slots) + 1)
    for s in slots:
        d.set_view(s, *views[s])
    if keep:
        d.keep_runner_up(True)
    return d


def _sweep(d, case, ref=0, src=None):
    name, w, h, D, radius, trunc, src0, census, n_best, paths, p1, p2, _ = case
    kw = dict(cost="census" if census else "ad", best=n_best or None)
    src = src0 if src is None else src
    if paths:
        d.sweep_sgm(ref, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, p1, p2, paths, **kw)
    else:
        d.sweep(ref, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, **kw)


def _kind(case):
    """The index of the twin a case launches among KINDS."""
    census, n_best, paths = case[7], case[8], case[9]
    return 4 if paths else 2 * (n_best > 0) + census


def _profiles(d):
    """Every launch count of the four existing profile getters, in one list."""
    return [v[1] for g in (d.get_profile, d.get_sgm_profile, d.get_census_profile, d.get_best_profile) for v in g().values()]


def _unique_launches(d):
    return [v[1] for v in d.get_unique_profile().values()]


def _flat_swept(pkg, keep=True):
    """A handle with the flat-plane scene in slots 0, 1, 2, each swept against the other two as the table says."""
    scene, swept = _flat()
    d = _loaded(pkg, scene, (0, 1, 2), ds.W, ds.H, keep)
    row = us.FLAT_ROWS[0]
    for s in (0, 1, 2):
        d.sweep(s, [o for o in (0, 1, 2) if o != s], ds.W_MIN, ds.W_MAX, us.FLAT_PLANES, row[3], row[4])
    return d, scene, swept


@pytest.mark.parametrize("case", us.CASES, ids=[c[0] for c in us.CASES])
def test_runner_up_equals_the_oracle(pkg, case):
    name, w, h = case[:3]
    views, want = _case(case)
    d = _loaded(pkg, views, (0,) + tuple(case[6]), w, h)
    d.profile(True)
    _sweep(d, case)
    got = dict(d.depth(0), runner=d.runner_up(0))
    for key in MAPS + ("runner",):
        diff = int((_bits(got[key]) != _bits(want[key])).sum()) if key == "depth" else int((got[key] != want[key]).sum())
        print(name, key, "differing elements:", diff, "of", want[key].size)
    print(name, "absent:", int((got["runner"] == uo.ABSENT).sum()), "flat:", int((got["runner"] == got["cost"]).sum()))
    for key in MAPS + ("runner",):
        assert _same(got[key], want[key]), (name, key)
    assert _unique_launches(d) == [int(i == _kind(case)) for i in range(6)] and d.get_unique_profile()[KINDS[_kind(case)]][0] > 0
    _sweep(d, case)                                                 # a repeated call gives identical bytes
    assert d.runner_up(0).tobytes() == got["runner"].tobytes()
    d.profile(False)
    d.close()


@pytest.mark.parametrize("case", us.KIND_CASES, ids=[c[0] for c in us.KIND_CASES])
def test_the_twins_write_the_four_maps_unchanged_and_the_switch_off_is_today(pkg, case):
    name, w, h = case[:3]
    views, want = _case(case)
    slots = (0,) + tuple(case[6])
    never = _loaded(pkg, views, slots, w, h, keep=False)           # a handle that never saw the switch
    never.profile(True)
    _sweep(never, case)
    off = never.depth(0)
    d = _loaded(pkg, views, slots, w, h)
    d.profile(True)
    _sweep(d, case)
    on = d.depth(0)
    assert all(on[k].tobytes() == off[k].tobytes() for k in off), name
    assert all(_same(on[k], want[k]) for k in MAPS)
    assert sum(_unique_launches(d)) == 1 and sum(_profiles(d)) == sum(_profiles(never)) - 1      # the twin stands in for one kernel
    # the switch off again: the kernels and counts of the handle that never saw it, and no runner-up map
    d.keep_runner_up(False)
    for handle in (d, never):                                       # the second sweep of either: its descriptors are fresh
        handle.profile(True)                                        # (clears the counts)
        _sweep(handle, case)
    prof_d, prof_never = _profiles(d), _profiles(never)
    print(name, "profiles", prof_d)
    assert prof_d == prof_never and sum(prof_d) > 0 and _unique_launches(d) == [0] * 6 == _unique_launches(never)
    assert all(d.depth(0)[k].tobytes() == off[k].tobytes() for k in off)
    out = np.zeros((h, w), np.uint32)
    for handle in (d, never):
        assert handle._lib.ekf_dense_get_runner_up(handle._h, 0, out.ctypes.data_as(C.c_void_p)) == 4
    with pytest.raises(pkg.EkfError) as ei:
        d.runner_up(0)
    assert ei.value.status == 4
    d.close()
    never.close()


def test_uniqueness_zero_is_the_existing_filter(pkg):
    d, scene, swept = _flat_swept(pkg, keep=False)                  # u = 0 needs no runner-up map
    d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE)
    old = d.depth(0, filtered=True)
    d.profile(True)
    src = np.array([1, 2], np.int32)
    assert d._lib.ekf_dense_filter_unique(d._h, 0, src.ctypes.data_as(C.c_void_p), 2, us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, 0) == 0
    new = d.depth(0, filtered=True)
    assert all(new[k].tobytes() == old[k].tobytes() for k in old)
    fd, fp = us.flat_filter(scene, swept, 0)
    assert _same(new["depth"], fd) and _same(new["plane"], fp)
    assert d.get_profile()["k_depth_filter_points"][1] == 1 and _unique_launches(d) == [0] * 6
    d.profile(False)
    d.close()


def test_the_filter_its_points_and_the_fusion_equal_the_oracle(pkg):
    d, scene, swept = _flat_swept(pkg)
    for s in (0, 1, 2):
        assert _same(d.runner_up(s), swept[s]["runner"]) and all(_same(d.depth(s)[k], swept[s][k]) for k in MAPS)
    d.profile(True)
    kept = {}
    for n, u in enumerate((5, 30, 100)):
        fd, fp = us.flat_filter(scene, swept, u)
        d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=u)
        f = d.depth(0, filtered=True)
        kept[u] = int((fd > 0).sum())
        print("u", u, "kept", kept[u], "of", int((swept[0]["depth"] > 0).sum()))
        assert _same(f["depth"], fd) and _same(f["plane"], fp)
        assert _same(d.points(0, filtered=True), do.points(fd, scene[0][1], scene[0][2]))
        assert _unique_launches(d) == [0] * 5 + [n + 1] and d.get_profile()["k_depth_filter_points"][1] == n + 1    # (the points)
    assert kept[5] > kept[30] > kept[100] == 0                      # an absolute difference of 0 somewhere: no curve is 100 % unique
    assert d.get_unique_profile()["k_depth_filter_unique"][0] > 0
    d.profile(False)
    # the filtered map integrates as any other map does
    fd, _ = us.flat_filter(scene, swept, 5)
    d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=5)
    origin, voxel, tr = np.array([-2.7, -1.8, 2.0]), 0.3, 0.6
    v = pkg.TsdfVolume(fs.DIMS, origin, voxel, tr)
    v.integrate(d, 0, True)
    vol = fo.empty_volume(fs.DIMS)
    fo.integrate(vol, fs.DIMS, origin, voxel, tr, fd, *scene[0])
    got = v.volume()
    print("voxels updated:", int(got["cnt"].sum()))
    assert _same(got["sum"], vol[0]) and _same(got["cnt"], vol[1]) and _same(got["gsum"], vol[2]) and int(got["cnt"].sum()) > 0
    v.close()
    d.close()


def test_errors_leave_the_earlier_maps_readable(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    d, scene, swept = _flat_swept(pkg)
    d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=5)
    fd, fp = us.flat_filter(scene, swept, 5)
    s12, out = np.array([1, 2], np.int32), np.zeros((ds.H, ds.W), np.uint32)

    def intact():
        f = d.depth(0, filtered=True)
        return (_same(f["depth"], fd) and _same(f["plane"], fp) and _same(d.runner_up(0), swept[0]["runner"])
                and all(_same(d.depth(0)[k], swept[0][k]) for k in MAPS))

    flt = lambda ref=0, s=s12, n=2, tol=us.FLAT_REL_TOL, agree=1, u=5: lib.ekf_dense_filter_unique(
        d._h, ref, None if s is None else P(s), n, tol, agree, u)
    assert intact()
    assert flt(u=-1) == 1 and b"uniqueness" in lib.ekf_dense_last_error(d._h) and flt(u=101) == 1 and intact()
    # everything ekf_dense_filter refuses
    assert flt(ref=3) == 1 and flt(s=None) == 1 and flt(n=0) == 1 and flt(agree=0) == 1 and flt(agree=3) == 1 and flt(tol=-0.1) == 1
    assert flt(tol=np.nan) == 1 and flt(s=np.array([1, 1], np.int32)) == 1 and flt(s=np.array([0, 1], np.int32)) == 1
    assert lib.ekf_dense_filter_unique(None, 0, P(s12), 2, 0.01, 1, 5) == 1 and lib.ekf_dense_keep_runner_up(None, 1) == 1
    assert lib.ekf_dense_get_runner_up(None, 0, P(out)) == 1 and lib.ekf_dense_get_runner_up(d._h, 0, None) == 1
    assert lib.ekf_dense_get_runner_up(d._h, -1, P(out)) == 1 and lib.ekf_dense_get_runner_up(d._h, 3, P(out)) == 1
    buf = np.zeros(6, np.float64)
    assert lib.ekf_dense_get_unique_profile(d._h, None, None) == 1 and lib.ekf_dense_get_unique_profile(None, P(buf), P(buf)) == 1
    assert intact()
    with pytest.raises(pkg.EkfError) as ei:
        d.filter(0, [1, 2], uniqueness=101)
    assert ei.value.status == 1 and intact()
    # u > 0 on a slot swept with the switch off: slot 1 is swept again without it; slot 0's maps stay
    d.keep_runner_up(False)
    row = us.FLAT_ROWS[0]
    d.sweep(1, [0, 2], ds.W_MIN, ds.W_MAX, us.FLAT_PLANES, row[3], row[4])
    assert lib.ekf_dense_get_runner_up(d._h, 1, P(out)) == 4
    assert flt(ref=1, s=np.array([0, 2], np.int32)) == 4 and b"runner-up" in lib.ekf_dense_last_error(d._h)
    assert flt(ref=1, s=np.array([0, 2], np.int32), u=0) == 0       # ... which u = 0 does not need
    assert intact()
    assert flt() == 0 and intact()                                  # slot 0 still has its map: the sources need none
    # a new pose takes the runner-up map with the swept maps
    d.set_pose(0, scene[0][2])
    assert lib.ekf_dense_get_runner_up(d._h, 0, P(out)) == 4 and lib.ekf_dense_get_depth(d._h, 0, 0, None, None, None, None) == 4
    assert flt() == 4
    assert _same(d.depth(2)["cost"], swept[2]["cost"]) and _same(d.runner_up(2), swept[2]["runner"])      # the other slots keep theirs
    d.keep_runner_up(True)
    d.sweep(0, [1, 2], ds.W_MIN, ds.W_MAX, us.FLAT_PLANES, row[3], row[4])
    assert flt() == 0 and intact()
    d.close()


def test_a_living_filter_is_untouched(pkg):
    """Sweeps with the runner-up and a uniqueness filter beside a filter: its state, Sigma and launch counters stay bitwise
    the same."""
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=16, dtype=np.float32)
    for i in range(4):
        assert g.addFeature((40.0 + 30.0 * i, 50.0 + 20.0 * i)) == 1
    g.synchronize()
    snap = lambda: (g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts())
    before = snap()
    for case in (us.PLAIN_CASES[1], us.SGM_CASES[0]):
        views, want = _case(case)
        d = _loaded(pkg, views, (0,) + tuple(case[6]), case[1], case[2])
        _sweep(d, case)
        assert _same(d.runner_up(0), want["runner"])
        d.close()
    d, scene, swept = _flat_swept(pkg)
    d.filter(0, [1, 2], us.FLAT_REL_TOL, us.FLAT_MIN_AGREE, uniqueness=5)
    assert _same(d.depth(0, filtered=True)["depth"], us.flat_filter(scene, swept, 5)[0])
    d.close()
    assert snap() == before
    g.close()


def test_recording_with_the_uniqueness_test(pkg, tmp_path):
    """Five small synthetic key frames, the middle of each image without texture, through
    depth_maps_from_recording(uniqueness=5) against the oracle driven from the same files; uniqueness=0 is today's output."""
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
    run = lambda **extra: pkg.depth_maps_from_recording(str(rec), None, neighbours=1, rel_tol=0.3, min_agree=1, **kw, **extra)
    dropped = 0
    for u, maps in ((5, run(uniqueness=5)), (0, run(uniqueness=0)), (0, run())):
        for i, m in enumerate(maps):
            fd, fp = uo.unique_filter(swept[i]["depth"], swept[i]["plane"], swept[i]["cost"], swept[i]["runner"], K, poses[i],
                                      [(swept[j]["depth"], K, poses[j]) for j in near[i]], 0.3, 1, u)
            assert _same(m.swept_depth, swept[i]["depth"]) and _same(m.cost, swept[i]["cost"]) and _same(m.views, swept[i]["views"]), i
            assert _same(m.depth, fd) and _same(m.plane, fp) and _same(m.points, do.points(fd, K, poses[i])), (u, i)
            if u:
                assert _same(m.runner_up, swept[i]["runner"])
                plain = do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i],
                                            [(swept[j]["depth"], K, poses[j]) for j in near[i]], 0.3, 1)[0]
                dropped += int(((plain > 0) & ~(fd > 0)).sum())
            else:
                assert m.runner_up is None
    print("pixels the uniqueness test dropped over the five maps:", dropped)
    assert dropped > 0
    with pytest.raises(ValueError):
        run(uniqueness=101)
