"""The best-K source selection on the device against tests/best_oracle.py: the four maps and, where the case
aggregates, both volumes exactly equal on the cases of tests/best_scene.py; n_best = n_src against the four existing sweeps
byte for byte, through the new kernels (the profiles); the filter, the points and the fusion on a best-K map; the argument
and state errors; a living filter; and a recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py)

import best_oracle as bo
import best_scene as bs
import dense_oracle as do
import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs

pytestmark = pytest.mark.gpu

MAPS = ("plane", "cost", "views", "depth")
BEST_KINDS = ("k_plane_sweep_best", "k_plane_sweep_best_census", "k_sweep_volume_best", "k_sweep_volume_best_census")
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


def _loaded(pkg, views, slots, w, h):
    d = pkg.DenseStereo(w, h, max_views=bs.MAX_VIEWS)
    for s in slots:
        d.set_view(s, *views[s])
    return d


def _case(case):
    """(views, the oracle's result) of a case, computed once and shared."""
    if case[0] not in _ORACLE:
        _ORACLE[case[0]] = bs.case_oracle(case)
    return _ORACLE[case[0]]


def _sweep(d, case, ref=0, src=None):
    name, w, h, D, radius, trunc, src0, n_best, census, paths, p1, p2 = case
    cost = "census" if census else "ad"
    src = src0 if src is None else src
    if paths:
        d.sweep_sgm(ref, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, p1, p2, paths, cost=cost, best=n_best)
    else:
        d.sweep(ref, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost=cost, best=n_best)


def _launches(d):
    return [v[1] for v in d.get_best_profile().values()]


@pytest.mark.parametrize("case", bs.CASES, ids=[c[0] for c in bs.CASES])
def test_maps_and_volumes_equal_the_oracle(pkg, case):
    name, w, h, D, radius, trunc, src, n_best, census, paths, p1, p2 = case
    views, want = _case(case)
    d = _loaded(pkg, views, (0,) + tuple(src), w, h)
    _sweep(d, case)
    got = d.depth(0)
    keys = MAPS
    if paths:
        got.update(C=d.volume(0, aggregated=False), S=d.volume(0))
        keys = ("C", "S") + MAPS
    for key in keys:
        diff = int((_bits(got[key]) != _bits(want[key])).sum()) if key == "depth" else int((got[key] != want[key]).sum())
        print(name, key, "differing elements:", diff, "of", want[key].size)
    for key in keys:
        assert _same(got[key], want[key]), (name, key)
    assert (got["views"] > 0).any()
    _sweep(d, case)                                                 # a repeated call gives identical bytes
    again = d.depth(0)
    assert all(again[key].tobytes() == got[key].tobytes() for key in MAPS)
    if paths:
        assert d.volume(0).tobytes() == got["S"].tobytes() and d.volume(0, aggregated=False).tobytes() == got["C"].tobytes()
    else:
        with pytest.raises(pkg.EkfError) as ei:                     # a pixel-wise best sweep owns no volume
            d.volume(0)
        assert ei.value.status == 4
    d.close()


@pytest.mark.parametrize("case", bs.IDENTITY_CASES, ids=[c[0] for c in bs.IDENTITY_CASES])
def test_all_sources_equals_the_existing_sweep_through_the_new_kernel(pkg, case):
    name, radius, trunc, src, census, paths = case
    views = bs.case_views(ds.W, ds.H)
    cost = "census" if census else "ad"
    args = (0, src, ds.W_MIN, ds.W_MAX, ds.PLANES, radius, trunc)
    p = bo.default_penalties(radius, len(src))
    d = _loaded(pkg, views, (0,) + tuple(src), ds.W, ds.H)
    if paths:
        d.sweep_sgm(*args, *p, paths, cost=cost)
        old = dict(d.depth(0), C=d.volume(0, aggregated=False), S=d.volume(0))
    else:
        d.sweep(*args, cost=cost)
        old = d.depth(0)
    d.profile(True)
    if paths:
        d.sweep_sgm(*args, None, None, paths, cost=cost, best=len(src))      # the default penalties: n = (2 r + 1)^2 best
        new = dict(d.depth(0), C=d.volume(0, aggregated=False), S=d.volume(0))
    else:
        d.sweep(*args, cost=cost, best=len(src))
        new = d.depth(0)
    assert all(new[k].tobytes() == old[k].tobytes() for k in old), name
    assert (new["views"] > 0).any() and (new["cost"] > 0).any()
    # one launch of the new kernel of this cost and stage, none of the old sweep kernels
    prof = d.get_best_profile()
    print(name, "best profile", prof)
    kind = 2 * (paths != 0) + census
    assert _launches(d) == [int(i == kind) for i in range(4)] and prof[BEST_KINDS[kind]][0] > 0
    assert d.get_profile()["k_plane_sweep"][1] == 0
    cp, sp = d.get_census_profile(), [v[1] for v in d.get_sgm_profile().values()]
    assert cp["k_plane_sweep_census"][1] == 0 and cp["k_sweep_volume_census"][1] == 0 and cp["k_census"][1] == 0    # descriptors were fresh
    assert sp == ([0] + [1] * paths + [0] * (8 - paths) + [1] if paths else [0] * 10)
    d.profile(False)
    d.close()


def test_stale_descriptors_count_under_the_census_profile(pkg):
    case = [c for c in bs.CASES if c[0] == "census_v2_b1"][0]
    views, want = _case(case)
    d = _loaded(pkg, views, (0, 1, 2), ds.W, ds.H)
    d.profile(True)
    _sweep(d, case)
    assert d.get_census_profile()["k_census"][1] == 3 and _launches(d) == [0, 1, 0, 0]
    d.set_view(2, *views[2])
    _sweep(d, case)
    assert d.get_census_profile()["k_census"][1] == 4 and _launches(d) == [0, 2, 0, 0]
    assert all(_same(d.depth(0)[k], want[k]) for k in MAPS)
    d.profile(False)
    d.close()


def test_filter_points_and_fusion_on_a_best_map(pkg):
    case = [c for c in bs.CASES if c[0] == "small_b1"][0]
    name, w, h, D, radius, trunc, src, n_best, census, paths, p1, p2 = case
    views = bs.case_views(w, h)
    slots = (0,) + tuple(src)
    d = _loaded(pkg, views, slots, w, h)
    swept = {}
    for r in slots:
        others = [s for s in slots if s != r]
        _sweep(d, case, r, others)
        swept[r] = bo.sweep(views[r][0], views[r][1], views[r][2], [views[s] for s in others], n_best, ds.W_MIN, ds.W_MAX, D,
                            radius, trunc)
    assert all(_same(d.depth(0)[k], swept[0][k]) for k in MAPS)
    fd, fp = do.geometric_filter(swept[0]["depth"], swept[0]["plane"], views[0][1], views[0][2],
                                 [(swept[s]["depth"], views[s][1], views[s][2]) for s in src], 0.05, 2)
    d.filter(0, src, 0.05, 2)
    f = d.depth(0, filtered=True)
    print("kept by the filter:", int((fd > 0).sum()), "of", int((swept[0]["depth"] > 0).sum()))
    assert (fd > 0).any() and _same(f["depth"], fd) and _same(f["plane"], fp)
    assert _same(d.points(0), do.points(swept[0]["depth"], views[0][1], views[0][2]))
    assert _same(d.points(0, filtered=True), do.points(fd, views[0][1], views[0][2]))
    origin, voxel, tr = np.array([-2.7, -1.8, 2.0]), 0.3, 0.6
    for filtered, depth in ((False, swept[0]["depth"]), (True, fd)):
        v = pkg.TsdfVolume(fs.DIMS, origin, voxel, tr)
        v.integrate(d, 0, filtered)
        vol = fo.empty_volume(fs.DIMS)
        fo.integrate(vol, fs.DIMS, origin, voxel, tr, depth, *views[0])
        got = v.volume()
        print("filtered", filtered, "voxels updated:", int(got["cnt"].sum()))
        assert _same(got["sum"], vol[0]) and _same(got["cnt"], vol[1]) and _same(got["gsum"], vol[2]) and int(got["cnt"].sum()) > 0
        v.close()
    d.close()


def test_errors_leave_the_earlier_maps_readable(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    case = [c for c in bs.CASES if c[0] == "v2_b1_t20"][0]
    name, w, h, D, radius, trunc, src, n_best, census, paths, p1, p2 = case
    views, want = _case(case)
    d = _loaded(pkg, views, (0, 1, 2), w, h)
    _sweep(d, case)
    s12 = np.array(src, np.int32)
    best = lambda ref=0, s=s12, n=2, nb=1, w0=ds.W_MIN, w1=ds.W_MAX, pl=D, r=radius, t=trunc, c=0, k=0, a=0, b=0: lib.ekf_dense_sweep_best(
        d._h, ref, None if s is None else P(s), n, nb, w0, w1, pl, r, t, c, k, a, b)
    sgm = lambda **kw: best(**dict(dict(k=8, a=18, b=144), **kw))
    assert lib.ekf_dense_sweep_best(None, 0, P(s12), 2, 1, ds.W_MIN, ds.W_MAX, D, radius, trunc, 0, 0, 0, 0) == 1
    for f in (best, sgm, lambda **kw: best(c=1, **kw), lambda **kw: sgm(c=1, **kw)):      # everything the existing sweeps refuse
        assert f(pl=1) == 1 and f(pl=1025) == 1 and f(r=-1) == 1 and f(r=5) == 1 and f(t=0) == 1 and f(t=256) == 1
        assert f(n=0) == 1 and f(s=np.arange(1, 10, dtype=np.int32), n=9, nb=1) == 1 and f(s=None) == 1
        assert f(w0=0.0) == 1 and f(w0=0.4, w1=0.4) == 1 and f(w1=np.inf) == 1 and f(w0=np.nan) == 1
        assert f(s=np.array([1, 0], np.int32)) == 1 and f(s=np.array([1, 3], np.int32)) == 1 and f(ref=3) == 1     # slot 3 is not set
        assert f(s=np.array([1, 1], np.int32)) == 1 and f(ref=-1) == 1 and f(s=np.array([1, 9], np.int32)) == 1
        assert f(nb=0) == 1 and f(nb=3) == 1 and f(nb=-1) == 1 and f(n=1, nb=2) == 1                                 # n_best in 1 .. n_src
    assert best(c=2) == 1 and best(c=-1) == 1 and best(k=2) == 1 and best(k=16) == 1 and best(k=-4) == 1
    assert best(a=1) == 1 and best(b=1) == 1 and best(a=18, b=144) == 1                                              # paths 0: p1 = p2 = 0
    assert sgm(a=0) == 1 and sgm(a=145) == 1 and sgm(b=(1 << 20) + 1) == 1 and sgm(a=-3) == 1
    buf = np.zeros(4, np.float64)
    assert lib.ekf_dense_get_best_profile(d._h, None, None) == 1 and lib.ekf_dense_get_best_profile(None, P(buf), P(buf)) == 1
    assert lib.ekf_dense_get_best_profile(d._h, P(buf), None) == 1
    assert b"ekf_dense_sweep_best" in lib.ekf_dense_last_error(d._h)
    assert lib.ekf_dense_get_volume(d._h, 0, 1, P(np.zeros((D, h, w), np.uint32))) == 4       # EKF_ERR_STATE: no volume yet
    got = d.depth(0)                                                # ... and every earlier result is still there
    assert all(_same(got[k], want[k]) for k in MAPS)
    with pytest.raises(ValueError):
        d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost="ssd", best=1)
    # the state rules of the sweeps: a new pose takes the slot's maps, the filter refuses an unswept source
    d.set_pose(0, views[0][2])
    assert lib.ekf_dense_get_depth(d._h, 0, 0, None, None, None, None) == 4
    assert best() == 0 and lib.ekf_dense_filter(d._h, 0, P(s12), 2, 0.05, 1) == 4
    assert best(t=1) == 0 and best(t=255) == 0 and best(nb=2) == 0 and sgm(a=1, b=1, k=4) == 0 and sgm(c=1, nb=2) == 0    # the ends
    assert lib.ekf_dense_get_volume(d._h, 0, 1, P(np.zeros((D, h, w), np.uint32))) == 0
    assert best() == 0 and all(_same(d.depth(0)[k], want[k]) for k in MAPS)
    assert lib.ekf_dense_get_volume(d._h, 0, 1, P(np.zeros((D, h, w), np.uint32))) == 4       # a pixel-wise sweep took the volumes
    d.close()
    # the element cap: 1024 x 1024 x 257 > 2^28, refused before the device is touched
    big = pkg.DenseStereo(1024, 1024, max_views=2)
    img = np.zeros((1024, 1024), np.uint8)
    big.set_view(0, img, ds.K, ds.RIG[0])
    big.set_view(1, img, ds.K, ds.RIG[1])
    big.sweep(0, [1], ds.W_MIN, ds.W_MAX, 2, 0, 20, best=1)
    before = big.depth(0)
    one = np.array([1], np.int32)
    assert lib.ekf_dense_sweep_best(big._h, 0, P(one), 1, 1, ds.W_MIN, ds.W_MAX, 257, 0, 20, 0, 4, 1, 1) == 1
    assert b"2^28" in lib.ekf_dense_last_error(big._h)
    after = big.depth(0)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)
    big.close()


def test_a_living_filter_is_untouched(pkg):
    """Best-K sweeps beside a filter: its state, Sigma and launch counters stay bitwise the same."""
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=16, dtype=np.float32)
    for i in range(4):
        assert g.addFeature((40.0 + 30.0 * i, 50.0 + 20.0 * i)) == 1
    g.synchronize()
    snap = lambda: (g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts())
    before = snap()
    for name in ("v2_b1_t20", "sgm8_v3_b2"):
        case = [c for c in bs.CASES if c[0] == name][0]
        views, want = _case(case)
        d = _loaded(pkg, views, (0,) + tuple(case[6]), case[1], case[2])
        _sweep(d, case)
        assert _same(d.depth(0)["cost"], want["cost"])
        d.close()
    assert snap() == before
    g.close()


def test_recording_with_best_sources(pkg, tmp_path):
    """Five small synthetic key frames through depth_maps_from_recording(best=...), also with sgm=True and cost="census",
    against the oracle driven from the same files; the end frames have one neighbour and keep min(best, 1) sources."""
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
            keyframes.write_pgm(str(rec / ("%d.pgm" % kid)), img)
    kw = dict(w_min=0.1, w_max=0.6, planes=5, radius=1, trunc=50)
    Kf, fids, poses, images = dense.read_recording(str(rec))
    near = [dense.neighbours_of(i, n, 1) for i in range(n)]
    assert sorted({len(x) for x in near}) == [1, 2]

    def check(maps, swept):
        for i, m in enumerate(maps):
            fd, fp = do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i],
                                         [(swept[j]["depth"], K, poses[j]) for j in near[i]], 0.3, 1)
            assert m.sources == tuple(ids[j] for j in near[i]), i
            assert _same(m.swept_depth, swept[i]["depth"]) and _same(m.cost, swept[i]["cost"]) and _same(m.views, swept[i]["views"]), i
            assert _same(m.depth, fd) and _same(m.plane, fp) and _same(m.points, do.points(fd, K, poses[i])), i

    def oracle(i, best, census=False, sgm=False):
        keep = min(best, len(near[i]))
        pen = (8,) + bo.default_penalties(kw["radius"], keep) if sgm else (0, 0, 0)
        return bo.sweep(images[i], K, poses[i], [(images[j], K, poses[j]) for j in near[i]], keep, kw["w_min"], kw["w_max"], kw["planes"],
                        kw["radius"], kw["trunc"], census, *pen)

    run = lambda **extra: pkg.depth_maps_from_recording(str(rec), None, neighbours=1, rel_tol=0.3, min_agree=1, **kw, **extra)
    one = [oracle(i, 1) for i in range(n)]
    check(run(best=1), one)
    check(run(best=2), [oracle(i, 2) for i in range(n)])
    check(run(best=1, sgm=True), [oracle(i, 1, sgm=True) for i in range(n)])
    check(run(best=1, cost="census"), [oracle(i, 1, census=True) for i in range(n)])
    plain = [do.sweep(images[i], K, poses[i], [(images[j], K, poses[j]) for j in near[i]], kw["w_min"], kw["w_max"], kw["planes"],
                      kw["radius"], kw["trunc"]) for i in range(n)]
    check(run(), plain)                                             # best=None: today's sweep
    assert any(not _same(a["cost"], b["cost"]) for a, b in zip(one, plain))
    with pytest.raises(ValueError):
        run(best=0)
