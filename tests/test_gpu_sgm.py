"""The semi-global sweep on the device against tests/sgm_oracle.py: the raw and the aggregated volume, depth
(as bits), plane, cost and views exactly equal on the cases of tests/sgm_scene.py (each the smallest shape at which one
part of the kernels can go wrong); the filter and the points on its maps; that the plain sweep, a living filter and every
earlier result are untouched; when the volumes can be read; the argument limits; and a recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py)

import dense_oracle as do
import dense_scene as ds
import sgm_oracle as so
import sgm_scene as ss

pytestmark = pytest.mark.gpu

REL_TOL = 0.05
_ORACLE = {}
CASES = ss.CASES + ss.MANY_PLANES_CASES


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got) if got.dtype.kind == "f" else got,
                                                                                  _bits(want) if want.dtype.kind == "f" else want)


def _oracle(case, ref=0):
    """Computed once per (case, reference slot) and shared."""
    if (case[0], ref) not in _ORACLE:
        _ORACLE[(case[0], ref)] = ss.case_oracle(case, ref)
    return _ORACLE[(case[0], ref)]


def _loaded(pkg, case):
    views = ss.case_views(case)
    slots = (0,) + tuple(case[6])
    d = pkg.DenseStereo(case[1], case[2], max_views=5)
    for s in slots:
        d.set_view(s, *views[s])
    return d, views, slots


def _sgm(d, case, ref=0):
    name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
    slots = (0,) + tuple(src)
    d.sweep_sgm(ref, [s for s in slots if s != ref], ds.W_MIN, ds.W_MAX, D, radius, trunc, p1, p2, paths)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_volumes_and_maps_equal_the_oracle(pkg, case):
    d, views, slots = _loaded(pkg, case)
    want = _oracle(case)
    _sgm(d, case)
    got = d.depth(0)
    got.update(C=d.volume(0, aggregated=False), S=d.volume(0))
    for key in ("C", "S", "plane", "cost", "views", "depth"):
        diff = int((_bits(got[key]) != _bits(want[key])).sum()) if key == "depth" else int((got[key] != want[key]).sum())
        print(case[0], key, "differing elements:", diff, "of", want[key].size)
    for key in ("C", "S", "plane", "cost", "views", "depth"):
        assert _same(got[key], want[key]), (case[0], key)
    assert (got["views"] > 0).any()
    _sgm(d, case)                                                   # a repeated call gives identical bytes
    again = d.depth(0)
    again.update(C=d.volume(0, aggregated=False), S=d.volume(0))
    assert all(again[key].tobytes() == got[key].tobytes() for key in again)
    d.close()


def test_filter_and_points_on_the_aggregated_maps(pkg):
    case = ss.CASES[0]
    src = case[6]
    d, views, slots = _loaded(pkg, case)
    for r in slots:
        _sgm(d, case, r)
    swept = {r: _oracle(case, r) for r in slots}
    fd, fp = do.geometric_filter(swept[0]["depth"], swept[0]["plane"], views[0][1], views[0][2],
                                 [(swept[s]["depth"], views[s][1], views[s][2]) for s in src], REL_TOL, 2)
    d.filter(0, src, REL_TOL, 2)
    f = d.depth(0, filtered=True)
    print("kept by the filter:", int((fd > 0).sum()), "of", int((swept[0]["depth"] > 0).sum()))
    assert (fd > 0).any() and _same(f["depth"], fd) and _same(f["plane"], fp)
    assert _same(d.points(0), do.points(swept[0]["depth"], views[0][1], views[0][2]))
    assert _same(d.points(0, filtered=True), do.points(fd, views[0][1], views[0][2]))
    # the volumes are those of the last semi-global sweep (slot 2) alone
    assert _same(d.volume(slots[-1]), swept[slots[-1]]["S"])
    with pytest.raises(pkg.EkfError) as ei:
        d.volume(0)
    assert ei.value.status == 4
    d.close()


def test_the_plain_sweep_is_untouched_and_the_volumes_follow_their_slot(pkg):
    case = ss.CASES[0]
    name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
    d, views, slots = _loaded(pkg, case)
    fresh, _, _ = _loaded(pkg, case)
    fresh.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)
    plain = fresh.depth(0)
    want = do.sweep(views[0][0], views[0][1], views[0][2], [views[s] for s in src], ds.W_MIN, ds.W_MAX, D, radius, trunc)
    assert all(_same(plain[k], want[k]) for k in plain)
    d.profile(True)
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)          # before ...
    assert all(d.depth(0)[k].tobytes() == plain[k].tobytes() for k in plain)
    with pytest.raises(pkg.EkfError) as ei:                         # no semi-global sweep yet
        d.volume(0)
    assert ei.value.status == 4
    _sgm(d, case)
    agg = d.depth(0)
    assert not _same(agg["cost"], plain["cost"]) and _same(d.volume(0), _oracle(case)["S"])
    # the profile: one launch of each new kernel, the plain sweep's pair sees only the plain sweep
    prof, old = d.get_sgm_profile(), d.get_profile()
    print("profile", prof)
    assert [v[1] for v in prof.values()] == [1] * 10 and all(v[0] > 0 for v in prof.values())
    assert old["k_plane_sweep"][1] == 1 and old["k_depth_filter_points"][1] == 0
    d.profile(False)
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc)          # ... and after: the bytes of a fresh handle
    assert all(d.depth(0)[k].tobytes() == plain[k].tobytes() for k in plain)
    # a plain sweep of the slot, and every setter, takes the volumes from it
    gone = lambda: d._lib.ekf_dense_get_volume(d._h, 0, 1, np.zeros((D, h, w), np.uint32).ctypes.data_as(C.c_void_p))
    assert gone() == 4
    _sgm(d, case)
    assert gone() == 0
    d.set_pose(0, views[0][2])
    assert gone() == 4
    _sgm(d, case)
    d.set_view(0, *views[0])
    assert gone() == 4
    _sgm(d, case)
    d.set_view(0, np.ascontiguousarray(np.repeat(views[0][0][:, :, None], 3, axis=2)), views[0][1], views[0][2])   # colour
    assert gone() == 4
    _sgm(d, case)
    d.set_view(1, *views[1])                                        # a source's setter: slot 0 keeps its volumes and maps
    assert gone() == 0 and _same(d.depth(0)["cost"], agg["cost"])
    for x in (fresh, d):
        x.close()


def test_argument_errors_leave_the_results_readable(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    case = ss.CASES[0]
    name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
    d, views, slots = _loaded(pkg, case)
    _sgm(d, case)
    want = _oracle(case)
    s12 = np.array(src, np.int32)
    sgm = lambda ref=0, s=s12, n=2, w0=ds.W_MIN, w1=ds.W_MAX, pl=D, r=radius, t=trunc, a=p1, b=p2, k=paths: lib.ekf_dense_sweep_sgm(
        d._h, ref, None if s is None else P(s), n, w0, w1, pl, r, t, a, b, k)
    assert lib.ekf_dense_sweep_sgm(None, 0, P(s12), 2, ds.W_MIN, ds.W_MAX, D, radius, trunc, p1, p2, paths) == 1
    # everything ekf_dense_sweep refuses
    assert sgm(pl=1) == 1 and sgm(pl=1025) == 1 and sgm(r=-1) == 1 and sgm(r=5) == 1 and sgm(t=0) == 1 and sgm(t=256) == 1
    assert sgm(n=0) == 1 and sgm(s=np.arange(1, 10, dtype=np.int32), n=9) == 1 and sgm(s=None) == 1
    assert sgm(w0=0.0) == 1 and sgm(w0=0.4, w1=0.4) == 1 and sgm(w1=np.inf) == 1 and sgm(w0=np.nan) == 1
    assert sgm(s=np.array([1, 0], np.int32)) == 1 and sgm(s=np.array([1, 3], np.int32)) == 1 and sgm(ref=3) == 1
    assert sgm(s=np.array([1, 1], np.int32)) == 1 and sgm(ref=-1) == 1 and sgm(s=np.array([1, 5], np.int32)) == 1
    # the penalties and the paths
    assert sgm(a=0) == 1 and sgm(a=-3) == 1 and sgm(a=289) == 1 and sgm(b=(1 << 20) + 1) == 1 and sgm(a=1 << 21, b=1 << 21) == 1
    assert sgm(k=0) == 1 and sgm(k=2) == 1 and sgm(k=5) == 1 and sgm(k=16) == 1
    # the getters
    buf = np.zeros((D, h, w), np.uint32)
    assert lib.ekf_dense_get_volume(None, 0, 1, P(buf)) == 1 and lib.ekf_dense_get_volume(d._h, 0, 1, None) == 1
    assert lib.ekf_dense_get_volume(d._h, 0, 2, P(buf)) == 1 and lib.ekf_dense_get_volume(d._h, 5, 1, P(buf)) == 1
    assert lib.ekf_dense_get_volume(d._h, -1, 0, P(buf)) == 1 and lib.ekf_dense_get_volume(d._h, 1, 1, P(buf)) == 4
    assert lib.ekf_dense_get_sgm_profile(d._h, None, None) == 1 and lib.ekf_dense_get_sgm_profile(None, P(buf), P(buf)) == 1
    assert lib.ekf_dense_last_error(d._h)
    # ... and every earlier result is still there, the volumes included
    got = d.depth(0)
    assert all(_same(got[k], want[k]) for k in got) and _same(d.volume(0), want["S"]) and _same(d.volume(0, False), want["C"])
    assert sgm(a=1, b=1) == 0 and sgm(a=1 << 20, b=1 << 20) == 0 and sgm(k=4) == 0          # the ends of the ranges are taken
    d.close()
    # the element cap: 1024 x 1024 x 257 > 2^28, refused before the device is touched; 256 planes would be allowed
    big = pkg.DenseStereo(1024, 1024, max_views=2)
    img = np.zeros((1024, 1024), np.uint8)
    big.set_view(0, img, ds.K, ds.RIG[0])
    big.set_view(1, img, ds.K, ds.RIG[1])
    big.sweep(0, [1], ds.W_MIN, ds.W_MAX, 2, 0, 20)
    before = big.depth(0)
    one = np.array([1], np.int32)
    assert lib.ekf_dense_sweep_sgm(big._h, 0, P(one), 1, ds.W_MIN, ds.W_MAX, 257, 0, 20, 1, 1, 4) == 1
    assert b"2^28" in lib.ekf_dense_last_error(big._h)
    after = big.depth(0)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)
    big.close()


def test_a_living_filter_is_untouched(pkg):
    """A semi-global sweep beside a filter: its state, Sigma and launch counters stay bitwise the same."""
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=16, dtype=np.float32)
    for i in range(4):
        assert g.addFeature((40.0 + 30.0 * i, 50.0 + 20.0 * i)) == 1
    g.synchronize()
    snap = lambda: (g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts())
    before = snap()
    case = ss.CASES[1]
    d, views, slots = _loaded(pkg, case)
    _sgm(d, case)
    assert _same(d.volume(0), _oracle(case)["S"])
    assert snap() == before
    d.close()
    g.close()


def test_recording_with_and_without_sgm(pkg, tmp_path):
    """Five small synthetic key frames through depth_maps_from_recording: sgm=True and a dict against the oracle driven from
    the same files, sgm=None against the plain sweep's oracle (today's result)."""
    from ekf_monoslam_amd import dense, keyframes
    n, w, h = 5, 24, 16
    K = np.array([32.0, 32.0, 11.5, 7.5])
    rec = tmp_path / "rec"
    rec.mkdir()
    pkg.formats.write_camera(str(rec / "camera.txt"), K)
    rng = np.random.default_rng(23)
    ids = [3 + 2 * i for i in range(n)]
    with open(rec / "nodes_and_prjcts.txt", "w") as fh:
        for i, kid in enumerate(ids):
            pose = np.array([0.11 * i, 0.01 * (i % 3), 0.0, 1.0, 0.002 * i, -0.001 * i, 0.0], np.float32)
            fh.write(pkg.formats.pose_record(kid, pose, None))
            base = ds.texture(0.13 * np.arange(w)[None, :] + 0.11 * i, 0.17 * np.arange(h)[:, None])
            base[4:12, 6:18] = 128.0                                # a patch without texture
            keyframes.write_pgm(str(rec / ("%d.pgm" % kid)), np.clip(base + rng.integers(-6, 7, (h, w)) * (base != 128.0), 0, 255).astype(np.uint8))
    kw = dict(w_min=0.1, w_max=0.6, planes=5, radius=1, trunc=50)
    Kf, fids, poses, images = dense.read_recording(str(rec))
    near = [dense.neighbours_of(i, n, 1) for i in range(n)]

    def check(maps, swept):
        for i, m in enumerate(maps):
            fd, fp = do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i],
                                         [(swept[j]["depth"], K, poses[j]) for j in near[i]], 0.3, 1)
            assert m.sources == tuple(ids[j] for j in near[i]), i
            assert _same(m.swept_depth, swept[i]["depth"]) and _same(m.cost, swept[i]["cost"]) and _same(m.views, swept[i]["views"]), i
            assert _same(m.depth, fd) and _same(m.plane, fp) and _same(m.points, do.points(fd, K, poses[i])), i

    args = lambda i: (images[i], K, poses[i], [(images[j], K, poses[j]) for j in near[i]], kw["w_min"], kw["w_max"], kw["planes"],
                      kw["radius"], kw["trunc"])
    run = lambda **extra: pkg.depth_maps_from_recording(str(rec), None, neighbours=1, rel_tol=0.3, min_agree=1, **kw, **extra)
    plain = [do.sweep(*args(i)) for i in range(n)]
    check(run(), plain)
    check(run(sgm=None), plain)
    auto = [so.sweep_sgm(*args(i), *so.default_penalties(1, len(near[i])), 8) for i in range(n)]
    check(run(sgm=True), auto)
    assert any(not _same(a["cost"], b["cost"]) for a, b in zip(auto, plain))
    check(run(sgm=dict(p1=3, p2=40, paths=4)), [so.sweep_sgm(*args(i), 3, 40, 4) for i in range(n)])
    with pytest.raises(ValueError):
        run(sgm=dict(penalty=3))
