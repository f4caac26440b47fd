"""The census matching cost on the device against tests/census_oracle.py: the descriptors, the four maps of
the plain sweep and both volumes and the maps of the semi-global sweep exactly equal on the cases of tests/census_scene.py;
that a strictly increasing grey table changes no byte; that descriptors are computed once per image (through the profile);
that the plain sweeps and every earlier result are untouched; the argument and state errors; and a recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py)

import census_oracle as co
import census_scene as cs
import dense_oracle as do
import dense_scene as ds
import sgm_oracle as so

pytestmark = pytest.mark.gpu

MAPS = ("plane", "cost", "views", "depth")
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
    d = pkg.DenseStereo(w, h, max_views=5)
    for s in slots:
        d.set_view(s, *views[s])
    return d


def _sweep_case(case):
    """(views, slots, the oracle's maps) of a sweep case on the re-exposed step scene, computed once and shared."""
    name, w, h, D, radius, trunc, src = case
    if name not in _ORACLE:
        views = cs.exposed(ds.case_views(w, h))
        want = co.sweep(views[0][0], views[0][1], views[0][2], [views[s] for s in src], ds.W_MIN, ds.W_MAX, D, radius, trunc)
        _ORACLE[name] = (views, (0,) + tuple(src), want)
    return _ORACLE[name]


def _sgm_case(case):
    name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
    if "sgm_" + name not in _ORACLE:
        views = cs.exposed(cs.sgm_case_views(case))
        want = co.sweep_sgm(views[0][0], views[0][1], views[0][2], [views[s] for s in src], ds.W_MIN, ds.W_MAX, D, radius, trunc,
                            p1, p2, paths)
        _ORACLE["sgm_" + name] = (views, (0,) + tuple(src), want)
    return _ORACLE["sgm_" + name]


@pytest.mark.parametrize("case", cs.DESCRIPTOR_CASES, ids=[c[0] for c in cs.DESCRIPTOR_CASES])
def test_descriptors_equal_the_oracle(pkg, case):
    name, w, h, _ = case
    img = cs.descriptor_image(case)
    want = co.census(img)
    K = np.array([64.0, 64.0, 0.0, 0.0])
    d = pkg.DenseStereo(w, h, max_views=2)
    d.set_view(1, img, K, ds.REF)
    got = d.census(1)
    print(name, "differing descriptors:", int((got != want).sum()), "of", want.size)
    assert _same(got, want) and not (got >> np.uint64(62)).any()
    assert d.census(1).tobytes() == got.tobytes()
    with pytest.raises(pkg.EkfError) as ei:                          # an unset slot
        d.census(0)
    assert ei.value.status == 4
    d.close()


@pytest.mark.parametrize("case", cs.SWEEP_CASES, ids=[c[0] for c in cs.SWEEP_CASES])
def test_the_four_maps_equal_the_oracle(pkg, case):
    name, w, h, D, radius, trunc, src = case
    views, slots, want = _sweep_case(case)
    d = _loaded(pkg, views, slots, w, h)
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost="census")
    got = d.depth(0)
    for key in MAPS:
        diff = int((_bits(got[key]) != _bits(want[key])).sum()) if key == "depth" else int((got[key] != want[key]).sum())
        print(name, key, "differing elements:", diff, "of", want[key].size)
    for key in MAPS:
        assert _same(got[key], want[key]), (name, key)
    assert (got["views"] > 0).any()
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost="census")      # a repeated call gives identical bytes
    again = d.depth(0)
    assert all(again[key].tobytes() == got[key].tobytes() for key in got)
    d.close()


@pytest.mark.parametrize("case", cs.SGM_CASES, ids=[c[0] for c in cs.SGM_CASES])
def test_the_semi_global_volumes_and_maps_equal_the_oracle(pkg, case):
    name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
    views, slots, want = _sgm_case(case)
    d = _loaded(pkg, views, slots, w, h)
    d.sweep_sgm(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, p1, p2, paths, cost="census")
    got = d.depth(0)
    got.update(C=d.volume(0, aggregated=False), S=d.volume(0))
    for key in ("C", "S") + MAPS:
        diff = int((_bits(got[key]) != _bits(want[key])).sum()) if key == "depth" else int((got[key] != want[key]).sum())
        print(name, key, "differing elements:", diff, "of", want[key].size)
    for key in ("C", "S") + MAPS:
        assert _same(got[key], want[key]), (name, key)
    d.close()


def test_a_strictly_increasing_table_on_the_sources_changes_no_byte(pkg):
    name, w, h, D, radius, trunc, src = cs.SWEEP_CASES[1]
    views = ds.case_views(w, h)
    half = {s: (v[0] >> 1, v[1], v[2]) for s, v in views.items()}    # halved first: nothing clips
    table = cs.monotone_table()
    mapped = {s: ((table[v[0]] if s in src else v[0]), v[1], v[2]) for s, v in half.items()}
    assert any(not np.array_equal(mapped[s][0], half[s][0]) for s in src)
    out = []
    for vs in (half, mapped):
        d = _loaded(pkg, vs, (0,) + tuple(src), w, h)
        d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, 255, cost="census")
        out.append(d.depth(0))
        d.close()
    assert all(out[0][k].tobytes() == out[1][k].tobytes() for k in out[0]) and (out[0]["views"] > 0).any()


def test_descriptors_are_computed_once_per_image(pkg):
    case = cs.SWEEP_CASES[1]
    name, w, h, D, radius, trunc, src = case
    views, slots, want = _sweep_case(case)
    d = _loaded(pkg, views, slots, w, h)
    sweep = lambda: d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost="census")
    launches = lambda: [v[1] for v in d.get_census_profile().values()]
    d.profile(True)
    sweep()
    print("census profile", d.get_census_profile())
    assert launches() == [3, 1, 0] and all(v[0] > 0 for v in list(d.get_census_profile().values())[:2])
    d.profile(True)                                                 # the counters start from zero
    d.set_pose(1, views[1][2])
    d.set_pose(0, views[0][2])
    sweep()
    assert launches() == [0, 1, 0] and all(_same(d.depth(0)[k], want[k]) for k in MAPS)
    d.profile(True)
    d.set_view(2, *views[2])
    sweep()
    assert launches() == [1, 1, 0] and all(_same(d.depth(0)[k], want[k]) for k in MAPS)
    d.profile(True)
    d.set_view(1, np.ascontiguousarray(np.repeat(views[1][0][:, :, None], 3, axis=2)), views[1][1], views[1][2])    # colour
    d.set_view(0, torch.from_numpy(views[0][0]).cuda(), views[0][1], views[0][2])                                      # device
    d.sweep_sgm(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost="census")
    assert launches() == [2, 0, 1]
    # nothing is added to the plain pair; the semi-global ten see the directions and the winner, not a volume sweep
    assert [v[1] for v in d.get_profile().values()] == [0, 0]
    assert [v[1] for v in d.get_sgm_profile().values()] == [0] + [1] * 9
    assert _same(d.census(2), co.census(views[2][0])) and launches() == [2, 0, 1]     # the getter found them fresh
    d.profile(False)
    d.close()


def test_the_plain_sweeps_are_untouched_and_the_census_map_feeds_filter_and_points(pkg):
    case = cs.SWEEP_CASES[1]
    name, w, h, D, radius, trunc, src = case
    views, slots, want = _sweep_case(case)
    plain_args = (ds.W_MIN, ds.W_MAX, D, radius, trunc)
    fresh = _loaded(pkg, views, slots, w, h)
    fresh.sweep(0, src, *plain_args)
    plain = fresh.depth(0)
    ad = do.sweep(views[0][0], views[0][1], views[0][2], [views[s] for s in src], *plain_args)
    assert all(_same(plain[k], ad[k]) for k in plain)
    fresh.sweep_sgm(0, src, *plain_args)
    plain_sgm = fresh.depth(0)
    d = _loaded(pkg, views, slots, w, h)
    d.sweep(0, src, *plain_args)                                     # before ...
    assert all(d.depth(0)[k].tobytes() == plain[k].tobytes() for k in plain)
    swept = {}
    for r in slots:
        others = [s for s in slots if s != r]
        d.sweep(r, others, *plain_args, cost="census")
        swept[r] = co.sweep(views[r][0], views[r][1], views[r][2], [views[s] for s in others], *plain_args)
    got = d.depth(0)
    assert all(_same(got[k], want[k]) for k in MAPS) and not _same(got["cost"], plain["cost"])
    fd, fp = do.geometric_filter(swept[0]["depth"], swept[0]["plane"], views[0][1], views[0][2],
                                 [(swept[s]["depth"], views[s][1], views[s][2]) for s in src], 0.05, 2)
    d.filter(0, src, 0.05, 2)
    f = d.depth(0, filtered=True)
    print("kept by the filter:", int((fd > 0).sum()), "of", int((swept[0]["depth"] > 0).sum()))
    assert (fd > 0).any() and _same(f["depth"], fd) and _same(f["plane"], fp)
    assert _same(d.points(0), do.points(swept[0]["depth"], views[0][1], views[0][2]))
    assert _same(d.points(0, filtered=True), do.points(fd, views[0][1], views[0][2]))
    with pytest.raises(pkg.EkfError) as ei:                         # a plain census sweep owns no volume
        d.volume(0)
    assert ei.value.status == 4
    d.sweep(0, src, *plain_args)                                     # ... and after: the bytes of a fresh handle
    assert all(d.depth(0)[k].tobytes() == plain[k].tobytes() for k in plain)
    d.sweep_sgm(0, src, *plain_args, cost="census")
    d.sweep_sgm(0, src, *plain_args)
    assert all(d.depth(0)[k].tobytes() == plain_sgm[k].tobytes() for k in plain_sgm)
    with pytest.raises(ValueError):
        d.sweep(0, src, *plain_args, cost="ssd")
    with pytest.raises(ValueError):
        d.sweep_sgm(0, src, *plain_args, cost=None)
    for x in (fresh, d):
        x.close()


def test_errors_leave_the_earlier_maps_readable(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    case = cs.SWEEP_CASES[1]
    name, w, h, D, radius, trunc, src = case
    views, slots, want = _sweep_case(case)
    d = _loaded(pkg, views, slots, w, h)
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, trunc, cost="census")
    s12 = np.array(src, np.int32)
    plain = lambda ref=0, s=s12, n=2, w0=ds.W_MIN, w1=ds.W_MAX, pl=D, r=radius, t=trunc: lib.ekf_dense_sweep_census(
        d._h, ref, None if s is None else P(s), n, w0, w1, pl, r, t)
    sgm = lambda ref=0, s=s12, n=2, w0=ds.W_MIN, w1=ds.W_MAX, pl=D, r=radius, t=trunc, a=36, b=288, k=8: lib.ekf_dense_sweep_sgm_census(
        d._h, ref, None if s is None else P(s), n, w0, w1, pl, r, t, a, b, k)
    assert lib.ekf_dense_sweep_census(None, 0, P(s12), 2, ds.W_MIN, ds.W_MAX, D, radius, trunc) == 1
    assert lib.ekf_dense_sweep_sgm_census(None, 0, P(s12), 2, ds.W_MIN, ds.W_MAX, D, radius, trunc, 36, 288, 8) == 1
    for f in (plain, sgm):                                          # everything ekf_dense_sweep refuses
        assert f(pl=1) == 1 and f(pl=1025) == 1 and f(r=-1) == 1 and f(r=5) == 1 and f(t=0) == 1 and f(t=256) == 1
        assert f(n=0) == 1 and f(s=np.arange(1, 10, dtype=np.int32), n=9) == 1 and f(s=None) == 1
        assert f(w0=0.0) == 1 and f(w0=0.4, w1=0.4) == 1 and f(w1=np.inf) == 1 and f(w0=np.nan) == 1
        assert f(s=np.array([1, 0], np.int32)) == 1 and f(s=np.array([1, 3], np.int32)) == 1 and f(ref=3) == 1     # slot 3 is not set
        assert f(s=np.array([1, 1], np.int32)) == 1 and f(ref=-1) == 1 and f(s=np.array([1, 5], np.int32)) == 1
    assert sgm(a=0) == 1 and sgm(a=289) == 1 and sgm(b=(1 << 20) + 1) == 1 and sgm(k=2) == 1 and sgm(k=16) == 1
    # the getters: arguments, and the state of an unset slot
    buf = np.zeros((h, w), np.uint64)
    assert lib.ekf_dense_get_census(None, 0, P(buf)) == 1 and lib.ekf_dense_get_census(d._h, 0, None) == 1
    assert lib.ekf_dense_get_census(d._h, 5, P(buf)) == 1 and lib.ekf_dense_get_census(d._h, -1, P(buf)) == 1
    assert lib.ekf_dense_get_census(d._h, 3, P(buf)) == 4
    assert lib.ekf_dense_get_census_profile(d._h, None, None) == 1 and lib.ekf_dense_get_census_profile(None, P(buf), P(buf)) == 1
    assert lib.ekf_dense_last_error(d._h)
    assert lib.ekf_dense_get_volume(d._h, 0, 1, P(np.zeros((D, h, w), np.uint32))) == 4       # EKF_ERR_STATE: no volume yet
    got = d.depth(0)                                                # ... and every earlier result is still there
    assert all(_same(got[k], want[k]) for k in MAPS)
    # the state rules of the sweeps: a new pose takes the slot's maps, the filter refuses an unswept source
    d.set_pose(0, views[0][2])
    assert lib.ekf_dense_get_depth(d._h, 0, 0, None, None, None, None) == 4
    assert plain() == 0 and lib.ekf_dense_filter(d._h, 0, P(s12), 2, 0.05, 1) == 4
    assert plain(t=1) == 0 and plain(t=255) == 0 and sgm(a=1, b=1, k=4) == 0 and plain() == 0                  # the ends of the ranges
    assert all(_same(d.depth(0)[k], want[k]) for k in MAPS)
    d.close()


def test_recording_with_the_census_cost(pkg, tmp_path):
    """Five small synthetic key frames, every second one re-exposed, through depth_maps_from_recording(cost="census"), also
    with sgm=True, against the oracle driven from the same files; cost="ad" is today's result."""
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
            base = np.clip(ds.texture(0.13 * np.arange(w)[None, :] + 0.11 * i, 0.17 * np.arange(h)[:, None]), 0, 255).astype(np.uint8)
            keyframes.write_pgm(str(rec / ("%d.pgm" % kid)), cs.expose(base, *cs.EXPOSURE[1 + i % 2]))
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
    census = [co.sweep(*args(i)) for i in range(n)]
    check(run(cost="census"), census)
    check(run(cost="census", sgm=True), [co.sweep_sgm(*args(i), *so.default_penalties(1, len(near[i])), 8) for i in range(n)])
    plain = [do.sweep(*args(i)) for i in range(n)]
    check(run(cost="ad"), plain)
    assert any(not _same(a["cost"], b["cost"]) for a, b in zip(census, plain))
    with pytest.raises(ValueError):
        run(cost="ncc")
