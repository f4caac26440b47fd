"""The mesh-to-mesh distance on the device against tests/distance_oracle.py, bit for bit: dist, tri, closest, side
and every statistic, on the volumes of tests/test_gpu_texture.py (written with set_volume, so that no sweep runs) and on the
hand-built targets of tests/distance_scene.py.  Every comparison is exact equality of bits; the result is the same at every
setting of the grid."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import distance_oracle as do
import distance_scene as ds
import raster_scene as rs
import texture_scene as ts
from test_gpu_texture import (ARG, FACTOR, P, PRUNE, ROUNDS, SOURCES, STATE, _fetch, _same, _same_atlas, _same_mesh, _source, _texture,  # noqa: F401
                              _views, _volume, pkg)

pytestmark = pytest.mark.gpu
THR = 0.0625
ALL = SOURCES + ("mesh",)


def _equal(got, want):
    """A MeshDistance against an oracle dict."""
    return (_same(got.dist, want["dist"]) and _same(got.tri, want["tri"]) and _same(got.closest, want["closest"]) and
            _same(got.side, want["side"]))


def _same_result(a, b):
    return _equal(a, dict(dist=b.dist, tri=b.tri, closest=b.closest, side=b.side))


def _bits(x):
    return np.float64(x).view(np.uint64)


def _equal_stats(got, want):
    """A DistanceStats against the oracle's: the integers, and the bits of max, mean and rms."""
    return ((got.n, got.n_bad, got.argmax, got.within) == (want["n"], want["n_bad"], want["argmax"], want["within"]) and
            _bits(got.max) == _bits(want["max"]) and _bits(got.mean) == _bits(want["mean"]) and _bits(got.rms) == _bits(want["rms"]))


@functools.lru_cache(maxsize=None)
def _want(name):
    mesh, points = ds.scenes()[name]
    r = do.distance(mesh, points)
    return r, do.stats(r["dist"], THR), do.stats(r["dist"], 0.0)


@pytest.mark.parametrize("g", ds.GRIDS)
def test_every_hand_built_scene_at_every_grid(pkg, g):
    """Every scene of tests/distance_scene.py as source 4 with its points from the host, at g = 1, 2, 5, 7, 128 and automatic:
    the oracle's arrays and statistics, so identical to one another; 301 points (a ragged second workgroup) and 1 point; the same
    run twice; the profile's counts; the tie across shells goes to triangle 0."""
    from ekf_monoslam_amd import fusion
    v = _volume(pkg, "sphere")
    count = lambda d: [c for _, c in d.values()]
    try:
        v.profile(True)
        assert count(v.get_distance_profile()) == [0] * 9
        v.set_distance_grid(g)
        for name, (mesh, points) in sorted(ds.scenes().items()):
            want, st, st0 = _want(name)
            n_valid = int(do.valid(*do._mesh(mesh)).sum())
            v.set_distance_mesh(mesh["vertices"], mesh["faces"])
            v.profile(True)
            got = v.distance_points("mesh", points)
            assert _equal(got, want), name
            prof = v.get_distance_profile()
            assert list(prof) == list(fusion.DISTANCE_KERNELS) and count(prof) == [1] * 7 + [0, 0], (name, prof)
            assert _equal_stats(v.distance_stats(THR), st) and _equal_stats(v.distance_stats(0.0), st0), name
            assert count(v.get_distance_profile()) == [1] * 7 + [2, 2]
            grid = v.distance_grid()
            assert max(grid["cells"]) == (g or do.auto_g(n_valid)) and grid["longest"] >= 1
            if g == 1:
                assert grid["cells"] == (1, 1, 1) and grid["entries"] == grid["longest"] == n_valid
            if g != 128 or len(points) < 100:
                assert _same_result(v.distance_points("mesh", points), got)
            v.profile(False)
            print(g, name, len(mesh["faces"]), "triangles", len(points), "points: max", st["max"], "mean", st["mean"], "bad", st["n_bad"], grid)
        assert _want("tie")[0]["tri"][0] == 0 and _want("tie")[0]["dist"][0] == 1.0 and _want("tie")[1]["n_bad"] == 3
    finally:
        v.close()


def test_unused_feature_launches_nothing_and_a_target_of_invalid_triangles(pkg):
    """No k_dist_* launch while the feature is unused; a run leaves the other getters' counts alone; a target of invalid triangles
    only is EKF_ERR_STATE and leaves the last result readable."""
    v = _volume(pkg, "sphere")
    count = lambda d: [c for _, c in d.values()]
    try:
        v.profile(True)
        v.weld(1)
        v.simplify(FACTOR * v.voxel)
        v.rasterise((8, 8), rs.K, rs.POSE, "weld")
        assert count(v.get_distance_profile()) == [0] * 9
        v.profile(True)
        mesh, points = ds.scenes()["regions"]
        v.set_distance_mesh(mesh["vertices"], mesh["faces"])
        assert _equal(v.distance_points("mesh", points), _want("regions")[0])
        assert [int(s) for s in _want("regions")[0]["side"]] == [ds.REGION_SIDE.get(i, 0) for i in range(len(points))]
        assert all(tuple(_want("regions")[0]["closest"][i]) == c for i, c in ds.REGION_TRUTH.items())
        assert count(v.get_profile()) == [0] * 4 and count(v.get_mesh_profile()) == [0] * 5 and count(v.get_texture_profile()) == [0] * 4
        assert count(v.get_raster_profile()) == [0] * 4 and count(v.get_simplify_profile()) == [0] * 10
        v.profile(False)
        bad, pts = ds.only_degenerate()
        v.set_distance_mesh(bad["vertices"], bad["faces"])
        lib = pkg.load_library()
        assert lib.ekf_distance_run_points(v._h, 4, P(pts), len(pts)) == STATE
        assert lib.ekf_fusion_last_error(v._h).decode() == "ekf_distance_run_points: the target mesh has no valid triangle"
        assert _equal(v._distance(len(points)), _want("regions")[0])          # the last result stays
    finally:
        v.close()


def _chain(v):
    """All four sources of the handle at once, as tests/test_gpu_texture.py makes each of them."""
    return {"weld": v.weld(1), "pruned": v.prune(PRUNE), "smoothed": v.smooth(ROUNDS), "simplified": v.simplify(FACTOR * v.voxel)}


def _oracle_source(name, source):
    if source == "mesh":
        return ds.sphere_simplified(3.5)
    m = _source(name, source)
    return dict(vertices=m["vertices"], faces=m["faces"])


@pytest.mark.parametrize("name", ("sphere", "main", "sphere_colour", "main_colour"))
def test_distance_equals_the_oracle_between_all_five_sources(pkg, name):
    """Every source as target and as query, 25 pairs, smoothed -> weld and simplified <-> weld among them; every source's arrays,
    a raster image and the atlas are what they were; compare_meshes is the two runs."""
    v = _volume(pkg, name)
    try:
        src = _chain(v)
        own = _oracle_source(name, "mesh")
        v.set_distance_mesh(own["vertices"], own["faces"])
        atlas, _ = _texture(v, "simplified", 2, 3, _views(name, True))
        shape, K, pose = (ts.W, ts.H), ts.K, ts.POSES[1]
        image = v.rasterise(shape, K, pose, "weld", cover=True)
        for target in ALL:
            t = _oracle_source(name, target)
            for query in ALL:
                q = _oracle_source(name, query)
                want = do.distance(t, q["vertices"])
                got = v.distance(target, query)
                assert _equal(got, want), (target, query)
                assert _equal_stats(v.distance_stats(THR), do.stats(want["dist"], THR)), (target, query)
            print(name, target, len(t["faces"]), "triangles: mean from the weld's vertices",
                  do.stats(do.distance(t, _oracle_source(name, "weld")["vertices"])["dist"], 0.0)["mean"])
        for source in SOURCES:
            assert _same_mesh(_fetch(pkg, v, source, src[source]), src[source]), source
        again = v._mesh_render("weld", "vertex", True)
        assert all(_same(getattr(again, k), getattr(image, k)) for k in ("depth", "normal", "grey", "tri", "bary", "cover"))
        peek = v.texture_peek()
        assert _same(peek.atlas, atlas.atlas) and _same(peek.uv, atlas.uv) and _same(peek.view, atlas.view)
        ab, ba, sym = pkg.compare_meshes(v, "simplified", "weld", THR)
        w, s = _oracle_source(name, "weld"), _oracle_source(name, "simplified")
        assert _equal_stats(ab, do.stats(do.distance(w, s["vertices"])["dist"], THR))
        assert _equal_stats(ba, do.stats(do.distance(s, w["vertices"])["dist"], THR)) and sym == max(ab.max, ba.max)
    finally:
        v.close()


def test_regrowth_and_points_against_a_source(pkg):
    """301 points and 1 point against the weld, then the weld's 1298 vertices, then 1 point again: the buffers grow once and the
    arrays are the oracle's each time; a point that is not finite is counted as bad."""
    v = _volume(pkg, "sphere")
    try:
        v.weld(1)
        weld = _oracle_source("sphere", "weld")
        pts = ds.scenes()["spanning"][1] / 8.0
        for P_ in (pts, pts[3:4], weld["vertices"] * 1.03125, pts[5:6], pts):
            want = do.distance(weld, P_)
            for g in (0, 5):
                v.set_distance_grid(g)
                assert _equal(v.distance_points("weld", P_), want), (len(P_), g)
                assert _equal_stats(v.distance_stats(THR), do.stats(want["dist"], THR))
        assert do.stats(want["dist"], THR)["n_bad"] == 1
    finally:
        v.close()


def test_state_rules_and_argument_errors(pkg):
    lib = pkg.load_library()
    v = _volume(pkg, "sphere")
    err = lambda: lib.ekf_fusion_last_error(v._h).decode()
    n = C.c_ulonglong(0)
    run = lambda target=0, query=0: lib.ekf_distance_run(v._h, target, query, C.byref(n))
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    points = lambda target=0, xyz=pts, count=2: lib.ekf_distance_run_points(v._h, target, P(xyz), count)
    get = lambda dist=None, tri=None, closest=None, side=None, m=0: lib.ekf_distance_get(v._h, P(dist), P(tri), P(closest), P(side), m)
    stats = lambda thr=0.0: lib.ekf_distance_get_stats(v._h, C.c_double(thr), None, None, None, None, None, None, None)
    try:
        assert get() == STATE and err() == "ekf_distance_get: no ekf_distance_run"
        assert stats() == STATE and err() == "ekf_distance_get_stats: no ekf_distance_run"
        assert lib.ekf_distance_get_grid(v._h, None, None, None) == STATE
        v.reset()
        for source in range(3):
            assert run(source) == STATE and err() == "ekf_distance_run: no ekf_mesh_weld since the volume last changed"
            assert run(4, source) == STATE
        assert run(3) == STATE and err() == "ekf_distance_run: source 3 needs an ekf_simplify_run on the current mesh"
        assert run(4) == STATE and err() == "ekf_distance_run: source 4 needs an ekf_distance_set_mesh"
        assert points(4) == STATE and err() == "ekf_distance_run_points: source 4 needs an ekf_distance_set_mesh"
        v.weld(1)                                                            # of an empty volume
        assert run(0) == STATE and err() == "ekf_distance_run: the target mesh has no valid triangle"
        v.set_volume(*ds.fs.sphere_volume())
        v.weld(1)
        assert run(1) == STATE and err() == "ekf_distance_run: source 1 needs an ekf_components_prune since the last ekf_mesh_weld"
        assert run(0, 2) == STATE and err() == "ekf_distance_run: source 2 needs an ekf_smooth_run on the current mesh"
        for kw in (dict(target=-1), dict(target=5), dict(query=-1), dict(query=5)):
            assert run(**kw) == ARG and err() == "ekf_distance_run: target and query 0..4", kw
        msg = "ekf_distance_run_points: target 0..4; xyz not NULL; 0 < n_points < 2^32"
        for kw in (dict(target=-1), dict(target=5), dict(xyz=None), dict(count=0), dict(count=2 ** 32)):
            assert points(**kw) == ARG and err() == msg, kw
        assert get() == STATE                                                # none of them ran
        # the rasteriser's source 4 is another mesh
        X, F = np.array([[0.0, 0, 1], [0, 1, 1], [1, 0, 1]]), np.array([[0, 1, 2]], np.uint32)
        assert lib.ekf_raster_set_mesh(v._h, P(X), P(F), P(np.zeros(3, np.uint8)), None, 3, 1) == 0 and run(4) == STATE
        set_mesh = lambda X=X, F=F, nv=3, nt=1: lib.ekf_distance_set_mesh(v._h, P(X), P(F), nv, nt)
        msg = "ekf_distance_set_mesh: xyz and faces not NULL; 0 < n_vert, n_tri < 2^32; xyz finite; every index < n_vert"
        bad_X, bad_F = X.copy(), F.copy()
        bad_X[1, 2], bad_F[0, 2] = float("nan"), 3
        for kw in (dict(X=None), dict(F=None), dict(nv=0), dict(nt=0), dict(X=bad_X), dict(F=bad_F), dict(nv=2)):
            assert set_mesh(**kw) == ARG and err() == msg, kw
        assert run(4) == STATE and set_mesh() == 0
        assert run(4, 0) == 0 and n.value == 1298 and run(0, 4) == 0 and n.value == 3 and points() == 0
        # the getter: every pointer may be NULL; max_points must hold the run
        d = np.zeros(2)
        assert get() == 0 and get(dist=d, m=1) == ARG and err() == "ekf_distance_get: max_points is less than the points of the run"
        assert get(dist=d, m=2) == 0 and d[0] > 0
        for thr in (-0.5, float("nan")):
            assert stats(thr) == ARG and err() == "ekf_distance_get_stats: thr >= 0"
        assert stats(float("inf")) == 0
        # the arrays are a snapshot: a new weld, a change of the volume and a failed run leave them readable
        before = v._distance(2)
        v.weld(1)
        v.set_volume(*ds.fs.sphere_volume())
        assert run(0) == STATE and points(count=0) == ARG
        assert _same_result(v._distance(2), before)
        for bad in (-1, 129):
            assert lib.ekf_distance_set_grid(v._h, bad) == ARG and err() == "ekf_distance_set_grid: g in 0..128"
        assert lib.ekf_distance_set_grid(v._h, 128) == 0 and lib.ekf_distance_set_grid(v._h, 0) == 0
        ms_, cnt = np.zeros(9), np.zeros(9, np.int64)
        assert lib.ekf_distance_get_profile(v._h, None, P(cnt)) == ARG and lib.ekf_distance_get_profile(v._h, P(ms_), P(cnt)) == 0
        assert lib.ekf_distance_set_mesh(None, P(X), P(F), 3, 1) == ARG and lib.ekf_distance_run(None, 0, 0, None) == ARG
        for bad in ("soup", 4, None):
            with pytest.raises(ValueError):
                v.distance(bad, "weld")
    finally:
        v.close()
