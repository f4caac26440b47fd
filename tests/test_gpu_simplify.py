"""Vertex-clustering simplification of the welded, the pruned or the smoothed mesh on the device against
tests/simplify_oracle.py, bit for bit, on the volumes of tests/component_scene.py: written with set_volume, so that no sweep
runs.  Every comparison is exact equality of bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import component_oracle as co
import component_scene as cs
import fusion_scene as fs
import mesh_scene as ms
import simplify_oracle as so
import smooth_oracle as sm

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
ROWS = ("vertices", "grey", "colour", "normals", "key")
FACTORS = (1.0, 2.0, 3.5)
PRUNE, ROUNDS = 9, 2                               # the pruned source is prune(9), the smoothed one two rounds at the defaults
SCAN = 3                                           # of SIMPLIFY_KERNELS
ONCE = [1, 1, 1, 5, 1, 1, 1, 1, 1, 1]              # the launches of one run with a result that is not empty


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want):
    """Equal bit for bit (both None: equal)."""
    if got is None or want is None:
        return got is None and want is None
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _same_mesh(got, want):
    """An IndexedMesh against an oracle dict."""
    return (all(_same(getattr(got, k), want[k]) for k in ROWS) and got.faces.dtype == np.uint32 and
            got.faces.shape == (len(want["faces"]), 3) and np.array_equal(got.faces, want["faces"]))


def _volume(pkg, planes, dims, origin, voxel, trunc):
    v = pkg.TsdfVolume(dims, origin, voxel, trunc, colour=len(planes) > 3)
    v.set_volume(*planes[:3], csum=planes[3] if len(planes) > 3 else None)
    return v


@functools.lru_cache(maxsize=None)
def _source(name, mc, normals, source):
    """The oracle's source mesh of a case: its weld, that weld's prune(9), or that weld smoothed.  Computed once, shared, and left
    unchanged."""
    m = cs.oracle_mesh(name, mc, normals)
    if source == "pruned":
        return co.prune(m, PRUNE)
    if source == "smoothed":
        return sm.smooth(m, ROUNDS, normals=normals)
    return m


@functools.lru_cache(maxsize=None)
def _want(name, mc, normals, source, factor):
    _, dims, origin, voxel, _, _ = cs.cases()[name]
    return so.simplify(_source(name, mc, normals, source), origin, dims, voxel, factor * voxel)


def _counts(v):
    return [c for _, c in v.get_simplify_profile().values()]


def _make_source(v, mc, normals, source):
    """The device's source mesh, by the calls that make it."""
    m = v.weld(mc, normals)
    if source == "pruned":
        m = v.prune(PRUNE)
    if source == "smoothed":
        m = v.smooth(ROUNDS, normals=normals)
    return m


def _fetch(pkg, v, source, like):
    """The source's arrays as its getter delivers them now."""
    nv, nt = len(like.key), len(like.faces)
    back = pkg.IndexedMesh(np.zeros((nv, 3)), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint8),
                           None if like.colour is None else np.zeros((nv, 3), np.uint8),
                           None if like.normals is None else np.zeros((nv, 3), np.float32), np.zeros(nv, np.uint64))
    lib = pkg.load_library()
    getter = {"weld": lib.ekf_mesh_get, "pruned": lib.ekf_components_get_pruned, "smoothed": lib.ekf_smooth_get}[source]
    assert getter(v._h, P(back.vertices), P(back.faces), P(back.grey), P(back.colour), P(back.normals), P(back.key), nv, nt) == 0
    return back


def _check_run(v, want, factor, source, voxel):
    """One run against the oracle: every row, the map and the stats."""
    got = v.simplify(factor * voxel, source)
    assert _same_mesh(got, want), (source, factor)
    assert _same(v.simplify_map(), want["map"]), (source, factor)
    assert (v.simplify_stats.degenerate, v.simplify_stats.duplicate) == (want["n_degenerate"], want["n_duplicate"]), (source, factor)
    return got


@pytest.mark.parametrize("name", ("main", "tie", "sphere", "2x2x2", "16x16x3", "257x2x2"))
def test_simplification_equals_the_oracle_from_all_three_sources(pkg, name):
    """The wave volumes are colour volumes; every weld is made without and with normals."""
    planes, dims, origin, voxel, trunc, min_counts = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        for mc in min_counts:
            for normals in (False, True):
                for source in ("weld", "pruned", "smoothed"):
                    src = _make_source(v, mc, normals, source)
                    assert _same_mesh(src, _source(name, mc, normals, source)), (mc, normals, source)
                    for factor in FACTORS:
                        want = _want(name, mc, normals, source, factor)
                        got = _check_run(v, want, factor, source, voxel)
                        assert (got.normals is not None) == normals and (got.colour is not None) == v.colour
                        if normals and source == "weld":
                            print(name, "min_count", mc, "cell", factor, ":", len(src.faces), "->", len(got.faces), "triangles,", len(src.key), "->",
                                  len(got.key), "vertices,", want["n_degenerate"], "degenerate,", want["n_duplicate"], "duplicate")
                    # the same call twice gives the same bits, and the source is what it was
                    _check_run(v, _want(name, mc, normals, source, FACTORS[-1]), FACTORS[-1], source, voxel)
                    assert _same_mesh(_fetch(pkg, v, source, src), _source(name, mc, normals, source)), (mc, normals, source)
            assert len(v.extract(mc).key) == len(cs.oracle_mesh(name, mc)["faces"])
    finally:
        v.close()


def test_more_than_256_cell_blocks(pkg):
    """41 x 41 x 41 at 1 voxel: 68 921 cells, 270 cell blocks, so k_tsdf_scan's chunk is 2 for them."""
    name, mc = "41x41x41", 1
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        assert so.grid(dims, voxel, voxel) == (41, 41, 41)
        for source in ("weld", "pruned", "smoothed"):
            src = _make_source(v, mc, True, source)
            got = _check_run(v, _want(name, mc, True, source, 1.0), 1.0, source, voxel)
            assert 0 < len(got.faces) < len(src.faces)
            assert _same_mesh(_fetch(pkg, v, source, src), _source(name, mc, True, source))
    finally:
        v.close()


def test_the_sheet_of_512_triangle_workgroups(pkg):
    """131 072 triangles, 512 triangle workgroups, and the last vertex block holds one vertex."""
    name, mc = "sheet", 1
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        src = v.weld(mc)
        assert (len(src.key), len(src.faces)) == (66049, 131072) and len(src.key) % 256 == 1
        got = _check_run(v, _want(name, mc, False, "weld", 2.0), 2.0, "weld", voxel)
        assert (len(got.key), len(got.faces)) == (4225, 8192)
        _check_run(v, _want(name, mc, False, "weld", 2.0), 2.0, "weld", voxel)
        assert _same_mesh(_fetch(pkg, v, "weld", src), cs.oracle_mesh(name, mc))
    finally:
        v.close()


def test_one_handle_regrows_and_reuses_its_buffers(pkg):
    """Small, large, small on one handle: a coarse grid on a small mesh, the finest grid on a larger one, so that the scratch of
    the cells, of the vertices and of the triangles and the result's buffers all grow, and the first again in the buffers the
    larger one left.  The sizes are the oracle's, asserted so that the test cannot stop growing."""
    name = "41x41x41"
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    sizes = {(2, 3.5): (145, 128), (1, 1.0): (2718, 4693)}
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        for mc, factor in ((2, 3.5), (1, 1.0), (2, 3.5)):
            want = _want(name, mc, True, "weld", factor)
            assert (len(want["key"]), len(want["faces"])) == sizes[(mc, factor)]
            src = v.weld(mc, normals=True)
            _check_run(v, want, factor, "weld", voxel)
            assert _same_mesh(_fetch(pkg, v, "weld", src), cs.oracle_mesh(name, mc, True))
        # the result again, with room for the larger one of round two: the rows past the counts are not written
        (nv, nt), (big_v, big_t) = sizes[(2, 3.5)], sizes[(1, 1.0)]
        xyz, faces, grey = np.full((big_v, 3), -1.0), np.full((big_t, 3), 0xFFFFFFFF, np.uint32), np.full(big_v, 0xA5, np.uint8)
        bgr, nrm, key = np.full((big_v, 3), 0xA5, np.uint8), np.full((big_v, 3), -2.0, np.float32), np.full(big_v, 2**64 - 1, np.uint64)
        assert pkg.load_library().ekf_simplify_get(v._h, P(xyz), P(faces), P(grey), P(bgr), P(nrm), P(key), big_v, big_t) == 0
        got = pkg.IndexedMesh(xyz[:nv], faces[:nt], grey[:nv], bgr[:nv], nrm[:nv], key[:nv])
        assert _same_mesh(got, _want(name, 2, True, "weld", 3.5))
        assert (xyz[nv:] == -1.0).all() and (faces[nt:] == 0xFFFFFFFF).all() and (grey[nv:] == 0xA5).all()
        assert (bgr[nv:] == 0xA5).all() and (nrm[nv:] == -2.0).all() and (key[nv:] == 2**64 - 1).all()
    finally:
        v.close()


def test_a_source_without_triangles_launches_nothing(pkg):
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    try:
        v.profile(True)
        v.weld(1)
        for source in ("weld", "pruned", "smoothed"):
            if source == "pruned":
                v.prune(1)
            if source == "smoothed":
                v.smooth(1)
            m = v.simplify(2.0 * fs.VOXEL, source)
            assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.key.shape == (0,) and m.normals is None
            assert v.simplify_map().shape == (0,) and (v.simplify_stats.degenerate, v.simplify_stats.duplicate) == (0, 0)
        assert _counts(v) == [0] * 10
    finally:
        v.close()


def test_profile_counts(pkg):
    """Every kind once a run and k_tsdf_scan five times; neither k_simp_vertices nor k_simp_faces for an empty result; nothing
    in the six other getters."""
    from ekf_monoslam_amd import fusion
    planes, dims, origin, voxel, trunc, _ = cs.cases()["257x2x2"]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        v.weld(1)
        v.profile(True)
        assert list(v.get_simplify_profile()) == list(fusion.SIMPLIFY_KERNELS) and len(fusion.SIMPLIFY_KERNELS) == 10
        assert fusion.SIMPLIFY_KERNELS[SCAN] == "k_tsdf_scan"
        assert len(v.simplify(voxel).key) == 135
        assert _counts(v) == ONCE
        assert len(v.simplify(2.0 * voxel).key) == 0                 # an empty result: the map, but neither vertices nor faces
        assert _counts(v) == [2, 2, 2, 10, 2, 2, 2, 1, 1, 2]
        assert (v.simplify_map() == so.NONE).all() and v.simplify_stats.degenerate == 964
        assert all(t > 0 for t, _ in v.get_simplify_profile().values())
        count = lambda d: [c for _, c in d.values()]
        assert count(v.get_profile()) == [0] * 4 and count(v.get_mesh_profile()) == [0] * 5 and count(v.get_component_profile()) == [0] * 8
        assert count(v.get_raycast_profile()) == [0, 0] and count(v.get_colour_profile()) == [0, 0, 0] and count(v.get_smooth_profile()) == [0] * 7
        v.smooth(1)
        v.simplify(voxel, "smoothed")                                # from the smoothed mesh: the same launches, and the smoothing's own
        assert _counts(v) == [3, 3, 3, 15, 3, 3, 3, 2, 2, 3] and count(v.get_smooth_profile()) == [1, 1, 1, 1, 1, 2, 0]
    finally:
        v.close()


def test_invalidation_and_argument_errors(pkg):
    lib = pkg.load_library()
    maps = fs.synthetic_maps()
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    err = lambda: lib.ekf_fusion_last_error(v._h).decode()
    n = [C.c_ulonglong(77) for _ in range(4)]
    r = [C.byref(x) for x in n]
    STATE, ARG = 4, 1
    cell = 2.0 * fs.VOXEL
    run = lambda source=0, cell=cell, a=r[0], b=r[1], c=r[2], d=r[3]: lib.ekf_simplify_run(v._h, source, C.c_double(cell), a, b, c, d)
    get = lambda: lib.ekf_simplify_get(v._h, None, None, None, None, None, None, 0, 0)
    gmap = lambda: lib.ekf_simplify_get_map(v._h, None, 0)

    def no_run():
        assert get() == STATE and err() == "ekf_simplify_get: no ekf_simplify_run on the current mesh"
        assert gmap() == STATE and err() == "ekf_simplify_get_map: no ekf_simplify_run on the current mesh"

    def no_weld():
        for source in (0, 1, 2):
            assert run(source) == STATE and err() == "ekf_simplify_run: no ekf_mesh_weld since the volume last changed"
        no_run()

    try:
        no_weld()                                                    # before a weld
        for depth, img, K, pose in maps[:2]:
            v.integrate_host(depth, img, K, pose)
        no_weld()
        first = v.weld(1)
        no_run()                                                     # a weld alone has no simplified mesh
        assert run(1) == STATE and err() == "ekf_simplify_run: source 1 needs an ekf_components_prune since the last ekf_mesh_weld"
        assert run(2) == STATE and err() == "ekf_simplify_run: source 2 needs an ekf_smooth_run on the current mesh"
        # the argument errors, each with its message, before the device is touched; none of them touches a result
        msg = "ekf_simplify_run: source 0, 1 or 2, cell finite and >= the voxel, n_vert, n_tri, n_degenerate and n_duplicate not NULL"
        nan, inf = float("nan"), float("inf")
        for kw in (dict(source=3), dict(source=-1), dict(cell=nan), dict(cell=inf), dict(cell=-inf), dict(cell=0.0), dict(cell=-cell),
                   dict(cell=np.nextafter(fs.VOXEL, 0.0)), dict(a=None), dict(b=None), dict(c=None), dict(d=None)):
            assert run(**kw) == ARG and err() == msg, kw
        assert [x.value for x in n] == [77] * 4
        no_run()
        assert lib.ekf_simplify_run(None, 0, C.c_double(cell), *r) == ARG and lib.ekf_simplify_get_profile(None, None, None) == ARG
        assert lib.ekf_simplify_get(None, None, None, None, None, None, None, 0, 0) == ARG and lib.ekf_simplify_get_map(None, None, 0) == ARG
        ms_, cnt = np.zeros(10), np.zeros(10, np.int64)
        assert lib.ekf_simplify_get_profile(v._h, None, P(cnt)) == ARG and lib.ekf_simplify_get_profile(v._h, P(ms_), P(cnt)) == 0
        # the limit itself is allowed: a cell of exactly one voxel
        assert run(cell=fs.VOXEL) == 0 and n[0].value > 0 and n[1].value + n[2].value + n[3].value == len(first.faces)
        plain = v.simplify(cell)
        assert get() == 0 and gmap() == 0 and plain.normals is None and 0 < len(plain.faces) < len(first.faces)
        nrm, bgr = np.zeros((len(plain.key), 3), np.float32), np.zeros((len(plain.key), 3), np.uint8)
        assert lib.ekf_simplify_get(v._h, None, None, None, None, P(nrm), None, len(nrm), 0) == ARG
        assert err() == "ekf_simplify_get: normal must be NULL after an ekf_simplify_run on a source without normals"
        assert lib.ekf_simplify_get(v._h, None, None, None, P(bgr), None, None, len(bgr), 0) == ARG
        assert "ekf_simplify_get: bgr must be NULL on a plain volume" in err()
        # max_vert and max_tri cut the copies
        part, faces, vmap = np.full((5, 3), -1.0), np.full((4, 3), 7, np.uint32), np.full(6, 99, np.uint32)
        assert lib.ekf_simplify_get(v._h, P(part), P(faces), None, None, None, None, 3, 2) == 0
        assert _same(part[:3], plain.vertices[:3]) and (part[3:] == -1.0).all() and np.array_equal(faces[:2], plain.faces[:2]) and (faces[2:] == 7).all()
        assert lib.ekf_simplify_get_map(v._h, P(vmap), 4) == 0 and (vmap[4:] == 99).all() and np.array_equal(vmap[:4], v.simplify_map()[:4])
        # ekf_smooth_run keeps refusing source 2
        two = [C.c_ulonglong(0), C.c_ulonglong(0)]
        assert lib.ekf_smooth_run(v._h, 2, 1, C.c_double(0.5), C.c_double(-0.53), 0, 0, C.byref(two[0]), C.byref(two[1])) == ARG
        # a prune and a smooth run leave what was made from the weld
        v.prune(2)
        assert get() == 0
        v.smooth(1)
        assert get() == 0 and _same(v.simplify(cell).vertices, plain.vertices)
        # a new smooth run invalidates what was made from source 2, and nothing else
        v.simplify(cell, "smoothed")
        assert get() == 0
        v.smooth(1)
        no_run()
        v.simplify(cell, "pruned")
        v.smooth(1, source="pruned")
        assert get() == 0
        # a new prune invalidates what was made from the pruned or a smoothed pruned mesh
        v.prune(2)
        no_run()
        assert run(2) == STATE and err() == "ekf_simplify_run: source 2 needs an ekf_smooth_run on the current mesh"
        v.smooth(1, source="pruned")
        v.simplify(cell, "smoothed")
        assert get() == 0
        v.prune(2)
        no_run()
        v.simplify(cell, "pruned")
        v.components()                                               # drops the pruned mesh
        no_run()
        assert run(1) == STATE
        v.simplify(cell)
        # a new weld invalidates everything
        v.weld(1)
        no_run()
        assert run(1) == STATE and run(2) == STATE
        v.simplify(cell)
        v.integrate_host(*maps[2])                                   # the volume changes
        no_weld()
        v.weld(1)
        v.simplify(cell)
        v.reset()
        no_weld()
        v.set_volume(*ms.main_volume())
        no_weld()
        v.weld(1, normals=True)
        assert _same_mesh(v.simplify(2.0 * fs.VOXEL), _want("main", 1, True, "weld", 2.0))
        for bad in ("soup", 0, None, "smooth"):
            with pytest.raises(ValueError):
                v.simplify(cell, source=bad)
    finally:
        v.close()


def test_wall_recording_simplified_equals_the_oracle_on_the_same_call_without_it(pkg, tmp_path):
    """mesh_from_recording(simplify=...), alone and behind components=... and smooth=..., against simplify_oracle.simplify of
    the same call without it, on the synthetic recording the smooth tests use."""
    from ekf_monoslam_amd import keyframes
    rec = str(tmp_path / "wall")
    fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
    kw = dict(fs.REC_SWEEP)
    kw["sweep_trunc"] = kw.pop("trunc")
    mesh = lambda m: dict(vertices=m.vertices, faces=m.faces, grey=m.grey, colour=None, normals=m.normals,
                          key=np.arange(len(m.vertices), dtype=np.uint64))
    host = pkg.mesh_from_recording(rec, None, **kw)
    got = pkg.mesh_from_recording(rec, None, simplify=2.0, **kw)
    want = so.simplify(mesh(host), host.origin, host.dims, host.voxel, 2.0 * host.voxel)
    assert _same(got.vertices, want["vertices"]) and _same(got.grey, want["grey"]) and got.colour is None and got.normals is None
    assert got.faces.dtype == host.faces.dtype and np.array_equal(got.faces, want["faces"]) and 0 < len(got.faces) < len(host.faces)
    chain = dict(components=50, smooth=dict(iterations=2, mu=0.0, pin_boundary=True), normals=True)
    before = pkg.mesh_from_recording(rec, None, **chain, **kw)
    got = pkg.mesh_from_recording(rec, None, simplify=1.5, **chain, **kw)
    want = so.simplify(mesh(before), before.origin, before.dims, before.voxel, 1.5 * before.voxel)
    assert _same(got.vertices, want["vertices"]) and _same(got.normals, want["normals"]) and _same(got.grey, want["grey"])
    assert np.array_equal(got.faces, want["faces"]) and 0 < len(got.faces) < len(before.faces)
    for bad in (0, 0.5, -3, "two", True, float("nan"), float("inf"), {"cell": 2}):
        with pytest.raises(ValueError):
            pkg.mesh_from_recording(rec, None, simplify=bad, **kw)
