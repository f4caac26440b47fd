"""Taubin smoothing of the welded or pruned mesh and its own normals on the device against
tests/smooth_oracle.py, bit for bit, on the volumes of tests/component_scene.py: written with set_volume, so that no sweep
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
import smooth_oracle as so

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
ROWS = ("vertices", "grey", "colour", "normals", "key")
ADJACENCY, STEP, NORMALS = slice(0, 5), 5, 6       # of SMOOTH_KERNELS


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
def _source(name, mc, pruned):
    """The oracle's weld of a case, or its prune(9): computed once, shared, and left unchanged."""
    m = cs.oracle_mesh(name, mc)
    return co.prune(m, 9) if pruned else m


@functools.lru_cache(maxsize=None)
def _oracle(name, mc, iterations, mu, pin, pruned=False):
    """The oracle's run with normals; a run without them has the same positions."""
    return so.smooth(_source(name, mc, pruned), iterations, so.LAM, mu, pin, normals=True)


def _want(name, mc, iterations, mu, pin, normals, pruned=False):
    w = dict(_oracle(name, mc, iterations, mu, pin, pruned))
    if not normals:
        w["normals"] = None
    return w


def _counts(v):
    return [c for _, c in v.get_smooth_profile().values()]


def _check_adjacency(v, mesh):
    a = so.adjacency(mesh["faces"], len(mesh["key"]))
    got = v.adjacency()
    assert _same(got.inc, a.inc) and _same(got.deg, a.deg) and _same(got.boundary, a.boundary)
    return a


def _weld_back(pkg, v, like):
    """The weld's arrays as ekf_mesh_get delivers them now."""
    nv, nt = len(like.key), len(like.faces)
    back = pkg.IndexedMesh(np.zeros((nv, 3)), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint8),
                           None if like.colour is None else np.zeros((nv, 3), np.uint8),
                           None if like.normals is None else np.zeros((nv, 3), np.float32), np.zeros(nv, np.uint64))
    lib = pkg.load_library()
    assert lib.ekf_mesh_get(v._h, P(back.vertices), P(back.faces), P(back.grey), P(back.colour), P(back.normals), P(back.key), nv, nt) == 0
    return back


@pytest.mark.parametrize("name", cs.NAMES)
def test_smoothing_equals_the_oracle(pkg, name):
    planes, dims, origin, voxel, trunc, min_counts = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        for mc in min_counts:
            src = cs.oracle_mesh(name, mc)
            weld = v.weld(mc)
            assert _same_mesh(weld, src)
            v.profile(True)
            first = True
            for it in (1, 2, 10):
                for pin in (False, True):
                    for normals in (False, True):
                        got = v.smooth(it, pin_boundary=pin, normals=normals)
                        assert _same_mesh(got, _want(name, mc, it, so.MU, pin, normals)), (mc, it, pin, normals)
                        if first:
                            a = _check_adjacency(v, src)
                            print(name, "min_count", mc, ":", len(src["key"]), "vertices,", len(src["faces"]), "triangles,",
                                  int(a.boundary.sum()), "boundary vertices, longest lists", int(a.inc.max()), int(a.deg.max()))
                            first = False
            got = v.smooth(3, mu=0.0, normals=True)
            assert _same_mesh(got, _want(name, mc, 3, 0.0, False, True))
            # a second identical call: the same bits, three steps and the normals, and no adjacency kernel
            before = _counts(v)
            # (so far: four runs each of 2, 4 and 20 steps, half of them with normals, and three steps with normals)
            assert before == [1] * 5 + [4 * (2 + 4 + 20) + 3, 6 + 1]
            assert _same_mesh(v.smooth(3, mu=0.0, normals=True), _want(name, mc, 3, 0.0, False, True))
            after = _counts(v)
            assert after[ADJACENCY] == [1] * 5 and after[STEP] == before[STEP] + 3 and after[NORMALS] == before[NORMALS] + 1
            _check_adjacency(v, src)
            # the weld is what it was, and so is the soup
            assert _same_mesh(_weld_back(pkg, v, weld), src)
            assert len(v.extract(mc).key) == len(src["faces"])
    finally:
        v.close()


@pytest.mark.parametrize("name,mc", (("main", 1), ("41x41x41", 1), ("41x41x41", 2)))
def test_the_pruned_mesh_smoothed_equals_the_oracle_on_the_oracle_s_prune(pkg, name, mc):
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        weld = v.weld(mc)
        src = _source(name, mc, True)
        pruned = v.prune(9)
        assert _same_mesh(pruned, src) and 0 < len(pruned.key) < len(weld.key)
        v.profile(True)
        for it, pin, normals in ((1, False, False), (2, True, True), (10, False, True)):
            assert _same_mesh(v.smooth(it, pin_boundary=pin, normals=normals, source="pruned"), _want(name, mc, it, so.MU, pin, normals, True))
        _check_adjacency(v, src)
        assert _counts(v)[ADJACENCY] == [1] * 5
        # the weld smoothed after the pruned mesh: another mesh, another adjacency; both sources are what they were
        assert _same_mesh(v.smooth(2, normals=True), _want(name, mc, 2, so.MU, False, True))
        _check_adjacency(v, cs.oracle_mesh(name, mc))
        assert _counts(v)[ADJACENCY] == [2] * 5
        assert _same_mesh(_weld_back(pkg, v, weld), cs.oracle_mesh(name, mc))
        lib = pkg.load_library()
        back = pkg.IndexedMesh(np.zeros_like(pruned.vertices), np.zeros_like(pruned.faces), np.zeros_like(pruned.grey),
                               None if pruned.colour is None else np.zeros_like(pruned.colour), None, np.zeros_like(pruned.key))
        assert lib.ekf_components_get_pruned(v._h, P(back.vertices), P(back.faces), P(back.grey), P(back.colour), None, P(back.key),
                                             len(back.key), len(back.faces)) == 0
        assert _same_mesh(back, src)
    finally:
        v.close()


def test_a_colour_volume_with_weld_normals_keeps_its_rows_and_gets_normals_of_its_own(pkg):
    name, mc = "16x16x3", 2
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        weld = v.weld(mc, normals=True)
        assert v.colour and weld.colour is not None and _same_mesh(weld, cs.oracle_mesh(name, mc, True))
        plain = v.smooth(2)
        assert plain.normals is None and plain.colour is not None and _same_mesh(plain, _want(name, mc, 2, so.MU, False, False))
        own = v.smooth(2, normals=True)
        assert _same_mesh(own, _want(name, mc, 2, so.MU, False, True)) and not _same(own.normals, weld.normals)
        assert _same(own.colour, weld.colour) and _same(own.grey, weld.grey) and _same(own.key, weld.key) and _same(own.faces, weld.faces)
        assert _same_mesh(_weld_back(pkg, v, weld), cs.oracle_mesh(name, mc, True))
    finally:
        v.close()


def test_one_handle_regrows_and_reuses_its_mesh_buffers(pkg):
    """Three rounds of weld, prune and smooth on one handle: a mesh, a larger one, so that the buffers of all three grow, and the
    first again, in the buffers the larger one left.  The sizes are the oracle's, asserted so that the test cannot stop growing."""
    name = "41x41x41"
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    sizes = {2: (5099, 7154), 1: (7685, 13536)}
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        for mc in (2, 1, 2):
            src = cs.oracle_mesh(name, mc, True)
            assert (len(src["key"]), len(src["faces"])) == sizes[mc]
            cut = co.prune(src, 3)
            weld = v.weld(mc, normals=True)
            assert _same_mesh(weld, src), mc
            assert _same_mesh(v.prune(3), cut), mc
            assert _same_mesh(v.smooth(2, normals=True, source="pruned"), so.smooth(cut, 2, normals=True)), mc
            assert _same_mesh(_weld_back(pkg, v, weld), src), mc
        # the weld again, with room for the larger mesh of round two: the rows past the counts are not written
        (nv, nt), (big_v, big_t) = sizes[2], sizes[1]
        xyz, faces, grey = np.full((big_v, 3), -1.0), np.full((big_t, 3), 0xFFFFFFFF, np.uint32), np.full(big_v, 0xA5, np.uint8)
        bgr, nrm, key = np.full((big_v, 3), 0xA5, np.uint8), np.full((big_v, 3), -2.0, np.float32), np.full(big_v, 2**64 - 1, np.uint64)
        assert pkg.load_library().ekf_mesh_get(v._h, P(xyz), P(faces), P(grey), P(bgr), P(nrm), P(key), big_v, big_t) == 0
        got = pkg.IndexedMesh(xyz[:nv], faces[:nt], grey[:nv], bgr[:nv], nrm[:nv], key[:nv])
        assert _same_mesh(got, cs.oracle_mesh(name, 2, True))
        assert (xyz[nv:] == -1.0).all() and (faces[nt:] == 0xFFFFFFFF).all() and (grey[nv:] == 0xA5).all()
        assert (bgr[nv:] == 0xA5).all() and (nrm[nv:] == -2.0).all() and (key[nv:] == 2**64 - 1).all()
    finally:
        v.close()


def test_the_empty_volume_launches_nothing(pkg):
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    try:
        v.profile(True)
        v.weld(1)
        for source in ("weld", "pruned"):
            if source == "pruned":
                v.prune(1)
            m = v.smooth(3, normals=True, source=source)
            assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.key.shape == (0,) and m.normals.shape == (0, 3)
            a = v.adjacency()
            assert a.inc.shape == (0,) and a.deg.shape == (0,) and a.boundary.shape == (0,)
        assert _counts(v) == [0] * 7
    finally:
        v.close()


def test_profile_counts(pkg):
    """The adjacency once a mesh, a step `iterations` times, or twice that with mu != 0, the normals once on request, and
    nothing in the five other getters."""
    from ekf_monoslam_amd import fusion
    planes, dims, origin, voxel, trunc, _ = cs.cases()["main"]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        v.weld(1)
        v.profile(True)
        assert list(v.get_smooth_profile()) == list(fusion.SMOOTH_KERNELS) and len(fusion.SMOOTH_KERNELS) == 7
        v.smooth(4)
        assert _counts(v) == [1, 1, 1, 1, 1, 8, 0]
        v.smooth(5, mu=0.0, normals=True)
        assert _counts(v) == [1, 1, 1, 1, 1, 13, 1]
        v.smooth(1, pin_boundary=True)
        assert _counts(v) == [1, 1, 1, 1, 1, 15, 1]
        assert all(t > 0 for t, _ in v.get_smooth_profile().values())
        count = lambda d: [c for _, c in d.values()]
        assert count(v.get_profile()) == [0] * 4 and count(v.get_mesh_profile()) == [0] * 5 and count(v.get_component_profile()) == [0] * 8
        assert count(v.get_raycast_profile()) == [0, 0] and count(v.get_colour_profile()) == [0, 0, 0]
        v.weld(1)                                                    # a new weld: the adjacency again
        v.profile(True)
        v.smooth(1, mu=0.0)
        assert _counts(v) == [1, 1, 1, 1, 1, 1, 0]
        v.prune(3)                                                   # the weld's adjacency stays until a run on the pruned mesh replaces it
        v.smooth(1, mu=0.0)
        assert _counts(v) == [1, 1, 1, 1, 1, 2, 0]
        v.smooth(1, source="pruned")
        assert _counts(v) == [2, 2, 2, 2, 2, 4, 0]
        v.prune(3)                                                   # a new prune: its adjacency again
        v.smooth(1, source="pruned")
        assert _counts(v) == [3, 3, 3, 3, 3, 6, 0]
    finally:
        v.close()


def test_invalidation_and_argument_errors(pkg):
    lib = pkg.load_library()
    maps = fs.synthetic_maps()
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    err = lambda: lib.ekf_fusion_last_error(v._h).decode()
    n = [C.c_ulonglong(77) for _ in range(2)]
    r = [C.byref(x) for x in n]
    STATE, ARG = 4, 1
    run = lambda source=0, it=1, lam=0.5, mu=-0.53, pin=0, nrm=0, a=r[0], b=r[1]: lib.ekf_smooth_run(v._h, source, it, lam, mu, pin, nrm, a, b)
    get = lambda: lib.ekf_smooth_get(v._h, None, None, None, None, None, None, 0, 0)
    adj = lambda: lib.ekf_smooth_get_adjacency(v._h, None, None, None, 0)

    def no_run():
        assert get() == STATE and err() == "ekf_smooth_get: no ekf_smooth_run on the current mesh"
        assert adj() == STATE and err() == "ekf_smooth_get_adjacency: no ekf_smooth_run on the current mesh"

    def no_weld():
        assert run() == STATE and err() == "ekf_smooth_run: no ekf_mesh_weld since the volume last changed"
        assert run(1) == STATE and err() == "ekf_smooth_run: no ekf_mesh_weld since the volume last changed"
        no_run()

    try:
        no_weld()                                                    # before a weld
        for depth, img, K, pose in maps[:2]:
            v.integrate_host(depth, img, K, pose)
        no_weld()
        first = v.weld(1)
        no_run()                                                     # a weld alone has no smoothed mesh
        assert run(1) == STATE and err() == "ekf_smooth_run: source 1 needs an ekf_components_prune since the last ekf_mesh_weld"
        # the argument errors, each with its message, before the device is touched; none of them touches a result
        msg = ("ekf_smooth_run: source 0 or 1, iterations 1..1024, 0 < lambda <= 1, -1 <= mu <= 0, pin_boundary and normals 0 or 1, "
               "n_vert and n_tri not NULL")
        nan, inf = float("nan"), float("inf")
        for kw in (dict(source=2), dict(source=-1), dict(it=0), dict(it=1025), dict(it=-5), dict(lam=0.0), dict(lam=1.5), dict(lam=-0.5),
                   dict(lam=nan), dict(lam=inf), dict(mu=0.1), dict(mu=-1.5), dict(mu=nan), dict(mu=-inf), dict(pin=2), dict(pin=-1),
                   dict(nrm=2), dict(nrm=-1), dict(a=None), dict(b=None)):
            assert run(**kw) == ARG and err() == msg, kw
        assert [x.value for x in n] == [77, 77]
        no_run()
        assert lib.ekf_smooth_run(None, 0, 1, 0.5, -0.53, 0, 0, r[0], r[1]) == ARG and lib.ekf_smooth_get_profile(None, None, None) == ARG
        assert lib.ekf_smooth_get(None, None, None, None, None, None, None, 0, 0) == ARG and lib.ekf_smooth_get_adjacency(None, None, None, None, 0) == ARG
        ms_, cnt = np.zeros(7), np.zeros(7, np.int64)
        assert lib.ekf_smooth_get_profile(v._h, None, P(cnt)) == ARG and lib.ekf_smooth_get_profile(v._h, P(ms_), P(cnt)) == 0
        # the limits themselves are allowed
        assert run(it=1024, lam=1.0, mu=-1.0) == 0 and [x.value for x in n] == [len(first.key), len(first.faces)]
        plain = v.smooth(2)
        assert get() == 0 and adj() == 0
        nrm, bgr = np.zeros((len(plain.key), 3), np.float32), np.zeros((len(plain.key), 3), np.uint8)
        assert lib.ekf_smooth_get(v._h, None, None, None, None, P(nrm), None, len(nrm), 0) == ARG
        assert err() == "ekf_smooth_get: normal must be NULL after an ekf_smooth_run without normals"
        assert lib.ekf_smooth_get(v._h, None, None, None, P(bgr), None, None, len(bgr), 0) == ARG
        assert "ekf_smooth_get: bgr must be NULL on a plain volume" in err()
        # max_vert and max_tri cut the copies
        part, faces, inc = np.full((5, 3), -1.0), np.full((4, 3), 7, np.uint32), np.full(6, 99, np.uint32)
        assert lib.ekf_smooth_get(v._h, P(part), P(faces), None, None, None, None, 3, 2) == 0
        assert _same(part[:3], plain.vertices[:3]) and (part[3:] == -1.0).all() and np.array_equal(faces[:2], first.faces[:2]) and (faces[2:] == 7).all()
        assert lib.ekf_smooth_get_adjacency(v._h, P(inc), None, None, 4) == 0 and (inc[4:] == 99).all() and (inc[:4] != 99).all()
        # a prune leaves what was made from the weld; a new prune invalidates what was made from the pruned mesh
        v.prune(2)
        assert get() == 0 and _same(v.smooth(2).vertices, plain.vertices)
        v.smooth(1, source="pruned")
        assert get() == 0
        v.prune(2)
        no_run()
        v.smooth(1, source="pruned")
        v.components()                                               # drops the pruned mesh
        no_run()
        assert run(1) == STATE
        v.smooth(1)
        # a new weld invalidates everything
        v.weld(1)
        no_run()
        assert run(1) == STATE
        v.smooth(1)
        v.integrate_host(*maps[2])                                   # the volume changes
        no_weld()
        v.weld(1)
        v.smooth(1)
        v.reset()
        no_weld()
        v.set_volume(*ms.main_volume())
        no_weld()
        v.weld(1)
        assert _same_mesh(v.smooth(2, normals=True), _want("main", 1, 2, so.MU, False, True))
        for bad in ("soup", 0, None):
            with pytest.raises(ValueError):
                v.smooth(source=bad)
    finally:
        v.close()


def test_wall_recording_smoothed_equals_the_oracle_on_the_same_call_without_it(pkg, tmp_path):
    """mesh_from_recording(smooth=...), alone and behind components=..., against smooth_oracle.smooth of the same call
    without it."""
    from ekf_monoslam_amd import keyframes
    rec = str(tmp_path / "wall")
    fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
    kw = dict(fs.REC_SWEEP)
    kw["sweep_trunc"] = kw.pop("trunc")
    mesh = lambda m: dict(vertices=m.vertices, faces=m.faces, grey=m.grey, colour=None, normals=None,
                          key=np.arange(len(m.vertices), dtype=np.uint64))
    host = pkg.mesh_from_recording(rec, None, **kw)
    got = pkg.mesh_from_recording(rec, None, smooth=3, **kw)
    want = so.smooth(mesh(host), 3)
    assert _same(got.vertices, want["vertices"]) and _same(got.grey, host.grey) and got.colour is None and got.normals is None
    assert got.faces.dtype == host.faces.dtype and np.array_equal(got.faces, host.faces) and not _same(got.vertices, host.vertices)
    cut = pkg.mesh_from_recording(rec, None, components=50, **kw)
    got = pkg.mesh_from_recording(rec, None, components=50, smooth=dict(iterations=2, mu=0.0, pin_boundary=True), normals=True, **kw)
    want = so.smooth(mesh(cut), 2, so.LAM, 0.0, True, normals=True)
    assert 0 < len(cut.faces) < len(host.faces)
    assert _same(got.vertices, want["vertices"]) and _same(got.normals, want["normals"]) and _same(got.grey, cut.grey)
    assert np.array_equal(got.faces, cut.faces)
    for bad in (0, -3, "ten", True, 2.5, {"rounds": 2}):
        with pytest.raises(ValueError):
            pkg.mesh_from_recording(rec, None, smooth=bad, **kw)
