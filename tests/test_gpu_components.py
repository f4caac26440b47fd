"""The connected components of the welded mesh and its pruned copy on the device against
tests/component_oracle.py, bit for bit, on the volumes of tests/component_scene.py: written with set_volume, so that no sweep
runs.  Everything is integers or copied bits: every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import component_oracle as co
import component_scene as cs
import fusion_scene as fs
import mesh_scene as ms

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
ROWS = ("vertices", "grey", "colour", "normals", "key")


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


# (case, min_count) -> a threshold that must remove something and keep something
SPLITS = {("257x2x2", 1): 9, ("16x16x3", 2): 41, ("main", 1): 3, ("main", 2): 9, ("41x41x41", 1): 9, ("41x41x41", 2): 41}


@pytest.mark.parametrize("name", cs.NAMES)
def test_components_and_prunes_equal_the_oracle(pkg, name):
    planes, dims, origin, voxel, trunc, min_counts = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        for mc in min_counts:
            want = cs.oracle_mesh(name, mc)
            weld = v.weld(mc)
            assert _same_mesh(weld, want)
            nv = len(want["key"])
            label, size, count = co.components(want["faces"], nv)
            got = v.components()
            print(name, "min_count", mc, ":", nv, "vertices,", len(want["faces"]), "triangles,", got.count, "components, sizes",
                  sorted(cs.sizes(size, label))[-4:])
            assert got.count == count and _same(got.label, label) and _same(got.size, size)
            top = int(size.max())
            for t in cs.THRESHOLDS + (top + 1,):
                for largest in (False, True):
                    expect = co.prune(want, t, largest)
                    pruned = v.prune(t, largest)
                    assert _same_mesh(pruned, expect), (t, largest)
                    assert v.pruned_components == expect["components"]
                    assert _same_mesh(v.prune(t, largest), expect)           # a second call gives the same bits
            assert len(v.prune(top + 1).key) == 0 and v.prune(top + 1).faces.shape == (0, 3)
            if (name, mc) in SPLITS:
                cut = v.prune(SPLITS[(name, mc)])
                assert 0 < len(cut.faces) < len(want["faces"]) and 0 < len(cut.key) < nv
            if count > 1:
                one = v.prune(largest=True)
                assert len(one.faces) == top and 0 < len(one.key) < nv
            again = v.components()                                           # the labels are what they were after the prunes
            assert again.count == count and _same(again.label, label) and _same(again.size, size)
    finally:
        v.close()


def test_the_four_way_tie_keeps_label_0(pkg):
    planes, dims, origin, voxel, trunc, _ = cs.cases()["tie"]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        v.weld(1)
        c = v.components()
        assert c.count == 4 and sorted(set(c.label.tolist())) == [0, 255, 510, 765] and set(c.size.tolist()) == {448}
        one = v.prune(largest=True)
        assert len(one.key) == 255 and len(one.faces) == 448 and v.pruned_components == 1
        assert _same(one.key, cs.oracle_mesh("tie", 1)["key"][:255])
        assert len(v.prune(448).faces) == 4 * 448 and len(v.prune(449).faces) == 0 and len(v.prune(449, True).faces) == 0
    finally:
        v.close()


def test_the_empty_volume_launches_nothing(pkg):
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    try:
        v.profile(True)
        v.weld(1)
        c = v.components()
        assert c.count == 0 and c.label.shape == (0,) and c.size.shape == (0,)
        for largest in (False, True):
            m = v.prune(1, largest)
            assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.key.shape == (0,) and v.pruned_components == 0
        assert [n for _, n in v.get_component_profile().values()] == [0] * 8
    finally:
        v.close()


def test_colour_and_normals_are_carried_through_and_the_weld_stays(pkg):
    name, mc = "16x16x3", 2
    planes, dims, origin, voxel, trunc, _ = cs.cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        want = cs.oracle_mesh(name, mc, True)
        weld = v.weld(mc, normals=True)
        assert v.colour and _same_mesh(weld, want)
        for t, largest in ((41, False), (1, True), (1, False)):
            expect = co.prune(want, t, largest)
            got = v.prune(t, largest)
            assert got.colour is not None and got.normals is not None and _same_mesh(got, expect)
            assert np.all(np.diff(got.key.astype(np.int64)) > 0)
        assert len(v.prune(41).key) < len(weld.key)
        # the weld's arrays after the prunes are what they were, and so is the soup
        nv, nt = len(weld.key), len(weld.faces)
        back = pkg.IndexedMesh(np.zeros((nv, 3)), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint8), np.zeros((nv, 3), np.uint8),
                               np.zeros((nv, 3), np.float32), np.zeros(nv, np.uint64))
        lib = pkg.load_library()
        assert lib.ekf_mesh_get(v._h, P(back.vertices), P(back.faces), P(back.grey), P(back.colour), P(back.normals), P(back.key), nv, nt) == 0
        assert _same_mesh(back, want)
        assert len(v.extract(mc).key) == nt
        # a weld without normals: the pruned mesh has none, and asking for them is an argument error with its message
        v.weld(mc)
        plain = v.prune(41)
        assert plain.normals is None and _same_mesh(plain, co.prune(cs.oracle_mesh(name, mc), 41))
        nrm = np.zeros((len(plain.key), 3), np.float32)
        assert lib.ekf_components_get_pruned(v._h, None, None, None, None, P(nrm), None, len(nrm), 0) == 1
        assert "normal must be NULL after an ekf_mesh_weld without normals" in lib.ekf_fusion_last_error(v._h).decode()
    finally:
        v.close()


def test_profile_counts(pkg):
    """Each kind once a call (the scan three times a prune), k_comp_largest only with `largest`, the components only once a
    weld, and nothing in the four other getters."""
    from ekf_monoslam_amd import fusion
    planes, dims, origin, voxel, trunc, _ = cs.cases()["main"]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        counts = lambda d: [c for _, c in d.values()]
        v.weld(1)
        v.profile(True)
        assert list(v.get_component_profile()) == list(fusion.COMPONENT_KERNELS) and len(fusion.COMPONENT_KERNELS) == 8
        v.components()                                               # init, union, count, and flags for the sizes
        assert counts(v.get_component_profile()) == [1, 1, 1, 0, 1, 0, 0, 0]
        v.prune(3)                                                   # the components are held: flags, three scans, vertices, faces
        assert counts(v.get_component_profile()) == [1, 1, 1, 0, 2, 3, 1, 1]
        v.prune(3, largest=True)
        assert counts(v.get_component_profile()) == [1, 1, 1, 1, 3, 6, 2, 2]
        v.prune(1000)                                                # an empty result: neither vertices nor faces
        assert counts(v.get_component_profile()) == [1, 1, 1, 1, 4, 9, 2, 2]
        assert all(t > 0 for t, _ in v.get_component_profile().values())
        assert counts(v.get_profile()) == [0] * 4 and counts(v.get_mesh_profile()) == [0] * 5
        assert counts(v.get_raycast_profile()) == [0, 0] and counts(v.get_colour_profile()) == [0, 0, 0]
        v.weld(1)                                                    # a new weld: a prune finds the components first, without flags of their own
        v.profile(True)
        v.prune(3)
        assert counts(v.get_component_profile()) == [1, 1, 1, 0, 1, 3, 1, 1]
        c = v.components()
        assert c.count == 3 and sorted(cs.sizes(c.size, c.label)) == [2, 8, 262]
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

    def no_weld():
        assert lib.ekf_components_find(v._h, r[0]) == STATE and "ekf_components_find: no ekf_mesh_weld since the volume last changed" in err()
        assert lib.ekf_components_prune(v._h, 1, 0, r[1], r[2], r[3]) == STATE and "ekf_components_prune: no ekf_mesh_weld since the volume last changed" in err()
        assert lib.ekf_components_get(v._h, None, None, 0) == STATE and "ekf_components_get: no ekf_components_find" in err()
        assert lib.ekf_components_get_pruned(v._h, None, None, None, None, None, None, 0, 0) == STATE and "ekf_components_get_pruned: no ekf_components_prune" in err()

    try:
        no_weld()                                                    # before a weld
        for depth, img, K, pose in maps[:2]:
            v.integrate_host(depth, img, K, pose)
        no_weld()
        first = v.weld(1)
        # a weld alone has neither labels nor a pruned mesh
        assert lib.ekf_components_get(v._h, None, None, 0) == STATE and lib.ekf_components_get_pruned(v._h, None, None, None, None, None, None, 0, 0) == STATE
        full = v.prune(1)
        assert all(_same(getattr(full, k), getattr(first, k)) for k in ROWS + ("faces",))     # the identity
        assert lib.ekf_components_get(v._h, None, None, 0) == 0                          # the prune found them
        # the argument errors, each with its message, before the device is touched; none of them touches a result
        msg = "ekf_components_prune: min_triangles >= 1, largest 0 or 1, n_vert, n_tri and n_kept not NULL"
        for args in ((0, 0), (1, 2), (1, -1)):
            assert lib.ekf_components_prune(v._h, args[0], args[1], r[1], r[2], r[3]) == ARG and err() == msg
        for skip in (1, 2, 3):
            a = [None if i == skip else r[i] for i in (1, 2, 3)]
            assert lib.ekf_components_prune(v._h, 1, 0, *a) == ARG and err() == msg
        assert lib.ekf_components_find(v._h, None) == ARG and err() == "ekf_components_find: n_comp not NULL"
        assert [x.value for x in n] == [77] * 4
        bgr = np.zeros((len(full.key), 3), np.uint8)
        assert lib.ekf_components_get_pruned(v._h, None, None, None, P(bgr), None, None, len(bgr), 0) == ARG
        assert "ekf_components_get_pruned: bgr must be NULL on a plain volume" in err()
        assert lib.ekf_components_find(None, r[0]) == ARG and lib.ekf_components_get(None, None, None, 0) == ARG
        assert lib.ekf_components_prune(None, 1, 0, r[1], r[2], r[3]) == ARG and lib.ekf_components_get_profile(None, None, None) == ARG
        assert lib.ekf_components_get_pruned(None, None, None, None, None, None, None, 0, 0) == ARG
        ms_, cnt = np.zeros(8), np.zeros(8, np.int64)
        assert lib.ekf_components_get_profile(v._h, None, P(cnt)) == ARG and lib.ekf_components_get_profile(v._h, P(ms_), P(cnt)) == 0
        # max_vert and max_tri cut the copies
        part, faces, lab = np.full((5, 3), -1.0), np.full((4, 3), 7, np.uint32), np.full(6, 9, np.uint32)
        assert lib.ekf_components_get_pruned(v._h, P(part), P(faces), None, None, None, None, 3, 2) == 0
        assert _same(part[:3], first.vertices[:3]) and (part[3:] == -1.0).all() and np.array_equal(faces[:2], first.faces[:2]) and (faces[2:] == 7).all()
        assert lib.ekf_components_get(v._h, P(lab), None, 4) == 0 and (lab[4:] == 9).all() and (lab[:4] != 9).all()
        # a new weld invalidates the labels and the pruned mesh
        v.weld(1)
        assert lib.ekf_components_get(v._h, None, None, 0) == STATE and lib.ekf_components_get_pruned(v._h, None, None, None, None, None, None, 0, 0) == STATE
        v.components()
        assert lib.ekf_components_get(v._h, None, None, 0) == 0 and lib.ekf_components_get_pruned(v._h, None, None, None, None, None, None, 0, 0) == STATE
        v.prune(2)
        v.integrate_host(*maps[2])                                   # the volume changes
        no_weld()
        v.weld(1)
        v.prune(2)
        v.reset()
        no_weld()
        v.set_volume(*ms.main_volume())
        no_weld()
        v.weld(1)
        assert v.components().count == 3
    finally:
        v.close()


def test_wall_recording_pruned_equals_the_oracle_prune_of_the_default_call(pkg, tmp_path):
    """mesh_from_recording(components=...) against component_oracle.prune of the same call without it."""
    from ekf_monoslam_amd import keyframes
    rec = str(tmp_path / "wall")
    fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
    kw = dict(fs.REC_SWEEP)
    kw["sweep_trunc"] = kw.pop("trunc")
    host = pkg.mesh_from_recording(rec, None, **kw)
    base = dict(vertices=host.vertices, faces=host.faces, grey=host.grey, colour=None, normals=None,
                key=np.arange(len(host.vertices), dtype=np.uint64))
    label, size, count = co.components(host.faces, len(host.vertices))
    print("wall: %d triangles in %d components, sizes %s" % (len(host.faces), count, sorted(cs.sizes(size, label))[-5:]))
    for arg, t, largest in ((50, 50, False), ("largest", 1, True)):
        got = pkg.mesh_from_recording(rec, None, components=arg, **kw)
        want = co.prune(base, t, largest)
        assert _same(got.vertices, want["vertices"]) and _same(got.grey, want["grey"]) and got.colour is None
        assert got.faces.dtype == host.faces.dtype and np.array_equal(got.faces, want["faces"])
    for bad in (0, -3, "smallest", True, 2.5):
        with pytest.raises(ValueError):
            pkg.mesh_from_recording(rec, None, components=bad, **kw)
