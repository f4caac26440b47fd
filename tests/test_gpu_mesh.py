"""The weld on the device and the vertex normals against the host weld of the same handle's soup and against
tests/mesh_oracle.py, bit for bit, on the shapes of tests/mesh_scene.py: volumes written with set_volume, so that no sweep
runs."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import mesh_scene as ms

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    """Equal bit for bit."""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got) if got.dtype.kind == "f" else got,
                                                                                  _bits(want) if want.dtype.kind == "f" else want)


def _cases():
    """name -> (planes, dims, origin, voxel, trunc): the wave shapes as colour volumes, the main volume and the sphere grey."""
    out = {ms.shape_id(d): (ms.wave_volume(d, 0, colour=True), d, fs.ORIGIN, ms.VOXEL, fs.TRUNC) for d in ms.WAVE_SHAPES}
    out["main"] = (ms.main_volume(), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    out["sphere"] = (fs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC)
    return out


NAMES = [ms.shape_id(d) for d in ms.WAVE_SHAPES] + ["main", "sphere"]


def _volume(pkg, planes, dims, origin, voxel, trunc):
    v = pkg.TsdfVolume(dims, origin, voxel, trunc, colour=len(planes) > 3)
    v.set_volume(*planes[:3], csum=planes[3] if len(planes) > 3 else None)
    return v


def _same_mesh(m, vertices, faces, grey, key, colour=None):
    return (_same(m.vertices, vertices) and m.faces.dtype == np.uint32 and np.array_equal(m.faces, faces) and _same(m.grey, grey) and
            _same(m.key, key) and (colour is None or _same(m.colour, colour)))


@pytest.mark.parametrize("name", NAMES)
def test_weld_equals_the_host_weld_of_the_same_handle_and_the_normals_the_oracle(pkg, name):
    planes, dims, origin, voxel, trunc = _cases()[name]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        for mc in (1, 2):
            soup = v.extract(mc)
            host = pkg.weld(soup, True) if v.colour else pkg.weld(soup) + (None,)
            key = np.unique(soup.key.reshape(-1))
            got = v.weld(mc)
            print(name, "min_count", mc, ":", len(soup.key), "triangles,", len(got.vertices), "vertices")
            assert got.normals is None and (got.colour is None) == (not v.colour)
            assert mc > 1 or len(got.vertices) > 0
            assert _same_mesh(got, host[0], host[1], host[2], key, host[3])
            want = mo.weld(planes, dims, origin, voxel, soup.key, mc, True)
            assert _same(got.key, want["key"]) and _same(got.vertices, want["vertices"]) and np.array_equal(got.faces, want["faces"])
            with_n = v.weld(mc, normals=True)
            assert _same(with_n.normals, want["normals"])
            assert _same_mesh(with_n, host[0], host[1], host[2], key, host[3])
            again = v.extract(mc)                                    # the soup is what it was
            assert _same(again.xyz, soup.xyz) and _same(again.key, soup.key) and _same(again.grey, soup.grey)
            assert not v.colour or _same(again.colour, soup.colour)
    finally:
        v.close()


def test_the_empty_volume_gives_empty_arrays(pkg):
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    try:
        for normals in (False, True):
            m = v.weld(1, normals)
            assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.grey.shape == (0,) and m.key.shape == (0,)
            assert (m.normals is None) if not normals else m.normals.shape == (0, 3)
        assert len(v.extract(1).key) == 0
    finally:
        v.close()


def test_profile_counts_and_the_re_extract_at_another_min_count(pkg):
    """A weld counts one launch of each of its five kernels and nothing in the fusion handle's own counts, unless the handle
    holds no soup of the weld's min_count: then exactly an extract's launches come first."""
    from ekf_monoslam_amd import fusion
    planes, dims, origin, voxel, trunc = _cases()["main"]
    v = _volume(pkg, planes, dims, origin, voxel, trunc)
    try:
        v.profile(True)
        counts = lambda d: [c for _, c in d.values()]
        v.extract(1)
        before = counts(v.get_profile())
        assert before == [0, 1, 1, 1] and counts(v.get_mesh_profile()) == [0] * 5
        v.weld(1)
        assert counts(v.get_profile()) == before and counts(v.get_mesh_profile()) == [1] * 5
        v.weld(1, normals=True)
        assert counts(v.get_profile()) == before and counts(v.get_mesh_profile()) == [2] * 5
        assert list(v.get_mesh_profile()) == list(fusion.MESH_KERNELS) and all(ms_ > 0 for ms_, _ in v.get_mesh_profile().values())
        m2 = v.weld(2)                                               # another min_count: count, scan, emit again
        assert counts(v.get_profile()) == [0, 2, 2, 2] and counts(v.get_mesh_profile()) == [3] * 5
        host = pkg.weld(v.extract(2))
        assert _same(m2.vertices, host[0]) and np.array_equal(m2.faces, host[1])
        assert counts(v.get_profile()) == [0, 3, 3, 3]
        v.weld(2)                                                    # the soup of the extract just made serves
        assert counts(v.get_profile()) == [0, 3, 3, 3] and counts(v.get_mesh_profile()) == [4] * 5
        assert counts(v.get_raycast_profile()) == [0, 0] and counts(v.get_colour_profile()) == [0, 0, 0]
        v.profile(True)
        v.set_volume(*planes)                                        # no soup at all: the weld extracts
        v.weld(1)
        assert counts(v.get_profile()) == [0, 1, 1, 1] and counts(v.get_mesh_profile()) == [1] * 5
    finally:
        v.close()


def test_a_change_of_the_volume_invalidates_the_weld_and_the_errors_have_their_messages(pkg):
    lib = pkg.load_library()
    maps = fs.synthetic_maps()
    steps, _ = fs.fused()
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    err = lambda: lib.ekf_fusion_last_error(v._h).decode()
    nv, nt = C.c_ulonglong(77), C.c_ulonglong(77)
    try:
        assert lib.ekf_mesh_get(v._h, None, None, None, None, None, None, 0, 0) == 4 and "no ekf_mesh_weld since the volume last changed" in err()
        for depth, img, K, pose in maps[:2]:
            v.integrate_host(depth, img, K, pose)
        first = v.weld(1)
        assert _same_mesh(first, *pkg.weld(v.extract(1)), np.unique(v.extract(1).key.reshape(-1)))
        v.integrate_host(*maps[2])
        assert lib.ekf_mesh_get(v._h, None, None, None, None, None, None, 0, 0) == 4 and "no ekf_mesh_weld" in err()
        got = v.weld(1, normals=True)                                # the weld sees the new volume
        xyz, key, grey, _ = fo.extract(steps[-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, 1)
        want = mo.weld(steps[-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, key, 1, True)
        assert _same_mesh(got, want["vertices"], want["faces"], want["grey"], want["key"]) and _same(got.normals, want["normals"])
        assert not _same(got.vertices, first.vertices)
        # the argument errors, each with its message; none of them touches the weld
        for args in ((0, 0), (65536, 0), (1, 2), (1, -1)):
            assert lib.ekf_mesh_weld(v._h, args[0], args[1], C.byref(nv), C.byref(nt)) == 1
            assert err() == "ekf_mesh_weld: min_count 1..65535, normals 0 or 1, n_vert and n_tri not NULL"
        assert lib.ekf_mesh_weld(v._h, 1, 0, None, C.byref(nt)) == 1 and lib.ekf_mesh_weld(v._h, 1, 0, C.byref(nv), None) == 1
        assert (nv.value, nt.value) == (77, 77)
        bgr = np.zeros((len(got.vertices), 3), np.uint8)
        assert lib.ekf_mesh_get(v._h, None, None, None, P(bgr), None, None, len(bgr), 0) == 1 and "bgr must be NULL on a plain volume" in err()
        nrm = np.zeros((len(got.vertices), 3), np.float32)
        assert lib.ekf_mesh_get(v._h, None, None, None, None, P(nrm), None, len(nrm), 0) == 0 and _same(nrm, want["normals"])
        v.weld(1)
        assert lib.ekf_mesh_get(v._h, None, None, None, None, P(nrm), None, len(nrm), 0) == 1
        assert "normal must be NULL after an ekf_mesh_weld without normals" in err()
        # max_vert and max_tri cut the copies
        part, faces = np.full((5, 3), -1.0), np.full((4, 3), 7, np.uint32)
        assert lib.ekf_mesh_get(v._h, P(part), P(faces), None, None, None, None, 3, 2) == 0
        assert _same(part[:3], want["vertices"][:3]) and (part[3:] == -1.0).all()
        assert np.array_equal(faces[:2], want["faces"][:2]) and (faces[2:] == 7).all()
        v.reset()
        assert lib.ekf_mesh_get(v._h, None, None, None, None, None, None, 0, 0) == 4
        ms_, cnt = np.zeros(5), np.zeros(5, np.int64)
        assert lib.ekf_mesh_get_profile(v._h, None, P(cnt)) == 1 and lib.ekf_mesh_get_profile(v._h, P(ms_), P(cnt)) == 0
    finally:
        v.close()


def test_wall_recording_welded_on_the_device_equals_the_default_call(pkg, tmp_path):
    """mesh_from_recording(weld="device") against the default call array for array; with normals=True the same arrays and the
    oracle's normals of the volume that the oracle fuses from the call's own depth maps."""
    from ekf_monoslam_amd import dense, keyframes
    rec = str(tmp_path / "wall")
    fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
    kw = dict(fs.REC_SWEEP)
    kw["sweep_trunc"] = kw.pop("trunc")
    host = pkg.mesh_from_recording(rec, None, **kw)
    dev = pkg.mesh_from_recording(rec, None, weld="device", **kw)
    with_n = pkg.mesh_from_recording(rec, None, normals=True, **kw)
    assert host.normals is None and dev.normals is None and len(host.faces) > 1000
    for got in (dev, with_n):
        assert _same(got.vertices, host.vertices) and _same(got.faces, host.faces) and _same(got.grey, host.grey)
        assert got.dims == host.dims and (got.voxel, got.trunc) == (host.voxel, host.trunc) and got.colour is None
    K, ids, poses, images = dense.read_recording(rec, None)
    vol = fo.empty_volume(host.dims)
    for m, img in zip(with_n.maps, images):
        fo.integrate(vol, host.dims, host.origin, host.voxel, host.trunc, m.depth, img, K, m.pose)
    key = mo.vertex_keys(vol, 2)
    xyz, grey, u, _ = mo.vertices(vol, host.dims, host.origin, host.voxel, key)
    assert _same(with_n.vertices, xyz) and _same(with_n.grey, grey)
    assert _same(with_n.normals, mo.normals(vol, host.dims, key, u, 2))
    n = with_n.normals.astype(np.float64)
    print("wall: %d vertices, %d with a normal, median n_z %.4f" % (len(n), int((n != 0).any(axis=1).sum()), float(np.median(n[:, 2]))))
    assert float(np.median(n[:, 2])) < -0.9                          # the wall faces the cameras, which look along +z
    path = str(tmp_path / "wall.ply")
    pkg.write_mesh_ply(path, with_n.vertices, with_n.faces, with_n.grey, normals=with_n.normals)
    v2, f2, g2, n2 = pkg.read_mesh_ply(path, normals=True)
    assert _same(v2, host.vertices) and np.array_equal(f2, host.faces) and _same(n2, with_n.normals)
