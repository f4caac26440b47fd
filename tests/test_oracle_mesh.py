"""The welded mesh and its vertex normals in tests/mesh_oracle.py alone: the gather rule (which edges carry a
vertex, from the signs and the cells' validity) against the sort of the extraction's soup on every shape of tests/mesh_scene.py
and on random volumes, the colours likewise, the normals on the analytic sphere, the PLY round trip, and the prototype table.
CPU only."""
import ctypes as C
import inspect

import numpy as np
import pytest

import colour_oracle as co
import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import mesh_scene as ms

NAMES = ("ekf_mesh_weld", "ekf_mesh_get", "ekf_mesh_get_profile")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _against_the_sort(vol, dims, origin, voxel, min_count):
    """The oracle's gather rule against weld(extract(.)) of the fusion oracle: vertices, faces, grey and keys; and the colours of
    a volume with colour planes against the colour oracle's.  Returns the welded mesh of the gather rule."""
    xyz, key, grey, _ = fo.extract(vol[:3], dims, origin, voxel, min_count)
    first, faces = fo.weld(key)
    got = mo.weld(vol, dims, origin, voxel, key, min_count)
    assert got["key"].dtype == np.uint64 and np.array_equal(got["key"], key.reshape(-1)[first])
    assert np.array_equal(_bits(got["vertices"]), _bits(xyz.reshape(-1, 3)[first]))
    assert np.array_equal(got["grey"], grey.reshape(-1)[first])
    assert got["faces"].shape == faces.shape and np.array_equal(got["faces"], faces)
    if len(vol) > 3:
        want = co.vertex_colours(vol, dims, key).reshape(-1, 3)[first]
        assert got["colour"].dtype == np.uint8 and np.array_equal(got["colour"], want)
    return got


@pytest.mark.parametrize("min_count", (1, 2, 4))
def test_gather_rule_equals_the_sort_on_the_main_volume(min_count):
    got = _against_the_sort(ms.main_volume(), fs.DIMS, fs.ORIGIN, fs.VOXEL, min_count)
    print("main, min_count", min_count, ":", len(got["vertices"]), "vertices,", len(got["faces"]), "faces")
    assert (len(got["vertices"]) > 0) == (min_count < 4)


def test_gather_rule_equals_the_sort_on_one_cell_the_sphere_and_nothing():
    tiny = fs.fused(fs.TINY_DIMS, fs.TINY_ORIGIN)[0][-1]
    _against_the_sort(tiny, fs.TINY_DIMS, fs.TINY_ORIGIN, fs.VOXEL, 1)
    one = (np.array([-1, 1, 1, 1, 1, 1, 1, 1], np.float32).reshape(2, 2, 2), np.ones((2, 2, 2), np.uint16), np.full((2, 2, 2), 9, np.uint32))
    got = _against_the_sort(one, (2, 2, 2), fs.TINY_ORIGIN, fs.VOXEL, 1)
    assert len(got["vertices"]) == 7 and len(got["faces"]) == 6       # corner 0 alone inside: every edge from it, a fan of six
    got = _against_the_sort(fs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    assert len(got["vertices"]) - 3 * len(got["faces"]) // 2 + len(got["faces"]) == 2     # closed, genus 0: V - E + F = 2
    empty = fo.empty_volume(fs.DIMS)
    got = _against_the_sort(empty, fs.DIMS, fs.ORIGIN, fs.VOXEL, 1)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["key"].shape == (0,)
    assert mo.weld(empty, fs.DIMS, fs.ORIGIN, fs.VOXEL, np.zeros((0, 3), np.uint64), 1, True)["normals"].shape == (0, 3)


@pytest.mark.parametrize("dims", ms.WAVE_SHAPES[:4], ids=ms.shape_id)
def test_gather_rule_equals_the_sort_on_the_gpu_shapes(dims):
    for mc in (1, 2):
        _against_the_sort(ms.wave_volume(dims, 0, colour=True), dims, fs.ORIGIN, ms.VOXEL, mc)


def test_gather_rule_equals_the_sort_on_random_volumes():
    """Random signs, cnt from {0, 1, 2, 3}: crossing edges all of whose cells are invalid occur (no vertex), and so do crossing
    edges with exactly one valid cell (a vertex)."""
    cases = ms.random_cases()
    assert len(cases) >= 20
    none_valid = one_valid = 0
    for dims, seed, mc in cases:
        vol = ms.random_volume(dims, seed)
        got = _against_the_sort(vol, dims, fs.ORIGIN, ms.VOXEL, mc)
        cells = mo.edge_cells(vol[1], mc)
        inside = vol[0] < 0
        nz, ny, nx = inside.shape
        for d in range(1, 8):
            dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
            cross = np.zeros(inside.shape, bool)
            cross[:nz - dz, :ny - dy, :nx - dx] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
            none_valid += int((cross & (cells[d] == 0)).sum())
            one_valid += int((cross & (cells[d] == 1)).sum())
            assert cells[d].max() <= (0, 4, 2, 1)[bin(d).count("1")]
        assert len(got["key"]) == int(sum(bin(int(m)).count("1") for m in mo.edge_masks(vol, mc).reshape(-1)))
    print("crossing edges without a valid cell:", none_valid, " with exactly one:", one_valid)
    assert none_valid > 0 and one_valid > 0


def test_a_cell_count_per_edge_kind():
    """4, 2 or 1 cells hold an axis edge, a face diagonal or the body diagonal, in the interior of a fully valid grid."""
    cells = mo.edge_cells(np.ones((5, 5, 5), np.uint16), 1)
    assert [int(cells[d][2, 2, 2]) for d in range(1, 8)] == [4, 4, 2, 4, 2, 2, 1]
    assert [int(cells[d][0, 0, 0]) for d in range(1, 8)] == [1, 1, 1, 1, 1, 1, 1]
    assert all(int(cells[d][4, 4, 4]) == 0 for d in range(1, 8))


def _sphere_normals():
    vol = fs.sphere_volume()
    _, key, _, _ = fo.extract(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    return mo.weld(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, key, 1, True)


def test_normals_of_the_sphere_point_outwards_and_have_unit_length():
    m = _sphere_normals()
    n = m["normals"].astype(np.float64)
    assert m["normals"].dtype == np.float32 and n.shape == m["vertices"].shape
    nz = (n != 0).any(axis=1)
    radial = ms.sphere_radial(m["vertices"])
    dot = (n * radial).sum(axis=1)
    length = np.sqrt((n * n).sum(axis=1))
    assert nz.sum() > 0 and (dot[nz] > 0).all()
    assert (np.abs(length[nz] - 1.0) <= 2.0 ** -22).all(), float(np.abs(length[nz] - 1.0).max())
    angle = np.degrees(np.arccos(np.clip(dot[nz], -1.0, 1.0)))
    f = m["faces"]
    A, B, Cc = (m["vertices"][f[:, i]] for i in range(3))
    geo = np.cross(B - A, Cc - A)
    agree = (geo * (n[f[:, 0]] + n[f[:, 1]] + n[f[:, 2]])).sum(axis=1) > 0
    area = (geo * geo).sum(axis=1) > 0
    print("sphere: %d vertices, %d with a normal; angle to the radial direction: largest %.3f deg, median %.3f deg; faces whose "
          "geometric normal agrees with the sum of their vertex normals: %.4f (of those with an area: %.4f)"
          % (len(n), int(nz.sum()), float(angle.max()), float(np.median(angle)), float(agree.mean()), float(agree[area].mean())))


def test_normals_use_only_counted_neighbours():
    """The four cases of the gradient on a line: both neighbours, the upper alone, the lower alone, none."""
    s = np.zeros((2, 2, 5), np.float32)
    s[:, :, :] = np.array([-3.0, -1.0, 2.0, 3.0, 7.0], np.float32)
    cnt = np.ones((2, 2, 5), np.uint16)
    g = mo.gradient((s, cnt), 1)
    assert g[0][0, 0].tolist() == [2.0, 2.5, 2.0, 2.5, 4.0] and not g[1].any() and not g[2].any()
    cnt[:, :, 1] = 0
    g = mo.gradient((s, cnt), 1)
    assert g[0][0, 0, 0] == 0.0 and g[0][0, 0, 2] == 1.0                # voxel 0: no usable neighbour on x; voxel 2: the upper alone
    cnt[:, :, 1], cnt[:, :, 3] = 1, 0
    assert mo.gradient((s, cnt), 1)[0][0, 0, 2] == 3.0                 # the lower alone
    cnt2 = np.full((2, 2, 5), 2, np.uint16)
    cnt2[:, :, 3] = 1
    g = mo.gradient((s, cnt2), 2)
    assert g[0][0, 0, 2] == 1.5 and g[0][0, 0, 4] == 0.0                # v = sum / cnt; a neighbour below min_count does not count


def test_ply_round_trip_with_normals(pkg, tmp_path):
    from ekf_monoslam_amd import fusion
    m = _sphere_normals()
    colour = (np.arange(3 * len(m["grey"])) % 251).astype(np.uint8).reshape(-1, 3)
    plain, with_n, both = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply"))
    fusion.write_mesh_ply(plain, m["vertices"], m["faces"], m["grey"])
    fusion.write_mesh_ply(with_n, m["vertices"], m["faces"], m["grey"], normals=m["normals"])
    fusion.write_mesh_ply(both, m["vertices"], m["faces"], m["grey"], colour, m["normals"])
    # a file without normals is what it was: the header and the rows of the writer as it stood before normals
    want = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar intensity\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % (len(m["vertices"]), len(m["faces"])))
    want += "".join("%.17g %.17g %.17g %d\n" % (x, y, z, int(g)) for (x, y, z), g in zip(m["vertices"], m["grey"]))
    want += "".join("3 %d %d %d\n" % (a, b, c) for a, b, c in m["faces"])
    assert open(plain).read() == want
    head = open(both).read().split("end_header")[0].splitlines()
    props = [ln for ln in head if ln.startswith("property") and "list" not in ln]
    assert props[-3:] == ["property float nx", "property float ny", "property float nz"] and props[-4] == "property uchar blue"
    v, f, g, n = fusion.read_mesh_ply(with_n, normals=True)
    assert np.array_equal(_bits(v), _bits(m["vertices"])) and np.array_equal(f, m["faces"]) and np.array_equal(g, m["grey"])
    assert n.dtype == np.float32 and np.array_equal(_bits(n), _bits(m["normals"]))
    v, f, g, c, n = fusion.read_mesh_ply(both, colour=True, normals=True)
    assert np.array_equal(c, colour) and np.array_equal(_bits(n), _bits(m["normals"])) and np.array_equal(_bits(v), _bits(m["vertices"]))
    assert len(fusion.read_mesh_ply(both)) == 3 and len(fusion.read_mesh_ply(with_n)) == 3
    with pytest.raises(ValueError):
        fusion.read_mesh_ply(plain, normals=True)


def test_header_prototypes_and_exports_agree(pkg):
    from ekf_monoslam_amd import capi, fusion
    lib = pkg.load_library()
    names = [n for n in pkg.declared_symbols() if n.startswith("ekf_mesh_")]
    assert sorted(names) == sorted(n for n in capi._PROTOS if n.startswith("ekf_mesh_")) == sorted(NAMES)
    for n in names:
        assert hasattr(lib, n), n
    assert [len(capi._PROTOS[n][1]) for n in NAMES] == [5, 9, 3] and lib.ekf_abi_version() == 6
    assert fusion.MESH_KERNELS == ("k_mesh_cells", "k_mesh_edges", "k_tsdf_scan", "k_mesh_vertices", "k_mesh_faces")
    assert hasattr(pkg, "IndexedMesh") and all(hasattr(fusion.TsdfVolume, n) for n in ("weld", "get_mesh_profile"))
    assert list(fusion.IndexedMesh.__dataclass_fields__) == ["vertices", "faces", "grey", "colour", "normals", "key"]
    sig = inspect.signature(fusion.TsdfVolume.weld).parameters
    assert sig["min_count"].default == 1 and sig["normals"].default is False
    for fn in (fusion.mesh_from_recording, fusion.audit_recording):
        sig = inspect.signature(fn).parameters
        assert sig["weld"].default == "host" and sig["normals"].default is False
        with pytest.raises(ValueError):
            fn("nowhere", weld="gpu")
    # the normals of a recording's mesh ride beside the dataclass fields (tests/test_oracle_colour.py keeps `colour` the last one)
    assert fusion.RecordingMesh.normals is None and "normals" not in fusion.RecordingMesh.__dataclass_fields__
    assert inspect.signature(fusion.write_mesh_ply).parameters["normals"].default is None
    assert inspect.signature(fusion.read_mesh_ply).parameters["normals"].default is False


def test_null_handle_calls_need_no_device(pkg):
    lib = pkg.load_library()
    nv, nt = C.c_ulonglong(5), C.c_ulonglong(5)
    assert lib.ekf_mesh_weld(None, 1, 0, C.byref(nv), C.byref(nt)) == 1 and (nv.value, nt.value) == (5, 5)
    assert lib.ekf_mesh_get(None, None, None, None, None, None, None, 0, 0) == 1
    assert lib.ekf_mesh_get_profile(None, None, None) == 1
