"""The component contract of the welded mesh on the CPU: the two implementations of
tests/component_oracle.py against each other, the consequences the contract states, and the presence of the interface.
CPU only."""
import os
import re

import numpy as np
import pytest

import component_oracle as co
import component_scene as cs
import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import mesh_scene as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("vertices", "grey", "colour", "normals", "key")
FUNCTIONS = ("ekf_components_find", "ekf_components_get", "ekf_components_prune", "ekf_components_get_pruned", "ekf_components_get_profile")


def _meshes():
    """(name, mesh) of every case of tests/component_scene.py and of the 24 random volumes of tests/mesh_scene.py."""
    for name in cs.NAMES:
        for mc in cs.cases()[name][5]:
            yield "%s min_count %d" % (name, mc), cs.oracle_mesh(name, mc)
    for dims, seed, mc in ms.random_cases():
        vol = ms.random_volume(dims, seed)
        _, soup_key, _, _ = fo.extract(vol[:3], dims, fs.ORIGIN, ms.VOXEL, mc)
        yield "random %s seed %d" % (ms.shape_id(dims), seed), mo.weld(vol, dims, fs.ORIGIN, ms.VOXEL, soup_key, mc)


MESHES = list(_meshes())


def _equal(a, b):
    return all((a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])) for k in ROWS) and \
        np.array_equal(a["faces"], b["faces"])


@pytest.mark.parametrize("name,mesh", MESHES, ids=[n for n, _ in MESHES])
def test_the_two_oracles_agree_and_the_contract_s_consequences_hold(name, mesh):
    faces, nv = np.asarray(mesh["faces"], np.int64), len(mesh["key"])
    label, size, count = co.components_union_find(faces, nv)
    label2, size2, count2 = co.components_flood(faces, nv)
    assert label.dtype == np.uint32 and size.dtype == np.uint32
    assert np.array_equal(label, label2) and np.array_equal(size, size2) and count == count2
    # every vertex lies in a triangle; a label is the least index of its component; a triangle's vertices share a component
    assert nv == 0 or np.array_equal(np.unique(faces), np.arange(nv))
    roots = np.unique(label)
    assert len(roots) == count and np.array_equal(label[roots], roots) and np.all(label <= np.arange(nv))
    assert all(int(np.nonzero(label == r)[0][0]) == int(r) for r in roots)
    assert len(faces) == 0 or (np.all(label[faces[:, 0]] == label[faces[:, 1]]) and np.all(label[faces[:, 0]] == label[faces[:, 2]]))
    assert int(size[roots].astype(np.int64).sum()) == len(faces)                     # the sizes add up to n_tri
    top = int(size.max()) if nv else 0
    for t in cs.THRESHOLDS + (top + 1,):
        for largest in (False, True):
            p = co.prune(mesh, t, largest)
            assert len(p["faces"]) == 0 or (p["faces"].min() >= 0 and p["faces"].max() < len(p["key"]))
            assert np.all(np.diff(p["key"].astype(np.int64)) > 0)                    # the keys stay ascending
            assert _equal(co.prune(p, t, largest), p)                                # idempotent
            assert np.array_equal(p["vertices"][p["faces"]], mesh["vertices"][faces[co.kept_vertices(label, size, t, largest)[faces[:, 0]]]]
                                  if len(faces) else p["vertices"][p["faces"]])      # the kept triangles, corner for corner
    assert _equal(co.prune(mesh, 1), {**mesh, "faces": faces})                       # the identity
    empty = co.prune(mesh, top + 1)
    assert len(empty["key"]) == 0 and empty["faces"].shape == (0, 3) and empty["components"] == 0
    if count:
        one = co.prune(mesh, 1, True)
        assert one["components"] == 1 and len(one["faces"]) == top


def test_the_sizes_of_the_named_cases():
    want = {("main", 1): [2, 8, 262], ("main", 2): [6, 114]}
    for (name, mc), sizes in want.items():
        m = cs.oracle_mesh(name, mc)
        label, size, _ = co.components(m["faces"], len(m["key"]))
        assert sorted(cs.sizes(size, label)) == sizes
    for name, mc, n, lo, hi in (("257x2x2", 1, 58, 2, 50), ("16x16x3", 2, 11, 2, 748), ("41x41x41", 1, 6, 2, 13500), ("41x41x41", 2, 46, 2, 5646)):
        m = cs.oracle_mesh(name, mc)
        label, size, count = co.components(m["faces"], len(m["key"]))
        assert (count, int(size.min()), int(size.max())) == (n, lo, hi)
    m = cs.oracle_mesh("sheet", 1)
    label, size, count = co.components(m["faces"], len(m["key"]))
    assert (len(m["key"]), len(m["faces"]), count) == (66049, 131072, 1) and (66049 + 255) // 256 == 259 and 66049 % 256 == 1
    assert co.components(np.zeros((0, 3), np.int64), 0)[2] == 0


def test_the_four_way_tie_keeps_the_least_label():
    m = cs.oracle_mesh("tie", 1)
    label, size, count = co.components(m["faces"], len(m["key"]))
    assert count == 4 and np.unique(label).tolist() == [0, 255, 510, 765] and set(size.tolist()) == {448}
    one = co.prune(m, 1, True)
    assert len(one["key"]) == 255 and len(one["faces"]) == 448 and np.array_equal(one["key"], m["key"][:255])
    assert len(co.prune(m, 448)["faces"]) == 1792 and len(co.prune(m, 449)["faces"]) == 0


def test_vertices_of_equal_coordinates_are_distinct():
    """Linking is by index: two triangles that meet in a point through two vertices of equal coordinates are two components."""
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    mesh = dict(vertices=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [-1, 0, 0], [0, -1, 0]], np.float64), faces=faces,
                grey=np.zeros(6, np.uint8), colour=None, normals=None, key=np.arange(6, dtype=np.uint64))
    label, size, count = co.components(faces, 6)
    assert count == 2 and label.tolist() == [0, 0, 0, 3, 3, 3] and size.tolist() == [1] * 6
    assert co.prune(mesh, 1, True)["key"].tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        co.prune(mesh, 0)


def test_the_interface_is_there():
    """The header, _PROTOS and the exports, and EKF_ERR_ARG for a NULL handle.  Fails on the parent."""
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi, fusion
    header = open(os.path.join(ROOT, "include", "ekf_monoslam.h")).read()
    for fn in FUNCTIONS:
        assert re.search(r"^int %s\(" % fn, header, flags=re.M) and fn in capi._PROTOS
    assert "by index, not by coordinate" in header and "by index, not by coordinate" in open(
        os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "csrc", "ekf_mesh_components.hpp")).read()
    assert hasattr(pkg, "MeshComponents") and all(hasattr(fusion.TsdfVolume, n) for n in ("components", "prune", "get_component_profile"))
    assert list(fusion.MeshComponents.__dataclass_fields__) == ["label", "size", "count"]
    assert fusion.COMPONENT_KERNELS == ("k_comp_init", "k_comp_union", "k_comp_count", "k_comp_largest", "k_comp_flags", "k_tsdf_scan",
                                        "k_comp_vertices", "k_comp_faces")
    import inspect
    for fn in (fusion.mesh_from_recording, fusion.audit_recording):
        assert inspect.signature(fn).parameters["components"].default is None
    hpp = open(os.path.join(ROOT, "include", "vslam_filter_hip.hpp")).read()
    assert all(n in hpp for n in ("Components components()", "IndexedMesh prune(", "IndexedMesh pruned()", "getComponentProfile"))
    lib = pkg.load_library()
    assert lib.ekf_abi_version() == 6
    assert lib.ekf_components_find(None, None) == 1 and lib.ekf_components_get(None, None, None, 0) == 1
    assert lib.ekf_components_prune(None, 1, 0, None, None, None) == 1 and lib.ekf_components_get_profile(None, None, None) == 1
    assert lib.ekf_components_get_pruned(None, None, None, None, None, None, None, 0, 0) == 1
