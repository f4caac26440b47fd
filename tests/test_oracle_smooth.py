"""The smoothing contract of the welded or pruned mesh on the CPU: the two restatements of
tests/smooth_oracle.py against each other bit for bit, the adjacency figures of the named cases, the consequences the
contract states, the effect of the scheme on the oracle alone, and the presence of the interface.  CPU only."""
import os
import re

import numpy as np
import pytest

import component_scene as cs
import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import mesh_scene as ms
import smooth_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ekf_smooth_run", "ekf_smooth_get", "ekf_smooth_get_adjacency", "ekf_smooth_get_profile")

# (case, min_count) -> (vertices, triangles, boundary vertices)
FIGURES = {("2x2x2", 1): (9, 8, 8), ("257x2x2", 1): (913, 964, 746), ("16x16x3", 2): (704, 970, 422), ("main", 1): (183, 272, 90),
           ("main", 2): (88, 120, 52), ("41x41x41", 1): (7685, 13536, 2013), ("41x41x41", 2): (5099, 7154, 2978),
           ("tie", 1): (1020, 1792, 240), ("sheet", 1): (66049, 131072, 1024), ("sphere", 1): (1298, 2592, 0)}


def _meshes():
    """(name, mesh) of every case of tests/component_scene.py, of the 24 random volumes of tests/mesh_scene.py and of the two
    hand-made face lists."""
    for name in cs.NAMES:
        for mc in cs.cases()[name][5]:
            yield "%s min_count %d" % (name, mc), cs.oracle_mesh(name, mc)
    for dims, seed, mc in ms.random_cases():
        vol = ms.random_volume(dims, seed)
        _, soup_key, _, _ = fo.extract(vol[:3], dims, fs.ORIGIN, ms.VOXEL, mc)
        yield "random %s seed %d" % (ms.shape_id(dims), seed), mo.weld(vol, dims, fs.ORIGIN, ms.VOXEL, soup_key, mc)
    yield "fan of 40", so.fan_mesh()
    yield "three on an edge", so.three_on_an_edge_mesh()


MESHES = list(_meshes())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name,mesh", MESHES, ids=[n for n, _ in MESHES])
def test_the_two_restatements_agree_and_the_contract_s_consequences_hold(name, mesh):
    faces, X = np.asarray(mesh["faces"], np.int64).reshape(-1, 3), mesh["vertices"]
    nv = len(X)
    a, b = so.adjacency(faces, nv), so.adjacency_loop(faces, nv)
    assert a.inc.dtype == np.uint32 and a.deg.dtype == np.uint32 and a.boundary.dtype == np.uint8
    assert all(_same(getattr(a, k), getattr(b, k)) for k in so.Adjacency._fields)
    assert int(a.inc.astype(np.int64).sum()) == 3 * len(faces)
    assert nv == 0 or (a.deg.min() >= 2 and a.inc.min() >= 1)
    for v in range(0, nv, max(1, nv // 50)):                          # the lists ascend and hold no v
        t, n = a.tri[a.tri_first[v]:a.tri_first[v + 1]], a.nbr[a.nbr_first[v]:a.nbr_first[v + 1]]
        assert np.all(np.diff(t) > 0) and np.all(np.diff(n) > 0) and v not in n and np.all((faces[t] == v).sum(axis=1) == 1)
    # the sheet's loop costs seconds a step: one round of one kind there, three rounds of three kinds elsewhere
    rounds = 1 if nv > 20000 else 3
    for pin, mu in (((True, so.MU),) if nv > 20000 else ((False, so.MU), (True, so.MU), (False, 0.0))):
        fast = so.smooth(mesh, rounds, so.LAM, mu, pin, normals=True)
        slow = so.smooth(mesh, rounds, so.LAM, mu, pin, normals=True, loop=True)
        assert _same(fast["vertices"], slow["vertices"]) and _same(fast["normals"], slow["normals"]), (pin, mu)
        assert fast["normals"].dtype == np.float32 and fast["normals"].shape == (nv, 3)
        assert all(fast[k] is mesh[k] for k in ("faces", "key", "grey", "colour"))
        if pin:
            keep = a.boundary != 0
            assert _same(fast["vertices"][keep], X[keep])              # pinned vertices keep their bits
            assert nv == 0 or keep.all() or not _same(fast["vertices"][~keep], X[~keep])
    assert so.smooth(mesh, 1)["normals"] is None


def test_the_adjacency_figures_of_the_named_cases():
    for (name, mc), want in FIGURES.items():
        m = cs.oracle_mesh(name, mc)
        a = so.adjacency(m["faces"], len(m["key"]))
        assert (len(m["key"]), len(m["faces"]), int(a.boundary.sum())) == want, (name, mc)
        assert int(a.mult.max()) == 2                                 # no edge lies in more than two triangles
        assert int(a.inc.max()) <= 9 and int(a.deg.max()) <= 9
    assert max(int(so.adjacency(cs.oracle_mesh(n, mc)["faces"], len(cs.oracle_mesh(n, mc)["key"])).inc.max()) for n, mc in FIGURES) == 9


def test_the_hand_made_face_lists():
    fan = so.fan_mesh()
    a = so.adjacency(fan["faces"], 41)
    assert a.inc[0] == 40 and a.deg[0] == 40 and a.boundary[0] == 0 and set(a.inc[1:].tolist()) == {2} and set(a.deg[1:].tolist()) == {3}
    assert a.boundary[1:].all() and np.array_equal(a.tri[:40], np.arange(40)) and np.array_equal(a.nbr[:40], np.arange(1, 41))
    edge = so.three_on_an_edge_mesh()
    a = so.adjacency(edge["faces"], 5)
    assert a.inc.tolist() == [3, 3, 1, 1, 1] and a.deg.tolist() == [4, 4, 2, 2, 2]
    assert a.mult[:4].tolist() == [3, 1, 1, 1] and a.boundary.tolist() == [1, 1, 1, 1, 1]
    # the edge (0, 1) itself marks no boundary: with the three outer edges of vertex 0 doubled, vertex 0 is interior
    closed = np.concatenate([edge["faces"], [[0, 2, 3], [0, 3, 4], [0, 4, 2]]])
    a = so.adjacency(closed, 5)
    assert a.mult[:4].tolist() == [3, 3, 3, 3] and a.boundary[0] == 0 and a.boundary[1] == 1


def test_runs_compose_and_mu_0_is_single_steps():
    for name, mc in (("main", 1), ("sphere", 1), ("16x16x3", 2)):
        m = cs.oracle_mesh(name, mc)
        a = so.adjacency(m["faces"], len(m["key"]))
        for pin in (False, True):
            three = so.smooth(m, 3, pin_boundary=pin)
            five = so.smooth(dict(m, vertices=three["vertices"]), 2, pin_boundary=pin)
            assert _same(five["vertices"], so.smooth(m, 5, pin_boundary=pin)["vertices"])
        X = m["vertices"]
        for _ in range(4):
            X = so.step(X, a, 0.5)
        assert _same(so.smooth(m, 4, 0.5, 0.0)["vertices"], X)
        assert _same(so.smooth(m, 1)["vertices"], so.step(so.step(m["vertices"], a, so.LAM), a, so.MU))
    sphere = cs.oracle_mesh("sphere", 1)
    assert _same(so.smooth(sphere, 2, pin_boundary=True)["vertices"], so.smooth(sphere, 2)["vertices"])    # no boundary to pin
    empty = dict(vertices=np.zeros((0, 3)), faces=np.zeros((0, 3), np.int64), grey=np.zeros(0, np.uint8), colour=None, normals=None,
                 key=np.zeros(0, np.uint64))
    out = so.smooth(empty, 3, normals=True)
    assert out["vertices"].shape == (0, 3) and out["normals"].shape == (0, 3) and out["normals"].dtype == np.float32


def test_the_effect_of_the_scheme_on_the_oracle():
    """Conditions on the oracle alone: the roughness at least halves, Taubin's scheme keeps the sphere's radius and plain
    Laplacian smoothing does not, and the smoothed sphere's own normals are radial."""
    for name, mc in (("sphere", 1), ("main", 1), ("41x41x41", 1)):
        m = cs.oracle_mesh(name, mc)
        a = so.adjacency(m["faces"], len(m["key"]))
        before, after = so.roughness(m["vertices"], a), so.roughness(so.smooth(m)["vertices"], a)
        print("%s: roughness %.4f -> %.4f, ratio %.3f" % (name, before, after, after / before))
        assert after < 0.5 * before
    m = cs.oracle_mesh("sphere", 1)
    a = so.adjacency(m["faces"], len(m["key"]))
    radius = lambda X: float(np.sqrt((X * X).sum(axis=1)).mean())
    taubin, laplace = so.smooth(m, normals=True), so.smooth(m, mu=0.0)
    r0, r1, r2 = radius(m["vertices"]), radius(taubin["vertices"]), radius(laplace["vertices"])
    cos = (taubin["normals"].astype(np.float64) * ms.sphere_radial(taubin["vertices"])).sum(axis=1)
    raw = so.normals(m["vertices"], m["faces"], a)
    print("sphere: radius %.4f, Taubin %+.3f %%, Laplace %+.3f %%, least cosine %.4f, %d zero normals unsmoothed"
          % (r0, 100 * (r1 / r0 - 1), 100 * (r2 / r0 - 1), cos.min(), int((~raw.any(axis=1)).sum())))
    assert abs(r1 / r0 - 1) < 0.005 and r2 / r0 - 1 < -0.02
    assert cos.min() > 0.99
    assert (~raw.any(axis=1)).any()                                   # the zero branch is real: u == 0 makes zero-area triangles
    assert np.all(np.abs(np.sqrt((taubin["normals"].astype(np.float64) ** 2).sum(axis=1)) - 1) < 1e-6)


def test_the_interface_is_there():
    """The header, _PROTOS and the exports, and EKF_ERR_ARG for a NULL handle.  Fails on the parent."""
    import inspect
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi, fusion
    header = open(os.path.join(ROOT, "include", "ekf_monoslam.h")).read()
    for fn in FUNCTIONS:
        assert re.search(r"^int %s\(" % fn, header, flags=re.M) and fn in capi._PROTOS
    assert "mu < -lambda" in header
    csrc = open(os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "csrc", "ekf_mesh_smooth.hpp")).read()
    assert "arrival order costs no bit" in csrc
    assert hasattr(pkg, "MeshAdjacency") and all(hasattr(fusion.TsdfVolume, n) for n in ("smooth", "adjacency", "get_smooth_profile"))
    assert list(fusion.MeshAdjacency.__dataclass_fields__) == ["inc", "deg", "boundary"]
    assert fusion.SMOOTH_KERNELS == ("k_smooth_count", "k_smooth_offsets", "k_tsdf_scan", "k_smooth_fill", "k_smooth_lists",
                                     "k_smooth_step", "k_smooth_normals")
    p = inspect.signature(fusion.TsdfVolume.smooth).parameters
    assert [(k, p[k].default) for k in list(p)[1:]] == [("iterations", 10), ("lam", 0.5), ("mu", -0.53), ("pin_boundary", False),
                                                        ("normals", False), ("source", "weld")]
    for fn in (fusion.mesh_from_recording, fusion.audit_recording):
        assert inspect.signature(fn).parameters["smooth"].default is None
    for bad in (0, -1, True, 2.5, "ten", {"rounds": 3}):
        with pytest.raises(ValueError):
            fusion._smooth_kwargs(bad)
    assert fusion._smooth_kwargs(None) is None and fusion._smooth_kwargs(3) == {"iterations": 3}
    hpp = open(os.path.join(ROOT, "include", "vslam_filter_hip.hpp")).read()
    assert all(n in hpp for n in ("IndexedMesh smooth(", "IndexedMesh smoothed()", "Adjacency adjacency()", "getSmoothProfile"))
    lib = pkg.load_library()
    assert lib.ekf_abi_version() == 6
    assert lib.ekf_smooth_run(None, 0, 1, 0.5, -0.53, 0, 0, None, None) == 1
    assert lib.ekf_smooth_get(None, None, None, None, None, None, None, 0, 0) == 1
    assert lib.ekf_smooth_get_adjacency(None, None, None, None, 0) == 1 and lib.ekf_smooth_get_profile(None, None, None) == 1
