"""The TSDF fusion contract on the numpy oracle alone, and what of the library can be checked without a
device: the ABI table, the argument errors, every class of voxel on the GPU test shapes, order independence, the
extraction on an analytic sphere (winding, closedness, vertices on their edges, exact welding), the accuracy condition and
the PLY round trip.  CPU only."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fusion_oracle as fo
import fusion_scene as fs


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


@pytest.fixture(scope="module")
def sphere():
    vol = fs.sphere_volume()
    xyz, key, grey, u = fo.extract(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    return dict(vol=vol, xyz=xyz, key=key, grey=grey, u=u)


def test_header_prototypes_and_exports_agree(pkg):
    from ekf_monoslam_amd import capi
    lib = pkg.load_library()
    names = [n for n in pkg.declared_symbols() if n.startswith("ekf_fusion_")]
    assert sorted(names) == sorted(n for n in capi._PROTOS if n.startswith("ekf_fusion_")) and len(names) == 12
    for n in names:
        assert hasattr(lib, n), n
    for n in ("ekf_fusion_create", "ekf_fusion_integrate", "ekf_fusion_integrate_host", "ekf_fusion_extract", "ekf_fusion_get_mesh",
              "ekf_fusion_set_volume"):
        assert n in names
    assert lib.ekf_abi_version() == 6
    assert all(hasattr(pkg, n) for n in ("TsdfVolume", "Mesh", "weld", "write_mesh_ply", "read_mesh_ply", "mesh_from_recording"))


def test_argument_errors_need_no_device(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    o = np.zeros(3)
    h = C.c_void_p()
    create = lambda nx=4, ny=4, nz=4, origin=o, voxel=0.1, trunc=0.4: lib.ekf_fusion_create(
        nx, ny, nz, None if origin is None else P(origin), voxel, trunc, 0, C.byref(h))
    for bad in (dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=1025), dict(ny=1025), dict(nz=1025), dict(nx=1024, ny=1024, nz=257),
                dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=np.nan), dict(voxel=np.inf), dict(trunc=0.0), dict(trunc=np.nan),
                dict(trunc=np.inf), dict(origin=None), dict(origin=np.array([0.0, np.nan, 0.0])), dict(origin=np.array([np.inf, 0, 0]))):
        assert create(**bad) == 1 and not h, bad
        assert b"ekf_fusion_create" in lib.ekf_fusion_last_error(None)
    assert lib.ekf_fusion_create(4, 4, 4, P(o), 0.1, 0.4, 0, None) == 1
    # a NULL handle is an argument error everywhere
    n = C.c_ulonglong(0)
    assert lib.ekf_fusion_integrate(None, None, 0, 0) == 1 and lib.ekf_fusion_integrate_host(None, None, None, 0, 0, 0, None, None) == 1
    assert lib.ekf_fusion_reset(None) == 1 and lib.ekf_fusion_get_volume(None, None, None, None, None) == 1
    assert lib.ekf_fusion_set_volume(None, None, None, None, -1) == 1 and lib.ekf_fusion_extract(None, 1, C.byref(n)) == 1
    assert lib.ekf_fusion_get_mesh(None, None, None, None, 0) == 1 and lib.ekf_fusion_profile(None, 1) == 1
    assert lib.ekf_fusion_get_profile(None, None, None) == 1
    lib.ekf_fusion_destroy(None)
    with pytest.raises(pkg.EkfError) as ei:
        pkg.TsdfVolume((1, 4, 4), o, 0.1, 0.4)
    assert ei.value.status == 1


def test_every_class_of_voxel_occurs_in_the_gpu_shapes():
    steps, classes = fs.fused()
    for n, cls in enumerate(classes):
        counts = [int((cls == c).sum()) for c in range(6)]
        print("map", n, dict(zip(fo.CLASS_NAMES, counts)))
        assert sum(counts) == cls.size == 2717 and all(c > 0 for c in counts), counts
    s_, c_, g_ = steps[-1]
    touched = sum(int(((cls == fo.FREE) | (cls == fo.NEAR)).sum()) for cls in classes)
    assert int(c_.sum()) == touched and int(c_.max()) == 3 and int((c_ == 0).sum()) > 0
    assert np.all(np.abs(s_) <= c_) and (s_ < 0).any() and (s_ > 0).any()


def test_integration_order_does_not_matter():
    maps = fs.synthetic_maps()[:2]
    (a, _), (b, _) = fs.fused(maps=maps, order=(0, 1)), fs.fused(maps=maps, order=(1, 0))
    sa, ca, ga = a[-1]
    sb, cb, gb = b[-1]
    assert np.array_equal(ca, cb) and np.array_equal(ga, gb) and int((ca == 2).sum()) > 0
    once = ca <= 1
    assert np.array_equal(sa[once].view(np.uint32), sb[once].view(np.uint32))
    assert np.allclose(sa, sb, rtol=0, atol=2 ** -23)                # two fp32 terms of at most 1: one rounding apart


def test_table_satisfies_the_winding_rule():
    """Every triangle of TET_TRIS, in every tetrahedron, for values in general position: ((B - A) x (C - A)) . (P_out - P_in) > 0."""
    rng = np.random.default_rng(5)
    corner = lambda c: np.array([c & 1, (c >> 1) & 1, c >> 2], np.float64)
    checked = 0
    for tet in fo.TETS:
        P = [corner(c) for c in tet]
        assert np.linalg.det(np.array([P[1] - P[0], P[2] - P[0], P[3] - P[0]])) > 0          # all of one orientation
        for mask in range(16):
            ins = [i for i in range(4) if mask >> i & 1]
            outs = [i for i in range(4) if not mask >> i & 1]
            assert len(fo.TET_TRIS[mask]) == (0 if len(ins) in (0, 4) else 2 if len(ins) == 2 else 1)
            for _ in range(4):
                v = rng.uniform(0.1, 1.0, 4) * np.where([i in ins for i in range(4)], -1.0, 1.0)
                for tri in fo.TET_TRIS[mask]:
                    pts = []
                    for e in tri:
                        a, b = fo.TET_EDGES[e]
                        assert (v[a] < 0) != (v[b] < 0)                                          # an edge the surface crosses
                        pts.append(P[a] + v[a] / (v[a] - v[b]) * (P[b] - P[a]))
                    nrm = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                    for i, o in itertools.product(ins, outs):
                        assert nrm @ (P[o] - P[i]) > 0, (tet, mask, tri)
                    checked += 1
    assert checked == 6 * 4 * (8 + 6 * 2)


def test_sphere_mesh_is_closed_and_consistently_oriented(sphere):
    s_ = sphere["vol"][0]
    assert int((s_ == 0).sum()) == 30                                 # the lattice points exactly on the sphere: outside
    key, xyz = sphere["key"], sphere["xyz"]
    first, faces = fo.weld(key)
    assert len(faces) == len(xyz) > 1000
    edges = {}
    for f in faces:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            assert a != b
            edges[(a, b)] = edges.get((a, b), 0) + 1
    assert all(n == 1 for n in edges.values())                        # no directed edge twice
    assert all((b, a) in edges for (a, b) in edges)                   # every edge once in each direction: closed, oriented
    assert len(first) - len(edges) // 2 + len(faces) == 2             # Euler: a sphere
    # the normals point away from the centre wherever the triangle is not degenerate
    nrm = np.cross(xyz[:, 1] - xyz[:, 0], xyz[:, 2] - xyz[:, 0])
    big = np.linalg.norm(nrm, axis=1) > 1e-9
    assert big.sum() > 0.9 * len(xyz) and (~big).any()
    assert np.all((nrm[big] * xyz[big].mean(axis=1)).sum(axis=1) > 0)


def test_sphere_vertices_lie_on_their_edges_and_equal_keys_are_bit_equal(sphere):
    xyz, key, grey, u = (sphere[k] for k in ("xyz", "key", "grey", "u"))
    assert np.all((u >= 0.0) & (u <= 1.0)) and (u == 0.0).any()
    nx, ny, nz = fs.SPHERE_DIMS
    lin, code = (key >> np.uint64(3)).astype(np.int64), (key & np.uint64(7)).astype(np.int64)
    assert code.min() >= 1
    ia = np.stack([lin % nx, (lin // nx) % ny, lin // (nx * ny)], axis=-1)
    ib = ia + np.stack([code & 1, (code >> 1) & 1, code >> 2], axis=-1)
    Pa, Pb = fs.SPHERE_ORIGIN + ia * fs.SPHERE_VOXEL, fs.SPHERE_ORIGIN + ib * fs.SPHERE_VOXEL
    assert np.all(ib < np.array([nx, ny, nz]))
    assert np.array_equal(xyz, Pa + u[..., None] * (Pb - Pa))
    assert np.all(xyz >= np.minimum(Pa, Pb)) and np.all(xyz <= np.maximum(Pa, Pb))
    r = np.linalg.norm(xyz.reshape(-1, 3), axis=1)
    print("sphere: radius of the vertices", r.min(), "..", r.max())
    assert np.abs(r - fs.SPHERE_RADIUS).max() < 0.1 * fs.SPHERE_VOXEL
    flat_k, flat_x, flat_g = key.reshape(-1), xyz.reshape(-1, 3).view(np.uint64), grey.reshape(-1)
    order = np.argsort(flat_k, kind="stable")
    same = flat_k[order][1:] == flat_k[order][:-1]
    assert same.sum() > 1000
    assert np.array_equal(flat_x[order][1:][same], flat_x[order][:-1][same]) and np.array_equal(flat_g[order][1:][same], flat_g[order][:-1][same])


def test_min_count_and_an_empty_volume_give_no_triangles():
    steps, _ = fs.fused()
    assert len(fo.extract(steps[-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, 1)[0]) > len(fo.extract(steps[-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, 2)[0]) > 0
    assert len(fo.extract(steps[-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, 4)[0]) == 0
    assert len(fo.extract(fo.empty_volume(fs.DIMS), fs.DIMS, fs.ORIGIN, fs.VOXEL, 1)[0]) == 0


def test_accuracy_condition():
    """At least 90 % of the welded vertices that lie trunc inside the common field of view of the three true depth maps of
    the plane scene are within one voxel of the plane (the oracle's share: 100 %, the largest distance 0.005 voxels)."""
    vol = fo.empty_volume(fs.ACC_DIMS)
    for m in fs.accuracy_maps():
        fo.integrate(vol, fs.ACC_DIMS, fs.ACC_ORIGIN, fs.ACC_VOXEL, fs.ACC_TRUNC, *m)
    xyz, key, _, _ = fo.extract(vol, fs.ACC_DIMS, fs.ACC_ORIGIN, fs.ACC_VOXEL, 1)
    first, _ = fo.weld(key)
    V = xyz.reshape(-1, 3)[first]
    inside = fs.in_common_view(V, fs.ACC_TRUNC)
    err = np.abs(V[inside, 2] - fs.ACC_Z)
    share = float((err <= fs.ACC_VOXEL).mean())
    print("vertices", len(V), "counted", int(inside.sum()), "share within one voxel", share, "largest distance / voxel", err.max() / fs.ACC_VOXEL)
    assert fs.ACC_VOXEL >= 2 * fs.ACC_Z / 64.0 and inside.sum() >= 100 and share >= 0.90


def test_mesh_ply_round_trip(pkg, sphere, tmp_path):
    mesh = pkg.Mesh(sphere["xyz"], sphere["key"], sphere["grey"])
    vertices, faces, grey = pkg.weld(mesh)
    first, want_faces = fo.weld(sphere["key"])
    assert np.array_equal(vertices.view(np.uint64), sphere["xyz"].reshape(-1, 3)[first].view(np.uint64))
    assert np.array_equal(faces, want_faces) and np.array_equal(grey, sphere["grey"].reshape(-1)[first])
    path = str(tmp_path / "sphere.ply")
    pkg.write_mesh_ply(path, vertices, faces, grey)
    v2, f2, g2 = pkg.read_mesh_ply(path)
    assert np.array_equal(v2.view(np.uint64), vertices.view(np.uint64)) and np.array_equal(f2, faces) and np.array_equal(g2, grey)
    head = open(path).read().split("end_header")[0]
    assert "property double x" in head and "property uchar intensity" in head and "property list uchar int vertex_indices" in head


def test_auto_grid_of_the_binding_equals_the_oracle(pkg):
    from ekf_monoslam_amd import fusion
    pts = [np.array([[[0.1, -0.2, 1.0], [np.nan, np.nan, np.nan]], [[0.9, 0.3, 1.4], [0.5, 0.0, 1.1]]])]
    for kw in (dict(), dict(voxel=0.05), dict(trunc=0.07), dict(bounds=([0, 0, 0], [1, 0.5, 0.25])), dict(voxel=0.02, bounds=([0, 0, 0], [1, 1, 1]))):
        a, b = fusion.auto_grid(pts, **kw), fo.auto_grid(pts, **kw)
        assert np.array_equal(a[0], b[0]) and tuple(a[1]) == tuple(int(v) for v in b[1]) and a[2:] == b[2:], kw
    o, dims, vx, tr = fusion.auto_grid(pts)
    assert vx == 0.8 / 128 and tr == 4 * vx and dims[0] == 128 + 8 + 1
    with pytest.raises(ValueError):
        fusion.auto_grid(pts, voxel=1e-4, bounds=([0, 0, 0], [1, 1, 1]))
