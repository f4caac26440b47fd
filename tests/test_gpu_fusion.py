"""TSDF fusion on the device against tests/fusion_oracle.py, bit for bit: the three planes of the 19 x 13 x 11
volume after each of three 37 x 19 maps with holes, a 2 x 2 x 2 volume, a map integrated straight from a dense slot, the
mesh of an injected analytic sphere and of the integrated volume (9 blocks of cells: the block offsets matter), repeated
runs, the empty cases, every error path with the earlier volume and mesh still readable, a living filter left untouched,
and end to end from a recording to a welded mesh and a PLY file."""
import ctypes as C
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import dense_oracle as do
import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs
import keyframe_gpu_common as kg
import keyframe_scene as ks
import rectify_scene as rs

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    """Equal bit for bit (NaNs at equal positions with equal payload included)."""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got) if got.dtype.kind == "f" else got,
                                                                                  _bits(want) if want.dtype.kind == "f" else want)


def _same_volume(got, want):
    return _same(got["sum"], want[0]) and _same(got["cnt"], want[1]) and _same(got["gsum"], want[2])


def _same_mesh(mesh, want):
    return _same(mesh.xyz, want[0]) and _same(mesh.key, want[1]) and _same(mesh.grey, want[2])


def _main():
    """The oracle on the main shape, computed once: the planes after each map and the meshes of the last."""
    if "main" not in _CACHE:
        steps, _ = fs.fused()
        _CACHE["main"] = dict(maps=fs.synthetic_maps(), steps=steps,
                              mesh={mc: fo.extract(steps[-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, mc) for mc in (1, 2, 4)})
    return _CACHE["main"]


def _sphere():
    if "sphere" not in _CACHE:
        vol = fs.sphere_volume()
        _CACHE["sphere"] = dict(vol=vol, mesh=fo.extract(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1))
    return _CACHE["sphere"]


def _volume(pkg, maps=3):
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    for m in _main()["maps"][:maps]:
        v.integrate_host(*m)
    return v


def test_integration_equals_the_oracle_after_each_map(pkg):
    o = _main()
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    assert _same_volume(v.volume(), fo.empty_volume(fs.DIMS)) and v.volume()["maps"] == 0
    for n, m in enumerate(o["maps"]):
        v.integrate_host(*m)
        got = v.volume()
        for key, want in zip(("sum", "cnt", "gsum"), o["steps"][n]):
            print("map", n, key, "differing voxels:", int((_bits(got[key]) != _bits(want)).sum()) if key == "sum" else int((got[key] != want).sum()))
        assert _same_volume(got, o["steps"][n]) and got["maps"] == n + 1, n
    assert int(got["cnt"].max()) == 3 and int((got["cnt"] == 0).sum()) > 0
    # a fresh handle gives the same bytes, and an image with a pitch is the same image
    again = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    for depth, img, K, pose in o["maps"]:
        wide = np.full((img.shape[0], img.shape[1] + 5), 0xA5, np.uint8)
        wide[:, :img.shape[1]] = img
        d = np.ascontiguousarray(depth)
        rc = again._lib.ekf_fusion_integrate_host(again._h, d.ctypes.data_as(C.c_void_p), wide.ctypes.data_as(C.c_void_p), wide.strides[0],
                                                  img.shape[1], img.shape[0], K.ctypes.data_as(C.c_void_p),
                                                  np.ascontiguousarray(pose).ctypes.data_as(C.c_void_p))
        assert rc == 0
    b = again.volume()
    assert all(b[k].tobytes() == got[k].tobytes() for k in ("sum", "cnt", "gsum"))
    # reset clears the planes and the counter
    again.reset()
    assert _same_volume(again.volume(), fo.empty_volume(fs.DIMS)) and again.volume()["maps"] == 0
    again.close()
    v.close()


def test_tiny_volume_equals_the_oracle(pkg):
    maps = _main()["maps"]
    vol = fo.empty_volume(fs.TINY_DIMS)
    v = pkg.TsdfVolume(fs.TINY_DIMS, fs.TINY_ORIGIN, fs.VOXEL, fs.TRUNC)
    for m in maps:
        fo.integrate(vol, fs.TINY_DIMS, fs.TINY_ORIGIN, fs.VOXEL, fs.TRUNC, *m)
        v.integrate_host(*m)
    assert _same_volume(v.volume(), vol) and int(vol[1].sum()) > 0
    want = fo.extract(vol, fs.TINY_DIMS, fs.TINY_ORIGIN, fs.VOXEL, 1)
    assert _same_mesh(v.extract(1), want) and len(want[0]) > 0                   # one cell, one block
    v.close()


def test_integration_from_a_dense_slot_equals_the_host_path(pkg):
    case = [c for c in ds.CASES if (c[1], c[2]) == (ds.SMALL_W, ds.SMALL_H)][0]
    name, w, h, D, radius, trunc, src = case
    views = ds.case_views(w, h)
    slots = (0,) + tuple(src)
    d = pkg.DenseStereo(w, h, max_views=3)
    for s in slots:
        d.set_view(s, *views[s])
    for r in slots:
        d.sweep(r, [s for s in slots if s != r], ds.W_MIN, ds.W_MAX, D, radius, trunc)
    d.filter(0, src, 0.05, 2)
    origin, voxel, tr = np.array([-2.7, -1.8, 2.0]), 0.3, 0.6
    for slot, filtered, pose in ((0, True, None), (0, False, None), (1, False, views[1][2])):
        a, b = pkg.TsdfVolume(fs.DIMS, origin, voxel, tr), pkg.TsdfVolume(fs.DIMS, origin, voxel, tr)
        a.integrate(d, slot, filtered)
        img, K, p = d.view(slot)                                                  # (slot 1: the pose as it was set, not re-normalised)
        depth = d.depth(slot, filtered)["depth"]
        b.integrate_host(depth, img, K, p if pose is None else pose)
        va, vb = a.volume(), b.volume()
        vol = fo.empty_volume(fs.DIMS)
        fo.integrate(vol, fs.DIMS, origin, voxel, tr, depth, img, K, p if pose is None else pose)
        print("slot", slot, "filtered", filtered, "voxels updated:", int(va["cnt"].sum()))
        assert all(va[k].tobytes() == vb[k].tobytes() for k in ("sum", "cnt", "gsum")) and _same_volume(va, vol), (slot, filtered)
        assert int(va["cnt"].sum()) > 0 and va["maps"] == 1
        a.close()
        b.close()
    d.close()


def test_extraction_equals_the_oracle_on_the_sphere_and_on_the_integrated_volume(pkg):
    sp = _sphere()
    v = pkg.TsdfVolume(fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC)
    assert len(v.extract(1).xyz) == 0                                            # an empty volume: no triangles, success
    v.set_volume(*sp["vol"])
    got = v.volume()
    assert _same_volume(got, sp["vol"]) and got["maps"] == 1                     # round trip; the counter follows the counts
    mesh = v.extract(1)
    print("sphere triangles", len(mesh.xyz), "oracle", len(sp["mesh"][0]))
    assert len(mesh.xyz) == len(sp["mesh"][0]) > 1000 and _same_mesh(mesh, sp["mesh"])
    again = v.extract(1)
    assert all(getattr(again, k).tobytes() == getattr(mesh, k).tobytes() for k in ("xyz", "key", "grey"))
    assert len(v.extract(2).xyz) == 0                                            # min_count above every count
    v.close()
    o = _main()
    v = _volume(pkg)
    for mc in (1, 2, 4):
        mesh = v.extract(mc)
        print("main volume, min_count", mc, "triangles", len(mesh.xyz), "oracle", len(o["mesh"][mc][0]))
        assert _same_mesh(mesh, o["mesh"][mc]), mc
    assert len(o["mesh"][1][0]) > len(o["mesh"][2][0]) > 0 == len(o["mesh"][4][0])
    # the welded mesh of the binding is the oracle's
    vertices, faces, grey = pkg.weld(v.extract(1))
    first, want_faces = fo.weld(o["mesh"][1][1])
    assert _same(vertices, o["mesh"][1][0].reshape(-1, 3)[first]) and np.array_equal(faces, want_faces)
    assert np.array_equal(grey, o["mesh"][1][2].reshape(-1)[first])
    v.close()


def test_error_paths_leave_the_volume_and_the_mesh_readable(pkg):
    lib = pkg.load_library()
    P = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    o = _main()
    h = C.c_void_p()
    assert lib.ekf_fusion_create(4, 4, 4, P(np.zeros(3)), 0.1, 0.4, 99, C.byref(h)) == 3 and not h
    v = _volume(pkg)
    mesh = v.extract(1)
    depth, img, K, pose = o["maps"][0]
    depth, img = np.ascontiguousarray(depth), np.ascontiguousarray(img)
    W, H = depth.shape[1], depth.shape[0]
    host = lambda dp=depth, im=img, pitch=W, w=W, hh=H, k=K, ps=pose: lib.ekf_fusion_integrate_host(v._h, P(dp), P(im), pitch, w, hh, P(k), P(ps))
    assert host(dp=None) == 1 and host(im=None) == 1 and host(k=None) == 1 and host(ps=None) == 1
    assert host(w=0) == 1 and host(hh=0) == 1 and host(w=8193, pitch=8193) == 1 and host(hh=8193) == 1 and host(pitch=W - 1) == 1
    assert host(k=np.array([0.0, 24, 18, 9])) == 1 and host(k=np.array([24.0, np.nan, 18, 9])) == 1
    assert host(ps=np.zeros(7)) == 1 and host(ps=np.array([np.inf, 0, 0, 1, 0, 0, 0])) == 1
    # a dense handle: NULL, a slot out of range, a slot without the map
    d = pkg.DenseStereo(W, H, max_views=2)
    d.set_view(0, img, K, pose)
    d.set_view(1, img, K, [0.1, 0, 0, 1, 0, 0, 0])
    assert lib.ekf_fusion_integrate(v._h, None, 0, 0) == 1
    assert lib.ekf_fusion_integrate(v._h, d._h, 2, 0) == 1 and lib.ekf_fusion_integrate(v._h, d._h, 0, 2) == 1
    assert lib.ekf_fusion_integrate(v._h, d._h, 0, 0) == 4                       # never swept
    d.sweep(0, [1], 0.5, 3.0, 4, 1, 40)
    assert lib.ekf_fusion_integrate(v._h, d._h, 0, 1) == 4                       # swept, never filtered
    assert b"ekf_fusion_integrate" in lib.ekf_fusion_last_error(v._h)
    # extract and set_volume
    n = C.c_ulonglong(7)
    assert lib.ekf_fusion_extract(v._h, 0, C.byref(n)) == 1 and lib.ekf_fusion_extract(v._h, 65536, C.byref(n)) == 1
    assert lib.ekf_fusion_extract(v._h, 1, None) == 1 and n.value == 7
    assert lib.ekf_fusion_set_volume(v._h, None, None, None, -2) == 1 and lib.ekf_fusion_set_volume(v._h, None, None, None, 65536) == 1
    assert lib.ekf_fusion_get_profile(v._h, None, None) == 1
    # ... and the volume and the mesh are what they were
    assert _same_volume(v.volume(), o["steps"][-1]) and v.volume()["maps"] == 3
    keep = pkg.Mesh(np.zeros_like(mesh.xyz), np.zeros_like(mesh.key), np.zeros_like(mesh.grey))
    assert lib.ekf_fusion_get_mesh(v._h, P(keep.xyz), P(keep.key), P(keep.grey), len(keep.xyz)) == 0 and _same_mesh(keep, o["mesh"][1])
    part = np.zeros((5, 3), np.uint64)
    assert lib.ekf_fusion_get_mesh(v._h, None, P(part), None, 5) == 0 and np.array_equal(part, o["mesh"][1][1][:5])   # max_tri < n_tri
    # the 65536th map: the counter is part of set_volume's contract
    v.set_volume(maps=65535)
    assert lib.ekf_fusion_get_mesh(v._h, None, None, None, 0) == 4               # the volume (may have) changed since the extract
    assert host() == 2 and lib.ekf_fusion_integrate(v._h, d._h, 0, 0) == 2
    got = v.volume()
    assert _same_volume(got, o["steps"][-1]) and got["maps"] == 65535
    v.set_volume(maps=3)
    # get_mesh without a current extract
    fresh = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    assert lib.ekf_fusion_get_mesh(fresh._h, None, None, None, 0) == 4           # before any extract
    fresh.close()
    assert _same_mesh(v.extract(1), o["mesh"][1])
    assert host() == 0 and lib.ekf_fusion_get_mesh(v._h, None, None, None, 0) == 4      # after an integration
    v.extract(1)
    v.reset()
    assert lib.ekf_fusion_get_mesh(v._h, None, None, None, 0) == 4                       # after a reset
    # the profile: one timed launch of each kernel
    for m in o["maps"]:
        v.integrate_host(*m)
    v.profile(True)
    v.integrate_host(*o["maps"][0])
    v.extract(1)
    prof = v.get_profile()
    print("profile", prof)
    assert [prof[k][1] for k in ("k_tsdf_integrate", "k_tsdf_count", "k_tsdf_scan", "k_tsdf_emit")] == [1, 1, 1, 1] and prof["k_tsdf_integrate"][0] > 0
    v.profile(True)                                                 # a second profile(True) starts from zero
    assert set(v.get_profile().values()) == {(0.0, 0)}
    v.profile(False)
    v.integrate_host(*o["maps"][0])                                 # switched off, launches leave the counts where they were
    v.extract(1)
    assert set(v.get_profile().values()) == {(0.0, 0)}
    d.close()
    v.close()


def test_a_living_filter_is_untouched(pkg):
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=16, dtype=np.float32)
    for i in range(6):
        assert g.addFeature((40.0 + 50.0 * i, 60.0 + 30.0 * i)) == 1
    g.predict()
    g.synchronize()
    snap = lambda: (g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts())
    before = snap()
    v = _volume(pkg)
    assert _same_mesh(v.extract(1), _main()["mesh"][1])
    v.close()
    assert snap() == before
    g.close()


def test_wall_recording_to_a_mesh_and_a_ply_file(pkg, tmp_path):
    """Five synthetic key frames of a textured wall -> mesh_from_recording with automatic bounds, voxel and trunc, against the
    oracles driven from the same files."""
    from ekf_monoslam_amd import dense, keyframes
    rec = str(tmp_path / "wall")
    ids = fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
    t0 = time.perf_counter()
    kw = dict(fs.REC_SWEEP)
    cost_trunc = kw.pop("trunc")
    got = pkg.mesh_from_recording(rec, None, sweep_trunc=cost_trunc, **kw)
    t1 = time.perf_counter()
    kw["trunc_cost"] = cost_trunc
    V, F, G, origin, dims, vx, tr = fs.oracle_mesh_from_recording(dense.read_recording, dense.neighbours_of, rec, **kw)
    print("wall: vertices", len(V), "faces", len(F), "dims", dims, "voxel", vx, "device path %.2f s, oracle %.2f s" % (t1 - t0, time.perf_counter() - t1))
    assert [m.id for m in got.maps] == ids and got.dims == dims and (got.voxel, got.trunc) == (vx, tr) and np.array_equal(got.origin, origin)
    assert max(dims) == 128 + 8 + 1 and tr == 4 * vx
    assert len(F) > 1000 and _same(got.vertices, V) and np.array_equal(got.faces, F) and np.array_equal(got.grey, G)
    assert abs(float(np.median(V[:, 2])) - fs.REC_Z) < 0.05                      # the wall is where it was put
    path = str(tmp_path / "wall.ply")
    pkg.write_mesh_ply(path, got.vertices, got.faces, got.grey)
    v2, f2, g2 = pkg.read_mesh_ply(path)
    assert _same(v2, V) and np.array_equal(f2, F) and np.array_equal(g2, G)


def _kf_filter(pkg):
    """The 61 x 47 filter of tests/rectify_scene.py with XYZ features, as in test_gpu_dense.py (so that Point4sba rows exist)."""
    g = pkg.VSlamFilter(rs.config(pkg.kinect_config(), rs.BARREL), capacity_features=16, dtype=np.float32)
    for i in range(ks.N_FEATURES):
        assert g.addFeature((8.0 + 8.0 * i, 8.0 + 6.0 * i)) == 1
    S = g.getFullSigma()
    n0 = g.camera_dim
    S[n0:, :] *= 1e-4
    S[:, n0:] *= 1e-4
    g.setSigmaBlock(S)
    g.convert2XYZ_ifLinearAll()
    return g


def test_recorder_to_sba_to_mesh_end_to_end(pkg, tmp_path):
    """KeyframeRecorder(rectify=True, images=True) over the walk -> sba_add -> mesh_from_recording with the adjusted poses,
    against the oracles driven from the same files (the automatic bounds included)."""
    from ekf_monoslam_amd import dense
    g = _kf_filter(pkg)
    sel = pkg.KeyframeSelector(g, ks.MOVE_THRESH, keep_current_projections=True)
    rec = pkg.KeyframeRecorder(sel, str(tmp_path / "rec"), images=True, rectify=True)
    for k, fr in enumerate(ks.scene_walk()[:9]):
        g.setFrame(kg.image_of(fr["id"], (rs.MH, rs.MW)))
        mu = g.getFullState()
        mu[:7] = fr["pose"]
        g.setFullState(mu)
        g.setSigmaBlock(fr["sigma"].astype(g.dtype), 0, 0)
        for i in range(ks.N_FEATURES):
            g.setFeatureTrack(i, in_innovation=int(fr["in_innovation"][i]),
                              center=np.array([6.25 + 8.5 * i + 0.125 * k, 5.75 + 6.25 * i + 0.375 * (k % 3)], np.float32))
        rec.observe(fr["id"])
    files = rec.finish()
    sel.close()
    g.close()
    assert len(rec.ids) >= 3
    nodes_out = str(tmp_path / "Nodes_Out.txt")
    pkg.sba_add(*files, camera=rec.camera_path, every=3, nodes_out=nodes_out)
    kw = dict(neighbours=1, w_min=0.02, w_max=0.3, planes=8, radius=1, rel_tol=0.2, min_agree=1)
    t0 = time.perf_counter()
    got = pkg.mesh_from_recording(rec.directory, nodes_out, min_count=1, sweep_trunc=60, **kw)
    t1 = time.perf_counter()
    kw["trunc_cost"] = 60
    V, F, G, origin, dims, vx, tr = fs.oracle_mesh_from_recording(dense.read_recording, dense.neighbours_of, rec.directory, nodes_out,
                                                                   min_count=1, **kw)
    print("recording: key frames", len(rec.ids), "vertices", len(V), "faces", len(F), "dims", dims, "voxel", vx,
          "device path %.2f s, oracle %.2f s" % (t1 - t0, time.perf_counter() - t1))
    assert [m.id for m in got.maps] == rec.ids and np.array_equal(np.array([m.pose for m in got.maps]), pkg.formats.read_nodes_out(nodes_out)[1])
    assert got.dims == dims and (got.voxel, got.trunc) == (vx, tr) and np.array_equal(got.origin, origin)
    assert _same(got.vertices, V) and np.array_equal(got.faces, F) and np.array_equal(got.grey, G)
    assert sum(int((m.depth > 0).sum()) for m in got.maps) > 0
