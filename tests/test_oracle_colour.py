"""The colour contract of the dense chain on the numpy oracle alone, and what of the library can be checked
without a device: the ABI table, the argument errors, the identities that tie the colour planes to the grey ones, that the GPU
test shapes contain every case, and the file formats (the kernel bodies on the host: tests/test_host_checks.py).
CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import colour_oracle as co
import colour_scene as cs
import fusion_oracle as fo
import fusion_scene as fs
import raycast_scene as rsc

DENSE_NAMES = ("ekf_dense_set_view_colour", "ekf_dense_set_view_colour_device", "ekf_dense_set_view_colour_from_keyframe",
               "ekf_dense_get_view_colour")
VOLUME_NAMES = ("ekf_colour_create", "ekf_colour_has", "ekf_colour_integrate_host", "ekf_colour_get_volume", "ekf_colour_set_volume",
                "ekf_colour_get_mesh", "ekf_colour_get_render", "ekf_colour_get_profile")
_CACHE = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


def _kw(c):
    c = dict(c)
    c["pose7"] = c.pop("pose")
    return c


def _fused(kind="pattern"):
    if kind not in _CACHE:
        _CACHE[kind] = cs.fused(maps=cs.colour_maps(kind))
    return _CACHE[kind]


def _renders():
    if "renders" not in _CACHE:
        _CACHE["renders"] = {k: (c, co.raycast(**_kw(c))) for k, c in cs.raycast_cases().items()}
    return _CACHE["renders"]


# ---- the library without a device --------------------------------------------------------------------------------------------
def test_header_prototypes_and_exports_agree(pkg):
    from ekf_monoslam_amd import capi, dense, fusion
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    assert sorted(n for n in declared if n.startswith("ekf_colour_")) == sorted(VOLUME_NAMES)
    assert sorted(n for n in capi._PROTOS if n.startswith("ekf_colour_")) == sorted(VOLUME_NAMES)
    for n in DENSE_NAMES + VOLUME_NAMES:
        assert n in declared and n in capi._PROTOS and hasattr(lib, n), n
    assert lib.ekf_abi_version() == 6
    assert all(hasattr(dense.DenseStereo, n) for n in ("view_colour", "has_colour")) and hasattr(dense, "read_ppm")
    assert hasattr(fusion.TsdfVolume, "get_colour_profile") and hasattr(fusion, "grey_image")
    for cls in (fusion.Mesh, fusion.Render, fusion.RecordingMesh):
        assert list(cls.__dataclass_fields__)[-1] == "colour" and cls.__dataclass_fields__["colour"].default is None
    assert list(fusion.FrameAudit.__dataclass_fields__)[-1] == "colour_error"
    m = fusion.Mesh(np.zeros((0, 3, 3)), np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.uint8))     # positional, as before
    assert m.colour is None


def test_argument_errors_need_no_device(pkg):
    lib = pkg.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    K, pose = np.array([24.0, 24.0, 18.0, 9.0]), np.array([0.0, 0, 0, 1, 0, 0, 0])
    bgr, depth, csum = np.zeros((19, 37, 3), np.uint8), np.zeros((19, 37), np.float32), np.zeros(24, np.uint32)
    ms, cnt = np.zeros(3), np.zeros(3, np.int64)
    assert lib.ekf_dense_set_view_colour(None, 0, P(bgr), 111, P(K), P(pose)) == 1
    assert lib.ekf_dense_set_view_colour_device(None, 0, P(bgr), 111, P(K), P(pose)) == 1
    assert lib.ekf_dense_set_view_colour_from_keyframe(None, 0, None, P(pose)) == 1
    assert lib.ekf_dense_get_view_colour(None, 0, None, 0) == 1
    assert lib.ekf_colour_has(None) == 0
    assert lib.ekf_colour_integrate_host(None, P(depth), P(bgr), 111, 37, 19, P(K), P(pose)) == 1
    assert lib.ekf_colour_get_volume(None, P(csum)) == 1 and lib.ekf_colour_set_volume(None, P(csum)) == 1
    assert lib.ekf_colour_get_mesh(None, None, 0) == 1 and lib.ekf_colour_get_render(None, None) == 1
    assert lib.ekf_colour_get_profile(None, P(ms), P(cnt)) == 1
    # the create rules are those of ekf_fusion_create, checked before the device is looked for
    h = C.c_void_p()
    o = np.zeros(3)
    for dims, voxel, trunc, origin in (((1, 4, 4), 0.1, 0.4, o), ((4, 4, 1025), 0.1, 0.4, o), ((4, 4, 4), 0.0, 0.4, o),
                                       ((4, 4, 4), 0.1, np.nan, o), ((4, 4, 4), 0.1, 0.4, np.array([0.0, np.inf, 0.0]))):
        assert lib.ekf_colour_create(*dims, P(origin), voxel, trunc, 0, C.byref(h)) == 1 and not h
    assert lib.ekf_colour_create(4, 4, 4, None, 0.1, 0.4, 0, C.byref(h)) == 1 and lib.ekf_colour_create(4, 4, 4, P(o), 0.1, 0.4, 0, None) == 1
    assert b"ekf_fusion_create" in lib.ekf_fusion_last_error(None)


# ---- the conversion ----------------------------------------------------------------------------------------------------------
def test_grey_of_equal_channels_is_the_channel():
    g = np.arange(256)
    assert 1868 + 9617 + 4899 == 1 << 14
    assert np.array_equal(co.bgr2gray(g, g, g), g)
    assert int(co.bgr2gray(255, 255, 255)) == 255 and int(co.bgr2gray(0, 0, 0)) == 0


def test_grey_of_the_binding_is_the_oracles(pkg):
    from ekf_monoslam_amd import fusion
    for w, h in cs.GREY_SHAPES + cs.TINY_GREY_SHAPES:
        img = cs.pattern(w, h, 2)
        assert np.array_equal(fusion.grey_image(img), co.grey_of(img)) and co.grey_of(img).shape == (h, w)
    b, g, r = (v.astype(np.int64) for v in np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 3), np.arange(0, 256, 7), indexing="ij"))
    assert np.array_equal(co.bgr2gray(b, g, r), (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14)


def test_the_grey_shapes_have_a_tail_and_none():
    counts = [w * h for w, h in cs.GREY_SHAPES]
    assert [c % 4 for c in counts] == [3, 3, 0] and counts[0] // 4 > 256 > counts[1] // 4       # more than one workgroup, and one
    assert [w * h for w, h in cs.TINY_GREY_SHAPES] == [1, 2, 5]


# ---- the volume --------------------------------------------------------------------------------------------------------------
def test_grey_planes_of_a_colour_volume_are_those_of_a_plain_volume():
    maps = cs.colour_maps()
    (steps, classes) = _fused()
    plain, plain_classes = fs.fused(maps=[(d, co.grey_of(im), K, p) for d, im, K, p in maps])
    for a, b, ca, cb in zip(steps, plain, classes, plain_classes):
        assert all(a[i].tobytes() == b[i].tobytes() for i in range(3)) and np.array_equal(ca, cb)
    assert steps[-1][3].shape == (3,) + steps[-1][0].shape and steps[-1][3].dtype == np.uint32
    # the planes differ from one another and from gsum: the pattern has three different channels
    cs_ = steps[-1][3]
    assert not np.array_equal(cs_[0], cs_[1]) and not np.array_equal(cs_[1], cs_[2]) and not np.array_equal(cs_[0], steps[-1][2])
    # a channel sum is bounded by 255 a map
    assert int(cs_.max()) <= 255 * int(steps[-1][1].max())


def test_integration_order_does_not_matter():
    a, b = cs.fused(order=(0, 1, 2))[0][-1], cs.fused(order=(2, 0, 1))[0][-1]
    assert all(a[i].tobytes() == b[i].tobytes() for i in (1, 2, 3))           # the integer planes, exactly
    assert np.allclose(a[0], b[0], rtol=0, atol=1e-5)                        # (sum is one fp32 add a map, in the maps' order)


def test_equal_channels_give_three_planes_equal_to_gsum():
    vol = _fused("equal")[0][-1]
    assert int(vol[2].sum()) > 0
    for c in range(3):
        assert np.array_equal(vol[3][c], vol[2])
    for mc in (1, 2):
        xyz, key, grey, colour = co.extract(vol, fs.DIMS, fs.ORIGIN, fs.VOXEL, mc)
        assert len(key) > 0 and all(np.array_equal(colour[..., c], grey) for c in range(3))
    r = co.raycast(**_kw(rsc.main_case(vol, 0, 1)))
    assert r["stats"]["hits"] > 0 and all(np.array_equal(r["colour"][..., c], r["grey"]) for c in range(3))
    s = cs.sphere_volume("equal")
    xyz, key, grey, colour = co.extract(s, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    assert all(np.array_equal(colour[..., c], grey) for c in range(3))


def test_a_map_without_colour_adds_its_grey_to_all_three_planes():
    grey = fs.synthetic_maps()
    vol = co.empty_volume(fs.DIMS)
    for m in grey:
        co.integrate(vol, fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, *m)
    want = fs.fused()[0][-1]
    assert all(vol[i].tobytes() == want[i].tobytes() for i in range(3))
    assert all(np.array_equal(vol[3][c], want[2]) for c in range(3))


def test_a_constant_image_gives_its_colour_everywhere():
    vol = _fused("constant")[0][-1]
    for c in range(3):
        assert np.array_equal(vol[3][c], vol[1].astype(np.uint32) * cs.CONSTANT[c])
    for mc in (1, 2):
        _, key, grey, colour = co.extract(vol, fs.DIMS, fs.ORIGIN, fs.VOXEL, mc)
        assert len(key) > 0 and (colour == np.array(cs.CONSTANT, np.uint8)).all()
        assert (grey == int(co.bgr2gray(*cs.CONSTANT))).all()
    for n, mc in ((0, 1), (1, 2)):
        r = co.raycast(**_kw(rsc.main_case(vol, n, mc)))
        hit = r["depth"] > 0
        assert hit.any() and not hit.all()
        assert (r["colour"][hit] == np.array(cs.CONSTANT, np.uint8)).all() and (r["colour"][~hit] == 0).all()
    s = cs.sphere_volume("constant")
    _, key, _, colour = co.extract(s, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    assert len(key) > 1000 and (colour == np.array(cs.CONSTANT, np.uint8)).all()


# ---- the mesh ----------------------------------------------------------------------------------------------------------------
def test_vertex_colours_from_the_keys_equal_the_extraction_of_each_channel_plane():
    """The kernel's way (from the key alone) against the grey oracle's way (from the cell and its corners) with the channel's
    plane in gsum's place."""
    for vol, dims, origin, voxel in ((_fused()[0][-1], fs.DIMS, fs.ORIGIN, fs.VOXEL),
                                     (cs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL)):
        xyz, key, grey, colour = co.extract(vol, dims, origin, voxel, 1)
        plain = fo.extract(vol[:3], dims, origin, voxel, 1)
        assert xyz.tobytes() == plain[0].tobytes() and np.array_equal(key, plain[1]) and np.array_equal(grey, plain[2])
        for c in range(3):
            _, k2, g2, _ = fo.extract((vol[0], vol[1], vol[3][c]), dims, origin, voxel, 1)
            assert np.array_equal(k2, key) and np.array_equal(g2, colour[..., c]), c
        assert len({tuple(v) for v in colour.reshape(-1, 3)[:2000]}) > 50             # and they are colours, not one value


def test_every_edge_delta_occurs_among_the_keys():
    for vol, dims, origin, voxel in ((_fused()[0][-1], fs.DIMS, fs.ORIGIN, fs.VOXEL),
                                     (cs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL)):
        key = co.extract(vol, dims, origin, voxel, 1)[1]
        assert sorted(set((key & np.uint64(7)).reshape(-1).tolist())) == [1, 2, 3, 4, 5, 6, 7]


def test_equal_keys_carry_equal_colours():
    _, key, _, colour = co.extract(cs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    k, c = key.reshape(-1), colour.reshape(-1, 3)
    order = np.argsort(k, kind="stable")
    same = k[order][1:] == k[order][:-1]
    assert same.any() and np.array_equal(c[order][1:][same], c[order][:-1][same])


# ---- the GPU shapes contain every case ---------------------------------------------------------------------------------------
def test_every_class_of_voxel_occurs_in_the_gpu_shapes():
    classes = _fused()[1]
    seen = set()
    for cl in classes:
        seen |= set(np.unique(cl).tolist())
    assert seen == set(range(6)), [fo.CLASS_NAMES[c] for c in sorted(set(range(6)) - seen)]


def test_the_last_pixel_of_a_map_is_sampled_by_some_voxel():
    """Its three bytes are the last three of the colour image: a read behind them would be a read behind the buffer."""
    hits = 0
    for depth, bgr, K, pose in cs.colour_maps():
        h, w = depth.shape
        mark = np.zeros((h, w), np.uint8)
        mark[h - 1, w - 1] = 1
        vol = fo.empty_volume(fs.DIMS)
        fo.integrate(vol, fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, depth, mark, K, pose)
        hits += int(vol[2].sum())
    assert hits > 0


def test_the_views_have_a_hit_and_a_miss():
    rd = _renders()
    for name in ("sphere_A", "sphere_B", "main_0_min1", "main_1_min2"):
        hit = rd[name][1]["depth"] > 0
        assert hit.any() and not hit.all(), name
        assert (rd[name][1]["colour"][~hit] == 0).all()
        assert len({tuple(v) for v in rd[name][1]["colour"][hit]}) > 20, name
    assert rd["sphere_away"][1]["stats"]["hits"] == 0 and not rd["sphere_away"][1]["colour"].any()


# ---- files -------------------------------------------------------------------------------------------------------------------
def test_ppm_round_trip_and_grey_recordings_read_as_before(pkg, tmp_path):
    from ekf_monoslam_amd import dense, keyframes
    img = cs.pattern(13, 7, 3)
    path = str(tmp_path / "a.ppm")
    keyframes.write_ppm(path, img)
    data = open(path, "rb").read()
    assert data.startswith(b"P6\n13 7\n255\n") and data[12:15] == bytes(img[0, 0, ::-1])          # R, G, B in the file
    back = dense.read_ppm(path)
    assert back.dtype == np.uint8 and back.flags["C_CONTIGUOUS"] and np.array_equal(back, img)
    keyframes.write_pgm(str(tmp_path / "g.pgm"), img[..., 0])
    with pytest.raises(ValueError):
        dense.read_ppm(str(tmp_path / "g.pgm"))
    # a grey recording: exactly the (H, W) arrays read_pgm gives
    grey = str(tmp_path / "grey")
    ids = fs.write_wall_recording(grey, pkg.formats, keyframes.write_pgm)
    K, got_ids, poses, images = dense.read_recording(grey)
    assert got_ids == ids and all(im.shape == (fs.REC_H, fs.REC_W) for im in images)
    assert all(np.array_equal(im, dense.read_pgm(os.path.join(grey, "%d.pgm" % i))) for i, im in zip(ids, images))
    # a colour recording: (H, W, 3), B G R; a .pgm beside a .ppm wins, as before
    col = str(tmp_path / "colour")
    ids = cs.write_colour_recording(col, pkg.formats, keyframes.write_ppm)
    K2, ids2, poses2, images2 = dense.read_recording(col)
    assert ids2 == ids and np.array_equal(K2, K) and np.array_equal(poses2, poses)
    assert all(im.shape == (fs.REC_H, fs.REC_W, 3) for im in images2)
    assert all(np.array_equal(a, cs.tint(b)) for a, b in zip(images2, images))
    keyframes.write_pgm(os.path.join(col, "%d.pgm" % ids[0]), images[0])
    assert dense.read_recording(col)[3][0].shape == (fs.REC_H, fs.REC_W)
    os.remove(os.path.join(col, "%d.pgm" % ids[0]))
    os.remove(os.path.join(col, "%d.ppm" % ids[1]))
    with pytest.raises(ValueError):
        dense.read_recording(col)


def test_coloured_ply_round_trip_and_the_grey_file_is_unchanged(pkg, tmp_path):
    from ekf_monoslam_amd import fusion
    vol = cs.sphere_volume()
    xyz, key, grey, colour = co.extract(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    mesh = fusion.Mesh(xyz, key, grey, colour)
    V, F, G, Cc = fusion.weld(mesh, colour=True)
    first, faces = fo.weld(key)
    assert len(fusion.weld(mesh)) == 3 and np.array_equal(Cc, colour.reshape(-1, 3)[first]) and np.array_equal(F, faces)
    with pytest.raises(ValueError):
        fusion.weld(fusion.Mesh(xyz, key, grey), colour=True)
    a, b = str(tmp_path / "grey.ply"), str(tmp_path / "colour.ply")
    fusion.write_mesh_ply(a, V, F, G)
    fusion.write_mesh_ply(b, V, F, G, colour=Cc)
    head = open(b).read().split("end_header")[0]
    assert head.index("intensity") < head.index("property uchar red") < head.index("green") < head.index("blue") < head.index("element face")
    assert "red" not in open(a).read().split("end_header")[0]
    first_vertex = open(b).read().split("end_header\n")[1].splitlines()[0].split()
    assert [int(t) for t in first_vertex[3:]] == [int(G[0]), int(Cc[0, 2]), int(Cc[0, 1]), int(Cc[0, 0])]     # intensity, R, G, B
    v2, f2, g2, c2 = fusion.read_mesh_ply(b, colour=True)
    assert v2.tobytes() == V.tobytes() and np.array_equal(f2, F) and np.array_equal(g2, G) and np.array_equal(c2, Cc)
    assert len(fusion.read_mesh_ply(b)) == 3 and np.array_equal(fusion.read_mesh_ply(b)[2], G)
    v3, f3, g3 = fusion.read_mesh_ply(a)
    assert v3.tobytes() == V.tobytes() and np.array_equal(f3, F) and np.array_equal(g3, G)
    with pytest.raises(ValueError):
        fusion.read_mesh_ply(a, colour=True)


def test_albedo_shading_and_the_audit_of_a_colour_frame(pkg):
    from ekf_monoslam_amd import fusion
    c, r = _renders()["sphere_A"]
    render = fusion.Render(r["depth"], r["normal"], r["grey"], r["colour"])
    lit = fusion.shade(render, albedo=True)
    lam = np.maximum(r["normal"].astype(np.float64) @ np.array([0.0, 0.0, -1.0]), 0.0)
    want = np.where((r["depth"] > 0)[..., None], np.floor(r["colour"].astype(np.float64) * lam[..., None] + 0.5), 0.0).astype(np.uint8)
    assert lit.shape == r["colour"].shape and np.array_equal(lit, want) and lit.any()
    assert np.array_equal(fusion.shade(render), fusion.shade(fusion.Render(r["depth"], r["normal"], r["grey"])))
    with pytest.raises(ValueError):
        fusion.shade(fusion.Render(r["depth"], r["normal"], r["grey"]), albedo=True)
    # the audit: against the render's own colour the error is 0, against a grey image it is NaN
    image = r["colour"].copy()
    image[..., 1] = np.where(image[..., 1] < 250, image[..., 1] + 3, image[..., 1] - 3)
    fa = fusion.audit_frame(4, render, np.where(r["depth"] > 0, r["depth"], 0).astype(np.float32), image)
    assert fa.colour_error == 1.0 and fa.median == 0.0
    assert fa.grey_error == float(np.abs(r["grey"][r["depth"] > 0].astype(np.float64) - co.grey_of(image)[r["depth"] > 0]).mean())
    assert np.isnan(fusion.audit_frame(4, render, r["depth"], r["grey"]).colour_error)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_colour_demo_compiles_against_the_mirror_header(pkg, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "ekf-monoslam_for_3d-reconstruction_amd", "lib")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                        os.path.join(root, "examples", "colour_demo.cpp"), "-o", str(tmp_path / "colour_demo"), "-L", libdir,
                        "-lekfslam_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
