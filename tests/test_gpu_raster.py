"""The rasteriser of the indexed meshes on the device against tests/raster_oracle.py, bit for bit: depth, normal,
grey, colour, triangle, barycentrics and cover, on the volumes of tests/test_gpu_texture.py (written with set_volume, so that no
sweep runs) and on the hand-built meshes of tests/raster_scene.py.  Every comparison is exact equality of bits."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import colour_scene as col
import fusion_scene as fs
import raster_oracle as ro
import raster_scene as rs
import raycast_scene as rsc
import texture_oracle as to
import texture_scene as ts
from test_gpu_texture import (ARG, P, SOURCES, STATE, _fetch, _make_source, _same, _same_atlas, _same_mesh, _same_render, _source,  # noqa: F401
                              _texture, _views, _volume, pkg)

pytestmark = pytest.mark.gpu


def _equal(got, want, cover=True):
    """A MeshRender against an oracle dict."""
    if (got.colour is None) != (want["colour"] is None) or (cover and got.cover is None):
        return False
    return (_same(got.depth, want["depth"]) and _same(got.normal, want["normal"]) and _same(got.grey, want["grey"]) and
            _same(got.tri, want["tri"]) and _same(got.bary, want["bary"]) and (got.colour is None or _same(got.colour, want["colour"])) and
            (not cover or _same(got.cover, want["cover"])))


def _same_images(a, b):
    return _equal(a, dict(depth=b.depth, normal=b.normal, grey=b.grey, colour=b.colour, tri=b.tri, bary=b.bary, cover=b.cover), b.cover is not None)


def _camera(name):
    """(shape, K, poses) of a volume's renders: the main shape is 37 x 19, no multiple of 8, with ragged last tiles."""
    if name.startswith("main"):
        return rsc.MAIN_SHAPE, fs.K_MAP, (fs.POSES[0], fs.POSES[2])
    return (ts.W, ts.H), ts.K, (ts.POSES[1], ts.AXES[2])


def _set_mesh(v, mesh):
    v.set_raster_mesh(mesh["vertices"], mesh["faces"], mesh["grey"], mesh.get("colour"))


@pytest.mark.parametrize("name", ("sphere", "main", "sphere_colour", "main_colour"))
def test_raster_equals_the_oracle_from_all_five_sources(pkg, name):
    """Culling on and off, with cover; vertex colours, and atlases of P = 2 with 3 channels and P = 8 with 1; the source's arrays
    through its own getter, the atlas through ekf_texture_get and the volume's render through ekf_raycast_get are what they were."""
    v = _volume(pkg, name)
    shape, K, poses = _camera(name)
    try:
        ray = v.raycast(shape, K, poses[0], rsc.MAIN_NEAR if name.startswith("main") else rsc.SPHERE_NEAR,
                        rsc.MAIN_FAR if name.startswith("main") else rsc.SPHERE_FAR)
        for source in SOURCES:
            src = _make_source(v, source)
            want_src = _source(name, source)
            for pose in poses:
                for cull in (True, False):
                    got = v.rasterise(shape, K, pose, source, 0.0, cull, "vertex", True)
                    assert _equal(got, ro.rasterise(want_src, shape, K, pose, 0.0, cull, cover=True)), (source, cull)
                    assert (got.colour is not None) == name.endswith("colour")
            hit = int((got.tri >= 0).sum())
            assert _same_mesh(_fetch(pkg, v, source, src), src), source
            for patch, channels in ((2, 3), (8, 1)):
                views = _views(name, True)
                atlas, _ = _texture(v, source, patch, channels, views)
                want_atlas = to.texture(want_src, patch, channels, views)
                assert _same_atlas(atlas, want_atlas)
                for cull in (True, False):
                    got = v.rasterise(shape, K, poses[0], source, 0.0, cull, "texture", True)
                    assert _equal(got, ro.rasterise(want_src, shape, K, poses[0], 0.0, cull, want_atlas["atlas"], patch, True)), (source, patch, cull)
                    assert (got.colour is not None) == (channels == 3)
                assert _same_atlas(v.texture_peek(), want_atlas) and _same_mesh(_fetch(pkg, v, source, src), src), (source, patch)
            print(name, source, len(src.faces), "triangles:", hit, "pixels hit of", shape)
        assert _same_render(v._render(), ray)
        # source 4: the simplified mesh given back by the caller shows what source 3 shows
        _set_mesh(v, want_src)
        for cull in (True, False):
            got = v.rasterise(shape, K, poses[1], "mesh", 0.0, cull, "vertex", True)
            assert _equal(got, ro.rasterise(want_src, shape, K, poses[1], 0.0, cull, cover=True)), cull
            assert _same_images(got, v.rasterise(shape, K, poses[1], "simplified", 0.0, cull, "vertex", True))
        assert _same_mesh(_fetch(pkg, v, source, src), src) and _same_render(v._render(), ray)
    finally:
        v.close()


def test_every_hand_built_scene_through_both_paths(pkg):
    """Every scene of tests/raster_scene.py as source 4, culling on and off, at small_limit 0, 64 and 65536: identical images, and
    the profile's counts say which path ran (k_rast_large is not launched when no box can exceed the limit).  1 x 1 and 64 x 48
    images, 301 triangles (a ragged second workgroup), the same render twice."""
    from ekf_monoslam_amd import fusion
    v = _volume(pkg, "sphere")
    count = lambda d: [c for _, c in d.values()]
    try:
        for name, (mesh, shape, z_near) in sorted(rs.scenes().items()):
            _set_mesh(v, mesh)
            for cull in (True, False):
                want = ro.rasterise(mesh, shape, rs.K, rs.POSE, z_near, cull, cover=True)
                for limit in rs.SMALL_LIMITS:
                    v.set_raster_small_limit(limit)
                    v.profile(True)
                    got = v.rasterise(shape, rs.K, rs.POSE, "mesh", z_near, cull, "vertex", True)
                    assert _equal(got, want), (name, cull, limit)
                    prof = v.get_raster_profile()
                    assert list(prof) == list(fusion.RASTER_KERNELS)
                    assert count(prof) == [1, 1, 1 if limit < shape[0] * shape[1] else 0, 1], (name, limit, prof)
                    assert _same_images(v.rasterise(shape, rs.K, rs.POSE, "mesh", z_near, cull, "vertex", True), got)
                    assert count(v.get_raster_profile())[0] == 2
                    v.profile(False)
            print(name, shape, int((want["tri"] >= 0).sum()), "pixels hit")
        v.set_raster_small_limit(64)
        # nothing in the other getters
        v.profile(True)
        v.rasterise((8, 8), rs.K, rs.POSE, "mesh")
        assert count(v.get_profile()) == [0] * 4 and count(v.get_mesh_profile()) == [0] * 5 and count(v.get_texture_profile()) == [0] * 4
        assert count(v.get_raycast_profile()) == [0, 0] and count(v.get_simplify_profile()) == [0] * 10
        v.profile(False)
    finally:
        v.close()


def test_regrowth_the_large_image_and_a_view_from_a_dense_slot(pkg):
    """116 x 92 (through both paths), then 1 x 1, then 116 x 92 again: the buffers grow once and the images are the oracle's each
    time; a render without cover after one with it; rasterise_view takes the slot's size, K and pose."""
    v = _volume(pkg, "sphere")
    d = pkg.DenseStereo(ts.W, ts.H, 2)
    try:
        _make_source(v, "weld")
        m = _source("sphere", "weld")
        want = ro.rasterise(m, rs.BIG_SHAPE, rs.BIG_K, ts.AXES[0], 0.0, True, cover=True)
        for limit in (64, 0):
            v.set_raster_small_limit(limit)
            assert _equal(v.rasterise(rs.BIG_SHAPE, rs.BIG_K, ts.AXES[0], "weld", cover=True), want), limit
        assert int((want["tri"] >= 0).sum()) == 4830 and int((want["cover"] == 2).sum()) == 10
        one = np.array([30.0, 30.0, 0.0, 0.0])
        assert _equal(v.rasterise((1, 1), one, rsc.POSE_A, "weld", cover=True), ro.rasterise(m, (1, 1), one, rsc.POSE_A, cover=True))
        got = v.rasterise(rs.BIG_SHAPE, rs.BIG_K, ts.AXES[0], "weld")
        assert got.cover is None and _equal(got, want, False)
        assert (v.rasterise((ts.W, ts.H), ts.K, rsc.AWAY, "weld", cull=False).tri == -1).all()
        inside = v.rasterise((ts.W, ts.H), ts.K, rs.CENTRE, "weld", cull=False, cover=True)
        assert (inside.tri >= 0).all() and (inside.cover == 1).all() and (v.rasterise((ts.W, ts.H), ts.K, rs.CENTRE, "weld").tri == -1).all()
        d.set_view(1, np.zeros((ts.H, ts.W), np.uint8), ts.K, ts.POSES[1])
        got = v.rasterise_view(d, 1, "weld", 0.0, False, "vertex", True)
        assert _equal(got, ro.rasterise(m, (ts.W, ts.H), ts.K, ts.POSES[1], 0.0, False, cover=True))
        lib, err = pkg.load_library(), lambda: lib.ekf_fusion_last_error(v._h).decode()
        view = lambda dense=d, slot=1, source=0: lib.ekf_raster_render_view(v._h, source, None if dense is None else dense._h, slot,
                                                                           C.c_double(0.0), 1, 0, 0)
        assert view(dense=None) == ARG and err() == "ekf_raster_render_view: a dense handle on the volume's device"
        for slot in (-1, 2):
            assert view(slot=slot) == ARG and err() == "ekf_raster_render_view: slot in 0..max_views-1"
        assert view(slot=0) == STATE and err() == "ekf_raster_render_view: the slot is not set"
        assert view(source=5) == ARG and view() == 0
    finally:
        d.close()
        v.close()


def test_state_rules_and_argument_errors(pkg):
    lib = pkg.load_library()
    v = _volume(pkg, "sphere")
    err = lambda: lib.ekf_fusion_last_error(v._h).decode()

    def render(source=0, w=ts.W, h=ts.H, K=ts.K, pose=rsc.POSE_A, z_near=0.0, cull=1, shading=0, cover=0):
        return lib.ekf_raster_render(v._h, source, w, h, None if K is None else P(np.ascontiguousarray(K, np.float64)),
                                     None if pose is None else P(np.ascontiguousarray(pose, np.float64)), C.c_double(z_near), cull, shading, cover)

    get = lambda **kw: lib.ekf_raster_get(v._h, *[kw.get(k) for k in ("depth", "normal", "grey", "bgr", "tri", "bary", "cover", "w", "h")])
    try:
        assert get() == STATE and err() == "ekf_raster_get: no ekf_raster_render"
        v.reset()
        for source in range(3):
            assert render(source) == STATE and err() == "ekf_raster_render: no ekf_mesh_weld since the volume last changed"
        assert render(3) == STATE and err() == "ekf_raster_render: source 3 needs an ekf_simplify_run on the current mesh"
        assert render(4) == STATE and err() == "ekf_raster_render: source 4 needs an ekf_raster_set_mesh"
        v.weld(1)
        assert render(0) == STATE and err() == "ekf_raster_render: the source mesh has no triangle"
        v.set_volume(*fs.sphere_volume())
        v.weld(1)
        assert render(1) == STATE and err() == "ekf_raster_render: source 1 needs an ekf_components_prune since the last ekf_mesh_weld"
        assert render(2) == STATE and err() == "ekf_raster_render: source 2 needs an ekf_smooth_run on the current mesh"
        assert get() == STATE
        # the view's arguments, then the render's, each before the device is touched
        nan, inf = float("nan"), float("inf")
        msg = "ekf_raster_render: 1 <= width, height <= 8192; K finite with fx, fy != 0; pose7 finite with q != 0"
        for kw in (dict(w=0), dict(h=0), dict(w=8193), dict(h=8193), dict(K=None), dict(K=[0.0, 30.0, 1.0, 1.0]), dict(K=[30.0, nan, 1.0, 1.0]),
                   dict(pose=None), dict(pose=np.zeros(7)), dict(pose=[inf, 0, 0, 1, 0, 0, 0])):
            assert render(**kw) == ARG and err() == msg, kw
        msg = "ekf_raster_render: source 0..4; z_near finite and >= 0; cull, shading and cover 0 or 1"
        for kw in (dict(source=-1), dict(source=5), dict(z_near=-0.5), dict(z_near=nan), dict(z_near=inf), dict(cull=2), dict(cull=-1),
                   dict(shading=2), dict(cover=2), dict(cover=-1)):
            assert render(**kw) == ARG and err() == msg, kw
        assert render(4, shading=1) == ARG and err() == "ekf_raster_render: shading 1 needs a source with a texture: 0, 1, 2 or 3"
        assert get() == STATE                                                # none of them rendered
        # shading 1 needs a finished texture of the source that is rendered
        need = "ekf_raster_render: shading 1 needs a finished texture (ekf_texture_finish) of the source that is rendered"
        assert render(0, shading=1) == STATE and err() == need
        v.texture_begin("weld", 2, 1)
        assert render(0, shading=1) == STATE and err() == need               # begun, not finished
        v.texture_finish()
        v.prune(2)
        assert render(0, shading=1) == 0 and render(1, shading=1) == STATE and err() == need      # the weld's texture, not the pruned mesh's
        # the getter: every pointer may be NULL; bgr and cover only where the render has them
        w, h = C.c_int(0), C.c_int(0)
        assert get(w=C.byref(w), h=C.byref(h)) == 0 and (w.value, h.value) == (ts.W, ts.H)
        buf = np.zeros(ts.W * ts.H * 3, np.uint32)
        msg = "ekf_raster_get: bgr must be NULL when the render has no colour image, and cover when it was rendered with cover = 0"
        assert get(bgr=P(buf)) == ARG and err() == msg and get(cover=P(buf)) == ARG and err() == msg
        assert render(0, cover=1) == 0 and get(cover=P(buf)) == 0 and buf[:ts.W * ts.H].max() == 1 and get(bgr=P(buf)) == ARG
        # the images are a snapshot: a new weld, a change of the volume and a failed render leave them readable
        before = v._mesh_render("weld", "vertex", True)
        v.weld(1)
        v.set_volume(*fs.sphere_volume())
        assert render(0) == STATE and render(w=0) == ARG
        assert _same_images(v._mesh_render("weld", "vertex", True), before) and (before.tri >= 0).sum() == 293
        # ekf_raster_set_mesh's checks, on the host
        X, F, g = np.array([[0.0, 0, 1], [0, 1, 1], [1, 0, 1]]), np.array([[0, 1, 2]], np.uint32), np.array([1, 2, 3], np.uint8)
        set_mesh = lambda X=X, F=F, g=g, c=None, nv=3, nt=1: lib.ekf_raster_set_mesh(v._h, P(X), P(F), P(g), P(c), nv, nt)
        msg = "ekf_raster_set_mesh: xyz, faces and grey not NULL; 0 < n_vert, n_tri < 2^32; xyz finite; every index < n_vert"
        bad_X, bad_F = X.copy(), F.copy()
        bad_X[1, 2], bad_F[0, 2] = nan, 3
        for kw in (dict(X=None), dict(F=None), dict(g=None), dict(nv=0), dict(nt=0), dict(X=bad_X), dict(F=bad_F), dict(nv=2)):
            assert set_mesh(**kw) == ARG and err() == msg, kw
        assert render(4) == STATE and set_mesh() == 0 and render(4, 4, 4, rs.K, rs.POSE) == 0
        assert _same_images(v._mesh_render("weld", "vertex", False), before) is False      # the next render replaced them
        limit = "ekf_raster_set_small_limit: limit in 0..65536"
        for bad in (-1, 65537):
            assert lib.ekf_raster_set_small_limit(v._h, bad) == ARG and err() == limit
        assert lib.ekf_raster_set_small_limit(v._h, 0) == 0 and lib.ekf_raster_set_small_limit(v._h, 65536) == 0
        ms_, cnt = np.zeros(4), np.zeros(4, np.int64)
        assert lib.ekf_raster_get_profile(v._h, None, P(cnt)) == ARG and lib.ekf_raster_get_profile(v._h, P(ms_), P(cnt)) == 0
        assert lib.ekf_raster_set_mesh(None, P(X), P(F), P(g), None, 3, 1) == ARG
        assert lib.ekf_raster_render_view(None, 0, None, 0, C.c_double(0.0), 1, 0, 0) == ARG
        for bad in ("soup", 4, None):
            with pytest.raises(ValueError):
                v.rasterise((4, 4), rs.K, rs.POSE, bad)
        with pytest.raises(ValueError):
            v.rasterise((4, 4), rs.K, rs.POSE, "mesh", shading="flat")
    finally:
        v.close()


def test_recordings_audited_through_the_mesh(pkg, tmp_path, monkeypatch):
    """audit_recording(render="mesh") on the wall recording and on the colour recording: every frame's ``mesh`` audit is
    ``audit_frame`` of the oracle's rasterisation of the mesh the audit returned, vertex colours without ``texture=`` and the atlas
    with it; shade() takes a MeshRender; with render=None the launches of an audit are today's: no rasteriser launch."""
    from ekf_monoslam_amd import dense, fusion, keyframes
    kw = dict(fs.REC_SWEEP)
    kw["sweep_trunc"] = kw.pop("trunc")
    for kind in ("wall", "colour"):
        rec = str(tmp_path / kind)
        if kind == "wall":
            fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
        else:
            col.write_colour_recording(rec, pkg.formats, keyframes.write_ppm)
        K, ids, poses, images = dense.read_recording(rec, None)
        for texture, extra in ((None, {}), (dict(patch=3, occlusion=False), dict(simplify=2.0))):
            audit = pkg.audit_recording(rec, None, texture=texture, render="mesh", **extra, **kw)
            m = audit.mesh
            mesh = dict(vertices=m.vertices, faces=m.faces, grey=m.grey, colour=m.colour)
            atlas = None if texture is None else m.texture.atlas
            h, w = images[0].shape[:2]
            for fr, dm, img in zip(audit.frames, m.maps, images):
                want = ro.rasterise(mesh, (w, h), K, dm.pose, 0.0, True, atlas, None if texture is None else 3)
                assert isinstance(fr.mesh, pkg.fusion.FrameAudit) and isinstance(fr.mesh.render, pkg.MeshRender)
                assert _equal(fr.mesh.render, want, False) and fr.mesh.id == fr.id and fr.mesh.mesh is None
                again = fusion.audit_frame(fr.id, fr.mesh.render, dm.depth, img)
                for k in ("overlap", "median", "p90", "grey_error", "colour_error"):
                    a, b = getattr(fr.mesh, k), getattr(again, k)
                    assert a == b or (a != a and b != b), k
                assert fr.mesh.overlap > 0 and pkg.shade(fr.mesh.render).shape == (h, w)
            print(kind, "texture" if texture else "vertex", ":", len(m.faces), "triangles; mesh overlap / grey error",
                  [(round(f.mesh.overlap, 3), round(f.mesh.grey_error, 2)) for f in audit.frames], "volume",
                  [(round(f.overlap, 3), round(f.grey_error, 2)) for f in audit.frames])
        # render=None makes today's launches: the volume's profile at its close has no rasteriser launch and no device weld
        seen = []
        real_init, real_close = fusion.TsdfVolume.__init__, fusion.TsdfVolume.close

        def init(self, *a, **k):
            real_init(self, *a, **k)
            self.profile(True)

        def close(self):
            if getattr(self, "_h", None):
                seen.append((self.get_raster_profile(), self.get_mesh_profile(), self.get_raycast_profile()))
            real_close(self)

        monkeypatch.setattr(fusion.TsdfVolume, "__init__", init)
        monkeypatch.setattr(fusion.TsdfVolume, "close", close)
        plain = pkg.audit_recording(rec, None, **kw)
        with_mesh = pkg.audit_recording(rec, None, render="mesh", **kw)
        monkeypatch.undo()
        count = lambda d: [c for _, c in d.values()]
        n = len(plain.frames)
        assert all(f.mesh is None for f in plain.frames) and len(seen) == 2
        assert count(seen[0][0]) == [0] * 4 and count(seen[0][1]) == [0] * 5
        assert count(seen[1][0]) == [n, n, n, n] and sum(count(seen[1][1])) > 0 and count(seen[0][2]) == count(seen[1][2])
    with pytest.raises(ValueError):
        pkg.audit_recording(rec, None, render="volume", **kw)
