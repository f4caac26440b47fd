"""The texture atlas of the welded, the pruned, the smoothed or the simplified mesh on the device against
tests/texture_oracle.py, bit for bit, on the volumes of tests/component_scene.py, tests/colour_scene.py and
tests/texture_scene.py: written with set_volume, so that no sweep runs.  Every comparison is exact equality of bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import colour_scene as col
import component_oracle as co
import component_scene as cs
import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import raycast_oracle as ro
import raycast_scene as rsc
import simplify_oracle as so
import smooth_oracle as sm
import texture_oracle as to
import texture_scene as ts

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
PRUNE, ROUNDS, FACTOR = 9, 2, 2.0                  # the pruned source is prune(9), the smoothed one two rounds, the simplified one 2 voxels
SOURCES = ("weld", "pruned", "smoothed", "simplified")
STATE, ARG = 4, 1


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _same_atlas(got, want, n_won=None):
    """A TextureAtlas against an oracle dict."""
    atlas = want["atlas"][:, :, 0] if want["atlas"].shape[2] == 1 else want["atlas"]
    return (_same(got.atlas, atlas) and _same(got.uv, want["uv"]) and _same(got.view, want["view"]) and _same(got.score, want["score"]) and
            got.n_textured == want["n_textured"] and (n_won is None or list(n_won) == want["n_won"]))


VOLUMES = {
    "sphere": lambda: cs.cases()["sphere"][:5],
    "main": lambda: cs.cases()["main"][:5],
    "sphere_colour": lambda: (col.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC),
    "main_colour": lambda: (col.fused()[0][-1], fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC),
    "occlusion": lambda: (ts.occlusion_volume(), ts.OCC_DIMS, ts.OCC_ORIGIN, ts.OCC_VOXEL, ts.OCC_TRUNC),
    "one": lambda: (ts.one_triangle_volume(), ts.ONE_DIMS, ts.ONE_ORIGIN, ts.ONE_VOXEL, ts.ONE_TRUNC),
}


@functools.lru_cache(maxsize=None)
def _source(name, source):
    """The oracle's source mesh of a volume: computed once, shared, and left unchanged."""
    planes, dims, origin, voxel, _ = VOLUMES[name]()
    _, soup_key, _, _ = fo.extract(planes[:3], dims, origin, voxel, 1)
    m = mo.weld(planes, dims, origin, voxel, soup_key, 1, False)
    if source == "pruned":
        return co.prune(m, PRUNE)
    if source == "smoothed":
        return sm.smooth(m, ROUNDS)
    if source == "simplified":
        return so.as_mesh(so.simplify(m, origin, dims, voxel, (ts.ONE_FACTOR if name == "one" else FACTOR) * voxel))
    return m


def _volume(pkg, name):
    planes, dims, origin, voxel, trunc = VOLUMES[name]()
    v = pkg.TsdfVolume(dims, origin, voxel, trunc, colour=len(planes) > 3)
    v.set_volume(*planes[:3], csum=planes[3] if len(planes) > 3 else None)
    return v


def _make_source(v, source, name=""):
    m = v.weld(1)
    if source == "pruned":
        m = v.prune(PRUNE)
    if source == "smoothed":
        m = v.smooth(ROUNDS)
    if source == "simplified":
        m = v.simplify((ts.ONE_FACTOR if name == "one" else FACTOR) * v.voxel)
    return m


def _fetch(pkg, v, source, like):
    """The source's arrays as its getter delivers them now: ekf_mesh_get, ekf_components_get_pruned, ekf_smooth_get or
    ekf_simplify_get, called directly, so that nothing is made again."""
    nv, nt = len(like.key), len(like.faces)
    back = pkg.IndexedMesh(np.full((nv, 3), -1.0), np.full((nt, 3), 0xFFFFFFFF, np.uint32), np.full(nv, 0xA5, np.uint8),
                           None if like.colour is None else np.full((nv, 3), 0xA5, np.uint8), None, np.full(nv, 2**64 - 1, np.uint64))
    lib = pkg.load_library()
    getter = {"weld": lib.ekf_mesh_get, "pruned": lib.ekf_components_get_pruned, "smoothed": lib.ekf_smooth_get,
              "simplified": lib.ekf_simplify_get}[source]
    assert getter(v._h, P(back.vertices), P(back.faces), P(back.grey), P(back.colour), None, P(back.key), nv, nt) == 0
    return back


def _same_mesh(a, b):
    """Two IndexedMesh equal bit for bit: vertices, faces, grey, colour and key."""
    return (_same(a.vertices, b.vertices) and _same(a.faces, b.faces) and _same(a.grey, b.grey) and _same(a.key, b.key) and
            ((a.colour is None and b.colour is None) or _same(a.colour, b.colour)))


def _same_render(a, b):
    return (_same(a.depth, b.depth) and _same(a.normal, b.normal) and _same(a.grey, b.grey) and
            ((a.colour is None and b.colour is None) or _same(a.colour, b.colour)))


def _texture(v, source, patch, channels, views, occlusion=None):
    """begin, every view from the host, finish: (TextureAtlas, the triangles every view won)."""
    v.texture_begin(source, patch, channels)
    n_won = [v.texture_add_view_host(w["image"], w["K"], w["pose"], occlusion, w.get("tol"), w.get("min_area2", 0.0)) for w in views]
    return v.texture_finish(), n_won


def _views(name, colour):
    return ts.main_views(colour) if name.startswith("main") else ts.views(colour)


@pytest.mark.parametrize("name", ("sphere", "main", "sphere_colour", "main_colour"))
def test_texture_equals_the_oracle_from_all_four_sources(pkg, name):
    """1 and 3 channels, grey and colour views, on a plain and on a colour volume (whose fallback blends B, G, R into a
    3-channel atlas and grey into a 1-channel one); the sphere has 2592 triangles and 1298 vertices, and AWAY wins nothing."""
    v = _volume(pkg, name)
    try:
        for source in SOURCES:
            src = _make_source(v, source)
            want_src = _source(name, source)
            assert _same(src.vertices, want_src["vertices"]) and np.array_equal(src.faces, want_src["faces"]), source
            assert _same_mesh(_fetch(pkg, v, source, src), src), source
            for patch, channels, colour in ((3, 3, True), (4, 1, False), (2, 3, False), (5, 1, True)):
                views = _views(name, colour)
                got, n_won = _texture(v, source, patch, channels, views)
                want = to.texture(want_src, patch, channels, views)
                assert _same_atlas(got, want, n_won), (source, patch, channels, colour)
                assert got.atlas.shape[0] == v._texture[0] and got.n_textured == int((got.view >= 0).sum())
                # the source is what it was: its getter's arrays before and after, and so are the meshes it was made from
                assert _same_mesh(_fetch(pkg, v, source, src), src), (source, patch)
            if source == "simplified":
                assert _same_mesh(_fetch(pkg, v, "weld", weld), weld)
            if source == "weld":
                weld = src
            print(name, source, len(src.faces), "triangles: won", n_won, "textured", got.n_textured, "atlas", got.atlas.shape)
        # the same sequence again gives the same bytes, and the source is what it was
        again, _ = _texture(v, source, patch, channels, views)
        assert _same_atlas(again, want) and _same_mesh(_fetch(pkg, v, source, src), src)
    finally:
        v.close()


def test_occlusion_from_the_handles_own_render(pkg):
    """The sphere with its ray cast as z-buffer, and the two sheets: with occlusion the view loses the back sheet's hidden part.
    The render stays readable and is what it was."""
    v = _volume(pkg, "sphere")
    try:
        src = _make_source(v, "weld")
        occ = (rsc.SPHERE_NEAR, rsc.SPHERE_FAR, 0.125, 1)
        views = []
        for w in ts.views(True):
            z = ro.raycast(fs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, rsc.SPHERE_SHAPE, w["K"], w["pose"], *occ)["depth"]
            views.append(dict(w, zbuf=z, tol=fs.SPHERE_VOXEL))
        got, n_won = _texture(v, "weld", 4, 3, ts.views(True), occ)          # tol: the default, the voxel
        want = to.texture(_source("sphere", "weld"), 4, 3, views)
        assert _same_atlas(got, want, n_won) and 0 < want["n_textured"] <= 909
        r = v._render()
        assert _same(r.depth, views[-1]["zbuf"])                             # the last view's render, still there
        # a render of the caller's own is only read: depth, normal and grey through ekf_raycast_get before and after
        before = v.raycast(rsc.SPHERE_SHAPE, ts.K, rsc.POSE_B, *occ)
        assert (before.depth > 0).any() and _same_render(v._render(), before)
        lib, n = pkg.load_library(), C.c_ulonglong(0)
        v.texture_begin("weld", 4, 3)
        w = ts.views(True)[1]
        assert lib.ekf_texture_add_view_host(v._h, P(w["image"]), w["image"].strides[0], 3, ts.W, ts.H, P(ts.K), P(rsc.POSE_B), 1,
                                             C.c_double(fs.SPHERE_VOXEL), C.c_double(0.0), C.byref(n)) == 0 and n.value > 0
        assert _same_render(v._render(), before)
        v.texture_finish()
        assert _same_render(v._render(), before) and _same_mesh(_fetch(pkg, v, "weld", src), src)
    finally:
        v.close()
    v = _volume(pkg, "occlusion")
    try:
        _make_source(v, "weld")
        occ = (ts.OCC_NEAR, ts.OCC_FAR, None, 1)
        m = ts.occlusion_mesh()
        for occluded in (True, False):
            w = ts.occlusion_view(occluded)
            got, n_won = _texture(v, "weld", 3, 1, [w], occ if occluded else None)
            assert _same_atlas(got, to.texture(m, 3, 1, [w]), n_won), occluded
            assert n_won == ([482] if occluded else [992])
    finally:
        v.close()


def test_views_from_the_slots_of_a_dense_handle(pkg):
    """A grey and a colour slot, read where they lie on the device, into 3 channels and into 1 (a colour slot's grey image);
    with occlusion the wrapper renders the slot's view first."""
    v = _volume(pkg, "sphere")
    d = pkg.DenseStereo(ts.W, ts.H, 3)
    try:
        _make_source(v, "weld")
        views = ts.views(True)
        views[1] = dict(views[1], image=np.ascontiguousarray(views[1]["image"][:, :, 0]))       # slot 1 is grey
        for n, w in enumerate(views):
            d.set_view(n, w["image"], w["K"], w["pose"])
        for channels in (3, 1):
            v.texture_begin("weld", 3, channels)
            n_won = [v.texture_add_view(d, n) for n in range(3)]
            assert _same_atlas(v.texture_finish(), to.texture(_source("sphere", "weld"), 3, channels, views), n_won), channels
        occ = (rsc.SPHERE_NEAR, rsc.SPHERE_FAR, 0.25, 1)
        zviews = [dict(w, tol=0.1, zbuf=ro.raycast(fs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, rsc.SPHERE_SHAPE,
                                                   w["K"], w["pose"], *occ)["depth"]) for w in views]
        v.texture_begin("weld", 2, 3)
        n_won = [v.texture_add_view(d, n, occ, tol=0.1) for n in range(3)]
        assert _same_atlas(v.texture_finish(), to.texture(_source("sphere", "weld"), 2, 3, zviews), n_won)
        other = pkg.DenseStereo(ts.W + 1, ts.H, 1)
        try:
            other.set_view(0, np.zeros((ts.H, ts.W + 1), np.uint8), ts.K, rsc.POSE_A)
            v.texture_begin("weld", 2, 1)
            v.raycast(rsc.SPHERE_SHAPE, ts.K, rsc.POSE_A, *occ)
            n = C.c_ulonglong(7)
            lib = pkg.load_library()
            assert lib.ekf_texture_add_view(v._h, other._h, 0, 1, C.c_double(0.1), C.c_double(0.0), C.byref(n)) == STATE and n.value == 7
            assert lib.ekf_fusion_last_error(v._h).decode() == ("ekf_texture_add_view: occlusion needs an ekf_raycast_render of the view's "
                                                                 "size since the volume last changed")
            msg = "ekf_texture_add_view: slot in 0..max_views-1, occlusion 0 or 1, tol and min_area2 finite and >= 0, n_won not NULL"
            nan, inf = float("nan"), float("inf")
            add = lambda dense=d, slot=0, occ=0, tol=0.1, area=0.0, out=C.byref(n): lib.ekf_texture_add_view(
                v._h, dense._h, slot, occ, C.c_double(tol), C.c_double(area), out)
            for kw in (dict(dense=other, slot=1), dict(slot=-1), dict(slot=3), dict(occ=2), dict(occ=-1), dict(tol=nan), dict(tol=-0.1),
                       dict(tol=inf), dict(area=nan), dict(area=-1.0), dict(area=inf), dict(out=None)):
                assert add(**kw) == ARG and lib.ekf_fusion_last_error(v._h).decode() == msg, kw
            assert n.value == 7 and v.texture_peek().n_textured == 0             # none of them counted as a view
            assert lib.ekf_texture_add_view(v._h, d._h, 2, 0, C.c_double(0.1), C.c_double(0.0), C.byref(n)) == 0 and n.value == 0
            assert lib.ekf_texture_add_view(v._h, None, 0, 0, C.c_double(0.1), C.c_double(0.0), C.byref(n)) == ARG
            assert lib.ekf_fusion_last_error(v._h).decode() == "ekf_texture_add_view: a dense handle on the volume's device"
            d2 = pkg.DenseStereo(ts.W, ts.H, 2)
            try:
                assert lib.ekf_texture_add_view(v._h, d2._h, 1, 0, C.c_double(0.1), C.c_double(0.0), C.byref(n)) == STATE
                assert lib.ekf_fusion_last_error(v._h).decode() == "ekf_texture_add_view: the slot is not set"
            finally:
                d2.close()
        finally:
            other.close()
    finally:
        d.close()
        v.close()


def test_one_triangle_and_the_smallest_views(pkg):
    """n_tri = 1 (the hand-set volume simplified at 1.5 voxels): Q = 1, and half of the one block is padding.  A view that sees
    the triangle's back wins nothing; neither can a 2 x 1 or a 1 x 1 view (a triangle with an area does not fit between the
    centres of one row of pixels), which still run k_tex_project and k_tex_select; a 2 x 2 view wins it, every tap on the image's
    edge, and the full view then takes it over.  P = 2 divides by 1 and P = 32 is the largest patch."""
    v = _volume(pkg, "one")
    try:
        src = _make_source(v, "simplified", "one")
        m = ts.one_triangle_mesh()
        assert len(src.faces) == 1 and _same(src.vertices, m["vertices"])
        views = [dict(image=col.pattern(ts.W, ts.H, 1), K=ts.K, pose=ts.ONE_BEHIND),
                 dict(image=np.array([[[10, 20, 30], [200, 100, 50]]], np.uint8), K=np.array([1.0, 1.0, 0.5, 0.0]), pose=ts.ONE_POSE),
                 dict(image=np.array([[77]], np.uint8), K=np.array([1.0, 1.0, 0.0, 0.0]), pose=ts.ONE_POSE),
                 dict(image=np.array([[[10, 20, 30], [200, 100, 50]], [[90, 0, 255], [1, 2, 3]]], np.uint8),
                      K=np.array([5.0, 5.0, 0.5, 0.2]), pose=ts.ONE_POSE),
                 dict(image=col.pattern(ts.W, ts.H, 2), K=ts.K, pose=ts.ONE_POSE)]
        for patch in (2, 32, 7):
            for channels in (1, 3):
                for seq in (views, views[:-1]):
                    got, n_won = _texture(v, "simplified", patch, channels, seq)
                    assert _same_atlas(got, to.texture(m, patch, channels, seq), n_won), (patch, channels, len(seq))
                    assert got.atlas.shape[:2] == (patch + 2, patch + 2) and n_won == [0, 0, 0, 1, 1][:len(seq)]
        print("one triangle: won", n_won, "score", got.score)
    finally:
        v.close()


def test_shapes_where_the_kernels_can_go_wrong(pkg):
    """The sphere simplified at 2 voxels (218 triangles, Q = 11: 12 blocks of padding, a whole block row of them, for which
    nothing is launched) at P = 32 (A = 374: no multiple of 64, 497 workgroups, the last one ragged); simplified at 1.75 voxels
    (269 triangles: an odd number, so the last block's upper half is padding, and two workgroups of triangles); and a camera
    whose cx puts every vertex of the plane x = 0 exactly onto sx = W - 1."""
    v = _volume(pkg, "sphere")
    try:
        src = _make_source(v, "simplified")
        m = _source("sphere", "simplified")
        assert len(src.faces) == 218 and to.layout(218, 32) == (34, 11, 374) and 374 % 64 != 0 and (10 * 34 * 374) % 256 != 0
        got, n_won = _texture(v, "simplified", 32, 1, ts.views(False))
        assert _same_atlas(got, to.texture(m, 32, 1, ts.views(False)), n_won)
        assert (got.atlas[10 * 34:] == 0).all() and got.atlas[:10 * 34].any()   # the last block row is padding
        _, dims, origin, voxel, _ = VOLUMES["sphere"]()
        odd = so.as_mesh(so.simplify(_source("sphere", "weld"), origin, dims, voxel, 1.75 * voxel))
        assert len(v.simplify(1.75 * voxel).faces) == len(odd["faces"]) == 269
        for patch, channels in ((2, 3), (5, 1)):
            got, n_won = _texture(v, "simplified", patch, channels, ts.views(True))
            assert _same_atlas(got, to.texture(odd, patch, channels, ts.views(True)), n_won), patch
        # sx = W - 1 exactly: POSE_A is on the axis, so a vertex with x = 0 has p0 = 0 and sx = cx
        edge = np.array([30.0, 30.0, ts.W - 1.0, 11.0])
        weld = _make_source(v, "weld")
        on_edge = weld.vertices[:, 0] == 0.0
        _, sx, _ = to.project(weld.vertices, edge, *to._camera(dict(K=edge, pose=rsc.POSE_A))[1:])
        assert on_edge.sum() == 90 and (sx[on_edge] == ts.W - 1.0).all()
        views = [dict(image=col.pattern(ts.W, ts.H, 4), K=edge, pose=rsc.POSE_A)]
        got, n_won = _texture(v, "weld", 3, 3, views)
        want = to.texture(_source("sphere", "weld"), 3, 3, views)
        assert _same_atlas(got, want, n_won)
        assert (on_edge[weld.faces].any(axis=1) & (want["view"] == 0)).sum() > 0     # triangles with a vertex on the last column are won
    finally:
        v.close()


def test_finish_without_a_view_and_regrowth(pkg):
    """finish with no view at all gives the all-fallback atlas of the oracle; small, large, small on one handle."""
    v = _volume(pkg, "sphere_colour")
    try:
        for source, patch, channels in (("simplified", 2, 1), ("weld", 6, 3), ("simplified", 2, 1)):
            _make_source(v, source)
            got, n_won = _texture(v, source, patch, channels, [])
            want = to.texture(_source("sphere_colour", source), patch, channels, [])
            assert _same_atlas(got, want, n_won) and got.n_textured == 0 and (got.view == -1).all() and got.atlas.any()
        peek = v.texture_peek()
        assert _same_atlas(peek, want)
    finally:
        v.close()


def test_profile_counts(pkg):
    """One k_tex_project and one k_tex_select a view, one k_tex_fill a view that won a triangle (AWAY wins none), one
    k_tex_fallback; nothing in the other getters."""
    from ekf_monoslam_amd import fusion
    v = _volume(pkg, "sphere")
    try:
        _make_source(v, "weld")
        v.profile(True)
        assert list(v.get_texture_profile()) == list(fusion.TEXTURE_KERNELS) and len(fusion.TEXTURE_KERNELS) == 4
        count = lambda d: [c for _, c in d.values()]
        got, n_won = _texture(v, "weld", 3, 1, ts.views(False))
        assert n_won[2] == 0 and count(v.get_texture_profile()) == [3, 3, 2, 1]
        assert all(t > 0 for t, _ in v.get_texture_profile().values())
        assert count(v.get_profile()) == [0] * 4 and count(v.get_mesh_profile()) == [0] * 5 and count(v.get_component_profile()) == [0] * 8
        assert count(v.get_raycast_profile()) == [0, 0] and count(v.get_colour_profile()) == [0, 0, 0] and count(v.get_smooth_profile()) == [0] * 7
        assert count(v.get_simplify_profile()) == [0] * 10
        _texture(v, "weld", 3, 1, [])
        assert count(v.get_texture_profile()) == [3, 3, 2, 2]
    finally:
        v.close()


def test_state_rules_and_argument_errors(pkg):
    lib = pkg.load_library()
    v = _volume(pkg, "sphere")
    err = lambda: lib.ekf_fusion_last_error(v._h).decode()
    side, n = C.c_int(77), C.c_ulonglong(77)
    img = np.zeros((ts.H, ts.W), np.uint8)
    begin = lambda source=0, patch=4, channels=1, s=C.byref(side): lib.ekf_texture_begin(v._h, source, patch, channels, s)

    def add(img=img, pitch=ts.W, channels=1, w=ts.W, h=ts.H, K=ts.K, pose=rsc.POSE_A, occ=0, tol=0.0, area=0.0, out=C.byref(n)):
        return lib.ekf_texture_add_view_host(v._h, P(img), pitch, channels, w, h, P(np.ascontiguousarray(K, np.float64)),
                                             P(np.ascontiguousarray(pose, np.float64)), occ, C.c_double(tol), C.c_double(area), out)

    finish = lambda out=C.byref(n): lib.ekf_texture_finish(v._h, out)
    get = lambda: lib.ekf_texture_get(v._h, None, 0, None, None, None, 0)
    none = ": no ekf_texture_begin on the current mesh"

    def no_texture():
        assert add() == STATE and err() == "ekf_texture_add_view_host" + none
        assert finish() == STATE and err() == "ekf_texture_finish" + none
        assert get() == STATE and err() == "ekf_texture_get" + none

    try:
        v.reset()
        for source in range(3):
            assert begin(source) == STATE and err() == "ekf_texture_begin: no ekf_mesh_weld since the volume last changed"
        assert begin(3) == STATE and err() == "ekf_texture_begin: source 3 needs an ekf_simplify_run on the current mesh"
        no_texture()
        v.set_volume(*fs.sphere_volume())
        v.weld(1)
        assert begin(1) == STATE and err() == "ekf_texture_begin: source 1 needs an ekf_components_prune since the last ekf_mesh_weld"
        assert begin(2) == STATE and err() == "ekf_texture_begin: source 2 needs an ekf_smooth_run on the current mesh"
        assert begin(3) == STATE and err() == "ekf_texture_begin: source 3 needs an ekf_simplify_run on the current mesh"
        no_texture()
        msg = "ekf_texture_begin: source 0, 1, 2 or 3, patch 2..32, channels 1 or 3, atlas_side not NULL"
        for kw in (dict(source=-1), dict(source=4), dict(patch=1), dict(patch=33), dict(channels=0), dict(channels=2), dict(channels=4), dict(s=None)):
            assert begin(**kw) == ARG and err() == msg, kw
        assert side.value == 77
        no_texture()
        assert begin() == 0 and side.value == 36 * 6 and get() == 0
        # the argument errors of a view, each before the device is touched; none of them counts as a view
        nan, inf = float("nan"), float("inf")
        bad_K, bad_pose = np.array([0.0, 30.0, 1.0, 1.0]), np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        for kw in (dict(img=None), dict(pitch=ts.W - 1), dict(channels=2), dict(w=0), dict(h=0), dict(w=8193), dict(K=bad_K), dict(pose=bad_pose),
                   dict(occ=2), dict(occ=-1), dict(tol=nan), dict(tol=-1.0), dict(tol=inf), dict(area=nan), dict(area=-0.5), dict(area=inf), dict(out=None)):
            assert add(**kw) == ARG and err().startswith("ekf_texture_add_view_host: img, K, pose7 and n_won not NULL; channels 1 or 3;"), kw
        assert n.value == 77
        assert add(occ=1) == STATE and err() == ("ekf_texture_add_view_host: occlusion needs an ekf_raycast_render of the view's size since "
                                                 "the volume last changed")
        v.raycast((ts.W + 1, ts.H), ts.K, rsc.POSE_A, rsc.SPHERE_NEAR, rsc.SPHERE_FAR)
        assert add(occ=1) == STATE                                           # a render of another size
        v.raycast((ts.W, ts.H), ts.K, rsc.POSE_A, rsc.SPHERE_NEAR, rsc.SPHERE_FAR)
        assert add(occ=1, tol=0.25) == 0 and n.value > 0
        view = np.full(2592, 9, np.int32)
        assert lib.ekf_texture_get(v._h, None, 0, None, P(view), None, 2592) == 0 and set(np.unique(view)) == {-1, 0}   # the first view is 0
        atlas = np.zeros((216, 216), np.uint8)
        assert lib.ekf_texture_get(v._h, P(atlas), 215, None, None, None, 0) == ARG and err() == "ekf_texture_get: pitch >= atlas_side channels"
        wide = np.full((216, 300), 0xA5, np.uint8)
        assert lib.ekf_texture_get(v._h, P(wide), 300, None, None, None, 0) == 0 and (wide[:, 216:] == 0xA5).all()
        part = np.full(5, 9, np.int32)
        assert lib.ekf_texture_get(v._h, None, 0, None, P(part), None, 3) == 0 and (part[3:] == 9).all() and np.array_equal(part[:3], view[:3])
        assert finish(None) == ARG and err() == "ekf_texture_finish: n_textured must not be NULL"
        assert finish() == 0 and n.value == int((view >= 0).sum())
        assert lib.ekf_texture_get(v._h, P(atlas), 216, None, None, None, 0) == 0 and not np.array_equal(atlas, wide[:, :216])   # the fallback
        assert add() == STATE and err() == "ekf_texture_add_view_host: the texture is finished (ekf_texture_begin starts the next)"
        assert finish() == STATE and err() == "ekf_texture_finish: the texture is finished (ekf_texture_begin starts the next)"
        assert get() == 0                                                    # still readable
        assert lib.ekf_texture_begin(None, 0, 4, 1, C.byref(side)) == ARG and lib.ekf_texture_finish(None, C.byref(n)) == ARG
        assert lib.ekf_texture_get(None, None, 0, None, None, None, 0) == ARG and lib.ekf_texture_get_profile(None, None, None) == ARG
        ms_, cnt = np.zeros(4), np.zeros(4, np.int64)
        assert lib.ekf_texture_get_profile(v._h, None, P(cnt)) == ARG and lib.ekf_texture_get_profile(v._h, P(ms_), P(cnt)) == 0
        # whatever invalidates the source invalidates the texture
        assert begin() == 0
        v.prune(2)
        v.smooth(1)
        v.simplify(2.0 * v.voxel)
        assert get() == 0                                                    # made from the weld: a prune, a smooth and a simplify run leave it
        assert begin(3) == 0
        v.simplify(2.0 * v.voxel)                                            # a new simplify run
        no_texture()
        assert begin(2) == 0
        v.smooth(1)                                                          # a new smooth run
        no_texture()
        assert begin(1) == 0 and get() == 0
        v.prune(2)                                                           # a new prune
        no_texture()
        v.simplify(2.0 * v.voxel, "pruned")
        assert begin(3) == 0
        v.prune(2)                                                           # the simplified mesh's source goes, and the texture with it
        no_texture()
        assert begin(0) == 0
        v.weld(1)                                                            # a new weld
        no_texture()
        assert begin(0) == 0
        v.set_volume(*fs.sphere_volume())                                    # a change of the volume
        no_texture()
        for bad in ("soup", 0, None):
            with pytest.raises(ValueError):
                v.texture_begin(bad)
        # a source without a triangle
        v.reset()
        v.weld(1)
        assert begin(0) == STATE and err() == "ekf_texture_begin: the source mesh has no triangle"
    finally:
        v.close()


def test_an_atlas_of_more_than_16384_texels_a_side_is_refused(pkg):
    """The analytic sphere on 200^3 voxels welds to more than 462 722 triangles, so that P = 32 needs Q > 481 blocks a row and
    A = 34 Q > 16384: EKF_ERR_ARG with its message, before anything is allocated; atlas_side and the texture begun before stay
    as they were.  No oracle runs and nothing is copied to the host but the counts."""
    lib = pkg.load_library()
    n, voxel = 200, 0.0125
    origin = np.array([-1.25, -1.25, 1.0])
    x = origin[0] + np.arange(n) * voxel
    z = origin[2] + np.arange(n) * voxel
    c = (x[0] + x[-1]) / 2, (z[0] + z[-1]) / 2
    d2 = ((x[None, None, :] - c[0]) ** 2 + (x[None, :, None] - c[0]) ** 2) + (z[:, None, None] - c[1]) ** 2
    planes = (np.clip((np.sqrt(d2) - 0.35 * n * voxel) / (4 * voxel), -1, 1).astype(np.float32), np.ones((n, n, n), np.uint16),
              np.full((n, n, n), 128, np.uint32))
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    try:
        v.set_volume(*planes)
        nv, nt, side, won = C.c_ulonglong(0), C.c_ulonglong(0), C.c_int(77), C.c_ulonglong(0)
        assert lib.ekf_mesh_weld(v._h, 1, 0, C.byref(nv), C.byref(nt)) == 0
        B, Q, A = to.layout(nt.value, 32)
        assert nt.value > 462722 and A > 16384, nt.value
        assert lib.ekf_texture_begin(v._h, 0, 2, 1, C.byref(side)) == 0 and side.value == to.layout(nt.value, 2)[2]
        small = side.value
        assert lib.ekf_texture_begin(v._h, 0, 32, 1, C.byref(side)) == ARG and side.value == small
        assert lib.ekf_fusion_last_error(v._h).decode() == ("ekf_texture_begin: the atlas would be %d texels a side, more than 16384 (a smaller "
                                                             "patch, or ekf_simplify_run first)" % A)
        # the texture begun before is still there, at its own size
        row = np.full(small + 1, 0xA5, np.uint8)
        assert lib.ekf_texture_get(v._h, None, 0, None, None, None, 0) == 0
        assert lib.ekf_texture_get(v._h, P(row), small - 1, None, None, None, 0) == ARG
        assert lib.ekf_texture_finish(v._h, C.byref(won)) == 0 and won.value == 0
        print("200^3 sphere:", nt.value, "triangles; P = 32 would need", A, "texels a side")
    finally:
        v.close()


def test_recordings_textured_end_to_end(pkg, tmp_path):
    """audit_recording(texture=...) on the wall recording and on the colour recording against the oracle's restatement in
    tests/texture_scene.py, with occlusion (the z-buffers are the audit's own renders) and without, from the welded and from the
    simplified mesh; mesh_from_recording gives the same atlas."""
    from ekf_monoslam_amd import dense, keyframes
    kw = dict(fs.REC_SWEEP)
    kw["sweep_trunc"] = kw.pop("trunc")
    for kind in ("wall", "colour"):
        rec = str(tmp_path / kind)
        if kind == "wall":
            fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
        else:
            col.write_colour_recording(rec, pkg.formats, keyframes.write_ppm)
        K, ids, poses, images = dense.read_recording(rec, None)
        channels = 3 if kind == "colour" else 1
        for texture, extra in ((4, {}), (dict(patch=3, occlusion=False, min_area2=0.25), dict(simplify=2.0))):
            audit = pkg.audit_recording(rec, None, texture=texture, **extra, **kw)
            opts = dict(patch=texture) if isinstance(texture, int) else texture
            tol = None if not extra else 2.0 * audit.mesh.voxel
            want = ts.oracle_texture_of_audit(to, audit, K, images, opts["patch"], channels, opts.get("occlusion", True), tol,
                                              opts.get("min_area2", 0.0))
            got = audit.mesh.texture
            assert _same_atlas(got, want) and got.n_textured > 0, (kind, texture)
            print(kind, texture, ":", len(audit.mesh.faces), "triangles,", got.n_textured, "textured, atlas", got.atlas.shape)
        mesh = pkg.mesh_from_recording(rec, None, texture=dict(patch=3, occlusion=False, min_area2=0.25), simplify=2.0, **kw)
        assert _same_atlas(mesh.texture, want) and pkg.mesh_from_recording(rec, None, **kw).texture is None
    for bad in (1, 33, "eight", True, 4.0, dict(size=4)):
        with pytest.raises(ValueError):
            pkg.mesh_from_recording(rec, None, texture=bad, **kw)
