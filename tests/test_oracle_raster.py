"""The two forms of tests/raster_oracle.py against each other, bit for bit, and against what the contract
implies whatever they compute: on the hand-built meshes of tests/raster_scene.py, on the sphere's weld from the six cameras on
the axes and from pose B, on the two sheets of tests/texture_scene.py and on atlases of tests/texture_oracle.py; the header, the
prototypes and the exports.  CPU only."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

import raster_oracle as ro
import raster_scene as rs
import raycast_scene as rsc
import texture_oracle as to
import texture_scene as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_raster_set_mesh", "ekf_raster_render", "ekf_raster_render_view", "ekf_raster_get", "ekf_raster_set_small_limit",
         "ekf_raster_get_profile")


@functools.lru_cache(maxsize=None)
def _sphere(view, cull, big=False):
    """The vectorised oracle's render of the sphere's weld: computed once, shared, and left unchanged."""
    shape, K = (rs.BIG_SHAPE, rs.BIG_K) if big else ((ts.W, ts.H), ts.K)
    return ro.rasterise(rs.sphere(), shape, K, rs.SPHERE_VIEWS[view], 0.0, cull, cover=True)


@pytest.mark.parametrize("name", sorted(rs.scenes()))
def test_loop_and_vectorised_forms_agree_on_every_scene(name):
    mesh, shape, z_near = rs.scenes()[name]
    for cull in (True, False):
        a = ro.rasterise(mesh, shape, rs.K, rs.POSE, z_near, cull, cover=True)
        assert ro.same(a, ro.rasterise_loop(mesh, shape, rs.K, rs.POSE, z_near, cull, cover=True)), cull
        assert np.array_equal(a["cover"] > 0, a["tri"] >= 0) and np.array_equal(a["depth"] > 0, a["tri"] >= 0)
        assert (a["colour"] is None) == (mesh["colour"] is None) and a["tri"].max() < len(mesh["faces"])
        print(name, "cull", cull, ":", int((a["tri"] >= 0).sum()), "pixels hit, cover", np.bincount(a["cover"].ravel()))


def test_loop_and_vectorised_forms_agree_on_the_sphere_and_with_an_atlas():
    """Pose B with culling off (two layers), and both shadings' other branch: atlases of 1 and 3 channels, P = 2 and 8."""
    m = rs.sphere()
    assert ro.same(_sphere(6, False), ro.rasterise_loop(m, (ts.W, ts.H), ts.K, rs.SPHERE_VIEWS[6], 0.0, False, cover=True))
    for P, channels in ((2, 3), (8, 1)):
        atlas = to.texture(m, P, channels, ts.views(True))["atlas"]
        a = ro.rasterise(m, (ts.W, ts.H), ts.K, ts.POSES[1], 0.0, True, atlas, P)
        assert ro.same(a, ro.rasterise_loop(m, (ts.W, ts.H), ts.K, ts.POSES[1], 0.0, True, atlas, P)), P
        assert (a["colour"] is not None) == (channels == 3)
        assert ro.same(a, _sphere(6, True), ("depth", "normal", "tri", "bary"))           # the shading changes the colours alone


def test_the_sphere_is_covered_once_with_culling_and_twice_without():
    """At 29 x 23 every hit pixel is covered exactly once with culling on and exactly twice with it off, from the six cameras on
    the axes (293 pixels) and from pose B (270); at 116 x 92 no missed pixel has four hit neighbours, and the 10 pixels an
    axis camera sees covered twice lie where the silhouette folds."""
    for view in range(7):
        on, off = _sphere(view, True), _sphere(view, False)
        hit = on["tri"] >= 0
        assert int(hit.sum()) == (270 if view == 6 else 293) and np.array_equal(hit, off["tri"] >= 0)
        assert (on["cover"][hit] == 1).all() and (off["cover"][hit] == 2).all() and (on["cover"][~hit] == 0).all()
        assert ro.same(on, off, ("depth", "tri", "grey"))                                  # the front layer wins
        big = _sphere(view, True, True)
        hit = big["tri"] >= 0
        h = np.pad(hit, 1)
        assert not (~hit & h[:-2, 1:-1] & h[2:, 1:-1] & h[1:-1, :-2] & h[1:-1, 2:]).any()
        assert int(hit.sum()) == (4284 if view == 6 else 4830) and int((big["cover"] == 2).sum()) == (0 if view == 6 else 10)
        assert big["cover"].max() <= 2


def _runs(face, a, b):
    """Whether the triangle's corner order runs the edge from a to b."""
    f = [int(v) for v in face]
    return any(f[k] == a and f[(k + 1) % 3] == b for k in range(3))


def _owner(faces, a, b, front):
    """The triangle the rule gives a pixel on the edge between the vertices a < b: the one that runs the edge in ascending
    index order after its flip, that is b -> a in its own corner order if it is front, a -> b otherwise."""
    want = [t for t, f in enumerate(faces) if (_runs(f, b, a) if front else _runs(f, a, b))]
    assert len(want) == 1
    return want[0]


def test_ties_on_shared_edges_go_to_the_owner_the_rule_names():
    """The fan and the quads, as they are (front faces) and with every triangle reversed and culling off (back faces): every
    interior pixel is covered exactly once; a pixel on a spoke or on the diagonal shows the owner."""
    fan = rs.fan()
    spokes = {k: [(8 + s * dx, 8 + s * dy) for s in range(1, 6)] for k, (dx, dy) in
              enumerate([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)])}
    rim = [k if k < rs.FAN_CENTRE else k + 1 for k in range(8)]
    for front in (True, False):
        mesh = fan if front else dict(fan, faces=fan["faces"][:, ::-1].copy())
        r = ro.rasterise(mesh, rs.FAN_SHAPE, rs.K, rs.POSE, 0.0, front, cover=True)
        assert (r["cover"][rs.fan_interior()] == 1).all() and r["cover"].max() == 1
        for k, pixels in spokes.items():
            a, b = sorted((rs.FAN_CENTRE, rim[k]))
            for x, y in pixels:
                assert r["tri"][y, x] == _owner(mesh["faces"], a, b, front), (front, k, x, y)
        assert r["tri"][8, 8] >= 0                                            # the centre: one of the eight, once
        for order in range(3):
            quad = rs.quad(order)
            mesh = quad if front else dict(quad, faces=quad["faces"][:, ::-1].copy())
            r = ro.rasterise(mesh, rs.QUAD_SHAPE, rs.K, rs.POSE, 0.0, front, cover=True)
            assert (r["cover"][rs.quad_interior()] == 1).all() and r["cover"].max() == 1
            for d in range(2, 9):
                assert r["tri"][d, d] == _owner(mesh["faces"], 0, 2, front), (front, order, d)
    # a reversed mesh with culling on shows nothing
    assert (ro.rasterise(dict(fan, faces=fan["faces"][:, ::-1].copy()), rs.FAN_SHAPE, rs.K, rs.POSE)["tri"] == -1).all()


def test_the_coincident_pair_shows_the_lower_index():
    mesh, shape, _ = rs.scenes()["coincident"]
    r = ro.rasterise(mesh, shape, rs.K, rs.POSE, cover=True)
    hit = r["tri"] >= 0
    assert hit.sum() > 0 and (r["tri"][hit] == 0).all() and (r["cover"][hit] == 2).all()


def test_dropped_triangles_and_the_full_image_triangle():
    """clip: the triangle behind the camera, the one across z_near and the one outside the image give no pixel; the others do,
    the nearer one in front.  degenerate: only the triangle with an area shows.  full: every pixel is hit, the small triangles
    in front of the large one."""
    mesh, shape, z_near = rs.scenes()["clip"]
    r = ro.rasterise(mesh, shape, rs.K, rs.POSE, z_near, cover=True)
    assert set(np.unique(r["tri"])) == {-1, 0, 4, 5} and (r["tri"][5:10, 8:12] == 4)[r["cover"][5:10, 8:12] == 2].all()
    assert (ro.rasterise(mesh, shape, rs.K, rs.POSE, 0.0)["tri"] == 3).any()      # without the near plane it is there
    mesh, shape, _ = rs.scenes()["degenerate"]
    assert set(np.unique(ro.rasterise(mesh, shape, rs.K, rs.POSE, 0.0, False)["tri"])) == {-1, 2}
    mesh, shape, _ = rs.scenes()["full"]
    r = ro.rasterise(mesh, shape, rs.K, rs.POSE, cover=True)
    assert (r["tri"] >= 0).all() and len(np.unique(r["tri"])) == 301 and (r["tri"][r["cover"] == 2] > 0).all()
    assert np.array_equal(np.unique(r["depth"]), np.array([0.5, 1.0], np.float32))


def test_away_and_from_the_centre():
    """From AWAY nothing is hit.  From the sphere's centre nothing is hit with culling on, and every pixel with it off."""
    m = rs.sphere()
    assert (ro.rasterise(m, (ts.W, ts.H), ts.K, rsc.AWAY, 0.0, False)["tri"] == -1).all()
    assert (ro.rasterise(m, (ts.W, ts.H), ts.K, rs.CENTRE, 0.0, True)["tri"] == -1).all()
    inside = ro.rasterise(m, (ts.W, ts.H), ts.K, rs.CENTRE, 0.0, False, cover=True)
    assert (inside["tri"] >= 0).all() and (inside["cover"] == 1).all()


def test_the_front_sheet_wins_where_the_sheets_overlap():
    m = ts.occlusion_mesh()
    r = ro.rasterise(m, ts.OCC_SHAPE, ts.OCC_K, ts.OCC_POSE, 0.0, True, cover=True)
    z = np.asarray(m["vertices"])[np.asarray(m["faces"], np.int64)][:, :, 2]
    both = r["cover"] == 2
    assert both.sum() > 20 and (z[r["tri"][both]] < 1.5).all() and (r["depth"][both] < 1.5).all()
    assert (z[r["tri"][r["cover"] == 1]] > 1.5).any() and r["cover"].max() == 2


def test_the_atlas_of_a_constant_image_gives_the_constant_on_every_textured_triangle():
    m = rs.sphere()
    for channels, value in ((1, 77), (3, (17, 201, 94))):
        img = np.broadcast_to(np.array(value, np.uint8), (ts.H, ts.W) + ((3,) if channels == 3 else ())).copy()
        t = to.texture(m, 4, channels, [dict(image=img, K=ts.K, pose=p) for p in ts.POSES])
        r = ro.rasterise(m, (ts.W, ts.H), ts.K, ts.POSES[1], 0.0, True, t["atlas"], 4)
        textured = np.zeros(r["tri"].shape, bool)
        textured[r["tri"] >= 0] = t["view"][r["tri"][r["tri"] >= 0]] >= 0
        assert textured.sum() > 200
        if channels == 3:
            assert (r["colour"][textured] == np.array(value, np.uint8)).all() and (r["grey"][textured] == to.grey_of(np.array(value))).all()
        else:
            assert (r["grey"][textured] == value).all() and r["colour"] is None


def test_fidelity_the_atlas_is_closer_to_the_views_than_the_vertex_colours():
    """DESIGN.md §30.4's table, from tools/raster_timing.py at a quarter of its view width: shading 1 is closer to the views' own
    images than shading 0 on the weld and at cells of 1 and 2 voxels (§29.4's 7-, 5- and 3-fold gaps are the margin); 4 voxels
    and the depth against the ray cast are reported only."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    rows = __import__("raster_timing").fidelity(116)
    assert [r["triangles"] for r in rows] == [2592, 846, 218, 58]
    for r in rows[:3]:
        assert r["mean_abs_grey_error_shading_1"] < r["mean_abs_grey_error_shading_0"], r


def test_abi_the_header_the_prototypes_and_the_exports():
    """The header, _PROTOS and the exports, and EKF_ERR_ARG for a NULL handle.  Fails on the parent."""
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi, fusion
    header = open(os.path.join(ROOT, "include", "ekf_monoslam.h")).read()
    lib = pkg.load_library()
    for fn in NAMES:
        assert re.search(r"^int %s\(" % fn, header, flags=re.M) and fn in capi._PROTOS and hasattr(lib, fn), fn
    assert sorted(n for n in pkg.declared_symbols() if n.startswith("ekf_raster_")) == sorted(NAMES)
    assert [len(capi._PROTOS[n][1]) for n in NAMES] == [7, 10, 8, 10, 2, 3] and lib.ekf_abi_version() == 6
    assert lib.ekf_raster_render(None, 0, 1, 1, None, None, C.c_double(0.0), 1, 0, 0) == 1
    assert lib.ekf_raster_get(None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.ekf_raster_set_small_limit(None, 64) == 1 and lib.ekf_raster_get_profile(None, None, None) == 1
    assert fusion.RASTER_KERNELS == ("k_rast_project", "k_rast_small", "k_rast_large", "k_rast_resolve")
    assert fusion.RASTER_SOURCES == dict(fusion.TEXTURE_SOURCES, mesh=4) and issubclass(pkg.MeshRender, pkg.Render)
    assert all(hasattr(fusion.TsdfVolume, n) for n in ("set_raster_mesh", "rasterise", "rasterise_view", "set_raster_small_limit",
                                                       "get_raster_profile"))
