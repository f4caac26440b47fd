"""The two forms of tests/texture_oracle.py against each other, bit for bit, and against what the contract
implies whatever they compute, on the meshes of tests/component_scene.py, on the sphere simplified at 2 voxels and on the
occlusion volume of tests/texture_scene.py.  CPU only."""
import functools

import numpy as np
import pytest

import component_scene as cs
import raycast_scene as rsc
import texture_oracle as to
import texture_scene as ts

MESHES = ("main", "sphere", "257x2x2", "2x2x2", "sphere/2")


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return ts.simplified("sphere", 1, 2.0) if name == "sphere/2" else cs.oracle_mesh(name, 1)


@functools.lru_cache(maxsize=None)
def _run(name, P, channels, colour_views=True):
    """The vectorised oracle's result of a case: computed once, shared, and left unchanged."""
    return to.texture(_mesh(name), P, channels, ts.views(colour_views))


@pytest.mark.parametrize("name", MESHES)
def test_loop_and_vectorised_forms_agree(name):
    """1 and 3 channels, colour and grey views, P = 2 (a division by 1) and 3; the wave volumes are colour volumes, so their
    fallback blends B, G, R."""
    m = _mesh(name)
    for P, channels, colour_views in ((2, 3, True), (3, 1, True), (3, 3, False), (2, 1, False)):
        a, b = _run(name, P, channels, colour_views), to.texture_loop(m, P, channels, ts.views(colour_views))
        assert to.same(a, b), (name, P, channels, colour_views)
        print(name, "P", P, "channels", channels, ":", len(m["faces"]), "triangles, atlas", a["atlas"].shape[0], "won", a["n_won"],
              "textured", a["n_textured"])
    if name == "sphere":
        assert _run(name, 2, 3)["n_won"][0] > 256 and _run(name, 2, 3)["n_won"][2] == 0        # AWAY sees nothing


def test_loop_and_vectorised_forms_agree_with_a_z_buffer():
    m = ts.occlusion_mesh()
    for occluded in (False, True):
        v = [ts.occlusion_view(occluded)]
        assert to.same(to.texture(m, 3, 1, v), to.texture_loop(m, 3, 1, v)), occluded


@pytest.mark.parametrize("n_tri,P", [(1, 2), (2, 2), (3, 5), (8, 2), (9, 3), (272, 8), (2592, 4), (11, 32)])
def test_every_texel_belongs_to_one_triangle_or_to_padding(n_tri, P):
    B, Q, A = to.layout(n_tri, P)
    assert Q * Q >= (n_tri + 1) // 2 and (Q == 1 or (Q - 1) * (Q - 1) < (n_tri + 1) // 2) and A == Q * (P + 2)
    tri, l0, l1, l2 = to.texel_map(n_tri, P)
    owners = np.zeros((A, A), np.int64)
    for t in range(n_tri):
        q = t >> 1
        ox, oy = (q % Q) * B, (q // Q) * B
        for a, b, *_ in to._texels_loop(P, t & 1):
            owners[oy + b, ox + a] += 1
            assert tri[oy + b, ox + a] == t
    assert np.array_equal(owners, (tri >= 0).astype(np.int64))
    # the corners' UVs are the centres of texels of the owning triangle, where its barycentrics are 1 0 0, 0 1 0 and 0 0 1
    uv = to.uv(n_tri, P)
    x, y = uv[:, :, 0] * A - 0.5, uv[:, :, 1] * A - 0.5
    xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    assert np.abs(x - xi).max() < 1e-9 and np.abs(y - yi).max() < 1e-9
    assert np.array_equal(tri[yi, xi], np.repeat(np.arange(n_tri)[:, None], 3, axis=1))
    for i, l in enumerate((l0, l1, l2)):
        assert np.array_equal(l[yi[:, i], xi[:, i]], np.ones(n_tri)), i
    assert np.array_equal(l0[yi, xi] + l1[yi, xi] + l2[yi, xi], np.ones((n_tri, 3)))


@pytest.mark.parametrize("name", MESHES)
def test_n_textured_counts_the_triangles_with_a_view(name):
    r = _run(name, 3, 3, False)
    assert r["n_textured"] == int((r["view"] >= 0).sum()) <= len(_mesh(name)["faces"])
    assert ((r["score"] > 0.0) == (r["view"] >= 0)).all() and r["view"].max() < 3 and r["view"].dtype == np.int32
    assert sum(r["n_won"]) >= r["n_textured"] and r["atlas"].dtype == np.uint8


def _texels_of(r, n_tri, P):
    tri = to.texel_map(n_tri, P)[0]
    return tri, tri >= 0


def test_constant_images_give_the_constant_in_every_texel_of_a_textured_triangle():
    m = _mesh("sphere")
    n = len(m["faces"])
    r = to.texture(m, 4, 3, [dict(image=np.broadcast_to(np.array([17, 201, 94], np.uint8), (ts.H, ts.W, 3)).copy(), K=ts.K, pose=p)
                             for p in ts.POSES])
    tri, inside = _texels_of(r, n, 4)
    textured = np.zeros(tri.shape, bool)
    textured[inside] = r["view"][tri[inside]] >= 0
    assert textured.sum() > 0 and (r["atlas"][textured] == np.array([17, 201, 94], np.uint8)).all()
    assert (r["atlas"][~inside] == 0).all()


def test_views_of_constant_grey_restate_the_view_of_every_triangle():
    m = _mesh("sphere")
    n = len(m["faces"])
    r = to.texture(m, 3, 1, ts.constant_views((40, 80, 120)))
    tri, inside = _texels_of(r, n, 3)
    view = r["view"][tri[inside]]
    got = r["atlas"][:, :, 0][inside]
    assert set(np.unique(r["view"])) == {-1, 0, 1}
    assert np.array_equal(got[view >= 0], (40 * (view[view >= 0] + 1)).astype(np.uint8))


def test_the_same_view_twice_wins_nothing_the_second_time():
    m = _mesh("sphere")
    v = ts.views()[:1]
    r = to.texture(m, 2, 3, v + v)
    assert r["n_won"][0] > 0 and r["n_won"][1] == 0 and to.same(dict(r, n_won=r["n_won"][:1]), to.texture(m, 2, 3, v))


def test_reversing_two_views_changes_only_the_triangles_with_tied_scores():
    m = _mesh("sphere")
    A, B = ts.views()[:2]
    twin = dict(A, image=255 - A["image"])                   # A's pose with another image: every score ties
    for first, second, some_tie in ((A, B, False), (A, twin, True)):
        r1, r2 = to.texture(m, 2, 3, [first, second]), to.texture(m, 2, 3, [second, first])
        back = np.where(r2["view"] >= 0, 1 - r2["view"], -1)
        changed = r1["view"] != back
        s1, s2 = to.texture(m, 2, 3, [first])["score"], to.texture(m, 2, 3, [second])["score"]
        assert np.array_equal(r1["score"], r2["score"]) and np.array_equal(s1[changed], s2[changed]) and (s1[changed] > 0).all()
        assert changed.any() == some_tie
        if some_tie:                                         # the earlier view keeps every tie
            assert (r1["view"][changed] == 0).all() and (r2["view"][changed] == 0).all() and changed.sum() == r1["n_won"][0]


def test_sigma_a_triangle_seen_from_the_free_space_side_scores_positive():
    """Every triangle of the sphere's weld with an area is won by one of the six cameras on the axes, all outside the sphere; in
    each of them the candidates that face the camera score > 0 and those that face away do not; from AWAY, which looks away from
    the sphere, none does.  The weld has 228 triangles of area 0 (the field is exactly 0 at a voxel): they score 0 from
    everywhere and stay with the fallback."""
    m = _mesh("sphere")
    X, F = np.asarray(m["vertices"]), np.asarray(m["faces"], np.int64)
    normal = np.cross(X[F[:, 1]] - X[F[:, 0]], X[F[:, 2]] - X[F[:, 0]])
    area = np.sqrt((normal * normal).sum(axis=1))
    assert ((normal * X[F].mean(axis=1)).sum(axis=1)[area > 0] > 0).all()        # the weld's winding: outwards
    won = np.zeros(len(F), bool)
    grey = np.zeros((ts.H, ts.W), np.uint8)
    for pose in ts.AXES:
        r = to.texture(m, 2, 1, [dict(image=grey, K=ts.K, pose=pose)])
        p2, sx, sy = to.project(X, ts.K, *to._camera(dict(K=ts.K, pose=pose))[1:])
        vis = to.visible(p2, sx, sy, ts.W, ts.H, None, 0.0)
        cand = vis[F].all(axis=1)
        facing = (normal * (pose[:3] - X[F].mean(axis=1))).sum(axis=1) > 0
        assert np.array_equal(r["view"] >= 0, cand & facing) and (r["score"][cand & facing] > 0).all()
        won |= r["view"] >= 0
    assert np.array_equal(won, area > 0) and int((~won).sum()) == 228
    away = to.texture(m, 2, 1, [dict(image=grey, K=ts.K, pose=rsc.AWAY)])
    assert away["n_won"] == [0] and (away["view"] == -1).all() and (away["score"] == 0.0).all()


def test_the_z_buffer_takes_the_hidden_triangles_from_the_view():
    """Two sheets one behind the other, both facing the camera: without the z-buffer the view wins every triangle, with it only
    those of the front sheet and of the back sheet's part that the front one does not cover."""
    m = ts.occlusion_mesh()
    off, on = to.texture(m, 3, 1, [ts.occlusion_view(False)]), to.texture(m, 3, 1, [ts.occlusion_view(True)])
    differs = off["view"] != on["view"]
    assert differs.any() and (off["view"][differs] == 0).all() and (on["view"][differs] == -1).all()
    z = np.asarray(m["vertices"])[np.asarray(m["faces"], np.int64)][:, :, 2]
    assert (z[differs] > 1.5).all()                          # all of them on the back sheet
    assert (on["view"][(z < 1.5).all(axis=1)] == 0).all() and on["n_won"][0] < off["n_won"][0] == len(m["faces"])
    print("occlusion off", off["n_won"], "on", on["n_won"], "of", len(m["faces"]))
