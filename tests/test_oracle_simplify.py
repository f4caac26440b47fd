"""The two forms of tests/simplify_oracle.py against each other, bit for bit, and against what the contract
implies whatever they compute, on the meshes of tests/component_scene.py at cells of 1, 2 and 3.5 voxels and on hand-made
meshes.  CPU only."""
import functools

import numpy as np
import pytest

import component_scene as cs
import simplify_oracle as so

FACTORS = (1.0, 2.0, 3.5)
CASES = [(name, mc) for name in cs.NAMES for mc in cs.cases()[name][5]]


@functools.lru_cache(maxsize=None)
def _run(name, mc, factor, normals=True):
    """The vectorised oracle's result of a case: computed once, shared, and left unchanged."""
    _, dims, origin, voxel, _, _ = cs.cases()[name]
    return so.simplify(cs.oracle_mesh(name, mc, normals), origin, dims, voxel, factor * voxel)


def _check_invariants(src, r, origin, dims, voxel, cell):
    """What holds whatever the oracle computes."""
    F = np.asarray(src["faces"], np.int64).reshape(-1, 3)
    faces, key, vmap, kept, vc = r["faces"], r["key"], r["map"], r["kept"], r["cells"]
    G = r["grid"]
    assert G == so.grid(dims, voxel, cell) and all(1 <= g <= d for g, d in zip(G, dims))
    assert len(vc) == len(src["vertices"]) and ((vc >= 0) & (vc < G[0] * G[1] * G[2])).all()
    # every face has three distinct indices; no two share an unordered triple; every vertex is referenced
    assert ((faces[:, 0] != faces[:, 1]) & (faces[:, 0] != faces[:, 2]) & (faces[:, 1] != faces[:, 2])).all()
    assert len(np.unique(np.sort(faces, axis=1), axis=0)) == len(faces)
    assert np.array_equal(np.unique(faces), np.arange(len(key)))
    # keys ascend strictly; the counts add up; the kept faces are in source order, with the source's winding
    assert (np.diff(key.astype(np.int64)) > 0).all()
    assert len(faces) + r["n_degenerate"] + r["n_duplicate"] == len(F) and len(kept) == len(faces)
    assert (np.diff(kept) > 0).all() and np.array_equal(key.astype(np.int64)[faces], vc[F[kept]])
    # the map is consistent with the cells: a mapped vertex lies in the cell its output vertex has as key, an unmapped one in
    # a cell that no output vertex has
    hit = vmap != so.NONE
    assert np.array_equal(key.astype(np.int64)[vmap[hit]], vc[hit]) and not np.isin(vc[~hit], key.astype(np.int64)).any()
    # a dropped triangle is degenerate or has the triple of an earlier kept one
    tc = np.sort(vc[F], axis=1)
    dropped = np.setdiff1d(np.arange(len(F)), kept)
    deg = (tc[:, 0] == tc[:, 1]) | (tc[:, 1] == tc[:, 2])
    assert int(deg.sum()) == r["n_degenerate"] and not deg[kept].any()
    first = {tuple(t): i for i, t in zip(kept[::-1].tolist(), tc[kept][::-1].tolist())}
    assert all(deg[t] or first[tuple(tc[t])] < t for t in dropped.tolist())
    # a vertex lies inside the box of its members (where they are finite), a grey inside their range
    X = np.asarray(src["vertices"], np.float64)
    for i in range(0, len(key), max(1, len(key) // 50)):
        m = np.nonzero(vc == int(key[i]))[0]
        assert len(m)
        if np.isfinite(X[m]).all():
            assert (r["vertices"][i] >= X[m].min(axis=0) - 1e-12).all() and (r["vertices"][i] <= X[m].max(axis=0) + 1e-12).all()
        assert src["grey"][m].min() <= r["grey"][i] <= src["grey"][m].max()
    assert (r["normals"] is None) == (src["normals"] is None) and (r["colour"] is None) == (src["colour"] is None)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name,mc", CASES)
def test_the_two_forms_agree_and_the_contract_s_invariants_hold(name, mc, factor):
    _, dims, origin, voxel, _, _ = cs.cases()[name]
    src = cs.oracle_mesh(name, mc, True)
    r = _run(name, mc, factor)
    if len(src["faces"]) <= 20000:                                   # the loop form of the sheet's 131 072 triangles: once, below
        assert so.same(r, so.simplify_loop(src, origin, dims, voxel, factor * voxel))
    _check_invariants(src, r, origin, dims, voxel, factor * voxel)
    print(name, mc, factor, ":", len(src["faces"]), "->", len(r["faces"]), "triangles,", len(src["key"]), "->", len(r["key"]), "vertices,",
          r["n_degenerate"], "degenerate,", r["n_duplicate"], "duplicate, longest member list", int(np.bincount(r["cells"]).max()))


def test_the_two_forms_agree_on_the_sheet():
    _, dims, origin, voxel, _, _ = cs.cases()["sheet"]
    assert so.same(_run("sheet", 1, 2.0), so.simplify_loop(cs.oracle_mesh("sheet", 1, True), origin, dims, voxel, 2.0 * voxel))


def test_a_source_without_normals_gives_the_same_rows_without_normals():
    for name, mc in (("main", 1), ("16x16x3", 2)):
        a, b = _run(name, mc, 2.0), _run(name, mc, 2.0, False)
        assert b["normals"] is None and a["normals"] is not None
        assert so.same(dict(a, normals=None), b)


def test_the_cases_the_scenes_reach():
    """Duplicates, occupied but unused cells, an empty result, and the issue's prototype figures."""
    r = _run("main", 1, 3.5)
    assert (r["n_duplicate"], len(r["faces"])) == (9, 18)
    r = _run("257x2x2", 1, 1.0)
    assert len(np.unique(r["cells"])) == 257 and len(r["key"]) == 135 and int((r["map"] == so.NONE).sum()) > 0
    r = _run("257x2x2", 1, 2.0)
    assert len(r["key"]) == 0 and len(r["faces"]) == 0 and r["vertices"].shape == (0, 3) and (r["map"] == so.NONE).all()
    assert r["n_degenerate"] == 964
    figures = {("sphere", 1.0): (846, 425), ("sphere", 2.0): (218, 111), ("main", 1.0): (110, 71)}
    for (name, f), (nt, nv) in figures.items():
        r = _run(name, 1, f)
        assert (len(r["faces"]), len(r["key"])) == (nt, nv)
    assert int(np.bincount(_run("tie", 1, 3.5)["cells"]).max()) == 98


def _hand(mesh, cell):
    a = so.simplify(mesh, so.HAND_ORIGIN, so.HAND_DIMS, so.HAND_VOXEL, cell)
    assert so.same(a, so.simplify_loop(mesh, so.HAND_ORIGIN, so.HAND_DIMS, so.HAND_VOXEL, cell))
    _check_invariants(mesh, a, so.HAND_ORIGIN, so.HAND_DIMS, so.HAND_VOXEL, cell)
    return a


def test_of_two_triangles_of_opposite_winding_over_the_same_cells_the_first_is_kept():
    r = _hand(so.opposite_winding_mesh(), 1.0)
    assert r["kept"].tolist() == [0] and r["n_duplicate"] == 1 and r["n_degenerate"] == 0
    assert r["key"].tolist() == [0, 1, 5] and r["faces"].tolist() == [[0, 1, 2]] and r["map"].tolist() == [0, 1, 2, 0, 1, 2]
    # the mean of the two members of a cell, and of their greys with the half rounded up: (0 + 111 + 1) // 2
    assert r["vertices"][0].tolist() == [(0.2 + 0.7) / 2.0] * 3 and r["grey"].tolist() == [56, 93, 130]


def test_a_vertex_outside_the_box_is_clamped_and_one_that_is_not_finite_counts_as_zero():
    r = _hand(so.outside_mesh(), 1.0)
    # (-3.5 -> 0, 9 -> 4, 77 -> 4, inf -> 0, nan -> 0, -inf -> 0)
    assert r["cells"].tolist() == [0, 4, (4 * 5 + 2) * 5 + 0, (1 * 5 + 1) * 5 + 0, (0 * 5 + 3) * 5 + 0, (2 * 5 + 2) * 5 + 2]
    assert len(r["faces"]) == 2 and r["n_degenerate"] == 0


def test_a_cell_so_large_that_the_grid_is_one_cell_gives_the_empty_mesh():
    for mesh in (so.outside_mesh(), so.opposite_winding_mesh(), so.fan_mesh()):
        r = _hand(mesh, 1.0e9)
        assert r["grid"] == (1, 1, 1) and (r["cells"] == 0).all() and len(r["key"]) == 0 and r["n_degenerate"] == len(mesh["faces"])
    _, dims, origin, voxel, _, _ = cs.cases()["sphere"]
    r = so.simplify(cs.oracle_mesh("sphere", 1), origin, dims, voxel, 1.0e6)
    assert r["grid"] == (1, 1, 1) and len(r["faces"]) == 0 and r["n_degenerate"] == 2592


def test_a_fan_under_one_least_cell_keeps_each_triple_once():
    r = _hand(so.fan_mesh(), 1.0)
    assert (len(r["faces"]), r["n_degenerate"], r["n_duplicate"]) == (40, 0, 14) and r["kept"].tolist() == list(range(40))
    _hand(so.fan_mesh(), 2.0)


def test_the_grid_never_has_more_cells_than_the_volume_has_voxels():
    for dims, voxel in (((17, 15, 13), 0.25), ((257, 2, 2), 0.1), ((2, 2, 2), 1.0), ((1024, 3, 7), 0.0123)):
        for f in (1.0, 1.0 + 2.0 ** -52, 1.5, 2.0, 3.5, 1000.0):
            G = so.grid(dims, voxel, f * voxel)
            assert all(1 <= g <= d for g, d in zip(G, dims)), (dims, voxel, f, G)
