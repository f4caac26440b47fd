"""The mesh-to-mesh distance of DESIGN.md §31 on the CPU: the two numpy forms of tests/distance_oracle.py against each other and
against the model of the grid search, properties that hold whatever they compute, the figures of the 17 x 15 x 13 sphere that §31
records, and the header, the prototypes and the exports.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distance_oracle as do
import distance_scene as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_distance_set_mesh", "ekf_distance_run", "ekf_distance_run_points", "ekf_distance_get", "ekf_distance_get_stats",
         "ekf_distance_set_grid", "ekf_distance_get_grid", "ekf_distance_get_profile")
KEYS = ("dist", "tri", "closest", "side", "d2")
MODEL_GRIDS = (1, 2, 5, 7, 0)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_result(a, b):
    return all(_same(a[k], b[k]) for k in KEYS)


def _walk_equals(mesh, points, want, g):
    w = do.grid_walk(mesh, points, g, want["matrix"])
    return _same(w["d2"], want["d2"]) and _same(w["tri"], want["tri"]), w


@pytest.mark.parametrize("name", sorted(ds.scenes()))
def test_the_loop_the_vectorised_form_and_the_grid_walk_agree(name):
    """Bit for bit on every scene: dist, tri, closest, side and d2 of the two forms, and the (d2, tri) that the grid search's
    model reaches at g = 1, 2, 5, 7 and automatic; the statistics of the two forms."""
    mesh, points = ds.scenes()[name]
    loop, vec = do.distance_loop(mesh, points), do.distance(mesh, points, want_d2=True)
    assert _same_result(loop, vec)
    for g in MODEL_GRIDS:
        ok, w = _walk_equals(mesh, points, vec, g)
        assert ok, g
        print(name, "g", g, w["grid"]["G"], "shells", int(w["shells"].max()), "evaluations", int(w["evals"].sum()), "longest list", w["longest"])
    for thr in (0.0, 0.0625, 3.0):
        a, b = do.stats(vec["dist"], thr), do.stats_loop(vec["dist"], thr)
        assert a.keys() == b.keys() and all(_same(np.float64(a[k]), np.float64(b[k])) for k in a), thr


def test_the_seven_regions_and_the_ties():
    mesh, points = ds.regions()
    r = do.distance(mesh, points)
    assert all(tuple(r["closest"][i]) == c for i, c in ds.REGION_TRUTH.items())
    assert [int(s) for s in r["side"]] == [ds.REGION_SIDE.get(i, 0) for i in range(len(points))]
    assert (r["dist"][[8, 9, 10, 11, 12]] == 0.0).all() and r["dist"][6] == 3.0 and r["dist"][7] == 3.0 and r["dist"][3] == 2.0
    for order in (0, 1):                                           # equidistant from both triangles: the lower index
        mesh, points = ds.shared_edge(order)
        r = do.distance(mesh, points, want_d2=True)
        assert _same(r["matrix"][:6, 0], r["matrix"][:6, 1]) and (r["tri"][:6] == 0).all()
        assert r["tri"][6] == order and r["tri"][7] == 1 - order
    mesh, points = ds.coincident()
    r = do.distance(mesh, points, want_d2=True)
    assert _same(r["matrix"][:, 0], r["matrix"][:, 1]) and (r["tri"] == 0).all()
    mesh, points = ds.degenerate()
    r = do.distance(mesh, points, want_d2=True)
    assert list(do.valid(*do._mesh(mesh))) == [False, False, False, True, True] and set(r["tri"]) <= {3, 4}
    assert np.isnan(r["matrix"][:, :3]).all() and do.distance(*ds.only_degenerate()) is None and do.distance_loop(*ds.only_degenerate()) is None


def test_the_tie_across_shells_needs_the_strict_rule():
    """All twelve d2 of the cube from the origin are exactly 1 and triangle 0 wins; with g = 5 face x = -1 lies in shell 0 and face
    x = +1 only in shell 1, and a rule that ends on equality gives triangle 2."""
    mesh, points = ds.tie_shells()
    r = do.distance(mesh, points, want_d2=True)
    assert (r["matrix"][0, :12] == 1.0).all() and r["tri"][0] == 0 and r["dist"][0] == 1.0
    w = do.grid_walk(mesh, points, 5, r["matrix"])
    assert w["grid"]["G"] == [5, 1, 1] and w["grid"]["h"][0] == 2.0 and w["shells"][0] >= 2 and w["tri"][0] == 0
    cells = do.file_triangles(*do._mesh(mesh), w["grid"])
    assert {2, 3} <= set(cells[(0, 0, 0)]) and not {0, 1} & set(cells[(0, 0, 0)]) and {0, 1} <= set(cells[(1, 0, 0)])
    assert do.grid_walk(mesh, points, 5, r["matrix"], strict=False, slack=0.0)["tri"][0] == 2
    # the points that are not finite, and those far outside
    assert np.isnan(r["dist"][14:17]).all() and (r["tri"][14:17] == do.NO_TRI).all() and (r["side"][14:17] == 0).all()
    assert r["tri"][3] == 12 and r["dist"][3] == 1000000.0 - 9.0
    s = do.stats(r["dist"], 1.0)
    assert (s["n"], s["n_bad"], s["argmax"]) == (15, 3, 4) and s["within"] == int((r["dist"] <= 1.0).sum())


def test_properties_of_the_result():
    """Whatever the routine computes: closest lies in the winner's box exactly and in its plane to rounding; the distance of a
    valid triangle's own vertices to their mesh is 0; the statistics' identities."""
    for name, (mesh, points) in list(ds.scenes().items()) + [("sphere", (ds.sphere_weld(), ds.sphere_simplified(2.0)["vertices"]))]:
        X, F = do._mesh(mesh)
        r = do.distance(mesh, points)
        ok = r["tri"] != do.NO_TRI
        T = X[F[r["tri"][ok]]]                                      # (n, 3 corners, 3)
        c = r["closest"][ok]
        assert (c >= T.min(axis=1)).all() and (c <= T.max(axis=1)).all(), name
        n = do.normals(X, F)[r["tri"][ok]]
        off = np.abs(((c - T[:, 0]) * n).sum(axis=1)) / np.sqrt((n * n).sum(axis=1))
        scale = np.abs(T).max(axis=(1, 2)) + np.abs(points[ok]).max(axis=1)
        assert (off <= 64 * 2.0 ** -52 * scale).all(), (name, float((off / scale).max()))
        assert _same(r["dist"][ok], np.sqrt(r["d2"][ok])) and (np.isnan(r["dist"]) == ~ok).all()
        own = np.unique(F[do.valid(X, F)])
        assert (do.distance(mesh, X[own])["dist"] == 0.0).all(), name
        for thr in (0.0, 0.5):
            s = do.stats(r["dist"], thr)
            d = r["dist"][ok]
            assert s["n"] + s["n_bad"] == len(points) and s["n"] == int(ok.sum()) and s["max"] == d.max() and s["argmax"] == int(np.flatnonzero(r["dist"] == d.max())[0])
            assert 0 <= s["within"] <= s["n"] and s["mean"] <= s["rms"] * (1 + 1e-15) <= s["max"] * (1 + 1e-14)
            assert abs(s["sum"] - float(np.sum(d))) <= 1e-12 * max(1.0, s["sum"]) and _same(np.float64(s["mean"]), np.float64(s["sum"] / s["n"]))
    e = do.stats(np.array([np.nan, np.nan]), 1.0)
    assert (e["n"], e["n_bad"], e["within"], e["argmax"]) == (0, 2, 0, do.NO_TRI) and e["max"] != e["max"] and e["mean"] != e["mean"]


def test_the_sphere_and_its_simplifications():
    """The 17 x 15 x 13 sphere, weld -> simplified and simplified -> weld at cells of 1, 2 and 3.5 voxels: both one-sided means
    grow with the cell, and the mean side-signed distance of the simplified vertices from the weld is negative: §28.4's shrinkage
    seen in 3-D.  The grid-walk model agrees at the automatic g and at 5.  §31.4 records the figures printed here."""
    weld = ds.sphere_weld()
    to_weld, to_simp, signed = [], [], []
    for factor in ds.FACTORS:
        simp = ds.sphere_simplified(factor)
        a = do.distance(weld, simp["vertices"], want_d2=True)       # simplified -> weld
        b = do.distance(simp, weld["vertices"], want_d2=True)       # weld -> simplified
        for g in (0, 5):
            assert _walk_equals(weld, simp["vertices"], a, g)[0] and _walk_equals(simp, weld["vertices"], b, g)[0], (factor, g)
        sa, sb = do.stats(a["dist"], 0.0625), do.stats(b["dist"], 0.0625)
        to_weld.append(sa["mean"])
        to_simp.append(sb["mean"])
        signed.append(float(np.mean(a["side"] * a["dist"])))
        print("cell %.1f voxels: %d vertices %d triangles; simplified -> weld mean %.6f rms %.6f max %.6f; weld -> simplified mean %.6f "
              "rms %.6f max %.6f within 0.0625: %d of %d; signed mean %.6f" % (factor, len(simp["vertices"]), len(simp["faces"]), sa["mean"],
                                                                            sa["rms"], sa["max"], sb["mean"], sb["rms"], sb["max"],
                                                                            sb["within"], sb["n"], signed[-1]))
    assert to_weld[0] < to_weld[1] < to_weld[2] and to_simp[0] < to_simp[1] < to_simp[2]
    assert all(s < 0.0 for s in signed)


def test_abi_the_header_the_prototypes_and_the_exports():
    """The header, _PROTOS and the exports, and EKF_ERR_ARG for a NULL handle.  Fails on the parent."""
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi, fusion
    header = open(os.path.join(ROOT, "include", "ekf_monoslam.h")).read()
    lib = pkg.load_library()
    for fn in NAMES:
        assert re.search(r"^int %s\(" % fn, header, flags=re.M) and fn in capi._PROTOS and hasattr(lib, fn), fn
    assert sorted(n for n in pkg.declared_symbols() if n.startswith("ekf_distance_")) == sorted(NAMES)
    assert [len(capi._PROTOS[n][1]) for n in NAMES] == [5, 4, 4, 6, 9, 2, 4, 3] and lib.ekf_abi_version() == 6
    assert lib.ekf_distance_set_mesh(None, None, None, 0, 0) == 1 and lib.ekf_distance_run(None, 0, 0, None) == 1
    assert lib.ekf_distance_run_points(None, 0, None, 0) == 1 and lib.ekf_distance_get(None, None, None, None, None, 0) == 1
    assert lib.ekf_distance_get_stats(None, C.c_double(0.0), None, None, None, None, None, None, None) == 1
    assert lib.ekf_distance_set_grid(None, 0) == 1 and lib.ekf_distance_get_grid(None, None, None, None) == 1
    assert lib.ekf_distance_get_profile(None, None, None) == 1
    assert fusion.DISTANCE_KERNELS == ("k_dist_box", "k_dist_grid", "k_dist_count", "k_dist_offsets", "k_tsdf_scan", "k_dist_fill",
                                       "k_dist_query", "k_dist_stats", "k_dist_reduce")
    assert fusion.DISTANCE_SOURCES == fusion.RASTER_SOURCES and pkg.MeshDistance and pkg.DistanceStats and pkg.compare_meshes
    assert all(hasattr(fusion.TsdfVolume, n) for n in ("set_distance_mesh", "distance", "distance_points", "distance_stats",
                                                       "set_distance_grid", "get_distance_profile"))
    text = open(os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "csrc", "ekf_mesh_distance.hpp")).read()
    assert text.count("__device__ __forceinline__ double dist_closest(") == 1 and "atomicAdd" not in text and "double*" in text
