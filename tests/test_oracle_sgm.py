"""The semi-global aggregation contract on the CPU: properties of tests/sgm_oracle.py that need no device,
the vectorised oracle against the recurrence spelled out pixel by pixel, the accuracy condition on the flat-patch scenes of
tests/sgm_scene.py (where the pixel-wise winner fails it) and on the textured scenes, and the ABI table."""
import numpy as np
import pytest

import dense_oracle as do
import dense_scene as ds
import sgm_oracle as so
import sgm_scene as ss


def _volume(shape, seed, high=500):
    return np.random.default_rng(seed).integers(0, high, shape).astype(np.int64)


def test_one_row_high_the_vertical_paths_have_length_one():
    """paths = 4 on an image one row high: S = L_r0 + L_r1 + 2 C."""
    C = _volume((7, 1, 13), 1)
    S = so.aggregate(C, 5, 40, 4)
    assert np.array_equal(S, so.path_cost(C, 5, 40, 1, 0) + so.path_cost(C, 5, 40, -1, 0) + 2 * C)
    assert np.array_equal(so.path_cost(C, 5, 40, 0, 1), C) and np.array_equal(so.path_cost(C, 5, 40, 0, -1), C)
    assert np.array_equal(so.path_cost(C, 5, 40, 1, -1), C)               # and so have the diagonal ones


def test_every_path_cost_lies_between_c_and_c_plus_p2():
    C = _volume((6, 9, 11), 2)
    for p1, p2 in ((17, 17), (3, 60)):
        for dx, dy in so.DIRECTIONS:
            L = so.path_cost(C, p1, p2, dx, dy)
            assert (L >= C).all() and (L <= C + p2).all(), (p1, p2, dx, dy)


def test_costs_that_do_not_depend_on_the_pixel_keep_their_winner():
    col = np.array([40, 12, 30, 12, 55, 90], np.int64)                    # two minima: the smaller plane wins both times
    C = np.broadcast_to(col[:, None, None], (6, 5, 8)).copy()
    V = np.ones_like(C)
    for paths in (4, 8):
        S = so.aggregate(C, 4, 30, paths)
        a, b = do.winner(S, V, 0.1, 0.5), do.winner(C, V, 0.1, 0.5)
        assert np.array_equal(a["plane"], b["plane"]) and (a["plane"] == 1).all()


@pytest.mark.parametrize("paths", [4, 8])
def test_the_vectorised_oracle_equals_the_recurrence_pixel_by_pixel(paths):
    C = _volume((5, 7, 9), 3)                                             # 9 x 7 pixels, 5 planes
    for p1, p2 in ((1, 1), (7, 50), (5000, 1 << 20)):
        assert np.array_equal(so.aggregate(C, p1, p2, paths), so.aggregate_brute(C, p1, p2, paths)), (p1, p2)


def test_default_penalties():
    assert so.default_penalties(1, 2) == (ss.P1, ss.P2) == (36, 288)


def _shares(scene, surface, paths):
    """(aggregated share, winner-take-all share, interior pixels) at radius 1, trunc 20, sources (1, 2)."""
    ref = scene[0]
    C, V = do.cost_volume(ref[0], ref[1], ref[2], [scene[1], scene[2]], ds.W_MIN, ds.W_MAX, ds.PLANES, 1, 20)
    res = do.winner(so.aggregate(C, ss.P1, ss.P2, paths), V, ds.W_MIN, ds.W_MAX)
    wta = do.winner(C, V, ds.W_MIN, ds.W_MAX)
    m = ds.interior(1)
    step = do.plane_step(ds.W_MIN, ds.W_MAX, ds.PLANES)
    truth = ds.true_inverse_depth(surface)
    share = lambda r: float((np.abs(r["inv_depth"] - truth) <= step)[m].mean())
    return share(res), share(wta), int(m.sum())


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", ["flat_plane", "flat_step"])
def test_accuracy_condition_on_the_flat_patch_scenes(name, paths):
    """At least 90 % of the interior pixels have a refined inverse depth within one plane step of the truth after the
    aggregation, and fewer than 90 % before it (the oracle's shares are in DESIGN.md §19.4)."""
    scene, surface = ((ss.flat_plane_scene(), ss.PLANE_SURFACE) if name == "flat_plane" else (ss.flat_step_scene(), ss.STEP_SURFACE))
    assert ss.flat_share(scene) > 0.1                                      # the patch is in the picture
    agg, wta, n = _shares(scene, surface, paths)
    print(name, "paths", paths, "interior pixels", n, "aggregated share", agg, "winner-take-all share", wta)
    assert n >= 400 and agg >= 0.90 and wta < 0.90


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", ["plane", "step"])
def test_accuracy_condition_on_the_textured_scenes(name, paths):
    scene, surface = ((ds.plane_scene(), ss.PLANE_SURFACE) if name == "plane" else (ds.step_scene(), ss.STEP_SURFACE))
    agg, wta, n = _shares(scene, surface, paths)
    print(name, "paths", paths, "interior pixels", n, "aggregated share", agg, "winner-take-all share", wta)
    assert n >= 400 and agg >= 0.90


def test_case_table_covers_every_kernel_shape():
    """The GPU cases take every instantiation they can reach at a few thousand pixels: 16 lanes a line (D <= 16), one, two
    and four planes a lane, both path counts, lines of one pixel."""
    D = sorted({c[3] for c in ss.CASES})
    assert D == [2, 12, 70, 130] and {c[9] for c in ss.CASES} == {4, 8}
    assert len({c[0] for c in ss.CASES}) == len(ss.CASES) == 11
    assert any(c[2] == 1 for c in ss.CASES) and any(c[1] == 1 for c in ss.CASES)


def test_prototype_table_covers_the_sgm_section():
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi
    names = set(pkg.declared_symbols())
    for n in ("ekf_dense_sweep_sgm", "ekf_dense_get_volume", "ekf_dense_get_sgm_profile"):
        assert n in names and n in capi._PROTOS
    assert all(hasattr(pkg.DenseStereo, m) for m in ("sweep_sgm", "volume", "get_sgm_profile"))


def test_the_sgm_keyword_reaches_the_sweep_through_the_fusion_drivers(monkeypatch):
    """mesh_from_recording and audit_recording hand ``sgm`` on to depth_maps_from_recording with their sweep keywords."""
    import __graft_entry__ as g
    g.load_package()
    from ekf_monoslam_amd import dense, fusion
    seen = []

    class Reached(Exception):
        pass

    def record(directory, nodes_out=None, **kw):
        seen.append(kw)
        raise Reached()

    monkeypatch.setattr(dense, "depth_maps_from_recording", record)
    for driver in (fusion.mesh_from_recording, fusion.audit_recording):
        with pytest.raises(Reached):
            driver("nowhere", None, sweep_trunc=20, planes=12, sgm=dict(p1=3, p2=40, paths=4))
    assert seen == [dict(trunc=20, planes=12, sgm=dict(p1=3, p2=40, paths=4))] * 2
