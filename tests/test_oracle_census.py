"""The census matching cost on the CPU: hand-worked descriptors, properties of tests/census_oracle.py that
need no device, the accuracy conditions on the re-exposed scenes of tests/census_scene.py (where the absolute-difference cost
fails them), and the ABI table.  The accuracy figures are conditions on the oracle, not measurements of the device code."""
import numpy as np
import pytest

import census_oracle as co
import census_scene as cs
import dense_oracle as do
import dense_scene as ds
import sgm_oracle as so
import sgm_scene as ss


def _bit(dx, dy):
    return 1 << co.OFFSETS.index((dx, dy))


def test_the_bit_order():
    assert co.BITS == 62 and co.OFFSETS[0] == (-4, -3) and co.OFFSETS[8] == (4, -3) and co.OFFSETS[9] == (-4, -2)
    assert co.OFFSETS[30] == (-1, 0) and co.OFFSETS[31] == (1, 0) and co.OFFSETS[61] == (4, 3)


def test_hand_worked_descriptors_on_three_by_three_and_one_by_one():
    img = np.array([[5, 9, 5],
                    [1, 7, 8],
                    [7, 2, 200]], np.uint8)
    T = co.census(img)
    # centre 7: less are 5 (-1, -1), 5 (+1, -1), 1 (-1, 0), 2 (0, +1); the other 7 is a tie, 9, 8 and 200 are greater
    assert int(T[1, 1]) == _bit(-1, -1) | _bit(1, -1) | _bit(-1, 0) | _bit(0, 1)
    # corner 200: all eight others are less, everything else lies outside the image
    assert int(T[2, 2]) == _bit(-2, -2) | _bit(-1, -2) | _bit(0, -2) | _bit(-2, -1) | _bit(-1, -1) | _bit(0, -1) | _bit(-2, 0) | _bit(-1, 0)
    # corner 5 at (0, 0): only the 1 below it and the 2 at (1, 2) are less
    assert int(T[0, 0]) == _bit(0, 1) | _bit(1, 2)
    assert int(T[1, 0]) == 0                                               # the least value of the image
    assert np.array_equal(T, co.census_brute(img))
    assert co.census(np.array([[255]], np.uint8)).tolist() == [[0]] and co.census(np.array([[0]], np.uint8)).tolist() == [[0]]


def test_a_constant_image_and_ties_give_zero():
    assert not co.census(np.full((11, 13), 77, np.uint8)).any()
    assert not co.census(np.full((5, 4), 255, np.uint8)).any()             # 255 beside the outside of the image
    two = np.full((9, 12), 40, np.uint8)
    two[:, 6:] = 41
    T = co.census(two)
    assert not T[:, :6].any() and T[:, 6:10].all() and not T[:, 10:].any()  # only the larger level, within 4 columns, sees a smaller one


@pytest.mark.parametrize("shape", [(47, 61), (19, 37), (1, 33), (19, 1), (16, 32)])
def test_only_bits_0_to_61_are_ever_set_and_the_vectorised_oracle_equals_the_definition(shape):
    img = np.random.default_rng(shape[0]).integers(0, 256, shape).astype(np.uint8)
    T = co.census(img)
    assert T.dtype == np.uint64 and not (T >> np.uint64(62)).any()
    assert np.array_equal(T, co.census_brute(img))
    assert np.array_equal(co.popcount(T), np.array([[bin(int(t)).count("1") for t in row] for row in T]))


def test_a_strictly_increasing_table_leaves_the_descriptor_alone():
    table = cs.monotone_table()
    for case in cs.DESCRIPTOR_CASES[:2] + cs.DESCRIPTOR_CASES[6:7]:
        img = cs.descriptor_image(case) >> 1                               # values <= 127
        assert np.array_equal(co.census(table[img]), co.census(img)), case[0]
    img = cs.descriptor_image(cs.DESCRIPTOR_CASES[0])
    assert not np.array_equal(co.census(255 - img), co.census(img))        # a decreasing one does not


def test_expose():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    up, down = cs.expose(img, *cs.EXPOSURE[1]).reshape(-1), cs.expose(img, *cs.EXPOSURE[2]).reshape(-1)
    assert up.dtype == np.uint8 and up[0] == 15 and up[100] == 140 and up[192] == 255 and up[255] == 255     # 1.25 I + 15
    assert down[0] == 0 and down[12] == 0 and down[13] == 0 and down[14] == 1 and down[255] == 194            # 0.8 I - 10


def _args(views, src, D, radius, trunc):
    return (views[0][0], views[0][1], views[0][2], [views[s] for s in src], ds.W_MIN, ds.W_MAX, D, radius, trunc)


def test_valid_view_counts_equal_the_plain_sweeps_and_the_cost_is_bounded():
    views = ds.step_scene()
    a = _args(views, (1, 2, 3), ds.PLANES, 4, 255)
    C, V = co.cost_volume(*a)
    assert np.array_equal(V, do.cost_volume(*a)[1])
    # an invalid warp costs trunc, a valid one at most min(62, trunc)
    assert 81 * 3 * 62 < int(C.max()) <= 81 * 3 * 255 and int(C.min()) >= 0
    C62, _ = co.cost_volume(*_args(views, (1, 2, 3), ds.PLANES, 4, 62))
    assert int(C62.max()) <= 81 * 3 * 62 and (C62 <= C).all()
    whole = np.stack([do.box_sum((V[k] == 3).astype(np.int64), 4) == 81 for k in range(ds.PLANES)])   # every warp of the window valid
    assert whole.any() and np.array_equal(C62[whole], C[whole])
    C7, _ = co.cost_volume(*_args(views, (1, 2, 3), ds.PLANES, 4, 7))
    assert int(C7.max()) <= 81 * 3 * 7 and (C7 <= C62).all()


def test_identity_pose_gives_cost_zero_and_plane_zero():
    views = ds.step_scene()
    twin = (views[0][0], views[0][1], views[0][2].copy())
    res = co.sweep(views[0][0], views[0][1], views[0][2], [twin], ds.W_MIN, ds.W_MAX, ds.PLANES, 2, 255)
    assert not res["cost"].any() and not res["plane"].any() and (res["views"] == 1).all()


def _share(res, surface, radius):
    m = ds.interior(radius + 3)
    step = do.plane_step(ds.W_MIN, ds.W_MAX, ds.PLANES)
    return float((np.abs(res["inv_depth"] - ds.true_inverse_depth(surface)) <= step)[m].mean()), int(m.sum())


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", ["plane", "step"])
def test_accuracy_condition_on_the_re_exposed_scenes(name, radius):
    """D = 12, sources (1, 2), the interior of ds.interior(radius + 3): at least 90 % of its pixels have a refined inverse
    depth within one plane step of the truth with the census cost (trunc 255), re-exposed or not, and fewer than 10 % with
    the absolute difference (trunc 20) once the sources are re-exposed.  The oracle's shares are in DESIGN.md §20.4."""
    scene, surface = ((ds.plane_scene(), ss.PLANE_SURFACE) if name == "plane" else (ds.step_scene(), ss.STEP_SURFACE))
    again = cs.exposed(scene)
    plain, n = _share(co.sweep(*_args(scene, (1, 2), ds.PLANES, radius, 255)), surface, radius)
    census, _ = _share(co.sweep(*_args(again, (1, 2), ds.PLANES, radius, 255)), surface, radius)
    ad_before, _ = _share(do.sweep(*_args(scene, (1, 2), ds.PLANES, radius, 20)), surface, radius)
    ad, _ = _share(do.sweep(*_args(again, (1, 2), ds.PLANES, radius, 20)), surface, radius)
    print(name, "radius", radius, "interior pixels", n, "census", plain, "census re-exposed", census, "AD", ad_before, "AD re-exposed", ad)
    assert n == {1: 351, 2: 275}[radius]
    assert plain >= 0.90 and census >= 0.90 and ad < 0.10


@pytest.mark.parametrize("name", ["flat_plane", "flat_step"])
def test_accuracy_condition_on_the_re_exposed_flat_patch_scenes(name):
    """Radius 1, trunc 20, P1 = 36, P2 = 288, 8 paths: census through the aggregation at least 90 %, the absolute difference
    through it fewer than 10 %."""
    scene, surface = ((ss.flat_plane_scene(), ss.PLANE_SURFACE) if name == "flat_plane" else (ss.flat_step_scene(), ss.STEP_SURFACE))
    a = _args(cs.exposed(scene), (1, 2), ds.PLANES, 1, 20)
    census, n = _share(co.sweep_sgm(*a, ss.P1, ss.P2, 8), surface, 1)
    ad, _ = _share(so.sweep_sgm(*a, ss.P1, ss.P2, 8), surface, 1)
    print(name, "interior pixels", n, "census + SGM", census, "AD + SGM", ad)
    assert n == 351 and census >= 0.90 and ad < 0.10


def test_case_tables():
    shapes = {(c[1], c[2]) for c in cs.DESCRIPTOR_CASES}
    assert {(61, 47), (37, 19), (32, 16), (65, 33), (33, 1), (1, 19)} <= shapes
    assert {c[3] for c in cs.DESCRIPTOR_CASES} == {"scene", "random", "constant", "border255"}
    assert cs.SWEEP_CASES is ds.CASES
    assert [(c[1], c[2], c[3], c[9]) for c in cs.SGM_CASES] == [(61, 47, 12, 8), (61, 47, 12, 4), (37, 19, 70, 8), (33, 1, 12, 8)]


def test_prototype_table_covers_the_census_section():
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi
    names = set(pkg.declared_symbols())
    for n in ("ekf_dense_sweep_census", "ekf_dense_sweep_sgm_census", "ekf_dense_get_census", "ekf_dense_get_census_profile"):
        assert n in names and n in capi._PROTOS
    assert all(hasattr(pkg.DenseStereo, m) for m in ("census", "get_census_profile"))
    import inspect
    from ekf_monoslam_amd import dense
    for fn in (pkg.DenseStereo.sweep, pkg.DenseStereo.sweep_sgm, dense.depth_maps_from_recording):
        assert inspect.signature(fn).parameters["cost"].default == "ad"
    with pytest.raises(ValueError):
        dense.depth_maps_from_recording("nowhere", cost="ssd")
    with pytest.raises(ValueError):
        dense._cost_entry(None, "Census", "ekf_dense_sweep")


def test_the_cost_keyword_reaches_the_sweep_through_the_fusion_drivers(monkeypatch):
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
            driver("nowhere", None, sweep_trunc=30, planes=12, cost="census")
    assert seen == [dict(trunc=30, planes=12, cost="census")] * 2
